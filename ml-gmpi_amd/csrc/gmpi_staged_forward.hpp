// gmpi_staged_forward.hpp -- what the two staged forwards that copy a tile's texel box to LDS as four fp32 channel planes hold in common:
// render_shared_forward_kernel (render_shared_forward.hip, which has the why of every piece) and render_shaded_forward_kernel (render_shaded.hip).
// One set of constants and the two rules of their *_forward_supports predicates.  The plane loops themselves stay written out in the two kernels:
// as ONE function body with a Source policy the loop compiles to another schedule and measured 1-5 % slower (profiles/staged_forward_frame.txt).
#pragma once
#include "gmpi_device.hpp"
#include "gmpi_shared.hpp"

namespace gmpi {

constexpr int kSFW = 32, kSFH = 16, kSFThreads = kSFW * kSFH;   // pixel tile, one pixel per thread
constexpr int kSFPitch = 56, kSFRows = 27;                      // staging buffer: texels per (row, channel) line, texel rows
constexpr int kSFTPI = 4, kSFCols = kSFPitch / kSFTPI;          // texels per loader item, items per line
constexpr int kSFBufFloats = kSFRows * 4 * kSFPitch;            // 6048 floats = 24 192 bytes
constexpr int kSFChunk = 64;                                    // planes per box-table refill
static_assert(kSFRows * kSFCols <= kSFThreads, "one loader item per thread and channel");
constexpr bool staged_forward_fits_lds(int table_bytes) { return 2 * kSFBufFloats * 4 + kSFChunk * table_bytes <= 53 * 1024; }   // 3 workgroups per CU

// ---- host side: what a tensor must satisfy to be loaded in items ---------------------------------------------------------------------------------
// base and strides on an item boundary (es: bytes per element)
inline __host__ bool staged_item_aligned(const void* base, int64_t es, int64_t s0, int64_t s1, int64_t s2 = 0, int64_t s3 = 0) {
    return reinterpret_cast<uintptr_t>(base) % static_cast<uintptr_t>(kSFTPI * es) == 0 && s0 % kSFTPI == 0 && s1 % kSFTPI == 0 && s2 % kSFTPI == 0 && s3 % kSFTPI == 0;
}
// the in-box byte offsets of an image with this row stride stay below 2^31
inline __host__ bool staged_offsets_fit(int64_t s_row, int64_t es) { return (kSFRows + 1) * s_row + 128 < (int64_t(1) << 31) / es; }

}  // namespace gmpi
