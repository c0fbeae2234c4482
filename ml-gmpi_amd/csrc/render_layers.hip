// render_layers.hip -- GMPI_VARIANT_LDS of gmpi_mpi_render_layers_launch: the tile frame of render_u8.hip over channels-last FLOAT layers.
//
// The volume is [M, D, Ht, Wt, 4] (channel stride 1, texel stride 4 elements): one texel = R, G, B, A = 16 bytes of fp32 or 8 bytes of fp16 / bf16
// (rgba32f_t / rgba16h_t / rgba16b_t, gmpi_device.hpp; strides in BYTES).  One workgroup of 512 threads owns a 32 x 16 pixel tile (one pixel per
// thread) and walks the D planes front to back; per plane the texel box spanned by the tile's four corner pixels is staged in LDS, two buffers, one
// barrier per plane, the loads of plane k + 1 in flight while plane k is composited; the per-plane table holds 64 planes (render_u8.hip and
// render_lds.hip have the why; tile decode, pixel, corner box and origin words are the tile frame of gmpi_device.hpp).
//
// The LDS image is the memory image: the raw texels of a 64 x 32 box, row after row.
//  * One loader item = 16 bytes = one buffer_load_dwordx4 through the plane's descriptor and one ds_write_b128, nothing in between: one fp32 texel,
//    or the 16-bit texel pair (x, x + 1) with x even.  fp32: 64 items per box row, 2048 per box, 4 per thread; 16-bit: 32 per row, 1024, 2 per thread.
//    The thread -> item map is fixed at compile time (item r of a thread lies 8 resp. 16 box rows below item r - 1).
//  * Items outside the box or outside the texture take the offset the hardware range check rejects (0x80000000 == num_records): zeros without a
//    memory access, which IS padding_mode="zeros"; nothing is exec-masked.  A 16-bit item never straddles the right border: Wt is even
//    (layers_variant_supports) and the box origin is rounded down to an even column.
//  * The prefetch does not cross a chunk of the table: the load behind a chunk's last plane is rejected as a whole (render_u8.hip).
//
// Pitch and read instruction, from the LDS banking table of MI355X_MICROARCH.md (section LDS):
//  * fp32: a footprint is the texels (x, x + 1) of rows y and y + 1: four ds_read_b128 (16-byte aligned by construction).  ds_read_b128 is served in
//    four groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32), bank = (a / 4) mod 64: a texel covers 4 banks, 16 texels
//    all 64.  A 32-lane half wave is one pixel row of the tile; under a near-identity warp its lanes read consecutive texels, and the lane numbers of
//    each group are distinct modulo 16: x mod 16 distinct -> conflict-free, 4 LDS cycles per instruction, the instruction's floor.  Row pitch
//    64 texels = 1024 bytes = a multiple of the 256 bytes of all banks: where a tilted pixel row steps from texel row y to y + 1, the two runs keep
//    their x mod 16, so the step adds no conflict.  A skewed pitch would buy nothing here and cost the power-of-two address.
//  * 16-bit: the pair (x, x + 1) of a row is 16 bytes at 8-byte alignment (x may be odd): ds_read_b128 cannot take it; it is ONE ds_read2_b64
//    (offsets 0, 1) per row, two per footprint.  The table charges ds_read2_b64 8 cycles per wave (two accesses of 4 x 16 lanes, bank (a / 4) mod 32):
//    16 consecutive 8-byte texels cover the 32 banks once -> conflict-free at one texel per pixel; pitch 64 texels = 512 bytes, a multiple of the
//    128 bytes of its banks.  Two separate ds_read_b64 would be 2 + 2 cycles by the same table ((a / 4) mod 64, 2 x 32 lanes: also conflict-free)
//    but twice the instructions; the compiler merges adjacent 8-byte reads into ds_read2_b64 anyway, and which of the two is faster HERE has not
//    been measured.
//  * More than one texel per pixel (minification; a tilted camera's wide boxes) wraps the lanes of a group around the banks in either layout.
//    Those conflict rates have NOT been measured (no SQ_LDS_BANK_CONFLICT run was made for this kernel).
//  * Stores: ds_write_b128, 8 groups of 8 contiguous lanes, consecutive lanes write consecutive 16-byte items of one box row: conflict-free.
//
// Arithmetic: every tap goes through to_f32 and the sample through bilerp<STRICT>, per channel, exactly as gather_sample does: in strict-order mode
// the kernel is bit-identical to the gather kernel and to the render of the planar copy; in default mode only the coordinate chain differs in form
// (plane_coord_recip: hoisted reciprocals, the same quotients -- div_by_recip).
//
// GMPI_FLAG_CHECK_RANGE tests every staged texel where the loader holds it in registers (bit patterns first, the exact test only when one is
// suspicious: -0.0 is legal); gather_plane tests its own taps.  So a texel that some pixel samples is always tested; a staged texel that no pixel
// samples is tested too (as in the other tile kernels).
//
// Falls back to gather_plane: a (tile, plane) whose box exceeds 64 x 32 texels (the same box for fp32 and 16-bit storage: fp32 keeps the full box,
// 2 x 32 KB), a box with NaN / inf corners, and a single pixel whose footprint lies outside its tile's box (a ray field that is no pinhole camera's).
//
// LDS: 2 x 32 KB + 3 KB of tables = 67 KB for fp32 (2 workgroups = 16 waves per CU), 2 x 16 KB + 3 KB = 35 KB for 16-bit (4 workgroups per CU by LDS; the
// registers allow 3: see the launch bounds below).
#include "gmpi_device.hpp"

namespace gmpi {

constexpr int kLW = 32, kLH = 16, kLThreads = kLW * kLH;   // pixel tile, one pixel per thread
constexpr int kLPitch = 64, kLRows = 32;                   // staging buffer: texels per row, rows
constexpr int kLChunk = 64;                                // planes per table refill

template <typename TexT>
struct LayerStage {
    static constexpr int kTexel = sizeof(TexT);                         // bytes per texel: 16 / 8
    static constexpr int kTPI = 16 / kTexel;                            // texels per 16-byte loader item: 1 / 2
    static constexpr int kCols = kLPitch / kTPI;                        // items per box row: 64 / 32
    static constexpr int kRowsPerPass = kLThreads / kCols;              // box rows the workgroup loads with one item per thread: 8 / 16
    static constexpr int kItems = kLRows / kRowsPerPass;                // items per thread: 4 / 2
    static constexpr int kBufWords = kLRows * kLPitch * kTexel / 4;     // dwords per buffer: 8192 / 4096
    static constexpr int kLdsBytes = 2 * kBufWords * 4 + kLChunk * 48;
    static_assert(kTexel == 16 || kTexel == 8, "whole texels of 16 or 8 bytes");
    static_assert(kItems * kRowsPerPass == kLRows && kCols * kRowsPerPass == kLThreads, "whole passes");
    static_assert(kLdsBytes <= (kTexel == 16 ? 72 : 40) * 1024, "2 (fp32) / 4 (16-bit) workgroups per CU");
};

typedef uint32_t lay_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t lay_u32x2 __attribute__((ext_vector_type(2)));

// channel c of a staged texel -> fp32, as to_f32 of the element
__device__ __forceinline__ float staged_chan(float, const lay_u32x4& t, int c) { return __uint_as_float(t[c]); }
__device__ __forceinline__ float staged_chan(bf16_t, const lay_u32x2& t, int c) { return __uint_as_float((c & 1) ? (t[c >> 1] & 0xffff0000u) : (t[c >> 1] << 16)); }
__device__ __forceinline__ float staged_chan(f16_t, const lay_u32x2& t, int c) {
    const uint16_t h = static_cast<uint16_t>((c & 1) ? (t[c >> 1] >> 16) : (t[c >> 1] & 0xffffu));
    return to_f32(f16_t{__builtin_bit_cast(_Float16, h)});
}
// [0, 1] on one loaded dword: the bit-pattern pre-test (non-negative values order like unsigned integers; a sign bit, NaN and inf compare above one)
// and the exact test behind it
__device__ __forceinline__ bool word_suspicious(float, uint32_t w) { return w > 0x3f800000u; }
__device__ __forceinline__ bool word_suspicious(bf16_t, uint32_t w) { return (w & 0xffffu) > 0x3f80u || (w >> 16) > 0x3f80u; }
__device__ __forceinline__ bool word_suspicious(f16_t, uint32_t w) { return (w & 0xffffu) > 0x3c00u || (w >> 16) > 0x3c00u; }
__device__ __forceinline__ bool word_out_of_unit(float, uint32_t w) { return !in_unit(__uint_as_float(w)); }
__device__ __forceinline__ bool word_out_of_unit(bf16_t, uint32_t w) { return !(in_unit(__uint_as_float(w << 16)) && in_unit(__uint_as_float(w & 0xffff0000u))); }
__device__ __forceinline__ bool word_out_of_unit(f16_t, uint32_t w) {
    const float lo = to_f32(f16_t{__builtin_bit_cast(_Float16, static_cast<uint16_t>(w & 0xffffu))});
    const float hi = to_f32(f16_t{__builtin_bit_cast(_Float16, static_cast<uint16_t>(w >> 16))});
    return !(in_unit(lo) && in_unit(hi));
}

template <typename TexT, bool AC, bool STRICT>
__device__ __forceinline__ void render_layers_tile(const KParams& p, const int tiles_x, const int tiles_y, const int n_tiles) {
    using S = LayerStage<TexT>;
    using E = typename FloatTexel<TexT>::elem;
    using TapT = std::conditional_t<S::kTexel == 16, lay_u32x4, lay_u32x2>;   // one staged texel
    // Per plane of the chunk, written once by one thread (render_u8.hip):
    //   box:  qx0 (a multiple of kTPI), by0, items per row (0: not staged), rows
    //   org:  byte address of the box origin (words 0, 1 of the plane's buffer descriptor), RN(1 / hh)
    //   geo:  zdiff = d - eye_z, hw = w / 2, hh = h / 2, RN(1 / hw)
    __shared__ int4 box[kLChunk];
    __shared__ int4 org[kLChunk];
    __shared__ float4 geo[kLChunk];
    __shared__ __attribute__((aligned(16))) uint32_t stage[2][S::kBufWords];

    const int tid = threadIdx.x;
    FwdTile ft;
    if (!fwd_tile(p, fwd_tile_id(p, blockIdx.x, tiles_x, tiles_y, n_tiles), tiles_x, tiles_y, n_tiles, ft)) return;
    const int n = ft.n;

    uint32_t bad = 0;
    const View vw = view_setup<AC>(p, n, bad);
    check_camera_behind(p, vw, ft.rem == 0 && tid == 0);   // once per view
    const int D = p.D, Ht = p.Ht, Wt = p.Wt, H = p.H, W = p.W;
    const int64_t HW = vw.HW;
    const float* __restrict__ rdv = vw.rays;
    const bool check_range = (p.flags & GMPI_FLAG_CHECK_RANGE) != 0;
    const TexT* __restrict__ vol = tex_offset(static_cast<const TexT*>(p.rgba), static_cast<int64_t>(vw.m) * p.s_mpi);

    const TileLane tl = tile_lane<kLW, kLH>(ft.txi, ft.tyi, tid, W, H);
    const int64_t pix = tl.pix;
    const float rx = rdv[pix], ry = rdv[HW + pix], rz = rdv[2 * HW + pix];
    const float dot = ray_dot(vw, rx, ry, rz);
    const float rcp_rz = 1.0f / rz;   // correctly rounded; hoisted out of the plane loop (div_by_recip)
    Accum A;
    const TileCorners tc = tile_corners<kLW, kLH>(ft.txi, ft.tyi, W, H);

    // ---- loader role: item column lcol of box rows lrow + r kRowsPerPass; byte offset from the box origin (below 2^31: layers_variant_supports) ----
    const int lrow = tid / S::kCols, lcol = tid - lrow * S::kCols;
    const uint32_t l_off = static_cast<uint32_t>(lrow) * static_cast<uint32_t>(p.s_row) + 16u * lcol;
    const uint32_t pass_off = static_cast<uint32_t>(S::kRowsPerPass) * static_cast<uint32_t>(p.s_row);
    const int dst_word = (lrow * kLPitch * S::kTexel + 16 * lcol) / 4;
    constexpr int kPassWords = S::kRowsPerPass * kLPitch * S::kTexel / 4;

    for (int kc = 0; kc < D; kc += kLChunk) {
        const int kn = min(kLChunk, D - kc);
        __syncthreads();   // the previous chunk's table and buffers are no longer read
        for (int t = tid; t < kn; t += kLThreads) {
            const int k = kc + t;
            const float zdiff = vw.dhw[3 * k] - vw.ez, ph = vw.dhw[3 * k + 1], pw = vw.dhw[3 * k + 2];
            bool fits;
            int4 bb = item_box<S::kTPI>(corner_extent<AC>(vw, rdv, W, zdiff, ph, pw, tc.cx0, tc.cx1, tc.cy0, tc.cy1), S::kCols, kLRows, fits);
            if (!fits) bb = make_int4(0, 0, 0, 0);
            box[t] = bb;
            const float hw = pw * 0.5f, hh = ph * 0.5f;   // exact halves: (2x) / w == x / (w / 2)
            const int2 o = origin_words(reinterpret_cast<uint64_t>(vol) +
                                        static_cast<uint64_t>(static_cast<int64_t>(k) * p.s_plane + bb.y * p.s_row + static_cast<int64_t>(S::kTexel) * bb.x));
            org[t] = make_int4(o.x, o.y, __float_as_int(1.0f / hh), 0);
            geo[t] = make_float4(zdiff, hw, hh, 1.0f / hw);
        }
        __syncthreads();   // table published

        // the loads of plane t of the chunk; past the end of the chunk, or for a box that is not staged, every offset is rejected.  Issued
        // unconditionally: with the same memory operations on every path the loads stay in flight across the compositing of the plane before.
        auto issue_loads = [&](int t, lay_u32x4 (&L)[S::kItems]) {
            const int4 bb = box[min(t, kn - 1)];
            const int4 oo = org[min(t, kn - 1)];
            const int qx0 = __builtin_amdgcn_readfirstlane(bb.x), by0 = __builtin_amdgcn_readfirstlane(bb.y);
            const int nq = t < kn ? __builtin_amdgcn_readfirstlane(bb.z) : 0, nrows = __builtin_amdgcn_readfirstlane(bb.w);
            const __amdgpu_buffer_rsrc_t rsrc = origin_rsrc(oo.x, oo.y);
            const int gx = qx0 + S::kTPI * lcol;   // (16-bit: gx and Wt are even -- an item lies inside the texture row or outside it)
            // (bitwise on purpose: `&&` would be lowered to exec-mask control flow)
            const bool col_ok = (lcol < nq) & (gx >= 0) & (gx < Wt);
#pragma unroll
            for (int r = 0; r < S::kItems; ++r) {
                const int row = lrow + r * S::kRowsPerPass, gy = by0 + row;
                const bool ok = col_ok & (row < nrows) & (gy >= 0) & (gy < Ht);
                const uint32_t off = ok ? l_off + static_cast<uint32_t>(r) * pass_off : 0x80000000u;   // == num_records: rejected, reads as zero
                L[r] = __builtin_bit_cast(lay_u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0));
            }
        };
        // registers -> LDS as they are; lanes outside the box stay idle.  The range test looks at what the lane holds (zeros outside the box).
        auto store_box = [&](int t, uint32_t* buf, const lay_u32x4 (&L)[S::kItems]) {
            const int4 bb = box[t];
            const int nq = __builtin_amdgcn_readfirstlane(bb.z), nrows = __builtin_amdgcn_readfirstlane(bb.w);
            bool suspicious = false;
#pragma unroll
            for (int r = 0; r < S::kItems; ++r) {
                if ((lcol < nq) & (lrow + r * S::kRowsPerPass < nrows)) *reinterpret_cast<lay_u32x4*>(buf + dst_word + r * kPassWords) = L[r];
#pragma unroll
                for (int c = 0; c < 4; ++c) suspicious |= word_suspicious(E{}, L[r][c]);
            }
            if (check_range && __builtin_expect(suspicious, 0)) {
#pragma unroll
                for (int r = 0; r < S::kItems; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (word_out_of_unit(E{}, L[r][c])) bad |= GMPI_STATUS_RGBA_RANGE;
            }
        };
        auto composite = [&](int t, const uint32_t* __restrict__ buf) {
            const int k = kc + t;
            const int4 bb = box[t];
            const int qx0 = __builtin_amdgcn_readfirstlane(bb.x), by0 = __builtin_amdgcn_readfirstlane(bb.y);
            const int nq = __builtin_amdgcn_readfirstlane(bb.z), nrows = __builtin_amdgcn_readfirstlane(bb.w);
            const float4 g = geo[t];
            if (nq == 0) {   // uniform: the box does not fit -- everybody takes the direct gather (exact doublings of the table's halves)
                gather_plane<TexT, AC, STRICT>(p, vw, vol, k, g.x, g.z + g.z, g.y + g.y, rx, ry, rz, dot, check_range, bad, A);
                return;
            }
            float ix, iy, s;
            if (STRICT) {
                float u, v;
                plane_coord<AC>(g.x, g.z + g.z, g.y + g.y, vw.ex, vw.ey, rx, ry, rz, vw.cx, vw.cy, ix, iy, s, u, v);
            } else {   // the same quotients through hoisted reciprocals (div_by_recip: correctly rounded, so ix, iy, s are the same bits)
                plane_coord_recip<AC>(g.x, g.y, g.z, g.w, __int_as_float(org[t].z), vw.ex, vw.ey, rx, ry, rz, rcp_rz, vw.cx, vw.cy, ix, iy, s);
            }
            // gather_sample's footprint: weights of taps outside the texture are zero (the box holds zeros there anyway: same products, same bits)
            Footprint f = footprint(ix, iy, Ht, Wt);
            const bool x0in = f.x0 >= 0 && f.x0 <= Wt - 1, x1in = f.x0 >= -1 && f.x0 <= Wt - 2;
            const bool y0in = f.y0 >= 0 && f.y0 <= Ht - 1, y1in = f.y0 >= -1 && f.y0 <= Ht - 2;
            if (!(x0in && y0in)) f.nw = 0.0f;
            if (!(x1in && y0in)) f.ne = 0.0f;
            if (!(x0in && y1in)) f.sw = 0.0f;
            if (!(x1in && y1in)) f.se = 0.0f;
            const int lx = f.x0 - qx0, ly = f.y0 - by0;
            const bool inb = (lx >= 0) & (ly >= 0) & (lx + 1 < S::kTPI * nq) & (ly + 1 < nrows);
            const bool any_w = (f.nw != 0.0f) | (f.ne != 0.0f) | (f.sw != 0.0f) | (f.se != 0.0f);
            if (__builtin_expect((!inb) & any_w, 0)) {   // per lane: a pixel whose taps the box does not hold (no pinhole ray field)
                gather_plane<TexT, AC, STRICT>(p, vw, vol, k, g.x, g.z + g.z, g.y + g.y, rx, ry, rz, dot, check_range, bad, A);
                return;
            }
            // a footprint outside the box with every weight zero (the sentinel corner of NaN / far-off coordinates) reads texel (0, 0) of the box
            const uint32_t idx = inb ? static_cast<uint32_t>(ly * kLPitch + lx) : 0u;
            const TapT* __restrict__ tx = reinterpret_cast<const TapT*>(buf);
            const TapT t_nw = tx[idx], t_ne = tx[idx + 1], t_sw = tx[idx + kLPitch], t_se = tx[idx + kLPitch + 1];
            float smp[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                smp[c] = bilerp<STRICT>(staged_chan(E{}, t_nw, c), staged_chan(E{}, t_ne, c), staged_chan(E{}, t_sw, c), staged_chan(E{}, t_se, c), f);
            blend<STRICT>(A, smp[0], smp[1], smp[2], smp[3], s, dot);
        };

        lay_u32x4 L[S::kItems];
        issue_loads(0, L);
        for (int t = 0; t < kn; ++t) {
            uint32_t* buf = stage[t & 1];
            store_box(t, buf, L);
            __syncthreads();          // box t visible; everybody is done reading box t - 1 (the other buffer)
            issue_loads(t + 1, L);    // in flight while plane t is composited
            composite(t, buf);
        }
    }
    const LastPlane lp = last_plane(p, vw);
    if (leaves_last_plane<AC>(vw, lp, rx, ry, rz)) bad |= GMPI_STATUS_OUT_OF_LAST_PLANE;
    store_pixel<STRICT>(p, n, HW, pix, A, dot, tl.active);
    report_status(p.status, bad);
}

// Waves per SIMD asked for.  fp32: what the LDS allows, 2 workgroups of 8 waves per CU = 4 (82-100 VGPRs).  16-bit: the LDS would allow 4 workgroups = 8
// waves per SIMD, but at 64 VGPRs every instance spills (12-56 bytes of scratch: two 16-byte items in flight next to the 8 tap dwords); at 7 the default
// instances take 67-72 VGPRs without scratch, the strict-order ones (16 conversions alive at once) need 6 (73-75): 3 workgroups per CU either way.
template <typename TexT, bool AC, bool STRICT>
__global__ __launch_bounds__(kLThreads, sizeof(TexT) == 16 ? 4 : STRICT ? 6 : 7) void render_layers_kernel(const KParams p, const int tiles_x, const int tiles_y, const int n_tiles) {
    render_layers_tile<TexT, AC, STRICT>(p, tiles_x, tiles_y, n_tiles);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
// Whether the staged kernel can take these layers (p's strides in bytes): every 16-byte item is a naturally aligned run of dwords -- fp32: any Wt,
// element alignment is dword alignment; 16-bit: two texels per item, so Wt even (an item of a box that touches the border does not straddle it) and
// the base pointer and the row / plane / MPI strides multiples of 4 bytes -- and the in-box byte offsets stay below 2^31.
bool layers_variant_supports(const KParams& p, int dtype) {
    if (reinterpret_cast<uintptr_t>(p.rgba) % 4 != 0 || p.s_row % 4 != 0 || p.s_plane % 4 != 0 || p.s_mpi % 4 != 0) return false;
    if (dtype != GMPI_DTYPE_F32 && p.Wt % 2 != 0) return false;
    return (kLRows + 1) * p.s_row + 16 * kLPitch + 128 < (int64_t(1) << 31);
}

template <typename TexT>
static hipError_t launch_layers_t(const KParams& p, hipStream_t stream) {
    const FwdTileGrid tg = fwd_tile_grid<kLW, kLH>(p);
    dispatch_ac_strict(p.flags, [&](auto AC, auto STRICT) {
        hipLaunchKernelGGL((render_layers_kernel<TexT, decltype(AC)::value, decltype(STRICT)::value>), tg.grid, dim3(kLThreads), 0, stream, p, tg.tiles_x, tg.tiles_y,
                           tg.n_tiles);
    });
    return hipGetLastError();
}
hipError_t launch_layers(const KParams& p, int dtype, hipStream_t stream) {
    switch (dtype) {
        case GMPI_DTYPE_F32: return launch_layers_t<rgba32f_t>(p, stream);
        case GMPI_DTYPE_F16: return launch_layers_t<rgba16h_t>(p, stream);
        case GMPI_DTYPE_BF16: return launch_layers_t<rgba16b_t>(p, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace gmpi
