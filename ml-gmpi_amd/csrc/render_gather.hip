// render_gather.hip -- GMPI_VARIANT_GATHER: one output pixel per lane, taps straight from global memory.
//
// This is the shape-agnostic kernel (any Ht/Wt/H/W, any rgba strides, any storage dtype): a
// wavefront covers 64 consecutive pixels of one image row, walks the D planes front to back
// (mpi.py:413 "the 1st plane is the closest one") and keeps colour/depth/transmittance in
// registers; nothing of the reference's [N*D, ...] temporaries (mpi.py:362-417) is materialised.
// Because the warp is near-identity (0.85-1.0 texel per pixel), the 64 lanes of a tap load touch
// 2-3 consecutive 128-byte lines -> coalesced through the vector L1; the 4x tap reuse is served by
// L1/L2, HBM sees each texel once per view.
#include "gmpi_device.hpp"

namespace gmpi {

constexpr int kGatherTileW = 64;  // one wavefront = 64 consecutive pixels of a row
constexpr int kGatherTileH = 4;   // 4 wavefronts per workgroup

// The kernel body.  Carry = CarryK: the instance of a plane-chunked render (gmpi_mpi_render_chunk_launch) -- the Accum comes from state_in and goes to
// state_out, the finished images are optional; everything between is the same text, so a pixel's bits do not depend on where the stack was cut.
template <typename TexT, bool AC, bool STRICT, typename Carry>
__device__ __forceinline__ void render_gather_pixel(const KParams& p, const Carry& carry) {
    const int n = blockIdx.z;
    const int px = blockIdx.x * kGatherTileW + threadIdx.x;
    const int py = blockIdx.y * kGatherTileH + threadIdx.y;
    uint32_t bad = 0;
    const View vw = view_setup<AC>(p, n, bad);
    check_camera_behind(p, vw, blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0);  // one lane per view
    // edge tiles: out-of-image lanes shadow the last pixel (keeps the wave converged for the status reduce)
    const bool active = px < p.W && py < p.H;
    const int64_t HW = vw.HW;
    const int64_t pix = static_cast<int64_t>(min(py, p.H - 1)) * p.W + min(px, p.W - 1);
    const float rx = vw.rays[pix], ry = vw.rays[HW + pix], rz = vw.rays[2 * HW + pix];
    const float dot = ray_dot(vw, rx, ry, rz);
    const bool check_range = (p.flags & GMPI_FLAG_CHECK_RANGE) != 0;
    const TexT* __restrict__ vol = tex_offset(static_cast<const TexT*>(p.rgba), static_cast<int64_t>(vw.m) * p.s_mpi);

    Accum A = load_carry(carry, n, HW, pix);
#pragma unroll 2
    for (int k = 0; k < p.D; ++k) {  // gather_plane's body, written out: through the helper one instance (fp16, align_corners, strict) takes 2 VGPRs more
        const float d = vw.dhw[3 * k + 0], ph = vw.dhw[3 * k + 1], pw = vw.dhw[3 * k + 2];
        float ix, iy, s, u, v;
        plane_coord<AC>(d - vw.ez, ph, pw, vw.ex, vw.ey, rx, ry, rz, vw.cx, vw.cy, ix, iy, s, u, v);
        float smp[4];
        gather_sample<TexT, STRICT>(tex_offset(vol, static_cast<int64_t>(k) * p.s_plane), p.s_chan, p.s_row, p.Ht, p.Wt, ix, iy, check_range, bad, smp);
        blend<STRICT>(A, smp[0], smp[1], smp[2], smp[3], s, dot);
    }
    const LastPlane lp = last_plane(p, vw);
    if (leaves_last_plane<AC>(vw, lp, rx, ry, rz)) bad |= GMPI_STATUS_OUT_OF_LAST_PLANE;
    store_pixel<STRICT>(p, n, HW, pix, A, dot, active, carry);
    report_status(p.status, bad);
}

template <typename TexT, bool AC, bool STRICT>
__global__ __launch_bounds__(kGatherTileW* kGatherTileH) void render_gather_kernel(const KParams p) {
    render_gather_pixel<TexT, AC, STRICT>(p, NoCarry{});
}
template <typename TexT, bool AC, bool STRICT>
__global__ __launch_bounds__(kGatherTileW* kGatherTileH) void render_gather_chunk_kernel(const KParams p, const CarryK carry) {
    render_gather_pixel<TexT, AC, STRICT>(p, carry);
}

template <typename TexT>
static hipError_t launch_gather_t(const KParams& p, const CarryK* carry, hipStream_t stream) {
    const dim3 block(kGatherTileW, kGatherTileH);
    const dim3 grid((p.W + kGatherTileW - 1) / kGatherTileW, (p.H + kGatherTileH - 1) / kGatherTileH, p.N);
    dispatch_ac_strict(p.flags, [&](auto AC, auto STRICT) {
        if (carry != nullptr) hipLaunchKernelGGL((render_gather_chunk_kernel<TexT, decltype(AC)::value, decltype(STRICT)::value>), grid, block, 0, stream, p, *carry);
        else hipLaunchKernelGGL((render_gather_kernel<TexT, decltype(AC)::value, decltype(STRICT)::value>), grid, block, 0, stream, p);
    });
    return hipGetLastError();
}

// carry: nullptr = the one-shot kernels, else their carry instances
static hipError_t launch_gather_any(const KParams& p, const CarryK* carry, int dtype, hipStream_t stream) {
    if (dtype == GMPI_DTYPE_U8 && u8_interleaved(p)) return launch_gather_t<rgba8_t>(p, carry, stream);  // (channels-last codes: one texel load per tap)
    if (dtype == GMPI_DTYPE_U8) return launch_gather_t<u8_t>(p, carry, stream);  // (8-bit codes: to_f32 is the division by 255; only the forward takes them)
    return dispatch_dtype(dtype, [&](auto t) { return launch_gather_t<typename decltype(t)::type>(p, carry, stream); });
}
hipError_t launch_gather(const KParams& p, int dtype, hipStream_t stream) { return launch_gather_any(p, nullptr, dtype, stream); }
hipError_t launch_gather_chunk(const KParams& p, const CarryK& carry, int dtype, hipStream_t stream) { return launch_gather_any(p, &carry, dtype, stream); }

// Channels-last float layers (gmpi_mpi_render_layers_launch): the instances over the texel types of gmpi_device.hpp -- one load per tap, the planar
// instance's arithmetic behind it, hence its bits in both modes.  p's strides count bytes.  One-shot only: the layout has no chunked form.
template <typename TexT>
static hipError_t launch_gather_layers_t(const KParams& p, hipStream_t stream) {
    const dim3 block(kGatherTileW, kGatherTileH);
    const dim3 grid((p.W + kGatherTileW - 1) / kGatherTileW, (p.H + kGatherTileH - 1) / kGatherTileH, p.N);
    dispatch_ac_strict(p.flags, [&](auto AC, auto STRICT) {
        hipLaunchKernelGGL((render_gather_kernel<TexT, decltype(AC)::value, decltype(STRICT)::value>), grid, block, 0, stream, p);
    });
    return hipGetLastError();
}
hipError_t launch_gather_layers(const KParams& p, int dtype, hipStream_t stream) {
    switch (dtype) {
        case GMPI_DTYPE_F32: return launch_gather_layers_t<rgba32f_t>(p, stream);
        case GMPI_DTYPE_F16: return launch_gather_layers_t<rgba16h_t>(p, stream);
        case GMPI_DTYPE_BF16: return launch_gather_layers_t<rgba16b_t>(p, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace gmpi
