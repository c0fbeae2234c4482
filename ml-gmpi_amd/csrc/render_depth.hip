// render_depth.hip -- the depth-alpha layout (gmpi_mpi_render_depth_launch / _backward_launch, include/gmpi_render.h): ONE colour image and ONE depth
// image per MPI and, optionally, a separate colour image for the last plane -- what GMPI's "depth2alpha" generator produces
// (networks_vanilla_depth2alpha.py:650-663).  The alpha of a texel on plane k is a ramp of plane_z[k] - depth (depth_ramp, gmpi_shared.hpp); by
// definition the result is the render of the volume expand_depth_alpha (depth_alpha.py) builds.  Per tap the ramp is formed exactly as there, the four
// ramp values are interpolated like the taps of a stored alpha plane, and everything around that is the shared-colour kernels' arithmetic (plane_coord,
// make_taps, bilerp, blend; BwdPixel::plane, XT): the strict-order forward is bit-identical to render_gather.hip on the expanded volume.
//
//   render_depth_kernel           forward, one pixel per lane, any shape / stride / dtype / ray field, every flag
//   render_depth_backward_kernel  backward, one pixel per lane; the gradient of all D alpha planes lands in one depth image
//
// A PLANE WHOSE ALPHA SAMPLE IS EXACTLY 0 IS SKIPPED by the forward (its 12 colour taps and its blend): in front of the surface every ramp tap is
// clamped to 0, and blend() with a = 0 is the identity in fp32 -- w = 0 adds nothing to colour and depth (finite colours, finite 1/(1/(s dot))), om = (1 - 0) + 1e-10
// rounds to 1.  GMPI_FLAG_CHECK_RANGE therefore covers the colour texels of the planes that are blended, and every computed alpha tap.
//
// KParams carries the depth image in its volume fields: rgba = depth [M,1,1,Ht,Wt], s_mpi / s_row its strides (s_plane, s_chan unused).
#include "gmpi_backward.hpp"
#include "gmpi_shared.hpp"

namespace gmpi {

// ---- forward -------------------------------------------------------------------------------------------------------------------------------------
template <typename TexT, bool AC, bool STRICT>
__global__ __launch_bounds__(256) void render_depth_kernel(const KParams p, const SharedK sh, const DepthK dk) {
    const int n = blockIdx.z;
    const int px = blockIdx.x * 64 + threadIdx.x;
    const int py = blockIdx.y * 4 + threadIdx.y;
    uint32_t bad = 0;
    const View vw = view_setup<AC>(p, n, bad);
    const int m = vw.m;
    check_camera_behind(p, vw, blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0);  // one lane per view, as the gather kernel
    const bool active = px < p.W && py < p.H;
    const int64_t HW = vw.HW;
    const int64_t pix = static_cast<int64_t>(min(py, p.H - 1)) * p.W + min(px, p.W - 1);
    const float rx = vw.rays[pix], ry = vw.rays[HW + pix], rz = vw.rays[2 * HW + pix];
    const float dot = ray_dot(vw, rx, ry, rz);
    const int Ht = p.Ht, Wt = p.Wt;
    const bool check_range = (p.flags & GMPI_FLAG_CHECK_RANGE) != 0;
    const bool check_last = (p.flags & GMPI_FLAG_CHECK_LAST_PLANE) != 0;
    const TexT* __restrict__ depth = static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(m) * p.s_mpi;
    const TexT* __restrict__ rgb = static_cast<const TexT*>(sh.rgb) + static_cast<int64_t>(m) * sh.rs_mpi;
    const TexT* __restrict__ bgi = sh.bg ? static_cast<const TexT*>(sh.bg) + static_cast<int64_t>(m) * sh.bs_mpi : nullptr;
    const float* __restrict__ pz = dk.plane_z + static_cast<int64_t>(m) * dk.pz_stride;

    Accum A;
    for (int k = 0; k < p.D; ++k) {
        float ix, iy, s, u, v;
        plane_coord<AC>(vw.dhw[3 * k] - vw.ez, vw.dhw[3 * k + 1], vw.dhw[3 * k + 2], vw.ex, vw.ey, rx, ry, rz, vw.cx, vw.cy, ix, iy, s, u, v);
        if (check_last && k == p.D - 1 && outside_pm1(u, v)) bad |= GMPI_STATUS_OUT_OF_LAST_PLANE;
        const Taps t = make_taps(ix, iy, Ht, Wt);
        const RampTaps r = ramp_taps<TexT, STRICT>(depth, p.s_row, t, pz[k], dk);
        if (check_range && !(in_unit(r.a[0]) && in_unit(r.a[1]) && in_unit(r.a[2]) && in_unit(r.a[3]))) bad |= GMPI_STATUS_RGBA_RANGE;   // (a NaN depth)
        const float a = bilerp<STRICT>(r.a[0], r.a[1], r.a[2], r.a[3], t.f);
        if (a != 0.0f) {   // (true for NaN)
            const bool last_bg = bgi != nullptr && k == p.D - 1;   // uniform
            const TexT* __restrict__ col = last_bg ? bgi : rgb;
            const int64_t c_chan = last_bg ? sh.bs_chan : sh.rs_chan, c_row = last_bg ? sh.bs_row : sh.rs_row;
            float smp[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) smp[c] = tap_sample<TexT, STRICT>(col + c * c_chan, c_row, t, check_range, bad);
            blend<STRICT>(A, smp[0], smp[1], smp[2], a, s, dot);
        }
    }
    store_pixel<STRICT>(p, n, HW, pix, A, dot, active);
    report_status(p.status, bad);
}

// ---- backward ------------------------------------------------------------------------------------------------------------------------------------
// (add_taps -- d times each of four tap weights, THE WEIGHT GATES THE ADDRESS -- and depth_total_transmittance live in gmpi_shared.hpp: the tile
// backward, render_depth_tile.hip, runs the same two texts.)
// The sweep starts from the pixel's final transmittance.  Behind the surface every plane is (almost) exactly opaque, om = 1e-10 per plane: the
// forward's T_out underflows for most pixels of this layout, so the front-to-back re-walk in the extended representation (XT) is the
// common path here.  It walks the ramp samples (total_transmittance reads alpha planes, which do not exist).
// A plane whose alpha sample is exactly 0 and none of whose taps lies on the ramp is the identity of the sweep (om = 1, w = 0, no gradient reaches
// the depth image): it is skipped, colour taps included.  With step-like ramps that is most planes in front of the surface; behind it the taps are
// clamped to 1 and only the colour receives a gradient.
template <typename TexT, bool AC>
__global__ __launch_bounds__(256) void render_depth_backward_kernel(const KParams p, const SharedK sh, const DepthK dk, const SharedG g) {
    const int n = blockIdx.z;
    const int px = blockIdx.x * 64 + threadIdx.x;
    const int py = blockIdx.y * 4 + threadIdx.y;
    if (px >= p.W || py >= p.H) return;
    uint32_t unused = 0;
    const BwdView vw = bwd_view<AC>(p, n);
    const int m = vw.m;
    const int Ht = p.Ht, Wt = p.Wt, D = p.D;
    const TexT* __restrict__ depth = static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(m) * p.s_mpi;
    const TexT* __restrict__ rgb = static_cast<const TexT*>(sh.rgb) + static_cast<int64_t>(m) * sh.rs_mpi;
    const TexT* __restrict__ bgi = sh.bg ? static_cast<const TexT*>(sh.bg) + static_cast<int64_t>(m) * sh.bs_mpi : nullptr;
    const float* __restrict__ pz = dk.plane_z + static_cast<int64_t>(m) * dk.pz_stride;
    float* __restrict__ g_rgb = g.g_rgb ? g.g_rgb + static_cast<int64_t>(m) * g.gr_mpi : nullptr;
    float* __restrict__ g_bg = (g.g_bg && bgi) ? g.g_bg + static_cast<int64_t>(m) * g.gb_mpi : nullptr;
    float* __restrict__ g_dep = g.g_alpha ? g.g_alpha + static_cast<int64_t>(m) * g.ga_mpi : nullptr;

    BwdPixel bp;
    bwd_pixel_setup_with<false>(bp, p, vw, n, px, py, true, g.g_out, g.g_depth, g.g_T,
                                [&](float t_fwd) { return depth_total_transmittance<TexT, AC>(p, vw, bp, depth, pz, dk, t_fwd); });
    for (int k = D - 1; k >= 0; --k) {
        float ix, iy, s;
        pixel_plane_coord<AC>(vw, bp, k, ix, iy, s);
        const Taps t = make_taps(ix, iy, Ht, Wt);
        const Footprint& f = t.f;
        const RampTaps r = ramp_taps<TexT, false>(depth, p.s_row, t, pz[k], dk);
        float smp[4], d_s[4];
        smp[3] = bilerp<false>(r.a[0], r.a[1], r.a[2], r.a[3], f);
        // weights of the taps the depth gradient reaches: inside the texture (make_taps zeroed the others) and on the ramp
        const float w_nw = r.in[0] ? f.nw : 0.0f, w_ne = r.in[1] ? f.ne : 0.0f, w_sw = r.in[2] ? f.sw : 0.0f, w_se = r.in[3] ? f.se : 0.0f;
        const bool on_ramp = g_dep != nullptr && (w_nw != 0.0f || w_ne != 0.0f || w_sw != 0.0f || w_se != 0.0f);
        if (smp[3] == 0.0f && !on_ramp) continue;
        const bool last_bg = bgi != nullptr && k == D - 1;
        const TexT* __restrict__ col = last_bg ? bgi : rgb;
        const int64_t c_chan = last_bg ? sh.bs_chan : sh.rs_chan, c_row = last_bg ? sh.bs_row : sh.rs_row;
#pragma unroll
        for (int c = 0; c < 3; ++c) smp[c] = tap_sample<TexT, false>(col + c * c_chan, c_row, t, false, unused);
        const float w = bp.plane(smp, s, d_s);
        float* __restrict__ gc = last_bg ? g_bg : g_rgb;
        if (gc != nullptr && w != 0.0f) {
            const int64_t gc_chan = last_bg ? g.gb_chan : g.gr_chan, gc_row = last_bg ? g.gb_row : g.gr_row;
#pragma unroll
            for (int c = 0; c < 3; ++c) add_taps(gc + c * gc_chan, gc_row, f, d_s[c], f.nw, f.ne, f.sw, f.se);
        }
        if (on_ramp) {   // d alpha / d depth = -1 / den on the ramp
            const float gq = -div_by_recip(d_s[3], dk.den, dk.rden);
            add_taps(g_dep, g.ga_row, f, gq, w_nw, w_ne, w_sw, w_se);
        }
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------
template <typename TexT>
static hipError_t launch_depth_t(const KParams& p, const SharedK& sh, const DepthK& dk, hipStream_t stream) {
    const dim3 block(64, 4);
    const dim3 grid((p.W + 63) / 64, (p.H + 3) / 4, p.N);
    dispatch_ac_strict(p.flags, [&](auto AC, auto STRICT) {
        hipLaunchKernelGGL((render_depth_kernel<TexT, decltype(AC)::value, decltype(STRICT)::value>), grid, block, 0, stream, p, sh, dk);
    });
    return hipGetLastError();
}

hipError_t launch_depth(const KParams& p, int dtype, const SharedK& sh, const DepthK& dk, hipStream_t stream) {
    return dispatch_dtype(dtype, [&](auto t) { return launch_depth_t<typename decltype(t)::type>(p, sh, dk, stream); });
}

template <typename TexT>
static hipError_t launch_depth_backward_t(const KParams& p, const SharedK& sh, const DepthK& dk, const SharedG& g, hipStream_t stream) {
    const dim3 block(64, 4);
    const dim3 grid((p.W + 63) / 64, (p.H + 3) / 4, p.N);
    dispatch_bool(p.flags & GMPI_FLAG_ALIGN_CORNERS, [&](auto AC) {
        hipLaunchKernelGGL((render_depth_backward_kernel<TexT, decltype(AC)::value>), grid, block, 0, stream, p, sh, dk, g);
    });
    return hipGetLastError();
}

hipError_t launch_depth_backward(const KParams& p, int dtype, const SharedK& sh, const DepthK& dk, const SharedG& g, hipStream_t stream) {
    return dispatch_dtype(dtype, [&](auto t) { return launch_depth_backward_t<typename decltype(t)::type>(p, sh, dk, g, stream); });
}

}  // namespace gmpi
