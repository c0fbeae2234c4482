// gmpi_shared.hpp -- kernel-side view of the shared-colour layout (GmpiSharedColor, include/gmpi_render.h): what gmpi_abi.hip hands render_shared.hip.
#pragma once
#include <stdint.h>

#include "gmpi_backward.hpp"
#include "gmpi_device.hpp"

namespace gmpi {

struct SharedK {
    const void* rgb;   // [M,3,Ht,Wt]
    const void* bg;    // [M,3,Ht,Wt] or nullptr: colour of plane D-1
    int64_t rs_mpi, rs_chan, rs_row, bs_mpi, bs_chan, bs_row;
};
struct SharedG {
    const float* g_out;    // [N,3,H,W]
    const float* g_depth;  // [N,1,H,W] or nullptr
    const float* g_T;      // [N,1,H,W] or nullptr
    float* g_rgb;          // [M,3,Ht,Wt] or nullptr, added into
    float* g_alpha;        // [M,D,1,Ht,Wt] or nullptr (depth-alpha layout: the gradient of the depth image [M,1,Ht,Wt]; ga_plane unused)
    float* g_bg;           // [M,3,Ht,Wt] or nullptr
    int64_t gr_mpi, gr_chan, gr_row, ga_mpi, ga_plane, ga_row, gb_mpi, gb_chan, gb_row;
};

// ---- device side: the direct sample of one plane, shared by render_shared.hip and render_shared_forward.hip ---------------------------------------
// The four taps of one footprint: clamped addresses, weights of taps outside the texture zeroed (gather_sample's rule).
struct Taps {
    Footprint f;
    int xa, xb, ya, yb;
    bool x0in, x1in, y0in, y1in;
};
__device__ __forceinline__ Taps make_taps(float ix, float iy, int Ht, int Wt) {
    Taps t;
    t.f = footprint(ix, iy, Ht, Wt);
    t.x0in = t.f.x0 >= 0 && t.f.x0 <= Wt - 1, t.x1in = t.f.x0 >= -1 && t.f.x0 <= Wt - 2;
    t.y0in = t.f.y0 >= 0 && t.f.y0 <= Ht - 1, t.y1in = t.f.y0 >= -1 && t.f.y0 <= Ht - 2;
    if (!(t.x0in && t.y0in)) t.f.nw = 0.0f;
    if (!(t.x1in && t.y0in)) t.f.ne = 0.0f;
    if (!(t.x0in && t.y1in)) t.f.sw = 0.0f;
    if (!(t.x1in && t.y1in)) t.f.se = 0.0f;
    t.xa = min(max(t.f.x0, 0), Wt - 1), t.xb = min(max(t.f.x0 + 1, 0), Wt - 1);
    t.ya = min(max(t.f.y0, 0), Ht - 1), t.yb = min(max(t.f.y0 + 1, 0), Ht - 1);
    return t;
}
template <typename TexT, bool STRICT>
__device__ __forceinline__ float tap_sample(const TexT* __restrict__ ch, int64_t s_row, const Taps& t, bool check_range, uint32_t& bad) {
    const int64_t oa = static_cast<int64_t>(t.ya) * s_row, ob = static_cast<int64_t>(t.yb) * s_row;
    const float t_nw = to_f32(ch[oa + t.xa]);
    const float t_ne = to_f32(ch[oa + t.xb]);
    const float t_sw = to_f32(ch[ob + t.xa]);
    const float t_se = to_f32(ch[ob + t.xb]);
    if (check_range && !(in_unit(t_nw) && in_unit(t_ne) && in_unit(t_sw) && in_unit(t_se))) bad |= GMPI_STATUS_RGBA_RANGE;
    return bilerp<STRICT>(t_nw, t_ne, t_sw, t_se, t.f);
}
// (r, g, b, alpha) of plane k for one pixel: colour from the shared image (the background on the last plane), alpha from its plane
template <typename TexT, bool STRICT>
__device__ __forceinline__ void shared_sample(const TexT* __restrict__ alpha_plane, int64_t a_row, const TexT* __restrict__ col, int64_t c_chan,
                                              int64_t c_row, const Taps& t, bool check_range, uint32_t& bad, float (&smp)[4]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) smp[c] = tap_sample<TexT, STRICT>(col + c * c_chan, c_row, t, check_range, bad);
    smp[3] = tap_sample<TexT, STRICT>(alpha_plane, a_row, t, check_range, bad);
}

// ---- loader items of the staged forwards (render_shared_forward.hip, render_depth_window.hip) ----------------------------------------------------
typedef uint32_t f_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t f_u32x2 __attribute__((ext_vector_type(2)));

// one loader item: 4 texels of storage -> fp32
template <typename TexT> struct Item4;
template <> struct Item4<float> {
    using Raw = f_u32x4;
    static __device__ __forceinline__ Raw load(__amdgpu_buffer_rsrc_t rsrc, uint32_t off) {
        return __builtin_bit_cast(Raw, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0));
    }
    static __device__ __forceinline__ float4 cvt(const Raw& v) {
        return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    }
};
template <> struct Item4<bf16_t> {
    using Raw = f_u32x2;
    static __device__ __forceinline__ Raw load(__amdgpu_buffer_rsrc_t rsrc, uint32_t off) {
        return __builtin_bit_cast(Raw, __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, 0));
    }
    static __device__ __forceinline__ float4 cvt(const Raw& v) {
        return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
    }
};
template <> struct Item4<f16_t> {
    using Raw = f_u32x2;
    static __device__ __forceinline__ Raw load(__amdgpu_buffer_rsrc_t rsrc, uint32_t off) {
        return __builtin_bit_cast(Raw, __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, 0));
    }
    static __device__ __forceinline__ float4 cvt(const Raw& v) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const uint32_t vx = v.x, vy = v.y;
        const h2 a = __builtin_bit_cast(h2, vx), b = __builtin_bit_cast(h2, vy);
        return make_float4(static_cast<float>(a.x), static_cast<float>(a.y), static_cast<float>(b.x), static_cast<float>(b.y));
    }
};

// [0, 1] test on fp32 bit patterns: non-negative floats order like unsigned ints; negative values, NaN and inf compare above 1.0; -0.0 is legal
__device__ __forceinline__ bool f_out_of_unit(float v) {
    const uint32_t b = __float_as_uint(v);
    return !(b <= 0x3f800000u || b == 0x80000000u);
}

// ---- depth-alpha layout (GmpiDepthAlpha, include/gmpi_render.h; render_depth.hip): no alpha planes, ONE depth image per MPI; the alpha of texel x on
// plane k is the ramp  (clamp(plane_z[k] - depth[x], lo, hi) - lo) / den,  one rounding per step (expand_depth_alpha, depth_alpha.py).
struct DepthK {
    const float* plane_z;   // [D], or [M, D] with pz_stride = its MPI stride (0: one table for all)
    int64_t pz_stride;
    float lo, hi, den;      // the ramp's three constants as the caller rounded them
    float rden;             // RN(1 / den), for div_by_recip
};
// The four taps of one footprint as ramp values; in[i]: tap i's difference lies inside [lo, hi], bounds included (where torch.clamp passes a gradient).
struct RampTaps {
    float a[4];   // nw, ne, sw, se
    bool in[4];
};
// STRICT: the IEEE division.  Otherwise the same quotient through the rounded reciprocal (div_by_recip is correctly rounded for these operands:
// the numerator is 0 or a multiple of ulp(lo), far from the denormals).  NaN stays NaN, as in torch.clamp.
template <bool STRICT>
__device__ __forceinline__ float depth_ramp(float pz, float d, const DepthK& dk, bool& inside) {
    float t = pz - d;
    inside = t >= dk.lo && t <= dk.hi;
    t = t < dk.lo ? dk.lo : t;
    t = t > dk.hi ? dk.hi : t;
    const float num = t - dk.lo;
    return STRICT ? num / dk.den : div_by_recip(num, dk.den, dk.rden);
}
template <typename TexT, bool STRICT>
__device__ __forceinline__ RampTaps ramp_taps(const TexT* __restrict__ depth, int64_t s_row, const Taps& t, float pz, const DepthK& dk) {
    const int64_t oa = static_cast<int64_t>(t.ya) * s_row, ob = static_cast<int64_t>(t.yb) * s_row;
    const float d_nw = to_f32(depth[oa + t.xa]), d_ne = to_f32(depth[oa + t.xb]);
    const float d_sw = to_f32(depth[ob + t.xa]), d_se = to_f32(depth[ob + t.xb]);
    RampTaps r;
    r.a[0] = depth_ramp<STRICT>(pz, d_nw, dk, r.in[0]), r.a[1] = depth_ramp<STRICT>(pz, d_ne, dk, r.in[1]);
    r.a[2] = depth_ramp<STRICT>(pz, d_sw, dk, r.in[2]), r.a[3] = depth_ramp<STRICT>(pz, d_se, dk, r.in[3]);
    return r;
}

// d times each of four tap weights added to the texels of a footprint.  THE WEIGHT GATES THE ADDRESS, as in render_shared.hip's scatter4: make_taps
// zeroes the weight of a tap outside the texture and leaves x0 / y0 unclamped (-2 .. Wt, -2 .. Ht), so only a tap whose weight is not zero may be
// written -- whatever d is (a NaN or infinite gradient times a zero weight is NaN, never a reason to write).  A term that is exactly zero costs no
// atomic either.
__device__ __forceinline__ void add_taps(float* __restrict__ ch, int64_t s_row, const Footprint& f, float d, float w_nw, float w_ne, float w_sw, float w_se) {
    const int64_t oa = static_cast<int64_t>(f.y0) * s_row + f.x0, ob = oa + s_row;
    const float v_nw = d * w_nw, v_ne = d * w_ne, v_sw = d * w_sw, v_se = d * w_se;
    if (w_nw != 0.0f && v_nw != 0.0f) atomicAdd(ch + oa, v_nw);
    if (w_ne != 0.0f && v_ne != 0.0f) atomicAdd(ch + oa + 1, v_ne);
    if (w_sw != 0.0f && v_sw != 0.0f) atomicAdd(ch + ob, v_sw);
    if (w_se != 0.0f && v_se != 0.0f) atomicAdd(ch + ob + 1, v_se);
}

// ---- the tap prefetch of the tile backwards (render_shared_tile_kernel, render_depth_tile_kernel) ------------------------------------------------
// Plane k for one pixel, first half: coordinates and the 16 tap loads, issued together one plane ahead of their use (the scatter of the plane before
// runs while they are in flight).  v: per channel the taps nw, ne, sw, se -- r, g, b from the colour image (the background on the last plane) and a
// fourth channel from fourth + k fourth_plane with row stride fourth_row (alpha plane k; the one depth image with a plane stride of 0).  An inactive
// lane gets the neutral footprint {-2, -2, no weight}: inside no box, nothing to add.
struct Tap { float s; Footprint f; float v[16]; };
template <bool AC, typename TexT>
__device__ __forceinline__ void fetch_taps(Tap& tp, bool active, const KParams& p, const BwdView& vw, const BwdPixel& bp, int k, const SharedK& sh,
                                           const TexT* __restrict__ rgb, const TexT* __restrict__ bgi, const TexT* __restrict__ fourth, int64_t fourth_plane,
                                           int64_t fourth_row) {
    tp.s = 0.0f;
    tp.f = Footprint{-2, -2, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 16; ++i) tp.v[i] = 0.0f;
    if (active) {
        float ix, iy;
        pixel_plane_coord<AC>(vw, bp, k, ix, iy, tp.s);
        const Taps t = make_taps(ix, iy, p.Ht, p.Wt);
        tp.f = t.f;
        const bool last_bg = bgi != nullptr && k == p.D - 1;
        const TexT* __restrict__ col = last_bg ? bgi : rgb;
        const int64_t c_chan = last_bg ? sh.bs_chan : sh.rs_chan, c_row = last_bg ? sh.bs_row : sh.rs_row;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const TexT* __restrict__ ch = c < 3 ? col + c * c_chan : fourth + static_cast<int64_t>(k) * fourth_plane;
            const int64_t s_row = c < 3 ? c_row : fourth_row;
            const int64_t oa = static_cast<int64_t>(t.ya) * s_row, ob = static_cast<int64_t>(t.yb) * s_row;
            tp.v[4 * c + 0] = to_f32(ch[oa + t.xa]), tp.v[4 * c + 1] = to_f32(ch[oa + t.xb]);
            tp.v[4 * c + 2] = to_f32(ch[ob + t.xa]), tp.v[4 * c + 3] = to_f32(ch[ob + t.xb]);
        }
    }
}

// The final transmittance the depth-alpha backward sweeps start from (bwd_pixel_setup_with's `total`; both backward kernels of the layout call this
// one text): the forward's value when it is usable (total_transmittance's rule), else a front-to-back walk over the RAMP samples in the extended
// representation -- total_transmittance reads alpha planes, which do not exist here.  bp: the pixel's ray (set before `total` is called).
// STRICT: the ramp and its bilinear sample as the strict-order forward rounds them (the geometry pass, whose strict-order sweep divides by those).
template <typename TexT, bool AC, bool STRICT = false>
__device__ __forceinline__ XT depth_total_transmittance(const KParams& p, const BwdView& vw, const BwdPixel& bp, const TexT* __restrict__ depth,
                                                        const float* __restrict__ pz, const DepthK& dk, float t_fwd) {
    XT t{1.0f, 0};
    if (p.T_out != nullptr && t_fwd >= 1e-30f) {   // the forward's value is usable (total_transmittance's rule)
        t.m = t_fwd;
        t.renorm();
        return t;
    }
    for (int k = 0; k < p.D; ++k) {
        float ix, iy, s;
        pixel_plane_coord<AC>(vw, bp, k, ix, iy, s);
        const Taps tp = make_taps(ix, iy, p.Ht, p.Wt);
        const RampTaps r = ramp_taps<TexT, STRICT>(depth, p.s_row, tp, pz[k], dk);
        const float a = bilerp<STRICT>(r.a[0], r.a[1], r.a[2], r.a[3], tp.f);
        t.m *= (1.0f - a) + 1e-10f;
        t.renorm();
    }
    return t;
}

// ---- LightRenderer.compute_depth for one texel: the composite and its back-to-front sweep, ONE text each ------------------------------------------
// Instances: alpha_depth_kernel (gmpi_abi.hip) and alpha_depth_backward_kernel (light_kernels.hip) hand in loads of alpha planes and a store per
// plane; ramp_depth_kernel and ramp_depth_backward_kernel (light_kernels.hip) hand in the ramp of one depth texel held in a register and a masked
// running sum.  alpha(k): the alpha of plane k; sink(k, v): what to do with dL/da_k.  ds: plane distances [D], wave-uniform.
// Op order (with -ffp-contract=off, what the bit-equality with the oracle rests on): w = a T; Z += w d; om = (1 - a) + 1e-10; T *= om.
template <typename AlphaF>
__device__ __forceinline__ void alpha_depth_composite(int D, const float* __restrict__ ds, AlphaF alpha, float& Tr, float& Z) {
#pragma unroll 4
    for (int k = 0; k < D; ++k) {
        const float al = alpha(k);
        const float w = al * Tr;           // weights = alpha * cumprod[:-1]
        const float wd = w * ds[k];
        Z = Z + wd;                        // torch.sum(weights * plane_ds, dim=1)
        float om = 1.0f - al;
        om = om + 1e-10f;
        Tr = Tr * om;
    }
}
// dL/da_k = T_k q_k - S_k / om_k, q_k = g d_k, S_k = gT T_out + sum_{j>k} a_j T_j q_j, back to front from the forward's final transmittance (same
// scheme as render_backward.hip: no cancellation behind opaque planes; T carried as mantissa x 2^exponent).  o: the texel's index in the three
// [B,1,H,W] images t_final, g_depth, g_T, each of which may be nullptr.
template <typename AlphaF, typename SinkF>
__device__ __forceinline__ void alpha_depth_sweep(int D, const float* __restrict__ ds, const float* __restrict__ t_final, const float* __restrict__ g_depth,
                                                  const float* __restrict__ g_T, int64_t o, AlphaF alpha, SinkF sink) {
    const float g = g_depth ? g_depth[o] : 0.0f;
    float tm = t_final ? t_final[o] : 0.0f;
    int te = 0;
    if (!(tm >= 1e-30f)) {  // missing or underflowed: rebuild front to back in the extended representation
        tm = 1.0f;
        for (int k = 0; k < D; ++k) {
            tm *= (1.0f - alpha(k)) + 1e-10f;
            te += __builtin_amdgcn_frexp_expf(tm);
            tm = __builtin_amdgcn_frexp_mantf(tm);
        }
    }
    float S = 0.0f;
    if (g_T) S = g_T[o] * __builtin_amdgcn_ldexpf(tm, te);   // (below 1e-30 * |gT| the term flushes: T_out itself underflows)
    for (int k = D - 1; k >= 0; --k) {
        const float al = alpha(k);
        const float om = (1.0f - al) + 1e-10f;
        tm = tm / om;
        te += __builtin_amdgcn_frexp_expf(tm);
        tm = __builtin_amdgcn_frexp_mantf(tm);
        const float Tk = __builtin_amdgcn_ldexpf(tm, te);
        const float q = g * ds[k];
        sink(k, Tk * q - S / om);
        S += al * Tk * q;
    }
}

}  // namespace gmpi
