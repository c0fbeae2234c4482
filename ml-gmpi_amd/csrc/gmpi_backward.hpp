// gmpi_backward.hpp -- the ONE home of what the backward kernels of the render share.  Nine kernels run the same back-to-front sweep
// (render_backward.hip: one pixel per lane, tile, tile2; render_backward_gather.hip: pixel_pass; render_backward_geometry.hip: geometry_pixel;
// render_shared.hip: shared_backward, shared_tile; render_depth.hip: depth_backward; render_depth_tile.hip: depth_tile), and the claims of DESIGN.md
// section 3.3 -- the forward's quotients and texels, bit-reproducible gather and geometry passes, gT entering S in every sweep -- hold because they
// all run THIS code:
//   BwdView / bwd_view              what is uniform over a view: the forward's View / view_setup (gmpi_device.hpp)
//   BwdPixel / bwd_pixel_setup(_with)   the per-pixel state: ray, dot, upstream gradients (OUT_PM1 applied), T = T_out, S = gT T -- or, for one chunk of a
//                                   plane-chunked stack, the sweep CONTINUED from T_in / S_in; bwd_store_suffix hands S to the chunk in front
//   BwdPixel::plane / plane_recip   one plane of the sweep (division form / the same quotients through a rounded reciprocal)
//   PairTaps / pair_tap_coord / fetch_pair_taps / pair_samples     the pair-load tap fetch and its bilinear sample
//   shade_pair_taps                 the pair-load form of the Shade policy of the shaded render (the *_shaded_kernel twins of render_backward.hip): colour
//                                   taps multiplied by the shading texel of their position and clipped, alpha raw.  The policy itself -- NoShade / ShadeK /
//                                   shade_texel / shaded_gather_sample -- lives in gmpi_device.hpp: the forwards of render_shaded.hip sample with it too
//   cvt_rpi_i32, fix_split, to_fix, abs_bits, lds_barrier, wave_max_u32, wave_max_bits     the fixed-point and wave primitives of the staged scatters
//   the cross-plane tile frame      what shared_tile and depth_tile stage their cross-plane sums with: the tile constants (kTileW .. kTilePlanes, kCW, kCH),
//                                   TileFrame / tile_frame / tile_frame_box / tile_grid, FixScale / fix_scale, lds_add_taps, MovingWindow and its flush
//                                   (their tap prefetch, fetch_taps, knows the shared-colour structs and lives in gmpi_shared.hpp; this lane's pixel, the
//                                   corner pixels and tile_box are the forward's, gmpi_device.hpp; render_depth_window.hip, a forward, borrows the constants)
// A change to the sweep or to the frame is made here, never in a kernel.
#pragma once
#include "gmpi_device.hpp"

#include <type_traits>

namespace gmpi {

struct BwdParams {
    const float* g_rgb;    // [N,3,H,W] gradient w.r.t. the colour the forward wrote ([0,1] or, with OUT_PM1, [-1,1])
    const float* g_depth;  // [N,1,H,W] or nullptr
    const float* g_T;      // [N,1,H,W] gradient w.r.t. the final transmittance, or nullptr: the sweep's S starts at gT * T_out
    float* g_rgba;        // [M,D,4,Ht,Wt] fp32, accumulated into (caller zero-fills)
    int64_t gs_mpi, gs_plane, gs_chan, gs_row;
    // The hand-over of a plane-chunked sweep (gmpi_mpi_render_chunk_backward_launch; the chunk instances of render_backward.hip read them, nobody else):
    const float* T_in = nullptr;   // [N,1,H,W] T in front of the chunk's first plane, or nullptr = 1
    const float* S_in = nullptr;   // [N,1,H,W] the suffix sum behind the chunk's last plane, or nullptr = 0
    float* S_out = nullptr;        // [N,1,H,W] or nullptr: the suffix sum in front of the chunk's first plane
};

constexpr float kTUsable = 1e-30f;   // a transmittance below this is rebuilt (XT) or, in front of a chunk, marks a pixel no plane behind it reaches

// transmittance as mantissa (in [0.5,1)) x 2^exponent
struct XT {
    float m;
    int e;
    __device__ __forceinline__ void renorm() {
        e += __builtin_amdgcn_frexp_expf(m);
        m = __builtin_amdgcn_frexp_mantf(m);
    }
    __device__ __forceinline__ float value() const { return __builtin_amdgcn_ldexpf(m, e); }
};

// Final transmittance of one pixel: the forward's value when it is usable, else a front-to-back walk of the alpha
// channel in the extended representation.
template <typename TexT, bool AC>
__device__ __forceinline__ XT total_transmittance(const KParams& p, const float* __restrict__ dhw, const TexT* __restrict__ vol,
                                                  float t_fwd, bool have_fwd, float ex, float ey, float ez, float rx, float ry,
                                                  float rz, float cx, float cy, float t_front = 1.0f) {
    XT t{t_front, 0};   // (t_front: T in front of plane 0 -- 1, or a chunk's T_in; the walk renormalises it with its first factor)
    if (have_fwd && t_fwd >= 1e-30f) {
        t.m = t_fwd;
        t.renorm();
        return t;
    }
    if (t_front != 1.0f) t.renorm();   // (a chunk's T_in may be tiny: its product with an om of 1e-10 must not leave the normal range)
    uint32_t unused = 0;
    for (int k = 0; k < p.D; ++k) {
        float ix, iy, s, u, v;
        plane_coord<AC>(dhw[3 * k] - ez, dhw[3 * k + 1], dhw[3 * k + 2], ex, ey, rx, ry, rz, cx, cy, ix, iy, s, u, v);
        float smp[4];
        gather_sample<TexT, false>(tex_offset(vol, static_cast<int64_t>(k) * p.s_plane), p.s_chan, p.s_row, p.Ht, p.Wt, ix, iy, false, unused, smp);
        t.m *= (1.0f - smp[3]) + 1e-10f;
        t.renorm();
    }
    return t;
}

// What is uniform over view n is the forward's View (gmpi_device.hpp): the backward reads the forward's constants.  A bad view index is only
// clamped here; the forward reports it.
using BwdView = View;
template <bool AC>
__device__ __forceinline__ BwdView bwd_view(const KParams& p, int n) {
    uint32_t bad_index = 0;
    return view_setup<AC>(p, n, bad_index);
}

// The state of one pixel through the back-to-front sweep.  A default-constructed one is a pixel that contributes nothing (a lane outside the
// image, a wave with another role).
struct BwdPixel {
    int64_t pix = 0;                                  // py W + px (clamped into the image)
    float rx = 0.0f, ry = 0.0f, rz = 1.0f;            // the ray
    float rrz = 1.0f;                                 // RN(1 / rz), for plane_coord_recip (a kernel that divides never reads it)
    float zx = 0.0f, zy = 0.0f, zz = 0.0f;            // the view's optical axis
    float dot = 0.0f;                                 // ray . z_dir: depth_k = s_k dot
    float gr = 0.0f, gg = 0.0f, gb = 0.0f, gz = 0.0f;   // upstream gradients (colour: w.r.t. C in [0, 1])
    XT T{1.0f, 0};                                    // T_{k+1} on entry of a plane, T_k on exit
    float S = 0.0f;                                   // sum_{j>k} w_j q_j on entry, sum_{j>=k} on exit

    // One plane: T_k = T_{k+1} / om_k, gradients d_s[4] of the sample (r, g, b, alpha), suffix sum update.  t_over_om = T.m / om, s_over_om = S / om.
    // Returns the plane's weight w_k = a_k T_k.
    __device__ __forceinline__ float step(const float (&smp)[4], float s, float t_over_om, float s_over_om, float (&d_s)[4]) {
        T.m = t_over_om;
        T.renorm();
        const float Tk = T.value();
        const float q = gr * smp[0] + gg * smp[1] + gb * smp[2] + gz * (s * dot);
        const float w = smp[3] * Tk;
        d_s[0] = gr * w, d_s[1] = gg * w, d_s[2] = gb * w;
        d_s[3] = Tk * q - s_over_om;
        S += w * q;
        return w;
    }
    // Division form.  plane_recip below gives the same quotients (div_by_recip is correctly rounded), hence the same gradients bit for bit.
    __device__ __forceinline__ float plane(const float (&smp)[4], float s, float (&d_s)[4]) {
        const float om = (1.0f - smp[3]) + 1e-10f;
        return step(smp, s, T.m / om, S / om, d_s);
    }
    // Both quotients through ONE reciprocal: v_rcp_f32, a Newton step (r = RN(1 / om) up to the last bit), Markstein's correction.
    __device__ __forceinline__ float plane_recip(const float (&smp)[4], float s, float (&d_s)[4]) {
        const float om = (1.0f - smp[3]) + 1e-10f;
        float r = __builtin_amdgcn_rcpf(om);
        r = __builtin_fmaf(__builtin_fmaf(-om, r, 1.0f), r, r);
        return step(smp, s, div_by_recip(T.m, om, r), div_by_recip(S, om, r), d_s);
    }
};

// The start of the sweep for pixel (px, py) of view n.  g_rgb / g_depth / g_T: the upstream gradients (g_depth, g_T may be nullptr); total(t_fwd): the
// pixel's final transmittance as an XT, given the forward's value (see MASKED for its default) -- total_transmittance for the layouts that store alpha
// planes (bwd_pixel_setup below), a walk over its own samples for the depth-alpha layout (render_depth.hip).
// MASKED: the workgroup keeps lanes outside the image (they pass its barriers): the pixel index is clamped, an inactive lane loads its ray but
// contributes nothing, and t_fwd defaults to 1.  Not MASKED: the lane is known to be inside the image (`active` is ignored), t_fwd defaults to 0.
template <bool MASKED, typename Total>
__device__ __forceinline__ void bwd_pixel_setup_with(BwdPixel& bp, const KParams& p, const BwdView& vw, int n, int px, int py, bool active,
                                                     const float* __restrict__ g_rgb, const float* __restrict__ g_depth, const float* __restrict__ g_T,
                                                     Total&& total, const float* S_in = nullptr) {
    if (!MASKED) active = true;
    const int64_t HW = vw.HW;
    const int64_t pix = MASKED ? static_cast<int64_t>(min(py, p.H - 1)) * p.W + min(px, p.W - 1) : static_cast<int64_t>(py) * p.W + px;
    bp.pix = pix;
    bp.rx = vw.rays[pix], bp.ry = vw.rays[HW + pix], bp.rz = vw.rays[2 * HW + pix];
    bp.rrz = 1.0f / bp.rz;
    bp.zx = vw.zx, bp.zy = vw.zy, bp.zz = vw.zz;
    bp.dot = ray_dot(vw, bp.rx, bp.ry, bp.rz);
    const float scale = (p.flags & GMPI_FLAG_OUT_PM1) ? 2.0f : 1.0f;  // forward wrote 2*C-1 (mpi_renderer.py:467)
    const float* __restrict__ g = g_rgb + static_cast<int64_t>(n) * 3 * HW + pix;
    bp.gr = active ? scale * g[0] : 0.f, bp.gg = active ? scale * g[HW] : 0.f, bp.gb = active ? scale * g[2 * HW] : 0.f;
    bp.gz = (active && g_depth) ? g_depth[static_cast<int64_t>(n) * HW + pix] : 0.0f;
    const float t_fwd = (active && p.T_out) ? p.T_out[static_cast<int64_t>(n) * HW + pix] : (MASKED ? 1.0f : 0.0f);
    if (active) bp.T = total(t_fwd);
    if (active && g_T) bp.S = g_T[static_cast<int64_t>(n) * HW + pix] * bp.T.value();   // dT_out/da_k = -T_out / om_k: T_out acts as a background
    // A sweep that is CONTINUED (the planes of this launch are a chunk of a longer stack): the suffix sum of the planes behind comes in, S = S_in + gT T.
    if (S_in != nullptr && active) bp.S = S_in[static_cast<int64_t>(n) * HW + pix] + bp.S;
}
// vol: channel 0 of the view's MPI -- the RGBA volume, or the alpha planes of the shared-colour layout (s_chan = 0).
// T_in, S_in (the chunk instances of render_backward.hip; nullptr, a compile-time constant, for everybody else): the planes of this launch are a chunk
// of a longer stack.  p.T_out is then T BEHIND the chunk and T_in the one in front of it; dL/da_k = T_k q_k - S_k / om_k and dL/drgb_k = g w_k hold
// unchanged with the GLOBAL T_k and S_k, so the sweep only starts elsewhere: T at the boundary value -- rebuilt, when that has underflowed, by the walk
// over the chunk's alpha from T_in instead of from 1 -- and S at S_in (+ gT T for the last chunk).  Where T_in itself is below 1e-30 (zero, denormals
// and NaN included) nothing behind reaches the pixel: it contributes nothing from this chunk (zero upstream gradients, T = 0, S = 0: every d_s is 0)
// and hands S_in on unchanged (bwd_store_suffix); the terms dropped are below 1e-20 D |q|.
template <typename TexT, bool AC, bool MASKED>
__device__ __forceinline__ void bwd_pixel_setup(BwdPixel& bp, const KParams& p, const BwdView& vw, int n, int px, int py, bool active,
                                                const float* __restrict__ g_rgb, const float* __restrict__ g_depth, const float* __restrict__ g_T,
                                                const TexT* __restrict__ vol, const float* T_in = nullptr, const float* S_in = nullptr) {
    bool dead = false;
    bwd_pixel_setup_with<MASKED>(bp, p, vw, n, px, py, active, g_rgb, g_depth, g_T, [&](float t_fwd) {
        float t_front = 1.0f;
        if (T_in != nullptr) {
            t_front = T_in[static_cast<int64_t>(n) * vw.HW + bp.pix];
            dead = !(t_front >= kTUsable);
            if (dead) return XT{0.0f, 0};
        }
        return total_transmittance<TexT, AC>(p, vw.dhw, vol, t_fwd, p.T_out != nullptr, vw.ex, vw.ey, vw.ez, bp.rx, bp.ry, bp.rz, vw.cx, vw.cy, t_front);
    }, S_in);
    if (T_in != nullptr && dead) bp.gr = bp.gg = bp.gb = bp.gz = 0.0f, bp.S = 0.0f;
}
// The hand-over to the chunk in front: after plane 0 of the launch the lane stores its suffix sum.  S_in == S_out is fine: a lane touches its own pixel only.
__device__ __forceinline__ void bwd_store_suffix(const BwdParams& b, const BwdPixel& bp, int n, int64_t HW, bool active) {
    if (b.S_out == nullptr || !active) return;
    const int64_t i = static_cast<int64_t>(n) * HW + bp.pix;
    const bool dead = b.T_in != nullptr && !(b.T_in[i] >= kTUsable);
    b.S_out[i] = dead ? (b.S_in != nullptr ? b.S_in[i] : 0.0f) : bp.S;
}

// Where the pixel's ray meets plane k of its view's MPI, by the forward's strict-order chain (compiler divisions).
template <bool AC>
__device__ __forceinline__ void pixel_plane_coord(const BwdView& vw, const BwdPixel& bp, int k, float& ix, float& iy, float& s) {
    float u, v;
    plane_coord<AC>(vw.dhw[3 * k] - vw.ez, vw.dhw[3 * k + 1], vw.dhw[3 * k + 2], vw.ex, vw.ey, bp.rx, bp.ry, bp.rz, vw.cx, vw.cy, ix, iy, s, u, v);
}

template <typename TexT> __device__ __forceinline__ void load_pair(const unsigned char* __restrict__ base, uint32_t byte_off, float& a, float& b) {
    const TexT* __restrict__ q = reinterpret_cast<const TexT*>(base + byte_off);
    a = to_f32(q[0]), b = to_f32(q[1]);
}
template <> __device__ __forceinline__ void load_pair<float>(const unsigned char* __restrict__ base, uint32_t byte_off, float& a, float& b) {
    float v[2];
    __builtin_memcpy(v, base + byte_off, 8);  // (one global_load_dwordx2 at dword alignment, uniform base + 32-bit lane offset)
    a = v[0], b = v[1];
}

// Host side: do all offsets inside one plane of a [.., 4, Ht, Wt] tensor -- 3 channels + Ht rows + Wt items of `es` bytes -- fit 31 bits?  The ONE test of
// every launcher whose kernel forms in-plane offsets in 32 bits (fetch_pair_taps; the 64 x 8 tile backward's gradient offsets, es = 1: they count items).
inline bool plane_offsets_fit_32(int64_t s_chan, int64_t s_row, int Ht, int Wt, int es) {
    if (s_chan < 0 || s_row < 0) return false;
    const int64_t lim = (int64_t(1) << 31) / es;   // (each term is compared on its own first: no product or sum below can overflow 64 bits)
    if (s_chan >= lim || s_row >= lim) return false;
    return 3 * s_chan + static_cast<int64_t>(Ht) * s_row + Wt < lim;
}

// ---- taps fetched as (x, x + 1) pairs: 8 loads of 8 bytes instead of 16 of 4 for fp32 volumes, at 32-bit offsets from a uniform base (the launcher
// checks Wt >= 2 and plane_offsets_fit_32).  What a plane keeps between the issue of its taps and their use:
struct PairTaps {
    float s, wx1, wy1;   // depth factor; ix - floor(ix), iy - floor(iy)
    int x0, y0;          // floor(ix), floor(iy); -2 = out of range (NaN / huge coordinates: all weights 0)
    float v[16];         // per channel (top p0, p1 | bottom p0, p1)
};
// Coordinates of the pixel on a plane (the default mode's chain; pa = zdiff, w/2, h/2, RN(2/w); rh = RN(2/h)): fills q.s .. q.y0, returns (ix, iy).
template <bool AC>
__device__ __forceinline__ void pair_tap_coord(PairTaps& q, const BwdPixel& bp, const BwdView& vw, const float4 pa, float rh, int Ht, int Wt, float& ix, float& iy) {
    plane_coord_recip<AC>(pa.x, pa.y, pa.z, pa.w, rh, vw.ex, vw.ey, bp.rx, bp.ry, bp.rz, bp.rrz, vw.cx, vw.cy, ix, iy, q.s);
    const float fx = floorf(ix), fy = floorf(iy);
    q.wx1 = ix - fx, q.wy1 = iy - fy;
    q.x0 = (fx >= -2.0f && fx <= static_cast<float>(Wt)) ? static_cast<int>(fx) : -2;
    q.y0 = (fy >= -2.0f && fy <= static_cast<float>(Ht)) ? static_cast<int>(fy) : -2;
}
// The 8 pair loads of q's footprint; pl = channel 0 of the plane, strides in bytes.
template <typename TexT>
__device__ __forceinline__ void fetch_pair_taps(PairTaps& q, const TexT* __restrict__ plane, uint32_t s_chan_b, uint32_t s_row_b, int Ht, int Wt) {
    constexpr int kES = static_cast<int>(sizeof(TexT));
    const int xa = min(max(q.x0, 0), Wt - 2);
    const int ya = min(max(q.y0, 0), Ht - 1), yb = min(max(q.y0 + 1, 0), Ht - 1);
    const unsigned char* __restrict__ pl = reinterpret_cast<const unsigned char*>(plane);
    const uint32_t oa = static_cast<uint32_t>(ya) * s_row_b + static_cast<uint32_t>(xa) * kES;
    const uint32_t ob = static_cast<uint32_t>(yb) * s_row_b + static_cast<uint32_t>(xa) * kES;
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
        load_pair<TexT>(pl, oa + c4 * s_chan_b, q.v[4 * c4 + 0], q.v[4 * c4 + 1]);
        load_pair<TexT>(pl, ob + c4 * s_chan_b, q.v[4 * c4 + 2], q.v[4 * c4 + 3]);
    }
}
// The same taps of channels-last float layers (rgba32f_t / rgba16h_t / rgba16b_t, gmpi_device.hpp; the texel instances of render_backward.hip): the pair
// (x, x + 1) of a row is two whole texels side by side -- ONE run of 32 bytes of fp32 (two 16-byte loads) or 16 bytes of 16-bit storage (one), loaded at
// the ELEMENT's alignment (a column slice may start a texel at any element), 32-bit offsets from a uniform base (the launcher checks Wt >= 2 and
// layers_offsets_fit_32).  Clamps, and hence the re-assigned border weights of pair_samples, are fetch_pair_taps'; the taps land in q.v in its order.
// plane: texel (0, 0) of the plane; the row stride in bytes.
template <typename TexT>
__device__ __forceinline__ void fetch_texel_pair_taps(PairTaps& q, const TexT* __restrict__ plane, uint32_t s_row_b, int Ht, int Wt) {
    using E = typename FloatTexel<TexT>::elem;
    constexpr uint32_t kTexel = sizeof(TexT);
    struct Pair { TexT t[2]; };
    const int xa = min(max(q.x0, 0), Wt - 2);
    const int ya = min(max(q.y0, 0), Ht - 1), yb = min(max(q.y0 + 1, 0), Ht - 1);
    const unsigned char* __restrict__ pl = reinterpret_cast<const unsigned char*>(plane);
    const uint32_t oa = static_cast<uint32_t>(ya) * s_row_b + static_cast<uint32_t>(xa) * kTexel;
    const uint32_t ob = static_cast<uint32_t>(yb) * s_row_b + static_cast<uint32_t>(xa) * kTexel;
    Pair top, bot;
    __builtin_memcpy(&top, __builtin_assume_aligned(pl + oa, alignof(E)), sizeof(Pair));
    __builtin_memcpy(&bot, __builtin_assume_aligned(pl + ob, alignof(E)), sizeof(Pair));
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
        q.v[4 * c4 + 0] = to_f32(top.t[0].c[c4]), q.v[4 * c4 + 1] = to_f32(top.t[1].c[c4]);
        q.v[4 * c4 + 2] = to_f32(bot.t[0].c[c4]), q.v[4 * c4 + 3] = to_f32(bot.t[1].c[c4]);
    }
}
// Host side, the texel twin of plane_offsets_fit_32: do all offsets inside one plane of [.., Ht, Wt, 4] layers -- Ht rows of s_row + Wt texels of 4 items,
// items of `es` bytes -- fit 31 bits?  (the layers: s_row in ELEMENTS, es = the element size; their fp32 gradient, whose offsets count dwords: es = 1)
inline bool layers_offsets_fit_32(int64_t s_row, int Ht, int Wt, int es) {
    if (s_row < 0) return false;
    const int64_t lim = (int64_t(1) << 31) / es;
    if (s_row >= lim) return false;
    return static_cast<int64_t>(Ht) * s_row + 4 * static_cast<int64_t>(Wt) < lim;
}
// The Shade policy's pair-load form (NoShade / ShadeK / shade_texel: gmpi_device.hpp), next to fetch_pair_taps: the two pair loads of the shading image
// at the footprint's rows and columns (fetch_pair_taps' addresses), then the multiply and clip of q.v[0..11].  sh: the MPI's shading image, row stride
// in bytes (the launcher checks that its offsets fit 32 bits, as for a plane of the volume, and Wt >= 2).
__device__ __forceinline__ void shade_pair_taps(PairTaps& q, const float* __restrict__ sh, uint32_t sh_row_b, int Ht, int Wt) {
    const int xa = min(max(q.x0, 0), Wt - 2);
    const int ya = min(max(q.y0, 0), Ht - 1), yb = min(max(q.y0 + 1, 0), Ht - 1);
    const unsigned char* __restrict__ pl = reinterpret_cast<const unsigned char*>(sh);
    float sv[4];   // top p0, p1 | bottom p0, p1
    load_pair<float>(pl, static_cast<uint32_t>(ya) * sh_row_b + static_cast<uint32_t>(xa) * 4u, sv[0], sv[1]);
    load_pair<float>(pl, static_cast<uint32_t>(yb) * sh_row_b + static_cast<uint32_t>(xa) * 4u, sv[2], sv[3]);
#pragma unroll
    for (int c4 = 0; c4 < 3; ++c4)
#pragma unroll
        for (int i = 0; i < 4; ++i) q.v[4 * c4 + i] = shade_texel(q.v[4 * c4 + i], sv[i]);
}

// The taps have landed: the bilinear samples (zeros padding: the weight of a tap outside the texture is 0).
__device__ __forceinline__ void pair_samples(const PairTaps& q, int Ht, int Wt, float (&smp)[4]) {
    const int x0 = q.x0, y0 = q.y0;
    const bool x0in = x0 >= 0 && x0 <= Wt - 1, x1in = x0 >= -1 && x0 <= Wt - 2;
    const bool y0in = y0 >= 0 && y0 <= Ht - 1, y1in = y0 >= -1 && y0 <= Ht - 2;
    const float wx0 = x0in ? 1.0f - q.wx1 : 0.0f, wx1 = x1in ? q.wx1 : 0.0f;
    const float wy0 = y0in ? 1.0f - q.wy1 : 0.0f, wy1 = y1in ? q.wy1 : 0.0f;
    // the pair (p0, p1) sits at columns (xa, xa + 1), xa = clamp(x0, 0, Wt - 2): at the left border (x0 = -1) the tap x0 + 1 is p0, at the
    // right border (x0 = Wt - 1) the tap x0 is p1
    const int sh = x0 - min(max(x0, 0), Wt - 2);
    const float a0 = sh == 0 ? wx0 : (sh < 0 ? wx1 : 0.0f), a1 = sh == 0 ? wx1 : (sh > 0 ? wx0 : 0.0f);
    const float w00 = a0 * wy0, w01 = a1 * wy0, w10 = a0 * wy1, w11 = a1 * wy1;
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
        float acc_s = q.v[4 * c4 + 0] * w00;
        acc_s = __builtin_fmaf(q.v[4 * c4 + 1], w01, acc_s);
        acc_s = __builtin_fmaf(q.v[4 * c4 + 2], w10, acc_s);
        smp[c4] = __builtin_fmaf(q.v[4 * c4 + 3], w11, acc_s);
    }
}

// ---- primitives of the staged (fixed-point, LDS) scatters ---------------------------------------------------------------------------------------
// round to nearest (floor(x + 0.5)) in one instruction: the staged sums must not be biased -- with a texture much coarser than the image a hundred
// taps meet in one texel, and a truncating conversion adds up to half a unit of the fixed-point grid PER TAP in one direction
__device__ __forceinline__ int cvt_rpi_i32(float x) {
    int r;
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
// w = hi * 2^12 + lo with integers hi = RN(w / 4096) and lo = RN(w - 4096 hi): the remainder is exact (one FMA: w has 24 significant bits) and
// |lo| <= 2048, so the pair is w rounded to the nearest integer; hi fits 32 bits for |w| < 2^43.
__device__ __forceinline__ void fix_split(float w, int& hi, int& lo) {
    hi = cvt_rpi_i32(w * (1.0f / 4096.0f));
    lo = cvt_rpi_i32(__builtin_fmaf(-static_cast<float>(hi), 4096.0f, w));
}
// fp32 -> 64-bit fixed point without a trip through fp64 (a double conversion and an f64 -> i64 expansion per add were most of the scatter's VALU
// work): v scale (a power of two: exact) as 4096 hi + lo (one v_mad_i64_i32).
__device__ __forceinline__ unsigned long long to_fix(float v, float scale) {
    int hi, lo;
    fix_split(v * scale, hi, lo);
    return static_cast<unsigned long long>(static_cast<long long>(hi) * 4096ll + static_cast<long long>(lo));
}
// |v| as a word that orders like the magnitude (non-negative floats order like their bit patterns), NaN / Inf on top
__device__ __forceinline__ uint32_t abs_bits(float v) { return (v != v) ? 0x7fc00000u : __float_as_uint(fabsf(v)); }
// Workgroup barrier that orders LDS only.  `__syncthreads()` is a workgroup-scope fence over EVERY address space: on this part it drains vmcnt, i.e.
// every plane would wait for its own tap prefetch and for the flush's global atomics.  Between the planes of a sweep only LDS state is shared.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// Maximum of an unsigned word over the 64 lanes of a wave (EVERY lane must be enabled).  Two forms, each kept where it was measured:
// wave_max_u32 -- a scalar result; four row shifts and two row broadcasts on the DPP path (tile2).  (Left to the compiler, `atomicMax` on a
// wave-uniform LDS address becomes a SCALAR loop over the lanes -- s_ff1 / v_readlane / s_max, 64 rounds of 7 instructions per wave and plane: it
// was two thirds of that kernel's pixel phase.)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    auto step = [&](auto ctrl, auto rows) {
        const uint32_t o = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), decltype(ctrl)::value, decltype(rows)::value, 0xf, true));
        v = max(v, o);
    };
    step(std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});   // row_shr:1
    step(std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});   // row_shr:2
    step(std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});   // row_shr:4
    step(std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});   // row_shr:8   -> lane 15 of a row: the row's maximum
    step(std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});   // row_bcast:15 into rows 1, 3
    step(std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});   // row_bcast:31 into rows 2, 3 -> lane 63: the wave's maximum
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}
// wave_max_bits -- the maximum in every lane, by xor shuffles (the shared-colour tile kernel).
__device__ __forceinline__ uint32_t wave_max_bits(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), o)));
    return v;
}

// ---- the cross-plane tile frame -------------------------------------------------------------------------------------------------------------------
// What render_shared_tile_kernel (render_shared.hip) and render_depth_tile_kernel (render_depth_tile.hip) share: one workgroup of kTileThreads lanes per
// kTileW x kTileH pixel tile, the planes' texel boxes in a table of kTilePlanes entries, and gradients that belong to ONE image summed across the planes in
// a window of kCW x kCH texels of 64-bit fixed-point words that moves with the boxes.  What a kernel keeps for itself: its LDS, its box limit, its
// scales and destinations (the flush's sink) and its BARRIERS -- nothing here contains one; the kernels' headers say which barrier orders what.
constexpr int kTileW = 32, kTileH = 16, kTileThreads = kTileW * kTileH;
constexpr int kCW = 64, kCH = 32;      // the window, per channel (64-bit words: 16 KiB a channel)
constexpr int kTilePlanes = 128;       // planes a tile launch can take (the box table; the bound on a cell's sum: 512 pixels x 128 planes = 2^16 terms)
constexpr int kFixBits = 40;           // a staged term is scaled to below 2^41 (to_fix takes |w| < 2^43)
inline bool tile_planes_fit(const KParams& p) { return p.D <= kTilePlanes; }

// The tile and the pixel of this lane.  tile < 0: the workgroup is one of the grid's padding (the grid is a multiple of 8) and returns as a whole.
struct TileFrame : TileLane, TileCorners {   // this lane's pixel and the tile's corner pixels (gmpi_device.hpp: the forward's)
    int tile, txi, tyi;
};
__device__ __forceinline__ TileFrame tile_frame(const KParams& p, int tiles_x) {
    const int n_tiles = tiles_x * ((p.H + kTileH - 1) / kTileH);
    const int tile = xcd_item_per_group(static_cast<int>(blockIdx.x), n_tiles, n_tiles);
    const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    return TileFrame{tile_lane<kTileW, kTileH>(txi, tyi, threadIdx.x, p.W, p.H), tile_corners<kTileW, kTileH>(txi, tyi, p.W, p.H), tile >= n_tiles ? -1 : tile, txi, tyi};
}
// the tile's texel box on plane k of the view; staged (nx > 0) when it fits pitch x rows
template <bool AC>
__device__ __forceinline__ int4 tile_frame_box(const KParams& p, const BwdView& vw, const TileFrame& t, int k, int pitch, int rows) {
    return tile_box<AC>(p, vw, vw.rays, vw.dhw[3 * k] - vw.ez, vw.dhw[3 * k + 1], vw.dhw[3 * k + 2], t.cx0, t.cx1, t.cy0, t.cy1, pitch, rows);
}
// host side: what tile_frame expects of the launch (grid.x tiles in xcd_item_per_group's order, grid.y views)
struct TileGrid { int tiles_x, n_tiles; dim3 grid; };
inline TileGrid tile_grid(const KParams& p) {
    const int tiles_x = (p.W + kTileW - 1) / kTileW, n_tiles = tiles_x * ((p.H + kTileH - 1) / kTileH);
    return TileGrid{tiles_x, n_tiles, dim3(xcd_grid_per_group(n_tiles, n_tiles), p.N)};
}

// The power-of-two scale of a fixed-point sum from max_bits = abs_bits of the largest term M: 2^(bits - e), e = floor(log2 M), so that a term is below
// 2^(bits + 1).  stage: M is neither zero nor Inf / NaN; otherwise nothing is staged and scale = inv = 0.
struct FixScale { bool stage; float scale, inv; };
__device__ __forceinline__ FixScale fix_scale(uint32_t max_bits, int bits) {
    const bool stage = max_bits != 0u && max_bits < 0x7f800000u;
    const int shf = min(bits - (static_cast<int>(max_bits >> 23) - 127), 126);
    return FixScale{stage, stage ? __builtin_amdgcn_ldexpf(1.0f, shf) : 0.0f, stage ? __builtin_amdgcn_ldexpf(1.0f, -shf) : 0.0f};
}
// d times each of four tap weights added to the 2 x 2 cells at `cell` of an LDS array of 64-bit fixed-point words: the LDS twin of add_taps
// (gmpi_shared.hpp), with its rule -- the weight gates the add (a zero weight marks a tap outside the texture or off the ramp).
__device__ __forceinline__ void lds_add_taps(unsigned long long* __restrict__ cell, int pitch, float d, float w_nw, float w_ne, float w_sw, float w_se,
                                             float scale) {
    if (w_nw != 0.0f) atomicAdd(cell, to_fix(d * w_nw, scale));
    if (w_ne != 0.0f) atomicAdd(cell + 1, to_fix(d * w_ne, scale));
    if (w_sw != 0.0f) atomicAdd(cell + pitch, to_fix(d * w_sw, scale));
    if (w_se != 0.0f) atomicAdd(cell + pitch + 1, to_fix(d * w_se, scale));
}

// The moving window: anchor (the texel of cell (0, 0)), the rows in use since they were last reset, and whether it has been anchored at all.  Every
// member is workgroup-uniform and lives in registers: all of it is computed from the box table and launch constants.  Channel c of the window is the
// kCW x kCH block at acc + c kCW kCH.  The boxes of a tile drift over the planes by parallax; when the next plane's box leaves the window the kernel
// flushes it and re-anchors it with the box at the end it drifts away from, so that the window's whole slack lies ahead (the direction is taken from
// the boxes of the two ends of the sweep: nearer planes lie towards box_front).
struct MovingWindow {
    int x0 = 0, y0 = 0, row0 = kCH, row1 = 0;
    bool open = false;

    __device__ __forceinline__ bool covers(const int4& bb) const {
        return open && bb.x >= x0 && bb.y >= y0 && bb.x + bb.z <= x0 + kCW && bb.y + bb.w <= y0 + kCH;
    }
    __device__ __forceinline__ void reset_rows() { row0 = kCH, row1 = 0; }
    __device__ __forceinline__ void anchor(const int4& bb, const int4& box_front) {
        x0 = (box_front.z > 0 && box_front.x < bb.x) ? bb.x + bb.z - kCW : bb.x;
        y0 = (box_front.z > 0 && box_front.y < bb.y) ? bb.y + bb.w - kCH : bb.y;
        reset_rows();
        open = true;
    }
    __device__ __forceinline__ void grow(const int4& bb) { row0 = min(row0, bb.y - y0), row1 = max(row1, bb.y + bb.w - y0); }
    // the footprint's 2 x 2 cells lie inside the window (whatever the box says: this is what keeps wild coordinates out); cell: the index of its nw cell
    __device__ __forceinline__ bool holds(const Footprint& f) const {
        const int wx = f.x0 - x0, wy = f.y0 - y0;
        return wx >= 0 && wy >= 0 && wx + 1 < kCW && wy + 1 < kCH;
    }
    __device__ __forceinline__ int cell(const Footprint& f) const { return (f.y0 - y0) * kCW + (f.x0 - x0); }
    // Channels [0, nc) of the rows in use -> sink(c, gx, gy, value): every non-zero cell is zeroed and, when its texel (gx, gy) lies inside the
    // texture, handed over as a float (the one rounding of a staged sum; the sink applies its scale's inverse and adds to its destination).  A wave
    // takes 64 consecutive texels of one row and channel.  The row range is left as it is.
    template <typename Sink>
    __device__ __forceinline__ void flush(unsigned long long* __restrict__ acc, int tid, int nc, int Ht, int Wt, Sink&& sink) const {
        if (row1 <= row0) return;
        const int rows = row1 - row0;
        for (int i = tid; i < rows * nc * kCW; i += kTileThreads) {
            const int line = i / kCW, x = i - line * kCW;   // line = (row, channel)
            const int lr = line / nc, c = line - lr * nc, row = row0 + lr;
            unsigned long long* __restrict__ src = acc + (c * kCH + row) * kCW + x;
            const long long v = static_cast<long long>(*src);
            if (v != 0) {
                *src = 0ull;
                const int gx = x0 + x, gy = y0 + row;
                // (a cell outside the texture only ever receives zero weights: belt and braces)
                if (gx >= 0 && gx < Wt && gy >= 0 && gy < Ht) sink(c, gx, gy, static_cast<float>(static_cast<double>(v)));
            }
        }
    }
};

}  // namespace gmpi
