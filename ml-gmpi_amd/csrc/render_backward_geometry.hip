// render_backward_geometry.hip -- gradient of the fused render w.r.t. the sample POSITIONS: the camera rays, the eye position, the optical axis
// and the plane geometry (an extension: the reference builds the sampling grid under torch.no_grad(), gmpi/core/mpi.py:65, so none of these get a
// gradient there).
//
// Per view n, pixel p, plane k (the forward's chain, gmpi_device.hpp):  s = (d_k - ez) / rz,  x = ex + rx s,  y = ey + ry s,  u = 2x / w_k,
// v = 2y / h_k,  ix / iy the unnormalised texel coordinates (align_corners, or the 0.95 narrowing inside [-1, 1] without it),  depth_k = s dot,
// dot = r . z_dir.  The back-to-front sweep of the volume backward (BwdPixel::plane_recip, gmpi_backward.hpp) gives d_s[c] = dL/d(sample c)
// and the depth term G_k = gZ w_k; the four taps it gathers give the bilinear derivatives (grid_sampler_2d, zeros padding, tx = ix - x0):
//     g_ix = sum_c d_s[c] ((t_ne - t_nw)(1 - ty) + (t_se - t_sw) ty),   g_iy = sum_c d_s[c] ((t_sw - t_nw)(1 - tx) + (t_se - t_ne) tx)
//     g_x = g_ix dix/dx,  g_y = g_iy diy/dy,  g_s = g_x rx + g_y ry + G_k dot      (dix/dx = (Wt - 1) / w_k, or c Wt / w_k with c = 0.95 | 1)
// and, summed over the planes:  dL/dray = (g_x s, g_y s, -g_s s / rz) + G_k s z_dir,  dL/deye = (g_x, g_y, -g_s / rz),  dL/dz_dir = G_k s r,
// dL/d(d_k, h_k, w_k) = (g_s / rz, -g_y y / h_k, -g_x x / w_k)  (the last two summed over every pixel of every view of the MPI).
//
// One pixel per lane, 64 x 4 pixel tiles.  The ray gradient is written once per pixel.  Everything summed over pixels is reduced inside the
// workgroup in a fixed order (DPP within a row of 16 lanes, the four rows by readlane, one LDS slot per wave and plane, the waves in order) and
// written to this tile's slot of a slab in the caller's workspace; geometry_reduce_kernel then sums the slabs in a fixed order.  No atomics: every
// output is bit-reproducible from run to run.  Any view_to_mpi, any ray field (each pixel gathers its own taps), 64-bit volume offsets.
//
// ONE frame (geometry_pixel_kernel), four TAP SOURCES, selected by the storage type and the layout structs the kernel is instantiated with (SourceOf).  The frame
// depends on the input layout in two places only: where the 4 x 4 tap values
// t[c][nw, ne, sw, se] of a plane come from, and where the sweep's starting transmittance comes from.  A source is a small struct with
//   start(bp, ...)            the per-pixel setup (bwd_pixel_setup / bwd_pixel_setup_with, gmpi_backward.hpp) with the layout's transmittance walk
//   taps<STRICT>(k, ix, iy, q)   the 16 tap values of plane k and the fractions; false = the plane is the identity of this pixel's sweep: skipped
//   VolumeSource   the RGBA volume (no layout struct): four channels of one plane; never skips.  float / bf16_t / f16_t, and u8_t: planar 8-bit codes read
//                  in place, every tap through to_f32(u8_t), the correctly rounded c / 255 the forward reads
//   TexelSource    the RGBA volume stored as whole texels, read in place (no layout struct; selected by the storage type): rgba8_t, channels-last
//                  8-bit codes, one 4-byte load per tap; rgba32f_t / rgba16h_t / rgba16b_t, channels-last float layers, one 16- / 8-byte load per
//                  tap at the element's alignment.  VolumeSource's values, padding and start: for equal values the volume entry's bits
//   SharedSource   the shared-colour layout (SharedK): channels 0-2 from rgb[m] (background[m] on plane D - 1 when one is
//                  given: uniform per plane), channel 3 from alpha[m, k]; the start is the volume's (KParams carries the alpha planes with s_chan = 0)
//   DepthSource    the depth-alpha layout (SharedK, DepthK): channel 3's taps are the RAMP of each depth tap (depth_ramp: the forward's
//                  correctly rounded quotient for the launch's mode), 0 outside the texture, so that the frame's bilinear sample and its dix[3] /
//                  diy[3] are, term for term, those of the expanded volume with zeros padding; the start is depth_total_transmittance (the re-walk
//                  is this layout's common path); in strict-order mode the alpha sample and the re-walk round as the strict forward does.  A plane whose four ramp taps are all exactly 0 is skipped WITHOUT loading its colour taps (the
//                  forward never reads colour under a zero alpha sample): with a = 0 and zero tap differences it adds nothing to any gradient and
//                  leaves T and S as they are (om rounds to 1).  NOT skipped: an alpha SAMPLE of 0 with a non-zero tap under a zero bilinear
//                  weight -- its one-sided position derivative is not zero.
// The layout kernels set no status bits.
#include "gmpi_backward.hpp"
#include "gmpi_shared.hpp"

#include <algorithm>

namespace gmpi {
namespace bwgeo {

constexpr int kGT = 256, kGTW = 64, kGTH = 4, kGWaves = kGT / 64;   // one pixel per lane, a wave = one pixel row of the tile
constexpr int kGChunk = 96;                                          // planes whose constants sit in LDS at a time
constexpr int kGRed = 256;                                           // threads of the slab reducer

// Sum over the 64 lanes, the same value in every lane; the order of the adds is fixed (bit-reproducible).
__device__ __forceinline__ float wave_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false));  // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, false));  // row_mirror
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
    return (r0 + r1) + (r2 + r3);
}

// The four taps of one plane (zeros padding: a tap outside the texture is 0, its address clamped) and the fractions -- what both the sample and
// its derivative w.r.t. (ix, iy) are formed from.  taps[c] = (nw, ne, sw, se) of channel c; wx1 = ix - floor(ix), wy1 = iy - floor(iy).
struct Taps {
    float t[4][4];
    float wx0, wx1, wy0, wy1;
};

// Where the four taps of a footprint are read (addresses clamped into the texture) and which of them lie inside it; fills q's fractions.
struct TapPos {
    int xa, xb, ya, yb;
    bool nw, ne, sw, se;
};
__device__ __forceinline__ TapPos tap_pos(int Ht, int Wt, float ix, float iy, Taps& q) {
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    q.wx1 = ix - fx0, q.wx0 = (fx0 + 1.0f) - ix;
    q.wy1 = iy - fy0, q.wy0 = (fy0 + 1.0f) - iy;
    const int x0 = (fx0 >= -2.0f && fx0 <= static_cast<float>(Wt)) ? static_cast<int>(fx0) : -2;   // (NaN / huge coordinates: out of range)
    const int y0 = (fy0 >= -2.0f && fy0 <= static_cast<float>(Ht)) ? static_cast<int>(fy0) : -2;
    const bool x0in = x0 >= 0 && x0 <= Wt - 1, x1in = x0 >= -1 && x0 <= Wt - 2;
    const bool y0in = y0 >= 0 && y0 <= Ht - 1, y1in = y0 >= -1 && y0 <= Ht - 2;
    TapPos tp;
    tp.xa = min(max(x0, 0), Wt - 1), tp.xb = min(max(x0 + 1, 0), Wt - 1);
    tp.ya = min(max(y0, 0), Ht - 1), tp.yb = min(max(y0 + 1, 0), Ht - 1);
    tp.nw = x0in && y0in, tp.ne = x1in && y0in, tp.sw = x0in && y1in, tp.se = x1in && y1in;
    return tp;
}
// the four texels of one channel as stored (a tap outside the texture reads the clamped border texel)
template <typename TexT>
__device__ __forceinline__ void load_taps(const TexT* __restrict__ ch, int64_t s_row, const TapPos& tp, float (&v)[4]) {
    const int64_t oa = static_cast<int64_t>(tp.ya) * s_row, ob = static_cast<int64_t>(tp.yb) * s_row;
    v[0] = to_f32(ch[oa + tp.xa]), v[1] = to_f32(ch[oa + tp.xb]), v[2] = to_f32(ch[ob + tp.xa]), v[3] = to_f32(ch[ob + tp.xb]);
}
// ... with zeros padding
__device__ __forceinline__ void pad_taps(const TapPos& tp, const float (&v)[4], float (&t)[4]) {
    t[0] = tp.nw ? v[0] : 0.0f, t[1] = tp.ne ? v[1] : 0.0f, t[2] = tp.sw ? v[2] : 0.0f, t[3] = tp.se ? v[3] : 0.0f;
}
template <typename TexT>
__device__ __forceinline__ void gather_channel(const TexT* __restrict__ ch, int64_t s_row, const TapPos& tp, float (&t)[4]) {
    float v[4];
    load_taps<TexT>(ch, s_row, tp, v);
    pad_taps(tp, v, t);
}

template <typename TexT>
__device__ __forceinline__ void gather_taps(const TexT* __restrict__ pl, int64_t s_chan, int64_t s_row, int Ht, int Wt, float ix, float iy, Taps& q) {
    const TapPos tp = tap_pos(Ht, Wt, ix, iy, q);
#pragma unroll
    for (int c = 0; c < 4; ++c) gather_channel<TexT>(pl + c * s_chan, s_row, tp, q.t[c]);
}

// ---- the tap sources (see the header) ----------------------------------------------------------------------------------------------------------
template <typename TexT>
struct VolumeSource {
    static constexpr bool kSkips = false;          // taps() never returns false
    static constexpr bool kPlaneZ = false;         // (the depth-alpha layout alone has a plane_z)
    static constexpr bool kForwardAlpha = false;   // the alpha sample is the frame's fma chain in both modes
    const TexT* __restrict__ vol;
    __device__ __forceinline__ VolumeSource(const KParams& p, const BwdView& vw)
        : vol(static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(vw.m) * p.s_mpi) {}
    template <bool AC, bool STRICT>
    __device__ __forceinline__ void start(BwdPixel& bp, const KParams& p, const BwdView& vw, const BwdParams& b, int n, int px, int py, bool active) const {
        bwd_pixel_setup<TexT, AC, true>(bp, p, vw, n, px, py, active, b.g_rgb, b.g_depth, b.g_T, vol);
    }
    template <bool STRICT>
    __device__ __forceinline__ bool taps(const KParams& p, int k, int Ht, int Wt, float ix, float iy, Taps& q) const {
        gather_taps<TexT>(vol + static_cast<int64_t>(k) * p.s_plane, p.s_chan, p.s_row, Ht, Wt, ix, iy, q);
        return true;
    }
};

// The RGBA volume stored as whole texels, read in place: rgba8_t (channels-last 8-bit codes: one 4-byte load per tap, then texel_code + unorm8_to_f32
// per channel -- to_f32(u8_t)'s value, the one the forward reads) and rgba32f_t / rgba16h_t / rgba16b_t (channels-last float layers: one 16- / 8-byte
// load per tap at the element's alignment).  KParams' strides count BYTES, s_chan is unused; offsets are 64-bit.  The padding is VolumeSource's
// (tap_pos / pad_taps: address clamped, value masked) and so is every value: the frame's results are, bit for bit, those of the planar fp32 /
// 16-bit volume of the same values.  The start is the volume's (total_transmittance walks the texels through gather_sample's texel forms).
template <typename TexT>
struct TexelSource {
    static constexpr bool kSkips = false;
    static constexpr bool kPlaneZ = false;
    static constexpr bool kForwardAlpha = false;
    const TexT* __restrict__ vol;
    __device__ __forceinline__ TexelSource(const KParams& p, const BwdView& vw)
        : vol(tex_offset(static_cast<const TexT*>(p.rgba), static_cast<int64_t>(vw.m) * p.s_mpi)) {}
    template <bool AC, bool STRICT>
    __device__ __forceinline__ void start(BwdPixel& bp, const KParams& p, const BwdView& vw, const BwdParams& b, int n, int px, int py, bool active) const {
        bwd_pixel_setup<TexT, AC, true>(bp, p, vw, n, px, py, active, b.g_rgb, b.g_depth, b.g_T, vol);
    }
    __device__ __forceinline__ static float chan(uint32_t t, int c) { return unorm8_to_f32(texel_code(t, c)); }
    template <typename T>
    __device__ __forceinline__ static float chan(const T& t, int c) { return to_f32(t.c[c]); }
    template <bool STRICT>
    __device__ __forceinline__ bool taps(const KParams& p, int k, int Ht, int Wt, float ix, float iy, Taps& q) const {
        constexpr int64_t kTexel = sizeof(TexT);
        const TexT* __restrict__ pl = tex_offset(vol, static_cast<int64_t>(k) * p.s_plane);
        const TapPos tp = tap_pos(Ht, Wt, ix, iy, q);
        const int64_t oa = static_cast<int64_t>(tp.ya) * p.s_row, ob = static_cast<int64_t>(tp.yb) * p.s_row;
        const auto t_nw = load_texel(pl, oa + kTexel * tp.xa), t_ne = load_texel(pl, oa + kTexel * tp.xb);
        const auto t_sw = load_texel(pl, ob + kTexel * tp.xa), t_se = load_texel(pl, ob + kTexel * tp.xb);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float v[4] = {chan(t_nw, c), chan(t_ne, c), chan(t_sw, c), chan(t_se, c)};
            pad_taps(tp, v, q.t[c]);
        }
        return true;
    }
};

// the colour image of plane k of MPI m: rgb, or the background on the last plane (uniform per plane)
template <typename TexT>
struct ColourImages {
    const TexT* __restrict__ rgb;
    const TexT* __restrict__ bgi;
    int64_t rs_chan, rs_row, bs_chan, bs_row;
    __device__ __forceinline__ ColourImages(const SharedK& sh, int m)
        : rgb(static_cast<const TexT*>(sh.rgb) + static_cast<int64_t>(m) * sh.rs_mpi),
          bgi(sh.bg ? static_cast<const TexT*>(sh.bg) + static_cast<int64_t>(m) * sh.bs_mpi : nullptr),
          rs_chan(sh.rs_chan), rs_row(sh.rs_row), bs_chan(sh.bs_chan), bs_row(sh.bs_row) {}
    __device__ __forceinline__ void taps(int k, int D, const TapPos& tp, Taps& q) const {
        const bool last_bg = bgi != nullptr && k == D - 1;
        const TexT* __restrict__ col = last_bg ? bgi : rgb;
        const int64_t c_chan = last_bg ? bs_chan : rs_chan, c_row = last_bg ? bs_row : rs_row;
#pragma unroll
        for (int c = 0; c < 3; ++c) gather_channel<TexT>(col + c * c_chan, c_row, tp, q.t[c]);
    }
};

template <typename TexT>
struct SharedSource {
    static constexpr bool kSkips = false;
    static constexpr bool kPlaneZ = false;
    static constexpr bool kForwardAlpha = false;   // (the volume path's sweep exactly)
    const TexT* __restrict__ alpha;   // KParams' volume fields: the alpha planes, s_chan = 0
    ColourImages<TexT> col;
    __device__ __forceinline__ SharedSource(const KParams& p, const BwdView& vw, const SharedK& sh)
        : alpha(static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(vw.m) * p.s_mpi), col(sh, vw.m) {}
    template <bool AC, bool STRICT>
    __device__ __forceinline__ void start(BwdPixel& bp, const KParams& p, const BwdView& vw, const BwdParams& b, int n, int px, int py, bool active) const {
        bwd_pixel_setup<TexT, AC, true>(bp, p, vw, n, px, py, active, b.g_rgb, b.g_depth, b.g_T, alpha);   // (the shared backward's setup)
    }
    template <bool STRICT>
    __device__ __forceinline__ bool taps(const KParams& p, int k, int Ht, int Wt, float ix, float iy, Taps& q) const {
        const TapPos tp = tap_pos(Ht, Wt, ix, iy, q);
        col.taps(k, p.D, tp, q);
        gather_channel<TexT>(alpha + static_cast<int64_t>(k) * p.s_plane, p.s_row, tp, q.t[3]);
        return true;
    }
};

// The tag that selects the PZ instances of the frame (the last of Extra; the depth-alpha layout only): the plane's share of dL/d plane_z too.
struct PlaneZGrad {};

template <typename TexT, bool PZ = false>
struct DepthSource {
    static constexpr bool kSkips = true;
    static constexpr bool kForwardAlpha = true;    // strict-order mode: bilerp<true> of the ramp taps, as render_depth_kernel
    static constexpr bool kPlaneZ = PZ;
    const TexT* __restrict__ depth;   // KParams' volume fields: the depth image (s_plane, s_chan unused)
    const float* __restrict__ pz;
    DepthK dk;
    ColourImages<TexT> col;
    __device__ __forceinline__ DepthSource(const KParams& p, const BwdView& vw, const SharedK& sh, const DepthK& d, PlaneZGrad = {})
        : depth(static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(vw.m) * p.s_mpi),
          pz(d.plane_z + static_cast<int64_t>(vw.m) * d.pz_stride), dk(d), col(sh, vw.m) {}
    template <bool AC, bool STRICT>
    __device__ __forceinline__ void start(BwdPixel& bp, const KParams& p, const BwdView& vw, const BwdParams& b, int n, int px, int py, bool active) const {
        bwd_pixel_setup_with<true>(bp, p, vw, n, px, py, active, b.g_rgb, b.g_depth, b.g_T,
                                   [&](float t_fwd) { return depth_total_transmittance<TexT, AC, STRICT>(p, vw, bp, depth, pz, dk, t_fwd); });
    }
    template <bool STRICT>
    __device__ __forceinline__ bool taps(const KParams& p, int k, int Ht, int Wt, float ix, float iy, Taps& q) const {
        const TapPos tp = tap_pos(Ht, Wt, ix, iy, q);
        float d[4], a[4];
        load_taps<TexT>(depth, p.s_row, tp, d);
        const float z = pz[k];
        bool inside;
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = depth_ramp<STRICT>(z, d[i], dk, inside);
        pad_taps(tp, a, q.t[3]);
        // (a NaN ramp value compares unequal to 0: such a plane is swept, as on the expanded volume)
        if (q.t[3][0] == 0.0f && q.t[3][1] == 0.0f && q.t[3][2] == 0.0f && q.t[3][3] == 0.0f) return false;
        col.taps(k, p.D, tp, q);
        return true;
    }
    // The PZ instances' form: on[i] says whether tap i lies inside the texture AND on the ramp (depth_ramp's `inside`, bounds included: where
    // torch.clamp passes the gradient, d a_i / d plane_z = 1 / den).  A tap exactly on the lower bound has alpha 0 and is on the ramp: the
    // plane is skipped only when, besides four zero ramp taps, no tap is on the ramp (the image backward's rule, render_depth.hip).
    template <bool STRICT>
    __device__ __forceinline__ bool taps(const KParams& p, int k, int Ht, int Wt, float ix, float iy, Taps& q, bool (&on)[4]) const {
        const TapPos tp = tap_pos(Ht, Wt, ix, iy, q);
        float d[4], a[4];
        load_taps<TexT>(depth, p.s_row, tp, d);
        const float z = pz[k];
        bool in[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = depth_ramp<STRICT>(z, d[i], dk, in[i]);
        pad_taps(tp, a, q.t[3]);
        on[0] = tp.nw && in[0], on[1] = tp.ne && in[1], on[2] = tp.sw && in[2], on[3] = tp.se && in[3];
        if (q.t[3][0] == 0.0f && q.t[3][1] == 0.0f && q.t[3][2] == 0.0f && q.t[3][3] == 0.0f && !(on[0] || on[1] || on[2] || on[3])) return false;
        col.taps(k, p.D, tp, q);
        return true;
    }
};

template <typename TexT, typename... Extra> struct SourceOf;
template <typename TexT> struct SourceOf<TexT> { using type = VolumeSource<TexT>; };   // (u8_t too: planar codes, every tap through to_f32(u8_t))
template <> struct SourceOf<rgba8_t> { using type = TexelSource<rgba8_t>; };
template <> struct SourceOf<rgba32f_t> { using type = TexelSource<rgba32f_t>; };
template <> struct SourceOf<rgba16h_t> { using type = TexelSource<rgba16h_t>; };
template <> struct SourceOf<rgba16b_t> { using type = TexelSource<rgba16b_t>; };
template <typename TexT> struct SourceOf<TexT, SharedK> { using type = SharedSource<TexT>; };
template <typename TexT> struct SourceOf<TexT, SharedK, DepthK> { using type = DepthSource<TexT>; };
template <typename TexT> struct SourceOf<TexT, SharedK, DepthK, PlaneZGrad> { using type = DepthSource<TexT, true>; };

// Slab layout (floats): component j of tile t of view n at ws[(j * N + n) * T + t];  j = 0..2 eye, 3..5 z_dir, 6 + 3k + (0, 1, 2) = plane k's
// (d, h, w); the PZ instances add one component per plane BEHIND those, 6 + (3D with dhw, else 0) + k = plane k's plane_z sum (times den), so that
// the layout without plane_z is what it was.  Every slot is written by exactly one workgroup.
//
// The frame.  Extra: the layout's structs -- none: the RGBA volume; SharedK: the shared-colour layout; SharedK, DepthK: the depth-alpha layout;
// SharedK, DepthK, PlaneZGrad: the depth-alpha layout with the gradient w.r.t. plane_z (the PZ instances: one more wave sum and slab component per
// plane, and the wider skip rule of DepthSource's second taps()) -- which select the tap source (SourceOf).
template <typename TexT, bool AC, bool STRICT, bool DHW, typename... Extra>
__global__ __launch_bounds__(kGT) void geometry_pixel_kernel(const KParams p, const BwdParams b, float* __restrict__ g_ray, float* __restrict__ slab,
                                                             const int tiles_x, const int n_tiles, const Extra... extra) {
    using Src = typename SourceOf<TexT, Extra...>::type;
    constexpr bool PZ = Src::kPlaneZ;                  // the plane_z term too (the instances with the PlaneZGrad tag)
    constexpr int kSums = (DHW ? 3 : 0) + (PZ ? 1 : 0);   // wave sums per plane: (d, h, w), then plane_z
    __shared__ float4 pcA[kGChunk];                    // zdiff, w, h, RN(2/w)
    __shared__ float pcB[kGChunk];                     // RN(2/h)
    __shared__ float red[kSums ? kGWaves * kGChunk * kSums : 1];   // per wave and plane: (d, h, w) and plane_z partial sums
    __shared__ float red6[kGWaves * 6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.y;
    const int tile = xcd_item_per_group(static_cast<int>(blockIdx.x), n_tiles, n_tiles);
    if (tile >= n_tiles) return;
    const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    const int px = txi * kGTW + lane, py = tyi * kGTH + wave;
    const bool active = px < p.W && py < p.H;
    const BwdView vw = bwd_view<AC>(p, n);
    const float* __restrict__ dhw = vw.dhw;
    const float ex = vw.ex, ey = vw.ey, cx = vw.cx, cy = vw.cy;
    const int64_t HW = vw.HW;
    const int Ht = p.Ht, Wt = p.Wt;
    const float rWt = 1.0f / static_cast<float>(Wt), rHt = 1.0f / static_cast<float>(Ht);
    const Src src(p, vw, extra...);
    BwdPixel bp;
    src.template start<AC, STRICT>(bp, p, vw, b, n, px, py, active);
    const float rx = bp.rx, ry = bp.ry, rz = bp.rz, rrz = bp.rrz, dot = bp.dot;
    float sx = 0.0f, sy = 0.0f, ss = 0.0f;      // sum_k g_x, g_y, g_s
    float srx = 0.0f, sry = 0.0f, srz = 0.0f;   // sum_k g_x s, g_y s, g_s s
    float sG = 0.0f;                            // sum_k G_k s

    const int64_t ncomp_stride = static_cast<int64_t>(p.N) * n_tiles;   // slab: distance between two components
    for (int kend = p.D; kend > 0; kend -= kGChunk) {  // chunks of planes, last chunk first
        const int kc = max(kend - kGChunk, 0), kn = kend - kc;
        __syncthreads();
        for (int t = tid; t < kn; t += kGT) {
            const int k = kc + t;
            const float pw = dhw[3 * k + 2], ph = dhw[3 * k + 1];
            pcA[t] = make_float4(dhw[3 * k] - vw.ez, pw, ph, 1.0f / (pw * 0.5f));
            pcB[t] = 1.0f / (ph * 0.5f);
        }
        __syncthreads();
        for (int t = kn - 1; t >= 0; --t) {
            const float4 a = pcA[t];
            const float rw = a.w, rh = pcB[t];
            float ix, iy, s;
            if (STRICT) {   // the forward's chain in strict-order mode (compiler divisions)
                float u, v;
                plane_coord<AC>(a.x, a.z, a.y, ex, ey, rx, ry, rz, cx, cy, ix, iy, s, u, v);
            } else {        // the default mode's chain: the same quotients through hoisted reciprocals
                plane_coord_recip<AC>(a.x, a.y * 0.5f, a.z * 0.5f, rw, rh, ex, ey, rx, ry, rz, rrz, cx, cy, ix, iy, s);
            }
            Taps q;
            float vd = 0.0f, vh = 0.0f, vw_ = 0.0f;   // this pixel's share of the plane's (d, h, w) sums
            float vz = 0.0f;                          // ... and of its plane_z sum (times den)
            bool on[4];                               // PZ: the taps inside the texture and on the ramp
            bool live;
            if constexpr (PZ) live = src.template taps<STRICT>(p, kc + t, Ht, Wt, ix, iy, q, on);
            else live = src.template taps<STRICT>(p, kc + t, Ht, Wt, ix, iy, q);
            if (!Src::kSkips || live) {   // (false: the plane is the identity of this pixel's sweep)
                const float w00 = q.wx0 * q.wy0, w01 = q.wx1 * q.wy0, w10 = q.wx0 * q.wy1, w11 = q.wx1 * q.wy1;
                float smp[4], dix[4], diy[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float acc = q.t[c][0] * w00;
                    acc = __builtin_fmaf(q.t[c][1], w01, acc);
                    acc = __builtin_fmaf(q.t[c][2], w10, acc);
                    smp[c] = __builtin_fmaf(q.t[c][3], w11, acc);
                    dix[c] = __builtin_fmaf(q.t[c][3] - q.t[c][2], q.wy1, (q.t[c][1] - q.t[c][0]) * q.wy0);
                    diy[c] = __builtin_fmaf(q.t[c][3] - q.t[c][1], q.wx1, (q.t[c][2] - q.t[c][0]) * q.wx0);
                }
                // (the strict-order forward of this layout rounds its alpha sample once per op: the sweep divides T_out by THAT om)
            if (STRICT && Src::kForwardAlpha) smp[3] = ((q.t[3][0] * w00 + q.t[3][1] * w01) + q.t[3][2] * w10) + q.t[3][3] * w11;
            // the sweep: T_k = T_{k+1} / om_k, sample gradients d_s
                float d_s[4];
                const float w = bp.plane_recip(smp, s, d_s);   // w_k = a_k T_k
                const float d0 = d_s[0], d1 = d_s[1], d2 = d_s[2], d3 = d_s[3];
                // position gradient
                const float g_ix = d0 * dix[0] + d1 * dix[1] + d2 * dix[2] + d3 * dix[3];
                const float g_iy = d0 * diy[0] + d1 * diy[1] + d2 * diy[2] + d3 * diy[3];
                float kx = cx, ky = cy;   // dix/du' (AC: (Wt-1)/2; else Wt/2 times the narrowing factor c of u' = c u)
                if (!AC) {
                    const float uu = (2.0f * ix + 1.0f) * rWt - 1.0f, vv = (2.0f * iy + 1.0f) * rHt - 1.0f;   // u' (|u'| <= 0.95 iff narrowed, else > 1)
                    kx = 0.5f * cx * (fabsf(uu) <= 0.975f ? kNarrowScale : 1.0f);
                    ky = 0.5f * cy * (fabsf(vv) <= 0.975f ? kNarrowScale : 1.0f);
                }
                const float g_x = g_ix * (kx * rw), g_y = g_iy * (ky * rh);   // du/dx = 2/w = rw
                const float Gk = bp.gz * w;
                const float g_s = g_x * rx + g_y * ry + Gk * dot;
                sx += g_x, sy += g_y, ss += g_s;
                srx += g_x * s, sry += g_y * s, srz += g_s * s;
                sG += Gk * s;
                if (DHW) {
                    const float x = ex + rx * s, y = ey + ry * s;
                    vd = g_s * rrz, vh = -0.5f * g_y * y * rh, vw_ = -0.5f * g_x * x * rw;   // d(2x/w)/dw = -(2/w)(x/w)
                    vd = active ? vd : 0.0f, vh = active ? vh : 0.0f, vw_ = active ? vw_ : 0.0f;
                }
                if constexpr (PZ) {   // d a_i / d plane_z = 1 / den on the ramp: d_s[3] sum_i w_i on_i (the reducer divides by den, once)
                    const float wz = (((on[0] ? w00 : 0.0f) + (on[1] ? w01 : 0.0f)) + (on[2] ? w10 : 0.0f)) + (on[3] ? w11 : 0.0f);
                    vz = active ? d3 * wz : 0.0f;
                }
            }
            if (DHW) {   // (every lane of the wave, skipped planes included: the wave sums are cross-lane)
                vd = wave_sum(vd), vh = wave_sum(vh), vw_ = wave_sum(vw_);
                if (lane == 0) {
                    float* o = red + (wave * kGChunk + t) * kSums;
                    o[0] = vd, o[1] = vh, o[2] = vw_;
                }
            }
            if constexpr (PZ) {
                vz = wave_sum(vz);
                if (lane == 0) red[(wave * kGChunk + t) * kSums + (kSums - 1)] = vz;
            }
        }
        if constexpr (kSums != 0) if (slab != nullptr) {   // this chunk's plane sums: the waves in order, one slot per (component, plane)
            __syncthreads();
            for (int i = tid; i < kSums * kn; i += kGT) {
                const int t = i / kSums, j = i - kSums * t;
                float v = red[t * kSums + j];
#pragma unroll
                for (int wv = 1; wv < kGWaves; ++wv) v += red[(wv * kGChunk + t) * kSums + j];
                int64_t comp = 6 + 3 * static_cast<int64_t>(kc + t) + j;
                if (PZ && j == kSums - 1) comp = 6 + (DHW ? 3 * static_cast<int64_t>(p.D) : 0) + (kc + t);   // behind the (d, h, w) components
                slab[comp * ncomp_stride + static_cast<int64_t>(n) * n_tiles + tile] = v;
            }
        }
    }
    if (active && g_ray != nullptr) {
        float* o = g_ray + static_cast<int64_t>(n) * 3 * HW + bp.pix;
        o[0] = srx + sG * bp.zx;
        o[HW] = sry + sG * bp.zy;
        o[2 * HW] = -srz * rrz + sG * bp.zz;
    }
    if (slab != nullptr) {
        float v[6] = {sx, sy, -ss * rrz, sG * rx, sG * ry, sG * rz};
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const float s = wave_sum(active ? v[j] : 0.0f);
            if (lane == 0) red6[wave * 6 + j] = s;
        }
        __syncthreads();
        if (tid < 6) {
            float s = red6[tid];
#pragma unroll
            for (int wv = 1; wv < kGWaves; ++wv) s += red6[wv * 6 + tid];
            slab[static_cast<int64_t>(tid) * ncomp_stride + static_cast<int64_t>(n) * n_tiles + tile] = s;
        }
    }
}

// The slab sums.  Block (j, i): component j of view i (j < 6: eye, z_dir) or of MPI i (j >= 6: plane geometry, summed over every view of the MPI
// in view order).  Each thread sums a fixed stride of the slots, then a fixed LDS tree: the same bits on every run.
__global__ __launch_bounds__(kGRed) void geometry_reduce_kernel(const KParams p, const float* __restrict__ slab, const int n_tiles, float* __restrict__ g_eye,
                                                                float* __restrict__ g_z, float* __restrict__ g_dhw) {
    __shared__ float part[kGRed];
    const int j = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
    const bool per_view = j < 6;
    if (per_view ? i >= p.N : i >= p.M) return;
    float* out = per_view ? (j < 3 ? g_eye : g_z) : g_dhw;
    if (out == nullptr) return;
    const int64_t cs = static_cast<int64_t>(p.N) * n_tiles;
    const float* __restrict__ comp = slab + static_cast<int64_t>(j) * cs;
    float acc = 0.0f;
    if (per_view) {
        for (int t = tid; t < n_tiles; t += kGRed) acc += comp[static_cast<int64_t>(i) * n_tiles + t];
    } else {
        for (int n = 0; n < p.N; ++n) {
            uint32_t bad = 0;
            if (view_mpi(p, n, bad) != i) continue;
            for (int t = tid; t < n_tiles; t += kGRed) acc += comp[static_cast<int64_t>(n) * n_tiles + t];
        }
    }
    part[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int w = kGRed / 2; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        if (per_view) out[3 * i + (j % 3)] = part[0];
        else out[static_cast<int64_t>(i) * p.D * 3 + (j - 6)] = part[0];
    }
}

// The plane_z sums (the PZ instances' components; comp0 = the first of them).  Block (k, i): plane k of MPI i, summed over every view of the MPI in
// view order, or (per_mpi false: ONE table for all MPIs) over all views in view order; the same strided sums and LDS tree, then 1 / den, once.
__global__ __launch_bounds__(kGRed) void plane_z_reduce_kernel(const KParams p, const float* __restrict__ comp0, const int n_tiles, const bool per_mpi,
                                                               const float den, float* __restrict__ g_pz) {
    __shared__ float part[kGRed];
    const int k = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
    const float* __restrict__ comp = comp0 + static_cast<int64_t>(k) * p.N * n_tiles;
    float acc = 0.0f;
    for (int n = 0; n < p.N; ++n) {
        uint32_t bad = 0;
        if (per_mpi && view_mpi(p, n, bad) != i) continue;
        for (int t = tid; t < n_tiles; t += kGRed) acc += comp[static_cast<int64_t>(n) * n_tiles + t];
    }
    part[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int w = kGRed / 2; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) g_pz[static_cast<int64_t>(i) * p.D + k] = part[0] / den;
}

static int tiles_x_of(const KParams& p) { return (p.W + kGTW - 1) / kGTW; }
static int tiles_of(const KParams& p) { return tiles_x_of(p) * ((p.H + kGTH - 1) / kGTH); }

}  // namespace bwgeo

uint64_t geometry_backward_workspace_bytes(const KParams& p, bool want_dhw, bool want_plane_z) {
    const uint64_t comps = 6u + (want_dhw ? 3u * static_cast<uint64_t>(p.D) : 0u);
    const uint64_t slots = p.N * static_cast<uint64_t>(bwgeo::tiles_of(p)) * sizeof(float);   // bytes per component
    // (the plane_z components lie directly behind the others; their bytes are rounded up on their own, so that asking for them always asks for more)
    return (comps * slots + 255) / 256 * 256 + (want_plane_z ? (p.D * slots + 255) / 256 * 256 : 0u);
}

// g_ray [N,3,H,W], g_eye / g_z [N,3], g_dhw [M,D,3]: overwritten; nullptr = not wanted.  p.ws must hold geometry_backward_workspace_bytes(p,
// g_dhw != nullptr, pz != nullptr) bytes when any of g_eye, g_z, g_dhw, the plane_z gradient is wanted (checked by the caller).  pixel(type, AC,
// STRICT, DHW, grid, b, slab, tiles_x, n_tiles) launches the layout's pixel kernel; the slab reducer is the same for all.  pz: the depth-alpha
// layout's DepthK when the gradient w.r.t. plane_z is wanted (g_pz [M,D], or [D] for one table: overwritten; `pixel` launches a PZ instance).
// types(f): calls f(TypeTag<storage type>{}) for the launch's storage type -- dispatch_dtype for the planar float volumes, the storage formats read in place below.
template <typename Types, typename Pixel>
static hipError_t launch_geometry_passes_over(const KParams& p, Types&& types, const float* g_rgb, const float* g_depth, const float* g_T, float* g_eye, float* g_z,
                                              float* g_dhw, hipStream_t stream, Pixel&& pixel, const DepthK* pz = nullptr, float* g_pz = nullptr) {
    using namespace bwgeo;
    BwdParams b{};
    b.g_rgb = g_rgb, b.g_depth = g_depth, b.g_T = g_T;
    const bool want_dhw = g_dhw != nullptr;
    float* slab = (g_eye || g_z || g_dhw || g_pz) ? static_cast<float*>(p.ws) : nullptr;
    const int tx = tiles_x_of(p), nt = tiles_of(p);
    const dim3 grid(xcd_grid_per_group(nt, nt), p.N);
    types([&](auto t) {
        dispatch_bool(p.flags & GMPI_FLAG_ALIGN_CORNERS, [&](auto AC) {
            dispatch_bool(p.flags & GMPI_FLAG_STRICT_ORDER, [&](auto STRICT) {
                dispatch_bool(want_dhw, [&](auto DHW) { pixel(t, AC, STRICT, DHW, grid, b, slab, tx, nt); });
            });
        });
    });
    if (g_eye || g_z || g_dhw) {
        const dim3 rgrid(6 + (want_dhw ? 3 * p.D : 0), std::max(p.N, p.M));
        hipLaunchKernelGGL(geometry_reduce_kernel, rgrid, dim3(kGRed), 0, stream, p, slab, nt, g_eye, g_z, g_dhw);
    }
    if (g_pz != nullptr) {
        const bool per_mpi = pz->pz_stride != 0;
        const float* comp0 = slab + (6 + (want_dhw ? 3 * static_cast<int64_t>(p.D) : 0)) * p.N * nt;
        hipLaunchKernelGGL(plane_z_reduce_kernel, dim3(p.D, per_mpi ? p.M : 1), dim3(kGRed), 0, stream, p, comp0, nt, per_mpi, pz->den, g_pz);
    }
    return hipGetLastError();
}
template <typename Pixel>
static hipError_t launch_geometry_passes(const KParams& p, int dtype, const float* g_rgb, const float* g_depth, const float* g_T, float* g_eye, float* g_z,
                                         float* g_dhw, hipStream_t stream, Pixel&& pixel, const DepthK* pz = nullptr, float* g_pz = nullptr) {
    return launch_geometry_passes_over(p, [&](auto&& f) { dispatch_dtype(dtype, f); }, g_rgb, g_depth, g_T, g_eye, g_z, g_dhw, stream, pixel, pz, g_pz);
}
#define GMPI_GEOMETRY_INSTANCE(kernel, ...) kernel<typename decltype(t)::type, decltype(AC)::value, decltype(STRICT)::value, decltype(DHW)::value, ##__VA_ARGS__>

hipError_t launch_backward_geometry(const KParams& p, int dtype, const float* g_rgb, const float* g_depth, const float* g_T, float* g_ray, float* g_eye,
                                    float* g_z, float* g_dhw, hipStream_t stream) {
    return launch_geometry_passes(p, dtype, g_rgb, g_depth, g_T, g_eye, g_z, g_dhw, stream,
                                  [&](auto t, auto AC, auto STRICT, auto DHW, dim3 grid, const BwdParams& b, float* slab, int tx, int nt) {
        hipLaunchKernelGGL((GMPI_GEOMETRY_INSTANCE(bwgeo::geometry_pixel_kernel)), grid, dim3(bwgeo::kGT), 0, stream, p, b, g_ray, slab, tx, nt);
    });
}

// The same passes over the RGBA volume in the formats it is STORED in, read in place: dtype GMPI_DTYPE_U8 -- planar codes (u8_t: VolumeSource) or, when
// to_kparams marked the strides channels-last (u8_interleaved), packed texels (rgba8_t) -- or, layers: channels-last float layers (rgba32f_t /
// rgba16h_t / rgba16b_t; p's strides in bytes, as to_kparams_layers leaves them).  The frame, the tiles, the slabs and the reducer are the volume's.
hipError_t launch_backward_geometry_inplace(const KParams& p, int dtype, bool layers, const float* g_rgb, const float* g_depth, const float* g_T, float* g_ray,
                                            float* g_eye, float* g_z, float* g_dhw, hipStream_t stream) {
    if (layers ? (dtype != GMPI_DTYPE_F32 && dtype != GMPI_DTYPE_F16 && dtype != GMPI_DTYPE_BF16) : dtype != GMPI_DTYPE_U8) return hipErrorInvalidValue;
    auto types = [&](auto&& f) {
        if (!layers) return u8_interleaved(p) ? f(TypeTag<rgba8_t>{}) : f(TypeTag<u8_t>{});
        if (dtype == GMPI_DTYPE_F32) return f(TypeTag<rgba32f_t>{});
        return dtype == GMPI_DTYPE_F16 ? f(TypeTag<rgba16h_t>{}) : f(TypeTag<rgba16b_t>{});
    };
    return launch_geometry_passes_over(p, types, g_rgb, g_depth, g_T, g_eye, g_z, g_dhw, stream,
                                       [&](auto t, auto AC, auto STRICT, auto DHW, dim3 grid, const BwdParams& b, float* slab, int tx, int nt) {
        hipLaunchKernelGGL((GMPI_GEOMETRY_INSTANCE(bwgeo::geometry_pixel_kernel)), grid, dim3(bwgeo::kGT), 0, stream, p, b, g_ray, slab, tx, nt);
    });
}

// The same passes over the shared-colour layout (dk == nullptr; p carries the alpha planes, s_chan = 0) and the depth-alpha layout (p carries the
// depth image; g_pz: its gradient w.r.t. plane_z, [M,D] or, with one table for all MPIs, [D]; nullptr = not wanted: today's instances).
hipError_t launch_backward_geometry_layout(const KParams& p, int dtype, const SharedK& sh, const DepthK* dk, const float* g_rgb, const float* g_depth,
                                           const float* g_T, float* g_ray, float* g_eye, float* g_z, float* g_dhw, float* g_pz, hipStream_t stream) {
    if (dk == nullptr) g_pz = nullptr;
    return launch_geometry_passes(p, dtype, g_rgb, g_depth, g_T, g_eye, g_z, g_dhw, stream,
                                  [&](auto t, auto AC, auto STRICT, auto DHW, dim3 grid, const BwdParams& b, float* slab, int tx, int nt) {
        if (g_pz != nullptr) {
            hipLaunchKernelGGL((GMPI_GEOMETRY_INSTANCE(bwgeo::geometry_pixel_kernel, SharedK, DepthK, bwgeo::PlaneZGrad)), grid, dim3(bwgeo::kGT), 0, stream, p, b,
                               g_ray, slab, tx, nt, sh, *dk, bwgeo::PlaneZGrad{});
        } else if (dk != nullptr) {
            hipLaunchKernelGGL((GMPI_GEOMETRY_INSTANCE(bwgeo::geometry_pixel_kernel, SharedK, DepthK)), grid, dim3(bwgeo::kGT), 0, stream, p, b, g_ray, slab, tx, nt, sh, *dk);
        } else {
            hipLaunchKernelGGL((GMPI_GEOMETRY_INSTANCE(bwgeo::geometry_pixel_kernel, SharedK)), grid, dim3(bwgeo::kGT), 0, stream, p, b, g_ray, slab, tx, nt, sh);
        }
    }, dk, g_pz);
}
#undef GMPI_GEOMETRY_INSTANCE

}  // namespace gmpi
