// render_backward_gather.hip -- the backward of the render WITHOUT atomics (round 6): gradient of the fused render w.r.t. the RGBA volume
// (the reference's G-step back-propagates through MPIRenderer.render into the generator: gmpi/train.py:740-779; the sampling grid carries no
// gradient, gmpi/core/mpi.py:65).
//
// Why.  The tile kernel (render_backward.hip) scatters every pixel's sample gradients into a copy of its tile's texel box in LDS and flushes the box
// with one global atomic per texel: it runs AT the part's rate for atomic 64-byte segments (20.8 G/s: profiles/r05_backward.txt, r06_backward.txt --
// 2.12 ms at 1024^2 x 32 x 4 where the launch without its global writes takes 1.27), needs a zero-filled gradient volume (0.32 ms) and, with the
// write path behind the L2s as the shared resource, cannot be helped by storing what a tile owns (built and measured in round 6).  This file replaces the
// scatter by a GATHER, so that every gradient cell is written exactly once, by the one workgroup that owns it:
//   pass 1 (pixel_pass_kernel), pixel-stationary: the back-to-front sweep of the tile kernel (gmpi_backward.hpp: the same functions), but instead of
//           scattering, every pixel WRITES its four sample gradients d_s = dL/d(r, g, b, alpha sample) per plane: G[n][k][py][px], 16 bytes,
//           coalesced -- no LDS boxes, no barriers in the plane loop, no flush waves;
//   pass 2 (texel_gather_kernel), texel-stationary: a workgroup owns a 64 x 16 texel tile of one plane of one MPI.  The pixels whose bilinear
//           footprint can touch the tile lie in the pre-image of the tile (grown by one texel) under the plane's homography; the workgroup stages
//           their exact sample positions -- recomputed with the forward's own coordinate chain -- and their d_s in LDS, and every texel sums
//           w(ix - x) w(iy - y) d_s over its candidates, w(t) = max(0, 1 - |t|): exactly the cells, weights and zeros padding of
//           F.grid_sample's backward, in a fixed order (the result is deterministic, which the atomics never were).  Membership is decided by the
//           exact positions; the homography only has to bound where to look.
// The homography pixel -> texel of a (view, plane) is solved in fp64 from the images of the four image-corner pixels (homography_kernel: a pinhole ray
// field maps pixel lines to lines -- the assumption every staged kernel of this library makes, include/gmpi_render.h); a (view, plane) whose solve is
// not trustworthy (degenerate rays, a plane behind the camera) is marked and its texel tiles look at EVERY pixel of the view: slow, still exact.
// align_corners = True only (mpi.py:98-99 makes the other mode's map discontinuous at |u| = 1: the tile kernel keeps that mode), uniform views per
// MPI (several views of one MPI are summed in registers), a workspace of N D H W 16 bytes lent by the caller (gmpi_render_backward_workspace_bytes).
// The same pair serves the shared-colour and depth-alpha layouts (section 4 below: gmpi_mpi_render_shared_backward_gather_launch /
// gmpi_mpi_render_depth_backward_gather_launch): the texel pass is ONE body, texel_gather_run, with what happens to a plane's sums as a policy (the sink).
#include "gmpi_backward.hpp"
#include "gmpi_shared.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>

namespace gmpi {
namespace bwdg {

typedef float f32x4 __attribute__((ext_vector_type(4)));   // (the element types of the sample-gradient and sample-position buffers: the non-temporal
typedef float f32x2 __attribute__((ext_vector_type(2)));   //  builtins want vector types)

// per (view, plane): the INVERSE homography texel -> pixel,  px = (a x + b y + c) / den,  py = (d x + e y + f) / den,  den = g x + h y + 1
struct HRec {
    float a, b, c, d, e, f, g, h;
    float valid;   // 1: usable; 0: look at every pixel
    float pad[3];
};
static_assert(sizeof(HRec) == 48, "record");

// ---- 1. homography of every (view, plane) ------------------------------------------------------------------------------------------------------------
// Closed form (unit square -> quadrilateral, Heckbert 1989) in fp64 from the exact images of the four image-corner pixels, then the adjugate: straight-line
// code, a few microseconds for the whole launch.  (A first version solved the 8 x 8 DLT system by Gaussian elimination out of scratch memory: 81 us.)
template <bool AC>
__global__ __launch_bounds__(64) void homography_kernel(const KParams p, HRec* __restrict__ recs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N * p.D) return;
    const int n = i / p.D, k = i - n * p.D;
    uint32_t bad_index = 0;
    const int m = view_mpi(p, n, bad_index);
    const float* __restrict__ dhw = p.dhw + (static_cast<int64_t>(m) * p.D + k) * 3;
    const float ex = p.eye_pos[3 * n + 0], ey = p.eye_pos[3 * n + 1], ez = p.eye_pos[3 * n + 2];
    const int64_t HW = static_cast<int64_t>(p.H) * p.W;
    const float* __restrict__ rdv = p.ray_dir + static_cast<int64_t>(n) * 3 * HW;
    const float cx = AC ? static_cast<float>(p.Wt - 1) * 0.5f : static_cast<float>(p.Wt), cy = AC ? static_cast<float>(p.Ht - 1) * 0.5f : static_cast<float>(p.Ht);
    HRec r{};
    r.valid = 0.0f;
    bool ok = p.W >= 2 && p.H >= 2;
    double X[4], Y[4];   // images of the pixels (0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1): the unit square's corners in order
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int qx = (c == 1 || c == 2) ? p.W - 1 : 0, qy = (c >= 2) ? p.H - 1 : 0;
        const int64_t q = static_cast<int64_t>(qy) * p.W + qx;
        float ix, iy, s, u, v;
        plane_coord<AC>(dhw[0] - ez, dhw[1], dhw[2], ex, ey, rdv[q], rdv[HW + q], rdv[2 * HW + q], cx, cy, ix, iy, s, u, v);
        ok = ok && fabsf(ix) < 1e6f && fabsf(iy) < 1e6f && s > 0.0f;   // (NaN fails; s > 0: the corner pixel sees the plane in front of the camera)
        X[c] = ix, Y[c] = iy;
    }
    if (ok) {
        // (u, v) in the unit square -> texel:  X = (a u + b v + c) / (g u + h v + 1), Y = (d u + e v + f) / (g u + h v + 1)
        const double sx = X[0] - X[1] + X[2] - X[3], sy = Y[0] - Y[1] + Y[2] - Y[3];
        const double dx1 = X[1] - X[2], dx2 = X[3] - X[2], dy1 = Y[1] - Y[2], dy2 = Y[3] - Y[2];
        const double den = dx1 * dy2 - dx2 * dy1;
        ok = fabs(den) > 1e-12;
        if (ok) {
            const double g = (sx * dy2 - dx2 * sy) / den, hh = (dx1 * sy - sx * dy1) / den;
            // pixel coordinates: u = px / (W - 1), v = py / (H - 1)
            const double iu = 1.0 / (p.W - 1), iv_ = 1.0 / (p.H - 1);
            double h[9];
            h[0] = (X[1] - X[0] + g * X[1]) * iu, h[1] = (X[3] - X[0] + hh * X[3]) * iv_, h[2] = X[0];
            h[3] = (Y[1] - Y[0] + g * Y[1]) * iu, h[4] = (Y[3] - Y[0] + hh * Y[3]) * iv_, h[5] = Y[0];
            h[6] = g * iu, h[7] = hh * iv_, h[8] = 1.0;
            // the forward denominators at the four corners must be positive (no pixel line of the image passes through the map's pole)
            ok = ok && 1.0 > 1e-6 && g + 1.0 > 1e-6 && g + hh + 1.0 > 1e-6 && hh + 1.0 > 1e-6;
            // inverse by the adjugate
            const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
            double iv[9];
            iv[0] = h[4] * h[8] - h[5] * h[7], iv[1] = h[2] * h[7] - h[1] * h[8], iv[2] = h[1] * h[5] - h[2] * h[4];
            iv[3] = h[5] * h[6] - h[3] * h[8], iv[4] = h[0] * h[8] - h[2] * h[6], iv[5] = h[2] * h[3] - h[0] * h[5];
            iv[6] = h[3] * h[7] - h[4] * h[6], iv[7] = h[1] * h[6] - h[0] * h[7], iv[8] = h[0] * h[4] - h[1] * h[3];
            ok = ok && fabs(det) > 1e-300 && fabs(iv[8]) > 1e-300;
            if (ok) {
                const double s8 = 1.0 / iv[8];
#pragma unroll
                for (int j = 0; j < 9; ++j) iv[j] *= s8;
                // the inverse takes the corners' images back to the corner pixels, with positive denominators
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double wantx = (c == 1 || c == 2) ? p.W - 1 : 0, wanty = (c >= 2) ? p.H - 1 : 0;
                    const double dn = iv[6] * X[c] + iv[7] * Y[c] + 1.0;
                    ok = ok && dn > 1e-9;
                    const double bx = (iv[0] * X[c] + iv[1] * Y[c] + iv[2]) / dn, by = (iv[3] * X[c] + iv[4] * Y[c] + iv[5]) / dn;
                    ok = ok && fabs(bx - wantx) < 1e-3 && fabs(by - wanty) < 1e-3;
                }
                if (ok) {
                    r.a = static_cast<float>(iv[0]), r.b = static_cast<float>(iv[1]), r.c = static_cast<float>(iv[2]);
                    r.d = static_cast<float>(iv[3]), r.e = static_cast<float>(iv[4]), r.f = static_cast<float>(iv[5]);
                    r.g = static_cast<float>(iv[6]), r.h = static_cast<float>(iv[7]);
                    r.valid = 1.0f;
                }
            }
        }
    }
    recs[i] = r;
}

// ---- 2. pixel pass: the back-to-front sweep; every pixel writes its sample position and its four sample gradients per plane ---------------------------
constexpr int kPT = 512, kPTW = 64, kPTH = 8;   // one pixel per thread; a wave = one pixel row of the tile
constexpr int kPChunk = 96;

template <typename TexT, bool AC>
__global__ __launch_bounds__(kPT, 6) void pixel_pass_kernel(const KParams p, const BwdParams b, f32x2* __restrict__ P, f32x4* __restrict__ G, const int tiles_x) {
    __shared__ float4 pcA[kPChunk];      // zdiff, w/2, h/2, RN(2/w)
    __shared__ float pcB[kPChunk];       // RN(2/h)
    constexpr int kES = static_cast<int>(sizeof(TexT));
    const int tid = threadIdx.x;
    const int n = blockIdx.y;
    const int n_tiles = tiles_x * ((p.H + kPTH - 1) / kPTH);
    const int tile = xcd_item_per_group(static_cast<int>(blockIdx.x), n_tiles, n_tiles);   // XCD x = blockIdx % 8 takes a contiguous run of the view's tiles
    if (tile >= n_tiles) return;
    const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    const int px = txi * kPTW + (tid % kPTW), py = tyi * kPTH + (tid / kPTW);
    const bool active = px < p.W && py < p.H;
    const BwdView vw = bwd_view<AC>(p, n);
    const float* __restrict__ dhw = vw.dhw;
    const int64_t HW = vw.HW;
    const int Ht = p.Ht, Wt = p.Wt;
    const TexT* __restrict__ vol = static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(vw.m) * p.s_mpi;
    const uint32_t s_chan_b = static_cast<uint32_t>(p.s_chan) * kES, s_row_b = static_cast<uint32_t>(p.s_row) * kES;
    BwdPixel bp;
    bwd_pixel_setup<TexT, AC, true>(bp, p, vw, n, px, py, active, b.g_rgb, b.g_depth, b.g_T, vol);
    const int64_t pix = bp.pix;

    struct Tap { PairTaps q; float ix, iy; };   // + the exact sample position (the forward's chain): the texel pass decides membership on it
    auto fetch = [&](int t, int k, Tap& tp) {   // coordinates of this pixel on plane k (chunk-local t) + its 8 pair loads
        pair_tap_coord<AC>(tp.q, bp, vw, pcA[t], pcB[t], Ht, Wt, tp.ix, tp.iy);
        fetch_pair_taps<TexT>(tp.q, vol + static_cast<int64_t>(k) * p.s_plane, s_chan_b, s_row_b, Ht, Wt);
    };
    auto grads = [&](const Tap& tp) -> float4 {   // the taps have landed: bilinear samples, the plane's gradients
        float smp[4], d[4];
        pair_samples(tp.q, Ht, Wt, smp);
        bp.plane_recip(smp, tp.q.s, d);
        return make_float4(d[0], d[1], d[2], d[3]);
    };

    f32x4* __restrict__ Gpix = G + static_cast<int64_t>(n) * p.D * HW + pix;   // + k * HW per plane
    f32x2* __restrict__ Ppix = P + static_cast<int64_t>(n) * p.D * HW + pix;
    for (int kend = p.D; kend > 0; kend -= kPChunk) {  // chunks of planes, last chunk first
        const int kc = max(kend - kPChunk, 0), kn = kend - kc;
        __syncthreads();
        for (int t = tid; t < kn; t += kPT) {
            const int k = kc + t;
            const float hw = dhw[3 * k + 2] * 0.5f, hh = dhw[3 * k + 1] * 0.5f;
            pcA[t] = make_float4(dhw[3 * k] - vw.ez, hw, hh, 1.0f / hw);
            pcB[t] = 1.0f / hh;
        }
        __syncthreads();
        if (active) {   // (no barrier below: a pixel is on its own through the planes; the taps of plane t - 1 fly while plane t's gradients are formed)
            Tap tq;
            fetch(kn - 1, kc + kn - 1, tq);
            for (int t = kn - 1; t >= 0; --t) {
                const f32x2 pv = {tq.ix, tq.iy};
                const float4 d = grads(tq);
                if (t >= 1) fetch(t - 1, kc + t - 1, tq);
                const f32x4 dv = {d.x, d.y, d.z, d.w};
                __builtin_nontemporal_store(pv, Ppix + static_cast<int64_t>(kc + t) * HW);   // (read once, by the texel pass: keep them out of the way of the taps)
                __builtin_nontemporal_store(dv, Gpix + static_cast<int64_t>(kc + t) * HW);
            }
        }
    }
}

// ---- 3. texel pass: every cell of the gradient volume is the sum over the pixels that sampled it -----------------------------------------------------
// A workgroup owns a 64 x 16 texel tile of one MPI over a run of planes; a thread the texels (tx, ty) and (tx, ty + 8).  Per (plane, view) the pixels that
// can reach the tile -- the pre-image of the tile grown by a texel, a convex quadrilateral, as a pixel box -- are staged in LDS (position 8 B + sample
// gradients 16 B) in chunks of up to kCap pixels; the loads of the NEXT chunk (registers) fly while the current one is gathered.
constexpr int kTT = 512, kTX = 64, kTY = 16;
constexpr int kCap = 2048;                          // staged pixels per chunk: 48 KB
constexpr int kSlots = kCap / kTT;                  // pixels a thread moves per chunk
constexpr int kChunkW = 512;                        // widest chunk (a pixel box wider than this is walked in column blocks)

template <typename Rec>
struct ChunkT {   // everything wave-uniform; Rec: the (view, plane)'s record as the sink keeps it (Sink::Rec)
    int k, v, n;             // plane, view of the MPI, view index
    int bx0, by0, cw, ch;    // pixel rectangle of this chunk
    int pxa, pxb, pya, pyb;  // pixel box of the (plane, view)
    int ncx, ncy;            // candidates per texel and axis (0: no usable homography -> every staged pixel)
    float rxu, ryu;          // the tile's radii
    Rec r;
};
// the record's nine numbers without its padding (a padding array carried in a chunk descriptor lives in scratch memory)
struct HRec9 {
    float a, b, c, d, e, f, g, h, valid;
};

// The texels a thread owns and the planes its workgroup runs over: what a sink is told.
struct Cell {
    int m, x, y0, y1;        // MPI; the texels (x, y0) and (x, y1 = y0 + 8)
    int k_first, k_last;     // the workgroup's planes [k_first, k_last)
};

// The texel pass of one workgroup: candidate discovery, staging and the fixed-order sums are the same for every layout; what happens to a plane's four
// sums is the SINK's business (a policy):
//   Sink::Rec, Sink::load_rec(r, q) the homography record as a chunk descriptor carries it
//   Sink::add(w, d, acc)            one candidate's term (four FMAs, gated on w != 0 in every sink: a branch for the volume, selects for the image layouts)
//   sink.begin(cell)                before the first plane
//   sink.store_plane(cell, k, acc0, acc1)   plane k is complete, called once per plane of the run in rising order: stores and resets what restarts per plane
//   sink.finish(cell)               after the last plane
// sXY / sD: the workgroup's staging buffers (kCap items each).
template <typename Sink>
__device__ __forceinline__ void texel_gather_run(const KParams& p, const f32x2* __restrict__ P, const f32x4* __restrict__ G, const HRec* __restrict__ recs,
                                                 const int tiles_x, const int tiles_y, const int planes_per_wg, float2* __restrict__ sXY,
                                                 float4* __restrict__ sD, Sink& sink) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_tiles = tiles_x * tiles_y;
    const int tile = xcd_item_per_group(static_cast<int>(blockIdx.x), n_tiles, n_tiles);
    if (tile >= n_tiles) return;
    const int m = blockIdx.z;
    const int k_first = blockIdx.y * planes_per_wg, k_last = min(k_first + planes_per_wg, p.D);   // [k_first, k_last)
    const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    const int X0 = txi * kTX, Y0 = tyi * kTY;
    const int x = X0 + lane, y0 = Y0 + wave, y1 = y0 + 8;   // this thread's two texels
    const float xf = static_cast<float>(x), yf0 = static_cast<float>(y0), yf1 = static_cast<float>(y1);
    const int Wt = p.Wt, Ht = p.Ht, W = p.W, H = p.H;
    const int64_t HW = static_cast<int64_t>(H) * W;
    const Cell cell{m, x, y0, y1, k_first, k_last};
    using Chunk = ChunkT<typename Sink::Rec>;

    auto inv_map = [&](const typename Sink::Rec& r, float tx, float ty, float& ppx, float& ppy, float& radx, float& rady) {
        // texel -> pixel: position and how far a texel's 2 x 2 support reaches in pixels (first order, with slack)
        const float den = __builtin_fmaf(r.g, tx, __builtin_fmaf(r.h, ty, 1.0f));
        const float rd = 1.0f / den;
        ppx = __builtin_fmaf(r.a, tx, __builtin_fmaf(r.b, ty, r.c)) * rd;
        ppy = __builtin_fmaf(r.d, tx, __builtin_fmaf(r.e, ty, r.f)) * rd;
        radx = (fabsf(r.a - r.g * ppx) + fabsf(r.b - r.h * ppx)) * fabsf(rd) * 1.03f + 0.08f;
        rady = (fabsf(r.d - r.g * ppy) + fabsf(r.e - r.h * ppy)) * fabsf(rd) * 1.03f + 0.08f;
    };
    // the pixel box of (plane k, view v): false when no pixel of the view reaches the tile
    auto open_view = [&](Chunk& c) -> bool {
        c.n = m * p.views_per_mpi + c.v;
        if (c.n >= p.N) return false;
        Sink::load_rec(c.r, recs[static_cast<int64_t>(c.n) * p.D + c.k]);
        int pxa = 0, pxb = W - 1, pya = 0, pyb = H - 1, ncx = 0, ncy = 0;
        float rxu = 0.0f, ryu = 0.0f;
        if (c.r.valid != 0.0f) {
            float mnx = 3e38f, mxx = -3e38f, mny = 3e38f, mxy = -3e38f, rxm = 0.0f, rym = 0.0f;
            bool okq = true;
#pragma unroll
            for (int q = 0; q < 4; ++q) {   // the tile grown by a texel on every side
                const float tx = static_cast<float>((q & 1) ? min(X0 + kTX, Wt) : X0 - 1), ty = static_cast<float>((q & 2) ? min(Y0 + kTY, Ht) : Y0 - 1);
                okq = okq && __builtin_fmaf(c.r.g, tx, __builtin_fmaf(c.r.h, ty, 1.0f)) > 1e-6f;
                float qx, qy, ax, ay;
                inv_map(c.r, tx, ty, qx, qy, ax, ay);
                mnx = fminf(mnx, qx), mxx = fmaxf(mxx, qx), mny = fminf(mny, qy), mxy = fmaxf(mxy, qy);
                rxm = fmaxf(rxm, ax), rym = fmaxf(rym, ay);
            }
            if (okq && mxx - mnx < 1e6f && mxy - mny < 1e6f && rxm < 64.0f && rym < 64.0f) {
                pxa = max(static_cast<int>(floorf(mnx - 0.25f)), 0), pxb = min(static_cast<int>(ceilf(mxx + 0.25f)), W - 1);
                pya = max(static_cast<int>(floorf(mny - 0.25f)), 0), pyb = min(static_cast<int>(ceilf(mxy + 0.25f)), H - 1);
                ncx = static_cast<int>(2.0f * rxm) + 1, ncy = static_cast<int>(2.0f * rym) + 1;   // integers in an interval of length 2 r: at most floor(2 r) + 1
                rxu = rxm, ryu = rym;
            }
            // (else: the inverse has a pole near the tile: every pixel is looked at, as for an invalid record)
        }
        c.pxa = __builtin_amdgcn_readfirstlane(pxa), c.pxb = __builtin_amdgcn_readfirstlane(pxb);
        c.pya = __builtin_amdgcn_readfirstlane(pya), c.pyb = __builtin_amdgcn_readfirstlane(pyb);
        c.ncx = __builtin_amdgcn_readfirstlane(ncx), c.ncy = __builtin_amdgcn_readfirstlane(ncy);
        c.rxu = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, rxu)));
        c.ryu = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, ryu)));
        if (c.pxa > c.pxb || c.pya > c.pyb) return false;
        c.bx0 = c.pxa, c.by0 = c.pya;
        c.cw = min(kChunkW, c.pxb - c.bx0 + 1);
        c.ch = min(kCap / c.cw, c.pyb - c.by0 + 1);
        return true;
    };
    // the first chunk at or after (plane c.k, view c.v); false: the planes of this workgroup are exhausted
    auto seek = [&](Chunk& c) -> bool {
        for (; c.k < k_last; ++c.k, c.v = 0)
            for (; c.v < p.views_per_mpi; ++c.v)
                if (open_view(c)) return true;
        return false;
    };
    auto next = [&](Chunk& c) -> bool {   // the chunk after c
        c.by0 += c.ch;
        if (c.by0 <= c.pyb) { c.ch = min(kCap / c.cw, c.pyb - c.by0 + 1); return true; }
        c.bx0 += c.cw;
        if (c.bx0 <= c.pxb) { c.cw = min(kChunkW, c.pxb - c.bx0 + 1); c.by0 = c.pya; c.ch = min(kCap / c.cw, c.pyb - c.by0 + 1); return true; }
        ++c.v;
        return seek(c);
    };
    f32x2 rp[kSlots];
    f32x4 rd[kSlots];
    auto load = [&](const Chunk& c) {   // the chunk's pixels into registers (row-major index i = tid + 512 s)
        const f32x2* __restrict__ Pv = P + (static_cast<int64_t>(c.n) * p.D + c.k) * HW;
        const f32x4* __restrict__ Gv = G + (static_cast<int64_t>(c.n) * p.D + c.k) * HW;
        const float inv_cw = 1.0f / static_cast<float>(c.cw);
        const int count = c.cw * c.ch;
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const int i = tid + s * kTT;
            const int ly = static_cast<int>((static_cast<float>(i) + 0.5f) * inv_cw);   // floor(i / cw): the fraction is at least 0.5 / cw away from an integer
            const int lx = i - ly * c.cw;
            const int64_t q = static_cast<int64_t>(c.by0 + ly) * W + (c.bx0 + lx);
            if (i < count) {
                rp[s] = __builtin_nontemporal_load(Pv + q);
                rd[s] = __builtin_nontemporal_load(Gv + q);
            }
        }
    };
    auto commit = [&](const Chunk& c) {   // registers -> LDS
        const int count = c.cw * c.ch;
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const int i = tid + s * kTT;
            if (i < count) {
                sXY[i] = make_float2(rp[s].x, rp[s].y);
                sD[i] = make_float4(rd[s].x, rd[s].y, rd[s].z, rd[s].w);
            }
        }
    };
    float acc0[4] = {0.f, 0.f, 0.f, 0.f}, acc1[4] = {0.f, 0.f, 0.f, 0.f};
    auto visit = [&](int idx, bool inside, float tyf, float (&acc)[4]) {
        const float2 pos = sXY[idx];
        const float4 d = sD[idx];
        const float wxx = fmaxf(1.0f - fabsf(pos.x - xf), 0.0f), wyy = fmaxf(1.0f - fabsf(pos.y - tyf), 0.0f);
        float w = wxx * wyy;
        w = (inside && w == w) ? w : 0.0f;   // (a NaN position -- a NaN ray -- samples nothing)
        Sink::add(w, d, acc);
    };
    auto gather = [&](const Chunk& c) {
        const int cw = c.cw, ch = c.ch;
        if (c.ncx > 0) {
            // this thread's candidate windows: [q - r, q + r] with the TILE's radius holds at most ncx integers
            float qx, qy, ax, ay;
            inv_map(c.r, xf, yf0, qx, qy, ax, ay);
            const int cxs0 = static_cast<int>(ceilf(qx - c.rxu)) - c.bx0, cys0 = static_cast<int>(ceilf(qy - c.ryu)) - c.by0;
            inv_map(c.r, xf, yf1, qx, qy, ax, ay);
            const int cxs1 = static_cast<int>(ceilf(qx - c.rxu)) - c.bx0, cys1 = static_cast<int>(ceilf(qy - c.ryu)) - c.by0;
            for (int jy = 0; jy < c.ncy; ++jy) {
                const int ly0 = cys0 + jy, ly1 = cys1 + jy;
                const bool iny0 = ly0 >= 0 && ly0 < ch, iny1 = ly1 >= 0 && ly1 < ch;
                for (int jx = 0; jx < c.ncx; ++jx) {
                    const int lx0 = cxs0 + jx, lx1 = cxs1 + jx;
                    const bool in0 = iny0 && lx0 >= 0 && lx0 < cw, in1 = iny1 && lx1 >= 0 && lx1 < cw;
                    visit(in0 ? ly0 * cw + lx0 : 0, in0, yf0, acc0);
                    visit(in1 ? ly1 * cw + lx1 : 0, in1, yf1, acc1);
                }
            }
        } else {   // no usable homography: every staged pixel is a candidate of every texel
            for (int idx = 0; idx < cw * ch; ++idx) {
                visit(idx, true, yf0, acc0);
                visit(idx, true, yf1, acc1);
            }
        }
    };
    auto store_plane = [&](int k) { sink.store_plane(cell, k, acc0, acc1); };

    sink.begin(cell);
    Chunk cur;
    cur.k = k_first, cur.v = 0;
    bool have = seek(cur);
    int k_done = k_first;   // planes [k_first, k_done) have been stored
    if (have) {
        load(cur);
        commit(cur);
    }
    while (have) {
        __syncthreads();   // cur's pixels are in LDS
        Chunk nxt = cur;
        const bool more = next(nxt);
        if (more) load(nxt);                 // in flight while cur is gathered
        for (; k_done < cur.k; ++k_done) store_plane(k_done);   // (planes nobody reaches: zeros; the plane before cur's: its sums)
        gather(cur);
        __syncthreads();   // everybody is done reading cur
        if (more) commit(nxt);
        cur = nxt;
        have = more;
    }
    for (; k_done < k_last; ++k_done) store_plane(k_done);
    sink.finish(cell);
}

// The volume's sink: every plane has its own four channels in grad_rgba; every cell once, the sums restart.
template <bool OVERWRITE>
struct VolumeSink {
    const BwdParams& b;
    int Ht, Wt;
    using Rec = HRec;
    static __device__ __forceinline__ void load_rec(HRec& r, const HRec& q) { r = q; }
    // A term is added only where its weight is not zero (as LayoutSink::add below and the atomic kernels' scatter gate theirs): 0 * inf is NaN, and
    // every candidate of a texel's window -- the stand-in index 0 of a candidate outside the chunk included -- would carry one pixel's non-finite
    // d_s into cells its footprints never touch.  Written as a branch: hipcc keeps it one (exec mask around the four FMAs); as four selects the
    // pair's backward was 6.5 % slower at 1024^2 x 32 x 4 (3.75 against 3.51 ms), as a branch 3.54 (profiles/upstream_gradients.txt).
    static __device__ __forceinline__ void add(float w, const float4& d, float (&acc)[4]) {
        if (w != 0.0f) {
            acc[0] = __builtin_fmaf(w, d.x, acc[0]), acc[1] = __builtin_fmaf(w, d.y, acc[1]);
            acc[2] = __builtin_fmaf(w, d.z, acc[2]), acc[3] = __builtin_fmaf(w, d.w, acc[3]);
        }
    }
    __device__ __forceinline__ void begin(const Cell&) {}
    __device__ __forceinline__ void finish(const Cell&) {}
    __device__ __forceinline__ void store_plane(const Cell& c, int k, float (&acc0)[4], float (&acc1)[4]) {
        const int x = c.x, y0 = c.y0, y1 = c.y1;
        float* __restrict__ gm = b.g_rgba + static_cast<int64_t>(c.m) * b.gs_mpi + static_cast<int64_t>(k) * b.gs_plane;
        if (x < Wt) {
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                if (y0 < Ht) {
                    float* cell = gm + c4 * b.gs_chan + static_cast<int64_t>(y0) * b.gs_row + x;
                    *cell = OVERWRITE ? acc0[c4] : *cell + acc0[c4];
                }
                if (y1 < Ht) {
                    float* cell = gm + c4 * b.gs_chan + static_cast<int64_t>(y1) * b.gs_row + x;
                    *cell = OVERWRITE ? acc1[c4] : *cell + acc1[c4];
                }
            }
        }
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) acc0[c4] = acc1[c4] = 0.0f;
    }
};

template <bool OVERWRITE>
__global__ __launch_bounds__(kTT, 6) void texel_gather_kernel(const KParams p, const BwdParams b, const f32x2* __restrict__ P, const f32x4* __restrict__ G,
                                                              const HRec* __restrict__ recs, const int tiles_x, const int tiles_y, const int planes_per_wg) {
    __shared__ float2 sXY[kCap];
    __shared__ float4 sD[kCap];
    VolumeSink<OVERWRITE> sink{b, p.Ht, p.Wt};
    texel_gather_run(p, P, G, recs, tiles_x, tiles_y, planes_per_wg, sXY, sD, sink);
}

// ---- 4. the same pair for the two image layouts (shared-colour, depth-alpha: gmpi_shared.hpp) --------------------------------------------------------
// The records are the volume pair's (sample position 8 B, d_s[0..3] 16 B per view, plane and pixel), so homography_kernel and texel_gather_run serve as
// they are.  New: a pixel pass whose taps come from the layout's images, and a sink whose colour sums -- and, depth-alpha, the one depth sum -- run
// ACROSS the planes of a workgroup's run instead of being stored per plane.
//
// Pixel pass: pixel_pass_kernel's frame (one pixel per thread, 64 x 8 tiles in xcd_item_per_group order, back to front, no barrier, non-temporal
// stores) around the sweep of render_shared_backward_kernel / render_depth_backward_kernel, term for term.  The taps are addressed with 64-bit
// offsets (tap_sample, ramp_taps): no plane table in LDS, any D, any stride.  DEPTH: a plane those kernels skip (alpha sample 0, no tap on the ramp)
// still writes its record, with d_s = 0: the texel pass reads every record.  Whether a tap lies on the ramp does not depend on which gradients
// the caller wants here, so the records -- and with them every gradient's bits -- are the same for every subset of outputs.
template <typename TexT, bool DEPTH>
__global__ __launch_bounds__(kPT) void layout_pixel_pass_kernel(const KParams p, const SharedK sh, const DepthK dk, const float* __restrict__ g_out,
                                                                const float* __restrict__ g_depth, const float* __restrict__ g_T, f32x2* __restrict__ P,
                                                                f32x4* __restrict__ G, const int tiles_x) {
    constexpr bool AC = true;
    const int tid = threadIdx.x;
    const int n = blockIdx.y;
    const int n_tiles = tiles_x * ((p.H + kPTH - 1) / kPTH);
    const int tile = xcd_item_per_group(static_cast<int>(blockIdx.x), n_tiles, n_tiles);
    if (tile >= n_tiles) return;
    const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    const int px = txi * kPTW + (tid % kPTW), py = tyi * kPTH + (tid / kPTW);
    if (px >= p.W || py >= p.H) return;   // (no barrier in this kernel)
    uint32_t unused = 0;
    const BwdView vw = bwd_view<AC>(p, n);
    const int m = vw.m;
    const int Ht = p.Ht, Wt = p.Wt, D = p.D;
    const int64_t HW = vw.HW;
    const TexT* __restrict__ mid = static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(m) * p.s_mpi;   // alpha planes | depth image
    const TexT* __restrict__ rgb = static_cast<const TexT*>(sh.rgb) + static_cast<int64_t>(m) * sh.rs_mpi;
    const TexT* __restrict__ bgi = sh.bg ? static_cast<const TexT*>(sh.bg) + static_cast<int64_t>(m) * sh.bs_mpi : nullptr;
    const float* __restrict__ pz = DEPTH ? dk.plane_z + static_cast<int64_t>(m) * dk.pz_stride : nullptr;

    BwdPixel bp;
    if (DEPTH) {
        bwd_pixel_setup_with<false>(bp, p, vw, n, px, py, true, g_out, g_depth, g_T,
                                    [&](float t_fwd) { return depth_total_transmittance<TexT, AC>(p, vw, bp, mid, pz, dk, t_fwd); });
    } else {
        bwd_pixel_setup<TexT, AC, false>(bp, p, vw, n, px, py, true, g_out, g_depth, g_T, mid);
    }
    f32x4* __restrict__ Gpix = G + static_cast<int64_t>(n) * D * HW + bp.pix;   // + k * HW per plane
    f32x2* __restrict__ Ppix = P + static_cast<int64_t>(n) * D * HW + bp.pix;
#pragma unroll 2
    for (int k = D - 1; k >= 0; --k) {
        float ix, iy, s;
        pixel_plane_coord<AC>(vw, bp, k, ix, iy, s);
        const Taps t = make_taps(ix, iy, Ht, Wt);
        const bool last_bg = bgi != nullptr && k == D - 1;
        const TexT* __restrict__ col = last_bg ? bgi : rgb;
        const int64_t c_chan = last_bg ? sh.bs_chan : sh.rs_chan, c_row = last_bg ? sh.bs_row : sh.rs_row;
        float smp[4], d_s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool skip = false;
        if (DEPTH) {
            const Footprint& f = t.f;
            const RampTaps r = ramp_taps<TexT, false>(mid, p.s_row, t, pz[k], dk);
            smp[3] = bilerp<false>(r.a[0], r.a[1], r.a[2], r.a[3], f);
            const bool on_ramp = (r.in[0] && f.nw != 0.0f) || (r.in[1] && f.ne != 0.0f) || (r.in[2] && f.sw != 0.0f) || (r.in[3] && f.se != 0.0f);
            skip = smp[3] == 0.0f && !on_ramp;   // the identity of the sweep: om = 1, w = 0, no gradient reaches the depth image
        } else {
            smp[3] = tap_sample<TexT, false>(mid + static_cast<int64_t>(k) * p.s_plane, p.s_row, t, false, unused);
        }
        if (!skip) {
#pragma unroll
            for (int c = 0; c < 3; ++c) smp[c] = tap_sample<TexT, false>(col + c * c_chan, c_row, t, false, unused);
            bp.plane(smp, s, d_s);
        }
        const f32x2 pv = {ix, iy};
        const f32x4 dv = {d_s[0], d_s[1], d_s[2], d_s[3]};
        __builtin_nontemporal_store(pv, Ppix + static_cast<int64_t>(k) * HW);   // (read once, by the texel pass)
        __builtin_nontemporal_store(dv, Gpix + static_cast<int64_t>(k) * HW);
    }
}

// What the layouts' texel pass needs besides the records: the three destinations, the run slabs, and (depth-alpha) the depth image and its ramp.
struct LayoutSinkParams {
    SharedG g;             // g_rgb, g_alpha (shared-colour: alpha planes; depth-alpha: the depth image), g_bg: each may be nullptr
    float* slabs;          // runs > 1: [M][runs][C][Ht][Wt] partial sums of the cross-plane channels (C = 3, depth-alpha 4: the depth sum last)
    int runs;              // plane runs per texel tile (grid.y)
    int has_bg;            // plane D - 1 takes its colour from the background image
    const void* depth;     // depth-alpha: the depth image, its dtype and strides in elements
    int dtype;
    int64_t d_mpi, d_row;
    DepthK dk;
};

template <bool OVERWRITE>
__device__ __forceinline__ void put_cell(float* __restrict__ cell, float v) { *cell = OVERWRITE ? v : *cell + v; }

__device__ __forceinline__ float load_texel(const void* __restrict__ base, int64_t i, int dtype) {
    if (dtype == GMPI_DTYPE_F32) return static_cast<const float*>(base)[i];
    if (dtype == GMPI_DTYPE_BF16) return to_f32(static_cast<const bf16_t*>(base)[i]);
    return to_f32(static_cast<const f16_t*>(base)[i]);
}

// The sink of the two layouts.  Channel 3: shared-colour stores it per plane (grad_alpha[m, k]); depth-alpha adds it to the cell's depth sum where the
// cell's depth texel -- held in a register for the whole run -- lies on plane k's ramp (depth_ramp's `inside`: the same fp32 subtraction, bounds
// included), and the depth gradient is -sum / z_den, divided once per cell.  Channels 0-2 are NOT reset per plane: they run over every plane of the
// workgroup's run that takes its colour from rgb; with a background, plane D - 1's sums go to grad_background (straight: one run owns that plane).
// One run per tile (runs == 1): the cross-plane sums go straight to their destinations (=, or read + add + write back: the cell has one owner).
// runs > 1: each run writes its partial sums to its slab and layout_reduce_kernel adds the runs up in run order.
// A term is added only where its weight is not zero, as add_taps gates its atomics: a pixel whose d_s is not finite reaches the cells of its footprints only.
template <bool OVERWRITE, bool DEPTH>
struct LayoutSink {
    const LayoutSinkParams& q;
    int Ht, Wt, D;
    float dz0 = 0.0f, dz1 = 0.0f;   // DEPTH: the two cells' depth texels
    float ds0 = 0.0f, ds1 = 0.0f;   //        and their depth sums
    const float* __restrict__ pz = nullptr;

    using Rec = HRec9;
    static __device__ __forceinline__ void load_rec(HRec9& r, const HRec& q) { r = HRec9{q.a, q.b, q.c, q.d, q.e, q.f, q.g, q.h, q.valid}; }
    static __device__ __forceinline__ void add(float w, const float4& d, float (&acc)[4]) {
        const bool on = w != 0.0f;
        acc[0] = on ? __builtin_fmaf(w, d.x, acc[0]) : acc[0], acc[1] = on ? __builtin_fmaf(w, d.y, acc[1]) : acc[1];
        acc[2] = on ? __builtin_fmaf(w, d.z, acc[2]) : acc[2], acc[3] = on ? __builtin_fmaf(w, d.w, acc[3]) : acc[3];
    }
    __device__ __forceinline__ bool in0(const Cell& c) const { return c.x < Wt && c.y0 < Ht; }
    __device__ __forceinline__ bool in1(const Cell& c) const { return c.x < Wt && c.y1 < Ht; }
    __device__ __forceinline__ float* slab(const Cell& c, int ch) const {
        constexpr int C = DEPTH ? 4 : 3;
        return q.slabs + ((static_cast<int64_t>(c.m) * q.runs + blockIdx.y) * C + ch) * (static_cast<int64_t>(Ht) * Wt);
    }
    __device__ __forceinline__ void begin(const Cell& c) {
        if (DEPTH) {
            pz = q.dk.plane_z + static_cast<int64_t>(c.m) * q.dk.pz_stride;
            const int64_t base = static_cast<int64_t>(c.m) * q.d_mpi + c.x;
            if (in0(c)) dz0 = load_texel(q.depth, base + static_cast<int64_t>(c.y0) * q.d_row, q.dtype);
            if (in1(c)) dz1 = load_texel(q.depth, base + static_cast<int64_t>(c.y1) * q.d_row, q.dtype);
        }
    }
    // the colour sums of the planes that use rgb: to grad_shared_rgb, or to this run's slab
    __device__ __forceinline__ void emit_rgb(const Cell& c, const float (&acc0)[4], const float (&acc1)[4]) {
        if (q.g.g_rgb == nullptr) return;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if (q.runs == 1) {
                float* __restrict__ gm = q.g.g_rgb + static_cast<int64_t>(c.m) * q.g.gr_mpi + ch * q.g.gr_chan + c.x;
                if (in0(c)) put_cell<OVERWRITE>(gm + static_cast<int64_t>(c.y0) * q.g.gr_row, acc0[ch]);
                if (in1(c)) put_cell<OVERWRITE>(gm + static_cast<int64_t>(c.y1) * q.g.gr_row, acc1[ch]);
            } else {
                float* __restrict__ sl = slab(c, ch) + c.x;
                if (in0(c)) sl[static_cast<int64_t>(c.y0) * Wt] = acc0[ch];
                if (in1(c)) sl[static_cast<int64_t>(c.y1) * Wt] = acc1[ch];
            }
        }
    }
    __device__ __forceinline__ void store_plane(const Cell& c, int k, float (&acc0)[4], float (&acc1)[4]) {
        // (q is re-read from LDS here: nothing derived from it -- seven destination addresses per cell -- stays live through the gather loops)
        asm volatile("" ::: "memory");
        if (DEPTH) {
            const float pzk = pz[k];
            bool on0, on1;
            depth_ramp<false>(pzk, dz0, q.dk, on0);
            depth_ramp<false>(pzk, dz1, q.dk, on1);
            if (on0) ds0 += acc0[3];
            if (on1) ds1 += acc1[3];
        } else if (q.g.g_alpha != nullptr) {
            float* __restrict__ gm = q.g.g_alpha + static_cast<int64_t>(c.m) * q.g.ga_mpi + static_cast<int64_t>(k) * q.g.ga_plane + c.x;
            if (in0(c)) put_cell<OVERWRITE>(gm + static_cast<int64_t>(c.y0) * q.g.ga_row, acc0[3]);
            if (in1(c)) put_cell<OVERWRITE>(gm + static_cast<int64_t>(c.y1) * q.g.ga_row, acc1[3]);
        }
        acc0[3] = acc1[3] = 0.0f;
        const bool bg_plane = q.has_bg != 0 && k == D - 1;
        if (bg_plane) {
            if (c.k_first == k) {   // no plane of this run uses rgb: its sum is zero, and is still this run's to write
                const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                emit_rgb(c, zero, zero);
            }
            if (q.g.g_bg != nullptr) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    float* __restrict__ gm = q.g.g_bg + static_cast<int64_t>(c.m) * q.g.gb_mpi + ch * q.g.gb_chan + c.x;
                    if (in0(c)) put_cell<OVERWRITE>(gm + static_cast<int64_t>(c.y0) * q.g.gb_row, acc0[ch]);
                    if (in1(c)) put_cell<OVERWRITE>(gm + static_cast<int64_t>(c.y1) * q.g.gb_row, acc1[ch]);
                }
            }
        } else if (k == c.k_last - 1 || (q.has_bg != 0 && k == D - 2)) {   // the last plane of the run that uses rgb
            emit_rgb(c, acc0, acc1);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc0[ch] = acc1[ch] = 0.0f;
        }
    }
    __device__ __forceinline__ void finish(const Cell& c) {
        if (DEPTH && q.g.g_alpha != nullptr) {
            if (q.runs == 1) {
                float* __restrict__ gm = q.g.g_alpha + static_cast<int64_t>(c.m) * q.g.ga_mpi + c.x;
                if (in0(c)) put_cell<OVERWRITE>(gm + static_cast<int64_t>(c.y0) * q.g.ga_row, -div_by_recip(ds0, q.dk.den, q.dk.rden));
                if (in1(c)) put_cell<OVERWRITE>(gm + static_cast<int64_t>(c.y1) * q.g.ga_row, -div_by_recip(ds1, q.dk.den, q.dk.rden));
            } else {
                float* __restrict__ sl = slab(c, 3) + c.x;
                if (in0(c)) sl[static_cast<int64_t>(c.y0) * Wt] = ds0;
                if (in1(c)) sl[static_cast<int64_t>(c.y1) * Wt] = ds1;
            }
        }
    }
};

// (kTT, 4): 128 VGPRs -- the cross-plane sums, the depth texels and the three destinations do not fit the volume kernel's 80 without scratch
template <bool OVERWRITE, bool DEPTH>
__global__ __launch_bounds__(kTT, 4) void layout_texel_gather_kernel(const KParams p, const LayoutSinkParams q, const f32x2* __restrict__ P,
                                                                     const f32x4* __restrict__ G, const HRec* __restrict__ recs, const int tiles_x,
                                                                     const int tiles_y, const int planes_per_wg) {
    __shared__ float2 sXY[kCap];
    __shared__ float4 sD[kCap];
    // The sink's parameters -- three destinations with their strides, the slabs, the ramp -- are read where a plane is stored, from LDS: held in scalar
    // registers through the gather loops (next to two chunk descriptors with their homographies) they spill.
    __shared__ LayoutSinkParams sq;
    if (threadIdx.x == 0) sq = q;
    __syncthreads();
    LayoutSink<OVERWRITE, DEPTH> sink{sq, p.Ht, p.Wt, p.D};
    texel_gather_run(p, P, G, recs, tiles_x, tiles_y, planes_per_wg, sXY, sD, sink);
}

// runs > 1: every cross-plane cell is the sum of its runs' partials, added up in run order by the one thread that owns it (geometry_reduce_kernel's
// shape: render_backward_geometry.hip).  Channel 3 (depth-alpha): the depth gradient -sum / z_den.
template <bool OVERWRITE, bool DEPTH>
__global__ __launch_bounds__(256) void layout_reduce_kernel(const LayoutSinkParams q, const int M, const int Ht, const int Wt) {
    constexpr int C = DEPTH ? 4 : 3;
    const int64_t plane = static_cast<int64_t>(Ht) * Wt, total = plane * C * M;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * 256) {
        const int64_t mc = i / plane, o = i - mc * plane;
        const int m = static_cast<int>(mc / C), ch = static_cast<int>(mc - static_cast<int64_t>(m) * C);
        const int y = static_cast<int>(o / Wt), x = static_cast<int>(o - static_cast<int64_t>(y) * Wt);
        float* __restrict__ dst = ch < 3 ? q.g.g_rgb : q.g.g_alpha;
        if (dst == nullptr) continue;
        float sum = 0.0f;
        for (int r = 0; r < q.runs; ++r) sum += q.slabs[((static_cast<int64_t>(m) * q.runs + r) * C + ch) * plane + o];
        if (ch < 3) {
            put_cell<OVERWRITE>(dst + static_cast<int64_t>(m) * q.g.gr_mpi + ch * q.g.gr_chan + static_cast<int64_t>(y) * q.g.gr_row + x, sum);
        } else {
            put_cell<OVERWRITE>(dst + static_cast<int64_t>(m) * q.g.ga_mpi + static_cast<int64_t>(y) * q.g.ga_row + x, -div_by_recip(sum, q.dk.den, q.dk.rden));
        }
    }
}

static uint64_t align256(uint64_t v) { return (v + 255) / 256 * 256; }
static uint64_t recs_bytes(const KParams& p) { return align256(static_cast<uint64_t>(p.N) * p.D * sizeof(HRec)); }

}  // namespace bwdg

// Can the atomics-free pair run this launch (workspace aside)?
bool backward_gather_supports(const KParams& p, int dtype) {
    if (!(p.flags & GMPI_FLAG_ALIGN_CORNERS)) return false;                                   // align_corners = True only (see the head of this file)
    if (p.view_to_mpi != nullptr) return false;                          // uniform views per MPI
    if (p.N > 65535 || p.M > 65535 || p.D > 65535) return false;         // grid.y / grid.z
    if (p.Wt < 2) return false;                                          // pair loads
    if (!plane_offsets_fit_32(p.s_chan, p.s_row, p.Ht, p.Wt, dtype == GMPI_DTYPE_F32 ? 4 : 2)) return false;   // ... at 32-bit byte offsets inside a plane
    if (static_cast<int64_t>(p.H) * p.W >= (int64_t(1) << 31)) return false;
    return true;
}
uint64_t backward_gather_workspace_bytes(const KParams& p, int dtype) {
    if (!backward_gather_supports(p, dtype)) return 0;
    return bwdg::recs_bytes(p) + static_cast<uint64_t>(p.N) * p.D * p.H * p.W * 24u;   // sample gradients 16 B + sample positions 8 B per pixel and plane
}

template <typename TexT>
static hipError_t launch_gather_t(const KParams& p, const BwdParams& b, bool overwrite, hipStream_t stream) {
    using namespace bwdg;
    const uint64_t npp = static_cast<uint64_t>(p.N) * p.D * p.H * p.W;   // pixel-planes
    HRec* recs = static_cast<HRec*>(p.ws);
    f32x4* G = reinterpret_cast<f32x4*>(static_cast<unsigned char*>(p.ws) + recs_bytes(p));
    f32x2* P = reinterpret_cast<f32x2*>(static_cast<unsigned char*>(p.ws) + recs_bytes(p) + npp * 16u);
    const int nrec = p.N * p.D;
    hipLaunchKernelGGL((homography_kernel<true>), dim3((nrec + 63) / 64), dim3(64), 0, stream, p, recs);
    {
        const int tx = (p.W + kPTW - 1) / kPTW, ty = (p.H + kPTH - 1) / kPTH;
        const dim3 grid(xcd_grid_per_group(tx * ty, tx * ty), p.N);
        hipLaunchKernelGGL((pixel_pass_kernel<TexT, true>), grid, dim3(kPT), 0, stream, p, b, P, G, tx);
    }
    {
        const int tx = (p.Wt + kTX - 1) / kTX, ty = (p.Ht + kTY - 1) / kTY;
        // planes per workgroup: 4-8 measured best at the G-step shapes (1 ... 32: within 5 %, profiles/r06_backward.txt); fewer when the launch is small
        int ppw = std::min(p.D, 8);
        while (ppw > 1 && static_cast<int64_t>(tx) * ty * p.M * ((p.D + ppw - 1) / ppw) < 1024) ppw = (ppw + 1) / 2;
#ifdef GMPI_TUNE  // GMPI_TUNE_PPW: planes per workgroup of the texel pass
        static const int env_ppw = [] { const char* e = getenv("GMPI_TUNE_PPW"); return e ? atoi(e) : 0; }();
        if (env_ppw > 0) ppw = std::min(env_ppw, p.D);
#endif
        const dim3 grid(xcd_grid_per_group(tx * ty, tx * ty), (p.D + ppw - 1) / ppw, p.M);
        dispatch_bool(overwrite, [&](auto OW) { hipLaunchKernelGGL((texel_gather_kernel<decltype(OW)::value>), grid, dim3(kTT), 0, stream, p, b, P, G, recs, tx, ty, ppw); });
    }
    return hipGetLastError();
}

// p.ws / p.ws_bytes: the caller's workspace (>= backward_gather_workspace_bytes).  overwrite: the gradient volume's content is not needed (every cell is
// WRITTEN); otherwise every cell is read, added to and written back -- by its one owner: no atomics either way.
hipError_t launch_backward_gather(const KParams& p, int dtype, const BwdParams& b, bool overwrite, hipStream_t stream) {
    return dispatch_dtype(dtype, [&](auto t) { return launch_gather_t<typename decltype(t)::type>(p, b, overwrite, stream); });
}

// ---- the pair for the shared-colour and depth-alpha layouts ---------------------------------------------------------------------------------------
// backward_gather_supports without the 32-bit offset test: the layouts' pixel pass addresses its taps with 64-bit offsets.
bool layout_gather_supports(const KParams& p) {
    if (!(p.flags & GMPI_FLAG_ALIGN_CORNERS)) return false;
    if (p.view_to_mpi != nullptr) return false;
    if (p.N > 65535 || p.M > 65535 || p.D > 65535) return false;
    if (p.Wt < 2) return false;
    if (static_cast<int64_t>(p.H) * p.W >= (int64_t(1) << 31)) return false;
    return true;
}

// Plane runs per texel tile.  The cross-plane sums want ONE run (its sums go straight to the outputs); a launch whose tiles do not fill the chip that
// way -- fewer than 1024 workgroups: four per CU -- halves the planes per run until they do.  A pure function of the launch's shape: the same launch
// sums in the same order every time.  g_force_runs: the test hook behind gmpi_render_layout_backward_gather_set_runs (0: the rule).
static std::atomic<int> g_force_runs{0};
void layout_gather_force_runs(int runs) { g_force_runs.store(runs > 0 ? runs : 0, std::memory_order_relaxed); }
static int layout_gather_planes_per_run(const KParams& p) {
    const int forced = g_force_runs.load(std::memory_order_relaxed);
    if (forced > 0) return (p.D + std::min(forced, p.D) - 1) / std::min(forced, p.D);
    const int64_t tiles = static_cast<int64_t>((p.Wt + bwdg::kTX - 1) / bwdg::kTX) * ((p.Ht + bwdg::kTY - 1) / bwdg::kTY) * p.M;
    int ppr = p.D;
    while (ppr > 1 && tiles * ((p.D + ppr - 1) / ppr) < 1024) ppr = (ppr + 1) / 2;
    return ppr;
}
int layout_gather_runs(const KParams& p) {
    const int ppr = layout_gather_planes_per_run(p);
    return (p.D + ppr - 1) / ppr;
}
static uint64_t layout_slab_bytes(const KParams& p, bool depth) {
    const int runs = layout_gather_runs(p);
    return runs > 1 ? static_cast<uint64_t>(p.M) * runs * (depth ? 4 : 3) * p.Ht * p.Wt * sizeof(float) : 0;
}
// The HRec records + 24 bytes per pixel and plane + the run slabs, rounded to 256; 0: the pair cannot take the launch.
uint64_t layout_gather_workspace_bytes(const KParams& p, bool depth) {
    if (!layout_gather_supports(p)) return 0;
    return bwdg::align256(bwdg::recs_bytes(p) + static_cast<uint64_t>(p.N) * p.D * p.H * p.W * 24u + layout_slab_bytes(p, depth));
}

template <typename TexT, bool DEPTH>
static hipError_t launch_layout_gather_t(const KParams& p, int dtype, const SharedK& sh, const DepthK& dk, const SharedG& g, bool overwrite, hipStream_t stream) {
    using namespace bwdg;
    const uint64_t npp = static_cast<uint64_t>(p.N) * p.D * p.H * p.W;   // pixel-planes
    unsigned char* ws = static_cast<unsigned char*>(p.ws);
    HRec* recs = static_cast<HRec*>(p.ws);
    f32x4* G = reinterpret_cast<f32x4*>(ws + recs_bytes(p));
    f32x2* P = reinterpret_cast<f32x2*>(ws + recs_bytes(p) + npp * 16u);
    const int nrec = p.N * p.D;
    hipLaunchKernelGGL((homography_kernel<true>), dim3((nrec + 63) / 64), dim3(64), 0, stream, p, recs);
    {
        const int tx = (p.W + kPTW - 1) / kPTW, ty = (p.H + kPTH - 1) / kPTH;
        const dim3 grid(xcd_grid_per_group(tx * ty, tx * ty), p.N);
        hipLaunchKernelGGL((layout_pixel_pass_kernel<TexT, DEPTH>), grid, dim3(kPT), 0, stream, p, sh, dk, g.g_out, g.g_depth, g.g_T, P, G, tx);
    }
    const int ppr = layout_gather_planes_per_run(p), runs = (p.D + ppr - 1) / ppr;
    LayoutSinkParams q{};
    q.g = g;
    q.slabs = reinterpret_cast<float*>(ws + recs_bytes(p) + npp * 24u);
    q.runs = runs;
    q.has_bg = sh.bg != nullptr;
    q.depth = DEPTH ? p.rgba : nullptr;
    q.dtype = dtype;
    q.d_mpi = p.s_mpi, q.d_row = p.s_row;
    q.dk = dk;
    {
        const int tx = (p.Wt + kTX - 1) / kTX, ty = (p.Ht + kTY - 1) / kTY;
        const dim3 grid(xcd_grid_per_group(tx * ty, tx * ty), runs, p.M);
        dispatch_bool(overwrite, [&](auto OW) {
            hipLaunchKernelGGL((layout_texel_gather_kernel<decltype(OW)::value, DEPTH>), grid, dim3(kTT), 0, stream, p, q, P, G, recs, tx, ty, ppr);
        });
    }
    if (runs > 1 && (g.g_rgb != nullptr || (DEPTH && g.g_alpha != nullptr))) {
        const int64_t total = static_cast<int64_t>(p.M) * (DEPTH ? 4 : 3) * p.Ht * p.Wt;
        const unsigned blocks = static_cast<unsigned>(std::min<int64_t>((total + 255) / 256, 256 * 64));
        dispatch_bool(overwrite, [&](auto OW) {
            hipLaunchKernelGGL((layout_reduce_kernel<decltype(OW)::value, DEPTH>), dim3(blocks), dim3(256), 0, stream, q, p.M, p.Ht, p.Wt);
        });
    }
    return hipGetLastError();
}

// dk: the depth-alpha layout's ramp, nullptr: shared-colour.  p.ws / p.ws_bytes: the caller's workspace (>= layout_gather_workspace_bytes).  overwrite:
// as for launch_backward_gather -- every cell inside [Ht, Wt] of the wanted gradients is WRITTEN, or read, added to and written back by its one owner.
hipError_t launch_layout_backward_gather(const KParams& p, int dtype, const SharedK& sh, const DepthK* dk, const SharedG& g, bool overwrite, hipStream_t stream) {
    return dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        return dk != nullptr ? launch_layout_gather_t<T, true>(p, dtype, sh, *dk, g, overwrite, stream)
                             : launch_layout_gather_t<T, false>(p, dtype, sh, DepthK{}, g, overwrite, stream);
    });
}

}  // namespace gmpi
