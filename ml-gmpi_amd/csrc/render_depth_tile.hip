// render_depth_tile.hip -- the tile backward of the depth-alpha layout (gmpi_mpi_render_depth_backward_tile_launch, include/gmpi_render.h).
//
//   render_depth_tile_kernel   backward, one workgroup per 32 x 16 pixel tile: ALL four gradient channels -- R, G, B of the colour image and the
//                              depth image -- are summed in LDS ACROSS the planes, in one moving window
//
// The arithmetic is render_depth_backward_kernel's (render_depth.hip), term for term: pixel_plane_coord, make_taps, the ramp of depth_ramp over the
// four depth taps with its inclusive mask, bilerp, BwdPixel::plane, -div_by_recip(d alpha, den, rden) on the ramp, the sweep started from
// depth_total_transmittance (gmpi_shared.hpp).  What differs is where the adds go.  The frame -- tile order, per-plane texel boxes, the moving window,
// the 64-bit fixed point -- is render_shared_tile_kernel's (render_shared.hip), which has the measurements behind it.
//
// ONE WINDOW.  In the shared-colour layout the alpha gradient has D destination planes and is flushed per plane.  Here the gradient of all D alpha
// planes lands in the one depth image, so the depth channel lives in the same window as the three colour channels: kCW x kCH texels x 4 channels of
// 64-bit words = 64 KiB (+ the 2 KiB box table and the maxima: 67.6 KB, two workgroups per CU), no per-plane box, no per-plane flush.  The boxes of
// a tile drift over the planes by parallax; when the next plane's box leaves the window, the window is flushed (one global atomicAdd per non-zero cell
// inside the texture) and re-anchored with the box at the end it drifts away from.  With a background image the last plane's colour belongs to
// another image: the three colour channels are flushed to it right after plane D - 1; the depth channel stays, it has one destination.
// A (tile, plane) whose box does not fit the window (strong minification, degenerate rays), a pixel whose footprint lies outside its tile's box (a ray
// field that is not a pinhole's) and a lane whose term is out of the fixed-point range (below) add straight to global memory with add_taps.
//
// GATING.  No add, to LDS or to global memory, is issued for a tap whose weight is zero, nor for a depth tap off the ramp: inf * 0 is NaN, and the
// address of a tap outside the texture is unclamped.  A plane whose alpha sample is exactly 0 with no tap on the ramp is the identity of the sweep and is
// skipped (BwdPixel::plane is not called: T and S keep their bits, as in the one-pixel kernel).  Its colour taps ARE loaded: the 16 loads of plane k - 1
// are issued together, one plane ahead, before the depth taps that decide have landed; waiting for those would put a load latency into every plane.
//
// FIXED POINT.  The window lives across the planes, so both scales are fixed per tile before the sweep.
//   colour: as render_shared_tile_kernel -- M_c = max over the tile's pixels of max(|gR|, |gG|, |gB|) (OUT_PM1's factor 2 included); a term is
//     gC w_k weight with w_k = a_k T_k <= (1 + 1e-10)^k and weight <= 1, so |term| <= M_c (1 + 2e-8).
//   depth: a term is d_s[3] weight / den with d_s[3] = T_k q_k - S / om_k, q_k = gR r + gG g + gB b + gZ s_k dot.  For colours in [0, 1]
//     |q_k| <= Q = |gR| + |gG| + |gB| + |gZ| max_k |s_k dot|.  S / om_k = T_k sum_{j>k} a_j (prod_{k<i<j} om_i) q_j + gT T_out / om_k; the weights
//     a_j prod (1 - a_i + 1e-10) sum to at most 1 (+ D 1e-10) and T_out / om_k = T_k prod_{i>k} om_i <= T_k (1 + 1e-10)^D, so
//     |d_s[3]| <= T_k (2 Q + |gT|) (1 + 2e-8) with T_k <= (1 + 1e-10)^k.  s_k = zdiff_k / rz, so max_k |s_k dot| <= max_k |zdiff_k| |dot / rz| up to three
//     roundings; max_k |zdiff_k| is uniform per view.  M_d = max over the tile's pixels of (2 Q + |gT|) / den bounds every depth term (to 1 + 1e-6).
//   Scaled by 2^(40 - e), e = floor(log2 M), a term is below 2^41 (1 + 1e-6).  Terms that can meet in one cell: a pixel adds a plane's sample to four
//   DIFFERENT texels, so at most one term per pixel, plane and channel: 512 D <= 2^9 x 2^7 = 2^16 (D <= 128).  |sum| < 2^57 (1 + 1e-6): 6 bits to spare in a
//   signed 64-bit word.  The bound assumes colours in [0, 1] and finite values; so a lane whose scaled term, colour or depth, is not below 2^42 -- or
//   is not finite: the comparison is false for NaN -- adds that plane's whole contribution straight to global memory.  Every staged term is then
//   below 2^42 and every sum below 2^58, whatever the inputs.  A tile whose maximum is not finite stages nothing in that channel group.
//
// BARRIERS.  The LDS state the threads share during the sweep is the window alone (box[] and the maxima are read-only after the two __syncthreads
// of the setup).  LDS adds are atomic and commute, so planes need no order among themselves; what needs order is (1) every add before a flush reads
// and zeroes its cell, and (2) the flush before the first add under the new anchor (or, after the background flush, into the colour channels again).
// So there is one lds_barrier() before and one after every flush, none per plane.  Every condition that leads to a barrier is computed from box[] and
// launch constants: workgroup-uniform.  Lanes outside the image stay in the loop (MASKED setup) and pass the barriers.
#include "gmpi_backward.hpp"
#include "gmpi_shared.hpp"

namespace gmpi {

constexpr int kDTW = 32, kDTH = 16, kDThreads = kDTW * kDTH;
constexpr int kCW = 64, kCH = 32;     // the window: 4 channels of kCW x kCH 64-bit words = 64 KiB
constexpr int kSPlanes = 128;         // planes a launch can take (the box table)
constexpr int kDBits = 40;            // largest staged term < 2^41 (to_fix takes |w| < 2^43)

template <typename TexT, bool AC>
__global__ __launch_bounds__(kDThreads) void render_depth_tile_kernel(const KParams p, const SharedK sh, const DepthK dk, const SharedG g, const int tiles_x) {
    __shared__ int4 box[kSPlanes];   // bx0, by0, nx (<= 0: not staged), ny
    __shared__ uint32_t cmax, dmax;  // the tile's M_c, M_d (fp32 bits)
    __shared__ uint32_t zmax;        // max_k |zdiff_k| of the view (fp32 bits)
    __shared__ unsigned long long acc[4 * kCW * kCH];
    const int tid = threadIdx.x;
    const int n = blockIdx.y;
    const int n_tiles = tiles_x * ((p.H + kDTH - 1) / kDTH);
    const int tile = xcd_item_per_group(static_cast<int>(blockIdx.x), n_tiles, n_tiles);
    if (tile >= n_tiles) return;   // (whole workgroup: the grid is padded to a multiple of 8)
    const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    const int px = txi * kDTW + (tid % kDTW), py = tyi * kDTH + (tid / kDTW);
    const bool active = px < p.W && py < p.H;
    const BwdView vw = bwd_view<AC>(p, n);
    const int m = vw.m, D = p.D;
    const int Ht = p.Ht, Wt = p.Wt;
    const TexT* __restrict__ depth = static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(m) * p.s_mpi;
    const TexT* __restrict__ rgb = static_cast<const TexT*>(sh.rgb) + static_cast<int64_t>(m) * sh.rs_mpi;
    const TexT* __restrict__ bgi = sh.bg ? static_cast<const TexT*>(sh.bg) + static_cast<int64_t>(m) * sh.bs_mpi : nullptr;
    const float* __restrict__ pz = dk.plane_z + static_cast<int64_t>(m) * dk.pz_stride;
    float* __restrict__ g_rgb = g.g_rgb ? g.g_rgb + static_cast<int64_t>(m) * g.gr_mpi : nullptr;
    float* __restrict__ g_bg = (g.g_bg && bgi) ? g.g_bg + static_cast<int64_t>(m) * g.gb_mpi : nullptr;
    float* __restrict__ g_dep = g.g_alpha ? g.g_alpha + static_cast<int64_t>(m) * g.ga_mpi : nullptr;

    BwdPixel bp;
    bwd_pixel_setup_with<true>(bp, p, vw, n, px, py, active, g.g_out, g.g_depth, g.g_T,
                               [&](float t_fwd) { return depth_total_transmittance<TexT, AC>(p, vw, bp, depth, pz, dk, t_fwd); });

    for (int i = tid; i < 4 * kCW * kCH; i += kDThreads) acc[i] = 0ull;
    if (tid == 0) cmax = 0u, dmax = 0u, zmax = 0u;
    __syncthreads();   // zmax = 0
    // ---- per-plane texel boxes of the tile (from its four corner pixels): a box is staged when it fits the window ------------------------------
    const int cx0 = txi * kDTW, cx1 = min(cx0 + kDTW - 1, p.W - 1);
    const int cy0 = tyi * kDTH, cy1 = min(cy0 + kDTH - 1, p.H - 1);
    for (int k = tid; k < D; k += kDThreads) {
        const float zdiff = vw.dhw[3 * k] - vw.ez;
        box[k] = tile_box<AC>(p, vw, vw.rays, zdiff, vw.dhw[3 * k + 1], vw.dhw[3 * k + 2], cx0, cx1, cy0, cy1, kCW, kCH);
        atomicMax(&zmax, abs_bits(zdiff));
    }
    __syncthreads();   // zero fill, box table, zmax, cmax = dmax = 0
    {   // the tile's maxima: one LDS atomic per wave and maximum
        float bound = 0.0f;
        if (active) {
            const float gt = g.g_T ? fabsf(g.g_T[static_cast<int64_t>(n) * vw.HW + bp.pix]) : 0.0f;
            const float Q = ((fabsf(bp.gr) + fabsf(bp.gg)) + fabsf(bp.gb)) + fabsf(bp.gz) * (__uint_as_float(zmax) * fabsf(bp.dot * bp.rrz));
            bound = (2.0f * Q + gt) * dk.rden;
        }
        const uint32_t wc = wave_max_bits(max(abs_bits(bp.gr), max(abs_bits(bp.gg), abs_bits(bp.gb))));
        const uint32_t wd = wave_max_bits(abs_bits(bound));
        if ((tid & 63) == 0 && wc != 0u) atomicMax(&cmax, wc);
        if ((tid & 63) == 0 && wd != 0u) atomicMax(&dmax, wd);
    }

    struct Tap { float s; Footprint f; float v[16]; };   // v: per channel (r, g, b, depth) the taps nw, ne, sw, se
    struct Grad {
        Footprint f;
        float d[3], gq;   // d colour sample, d depth sample (-d alpha / den)
        float wd[4];      // weights of the depth taps: inside the texture and on the ramp
        bool col, dep;    // the plane has a weight (w_k != 0) / a tap on the ramp
    };
    // plane k for this pixel, first half: coordinates and the 16 tap loads (issued one plane ahead of their use: the scatter of the plane before
    // runs while they are in flight)
    auto fetch = [&](int k, Tap& tp) {
        tp.s = 0.0f;
        tp.f = Footprint{-2, -2, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < 16; ++i) tp.v[i] = 0.0f;
        if (active) {
            float ix, iy;
            pixel_plane_coord<AC>(vw, bp, k, ix, iy, tp.s);
            const Taps t = make_taps(ix, iy, Ht, Wt);
            tp.f = t.f;
            const bool last_bg = bgi != nullptr && k == D - 1;
            const TexT* __restrict__ col = last_bg ? bgi : rgb;
            const int64_t c_chan = last_bg ? sh.bs_chan : sh.rs_chan, c_row = last_bg ? sh.bs_row : sh.rs_row;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const TexT* __restrict__ ch = c < 3 ? col + c * c_chan : depth;
                const int64_t s_row = c < 3 ? c_row : p.s_row;
                const int64_t oa = static_cast<int64_t>(t.ya) * s_row, ob = static_cast<int64_t>(t.yb) * s_row;
                tp.v[4 * c + 0] = to_f32(ch[oa + t.xa]), tp.v[4 * c + 1] = to_f32(ch[oa + t.xb]);
                tp.v[4 * c + 2] = to_f32(ch[ob + t.xa]), tp.v[4 * c + 3] = to_f32(ch[ob + t.xb]);
            }
        }
    };
    // second half: the ramp of the four depth taps (ramp_taps' arithmetic on the prefetched values), the samples (tap_sample's), BwdPixel::plane
    auto grads = [&](int k, const Tap& tp, Grad& G) {
        G.f = tp.f;
        G.d[0] = G.d[1] = G.d[2] = G.gq = 0.0f;
        G.wd[0] = G.wd[1] = G.wd[2] = G.wd[3] = 0.0f;
        G.col = G.dep = false;
        if (active) {
            const Footprint& f = tp.f;
            const float z = pz[k];
            RampTaps r;
#pragma unroll
            for (int i = 0; i < 4; ++i) r.a[i] = depth_ramp<false>(z, tp.v[12 + i], dk, r.in[i]);
            float smp[4], d_s[4];
            smp[3] = bilerp<false>(r.a[0], r.a[1], r.a[2], r.a[3], f);
            G.wd[0] = r.in[0] ? f.nw : 0.0f, G.wd[1] = r.in[1] ? f.ne : 0.0f, G.wd[2] = r.in[2] ? f.sw : 0.0f, G.wd[3] = r.in[3] ? f.se : 0.0f;
            const bool on_ramp = g_dep != nullptr && (G.wd[0] != 0.0f || G.wd[1] != 0.0f || G.wd[2] != 0.0f || G.wd[3] != 0.0f);
            if (!(smp[3] == 0.0f && !on_ramp)) {   // (else: the identity of the sweep)
#pragma unroll
                for (int c = 0; c < 3; ++c) smp[c] = bilerp<false>(tp.v[4 * c + 0], tp.v[4 * c + 1], tp.v[4 * c + 2], tp.v[4 * c + 3], f);
                const float w = bp.plane(smp, tp.s, d_s);
                G.d[0] = d_s[0], G.d[1] = d_s[1], G.d[2] = d_s[2];
                G.col = w != 0.0f;   // (true for NaN)
                if (on_ramp) {       // d alpha / d depth = -1 / den on the ramp
                    G.gq = -div_by_recip(d_s[3], dk.den, dk.rden);
                    G.dep = true;
                }
            }
        }
    };

    struct ColDst { float* base; int64_t s_chan, s_row; };   // where the colour gradient of plane k goes (base nullptr: nobody wants it)
    auto col_dst = [&](int k) {
        return (bgi != nullptr && k == D - 1) ? ColDst{g_bg, g.gb_chan, g.gb_row} : ColDst{g_rgb, g.gr_chan, g.gr_row};
    };
    // the window: anchor (texel of cell 0,0), the rows in use since it was anchored.  All workgroup-uniform.
    int wx0 = 0, wy0 = 0, wrow0 = kCH, wrow1 = 0;
    bool w_open = false;
    float cscale = 0.0f, cinv = 0.0f, dscale = 0.0f, dinv = 0.0f;
    bool cstage = false, dstage = false;
    // channels [0, nc) of the window -> global memory (one atomic per non-zero cell inside the texture; a wave = 64 consecutive texels of one row),
    // cells zeroed.  nc = 3: the colour channels (to ct), 4: with the depth channel.
    auto flush = [&](const ColDst& ct, int nc) {
        if (wrow1 <= wrow0) return;
        const int rows = wrow1 - wrow0;
        for (int i = tid; i < rows * nc * kCW; i += kDThreads) {
            const int line = i / kCW, x = i - line * kCW;      // line = (row, channel)
            const int lr = line / nc, c = line - lr * nc, row = wrow0 + lr;
            unsigned long long* __restrict__ src = acc + (c * kCH + row) * kCW + x;
            const long long v = static_cast<long long>(*src);
            if (v != 0) {
                *src = 0ull;
                const int gx = wx0 + x, gy = wy0 + row;
                if (gx >= 0 && gx < Wt && gy >= 0 && gy < Ht) {   // (a cell outside the texture only ever receives zero weights: belt and braces)
                    const float val = static_cast<float>(static_cast<double>(v));
                    if (c < 3) {
                        if (ct.base != nullptr) atomicAdd(ct.base + c * ct.s_chan + static_cast<int64_t>(gy) * ct.s_row + gx, val * cinv);
                    } else if (g_dep != nullptr) {
                        atomicAdd(g_dep + static_cast<int64_t>(gy) * g.ga_row + gx, val * dinv);
                    }
                }
            }
        }
    };
    // the adds of one plane: into the window, or straight to global memory
    auto scatter = [&](int k, const Grad& G, const ColDst& ct, bool win) {
        const bool col = G.col && ct.base != nullptr, dep = G.dep;
        if (!col && !dep) return;
        const Footprint& f = G.f;
        const int4 bb = box[k];
        const int lx = f.x0 - bb.x, ly = f.y0 - bb.y;
        const int wx = f.x0 - wx0, wy = f.y0 - wy0;
        // (the box lies inside the window; the second test keeps wild coordinates out whatever the box is)
        const bool in_win = win && bb.z > 0 && lx >= 0 && ly >= 0 && lx + 1 < bb.z && ly + 1 < bb.w && wx >= 0 && wy >= 0 && wx + 1 < kCW && wy + 1 < kCH;
        const float dm = fmaxf(fmaxf(fabsf(G.d[0]), fabsf(G.d[1])), fabsf(G.d[2]));
        // (x < 2^42 is false for NaN)
        const bool c_ok = !col || (cstage && dm * cscale < 4398046511104.0f);
        const bool d_ok = !dep || (dstage && fabsf(G.gq) * dscale < 4398046511104.0f);
        if (in_win && c_ok && d_ok) {
            unsigned long long* __restrict__ l0 = acc + wy * kCW + wx;
            if (col) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    unsigned long long* __restrict__ lc = l0 + c * (kCH * kCW);
                    const float d = G.d[c];
                    if (f.nw != 0.0f) atomicAdd(lc, to_fix(d * f.nw, cscale));
                    if (f.ne != 0.0f) atomicAdd(lc + 1, to_fix(d * f.ne, cscale));
                    if (f.sw != 0.0f) atomicAdd(lc + kCW, to_fix(d * f.sw, cscale));
                    if (f.se != 0.0f) atomicAdd(lc + kCW + 1, to_fix(d * f.se, cscale));
                }
            }
            if (dep) {
                unsigned long long* __restrict__ ld = l0 + 3 * (kCH * kCW);
                if (G.wd[0] != 0.0f) atomicAdd(ld, to_fix(G.gq * G.wd[0], dscale));
                if (G.wd[1] != 0.0f) atomicAdd(ld + 1, to_fix(G.gq * G.wd[1], dscale));
                if (G.wd[2] != 0.0f) atomicAdd(ld + kCW, to_fix(G.gq * G.wd[2], dscale));
                if (G.wd[3] != 0.0f) atomicAdd(ld + kCW + 1, to_fix(G.gq * G.wd[3], dscale));
            }
        } else {
            if (col) {
#pragma unroll
                for (int c = 0; c < 3; ++c) add_taps(ct.base + c * ct.s_chan, ct.s_row, f, G.d[c], f.nw, f.ne, f.sw, f.se);
            }
            if (dep) add_taps(g_dep, g.ga_row, f, G.gq, G.wd[0], G.wd[1], G.wd[2], G.wd[3]);
        }
    };

    // ---- back-to-front sweep, software-pipelined by one plane -----------------------------------------------------------------------------------
    Grad G;
    Tap tp;
    fetch(D - 1, tp);
    grads(D - 1, tp, G);
    __syncthreads();   // cmax, dmax complete
    {
        const uint32_t cm = cmax, dm = dmax;
        cstage = cm != 0u && cm < 0x7f800000u, dstage = dm != 0u && dm < 0x7f800000u;
        const int cs = min(kDBits - (static_cast<int>(cm >> 23) - 127), 126), ds = min(kDBits - (static_cast<int>(dm >> 23) - 127), 126);
        cscale = cstage ? __builtin_amdgcn_ldexpf(1.0f, cs) : 0.0f, cinv = cstage ? __builtin_amdgcn_ldexpf(1.0f, -cs) : 0.0f;
        dscale = dstage ? __builtin_amdgcn_ldexpf(1.0f, ds) : 0.0f, dinv = dstage ? __builtin_amdgcn_ldexpf(1.0f, -ds) : 0.0f;
    }
    const bool any_stage = (cstage && (g_rgb != nullptr || g_bg != nullptr)) || (dstage && g_dep != nullptr);
    const int4 box_front = box[0];
    for (int k = D - 1; k >= 0; --k) {
        const ColDst ct = col_dst(k);
        const int4 bb = box[k];
        const bool want_window = any_stage && bb.z > 0;   // uniform
        if (want_window) {
            const bool inside = w_open && bb.x >= wx0 && bb.y >= wy0 && bb.x + bb.z <= wx0 + kCW && bb.y + bb.w <= wy0 + kCH;
            if (!inside) {
                if (w_open) {
                    lds_barrier();   // the adds of the planes behind are complete
                    flush(col_dst(k + 1), 4);
                    lds_barrier();   // the window is clean before the first add under the new anchor
                }
                // re-anchor: the box at the end of the window it drifts away from (boxes of nearer planes: towards box_front)
                wx0 = (box_front.z > 0 && box_front.x < bb.x) ? bb.x + bb.z - kCW : bb.x;
                wy0 = (box_front.z > 0 && box_front.y < bb.y) ? bb.y + bb.w - kCH : bb.y;
                wrow0 = kCH, wrow1 = 0;
                w_open = true;
            }
            wrow0 = min(wrow0, bb.y - wy0), wrow1 = max(wrow1, bb.y + bb.w - wy0);
        }
        if (k > 0) fetch(k - 1, tp);   // (in flight across the scatter)
        scatter(k, G, ct, want_window);
        if (k > 0) grads(k - 1, tp, G);
        // the last plane's colour belongs to the background image: its own flush of the colour channels (the window and its depth channel stay)
        if (k == D - 1 && bgi != nullptr && w_open && D > 1) {
            lds_barrier();
            flush(ct, 3);
            lds_barrier();
        }
    }
    if (w_open) {
        lds_barrier();
        flush(col_dst(0), 4);
    }
}

// ---- launcher --------------------------------------------------------------------------------------------------------------------------------
bool depth_tile_supports(const KParams& p) { return p.D <= kSPlanes; }
int depth_tile_planes() { return kSPlanes; }

template <typename TexT>
static hipError_t launch_depth_backward_tile_t(const KParams& p, const SharedK& sh, const DepthK& dk, const SharedG& g, hipStream_t stream) {
    const int tiles_x = (p.W + kDTW - 1) / kDTW, n_tiles = tiles_x * ((p.H + kDTH - 1) / kDTH);
    const dim3 grid(xcd_grid_per_group(n_tiles, n_tiles), p.N);
    dispatch_bool(p.flags & GMPI_FLAG_ALIGN_CORNERS, [&](auto AC) {
        hipLaunchKernelGGL((render_depth_tile_kernel<TexT, decltype(AC)::value>), grid, dim3(kDThreads), 0, stream, p, sh, dk, g, tiles_x);
    });
    return hipGetLastError();
}

// (the caller has asked depth_tile_supports)
hipError_t launch_depth_backward_tile(const KParams& p, int dtype, const SharedK& sh, const DepthK& dk, const SharedG& g, hipStream_t stream) {
    return dispatch_dtype(dtype, [&](auto t) { return launch_depth_backward_tile_t<typename decltype(t)::type>(p, sh, dk, g, stream); });
}

}  // namespace gmpi
