// render_depth_tile.hip -- the tile backward of the depth-alpha layout (gmpi_mpi_render_depth_backward_tile_launch, include/gmpi_render.h).
//
//   render_depth_tile_kernel   backward, one workgroup per 32 x 16 pixel tile: ALL four gradient channels -- R, G, B of the colour image and the
//                              depth image -- are summed in LDS ACROSS the planes, in one moving window
//
// The arithmetic is render_depth_backward_kernel's (render_depth.hip), term for term: pixel_plane_coord, make_taps, the ramp of depth_ramp over the
// four depth taps with its inclusive mask, bilerp, BwdPixel::plane, -div_by_recip(d alpha, den, rden) on the ramp, the sweep started from
// depth_total_transmittance (gmpi_shared.hpp).  What differs is where the adds go.  The frame -- tile order, per-plane texel boxes, the moving window and
// its flush, the fixed-point scale and adds -- is "the cross-plane tile frame" of gmpi_backward.hpp, the text render_shared_tile_kernel (render_shared.hip)
// runs too; the tap prefetch is fetch_taps (gmpi_shared.hpp).
//
// ONE WINDOW.  In the shared-colour layout the alpha gradient has D destination planes and is flushed per plane.  Here the gradient of all D alpha
// planes lands in the one depth image, so the depth channel lives in the same MovingWindow as the three colour channels: 4 channels = 64 KiB (+ the
// 2 KiB box table and the maxima: 67.6 KB, two workgroups per CU), no per-plane box, no per-plane flush; a box is staged when it fits the window itself.
// With a background image the last plane's colour belongs to another image: the three colour channels are flushed to it right after plane D - 1; the
// depth channel stays, it has one destination -- so the window's row range is reset only when it is re-anchored, never by a flush.
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

template <typename TexT, bool AC>
__global__ __launch_bounds__(kTileThreads) void render_depth_tile_kernel(const KParams p, const SharedK sh, const DepthK dk, const SharedG g, const int tiles_x) {
    __shared__ int4 box[kTilePlanes];   // bx0, by0, nx (<= 0: not staged), ny
    __shared__ uint32_t cmax, dmax;  // the tile's M_c, M_d (fp32 bits)
    __shared__ uint32_t zmax;        // max_k |zdiff_k| of the view (fp32 bits)
    __shared__ unsigned long long acc[4 * kCW * kCH];
    const int tid = threadIdx.x;
    const int n = blockIdx.y;
    const TileFrame tf = tile_frame(p, tiles_x);
    if (tf.tile < 0) return;
    const bool active = tf.active;
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
    bwd_pixel_setup_with<true>(bp, p, vw, n, tf.px, tf.py, active, g.g_out, g.g_depth, g.g_T,
                               [&](float t_fwd) { return depth_total_transmittance<TexT, AC>(p, vw, bp, depth, pz, dk, t_fwd); });

    for (int i = tid; i < 4 * kCW * kCH; i += kTileThreads) acc[i] = 0ull;
    if (tid == 0) cmax = 0u, dmax = 0u, zmax = 0u;
    __syncthreads();   // zmax = 0
    for (int k = tid; k < D; k += kTileThreads) {   // a box is staged when it fits the window
        box[k] = tile_frame_box<AC>(p, vw, tf, k, kCW, kCH);
        atomicMax(&zmax, abs_bits(vw.dhw[3 * k] - vw.ez));
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

    struct Grad {
        Footprint f;
        float d[3], gq;   // d colour sample, d depth sample (-d alpha / den)
        float wd[4];      // weights of the depth taps: inside the texture and on the ramp
        bool col, dep;    // the plane has a weight (w_k != 0) / a tap on the ramp
    };
    auto fetch = [&](int k, Tap& tp) { fetch_taps<AC>(tp, active, p, vw, bp, k, sh, rgb, bgi, depth, 0, p.s_row); };
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
    MovingWindow win;
    FixScale cs{false, 0.0f, 0.0f}, ds{false, 0.0f, 0.0f};   // colour, depth
    // channels [0, nc) of the window -> global memory, one atomic per cell.  nc = 3: the colour channels (to ct), 4: with the depth channel.
    auto flush = [&](const ColDst& ct, int nc) {
        win.flush(acc, tid, nc, Ht, Wt, [&](int c, int gx, int gy, float v) {
            if (c < 3) {
                if (ct.base != nullptr) atomicAdd(ct.base + c * ct.s_chan + static_cast<int64_t>(gy) * ct.s_row + gx, v * cs.inv);
            } else if (g_dep != nullptr) {
                atomicAdd(g_dep + static_cast<int64_t>(gy) * g.ga_row + gx, v * ds.inv);
            }
        });
    };
    // the adds of one plane: into the window, or straight to global memory
    auto scatter = [&](int k, const Grad& G, const ColDst& ct, bool staged) {
        const bool col = G.col && ct.base != nullptr, dep = G.dep;
        if (!col && !dep) return;
        const Footprint& f = G.f;
        const int4 bb = box[k];
        const int lx = f.x0 - bb.x, ly = f.y0 - bb.y;
        // (the box lies inside the window; holds() keeps wild coordinates out whatever the box is)
        const bool in_win = staged && bb.z > 0 && lx >= 0 && ly >= 0 && lx + 1 < bb.z && ly + 1 < bb.w && win.holds(f);
        const float dm = fmaxf(fmaxf(fabsf(G.d[0]), fabsf(G.d[1])), fabsf(G.d[2]));
        // (x < 2^42 is false for NaN)
        const bool c_ok = !col || (cs.stage && dm * cs.scale < 4398046511104.0f);
        const bool d_ok = !dep || (ds.stage && fabsf(G.gq) * ds.scale < 4398046511104.0f);
        if (in_win && c_ok && d_ok) {
            unsigned long long* __restrict__ l0 = acc + win.cell(f);
            if (col) {
#pragma unroll
                for (int c = 0; c < 3; ++c) lds_add_taps(l0 + c * (kCH * kCW), kCW, G.d[c], f.nw, f.ne, f.sw, f.se, cs.scale);
            }
            if (dep) lds_add_taps(l0 + 3 * (kCH * kCW), kCW, G.gq, G.wd[0], G.wd[1], G.wd[2], G.wd[3], ds.scale);
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
    cs = fix_scale(cmax, kFixBits), ds = fix_scale(dmax, kFixBits);
    const bool any_stage = (cs.stage && (g_rgb != nullptr || g_bg != nullptr)) || (ds.stage && g_dep != nullptr);
    const int4 box_front = box[0];
    for (int k = D - 1; k >= 0; --k) {
        const ColDst ct = col_dst(k);
        const int4 bb = box[k];
        const bool want_window = any_stage && bb.z > 0;   // uniform
        if (want_window) {
            if (!win.covers(bb)) {
                if (win.open) {
                    lds_barrier();   // the adds of the planes behind are complete
                    flush(col_dst(k + 1), 4);
                    lds_barrier();   // the window is clean before the first add under the new anchor
                }
                win.anchor(bb, box_front);
            }
            win.grow(bb);
        }
        if (k > 0) fetch(k - 1, tp);   // (in flight across the scatter)
        scatter(k, G, ct, want_window);
        if (k > 0) grads(k - 1, tp, G);
        // the last plane's colour belongs to the background image: its own flush of the colour channels (the window and its depth channel stay)
        if (k == D - 1 && bgi != nullptr && win.open && D > 1) {
            lds_barrier();
            flush(ct, 3);
            lds_barrier();
        }
    }
    if (win.open) {
        lds_barrier();
        flush(col_dst(0), 4);
    }
}

// ---- launcher --------------------------------------------------------------------------------------------------------------------------------
bool depth_tile_supports(const KParams& p) { return tile_planes_fit(p); }
int depth_tile_planes() { return kTilePlanes; }

template <typename TexT>
static hipError_t launch_depth_backward_tile_t(const KParams& p, const SharedK& sh, const DepthK& dk, const SharedG& g, hipStream_t stream) {
    const TileGrid tg = tile_grid(p);
    dispatch_bool(p.flags & GMPI_FLAG_ALIGN_CORNERS, [&](auto AC) {
        hipLaunchKernelGGL((render_depth_tile_kernel<TexT, decltype(AC)::value>), tg.grid, dim3(kTileThreads), 0, stream, p, sh, dk, g, tg.tiles_x);
    });
    return hipGetLastError();
}

// (the caller has asked depth_tile_supports)
hipError_t launch_depth_backward_tile(const KParams& p, int dtype, const SharedK& sh, const DepthK& dk, const SharedG& g, hipStream_t stream) {
    return dispatch_dtype(dtype, [&](auto t) { return launch_depth_backward_tile_t<typename decltype(t)::type>(p, sh, dk, g, stream); });
}

}  // namespace gmpi
