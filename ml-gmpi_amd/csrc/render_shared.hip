// render_shared.hip -- the shared-colour layout (gmpi_mpi_render_shared_launch / _backward_launch, include/gmpi_render.h): ONE colour image per MPI,
// D alpha planes and, optionally, a separate colour image for the last plane -- what GMPI's generator produces before it expands and concatenates
// (networks_cond_on_pos_enc.py:950-975, gmpi.yml:137-145).  By definition the result is the render of the expanded volume; per plane and channel
// the arithmetic below IS the volume kernels' (plane_coord, footprint, bilerp, blend; BwdPixel::plane, XT, total_transmittance), so the strict-order
// forward is bit-identical to render_gather.hip on the expanded volume.
//
//   render_shared_kernel           forward, one pixel per lane, any shape / stride / dtype / ray field, every flag
//   render_shared_backward_kernel  backward, one pixel per lane, 16 global atomics per pixel and plane (the cross-check, and the fall-back for D > 128)
//   render_shared_tile_kernel      backward, one workgroup per 32 x 16 pixel tile: alpha gradient staged per plane, colour gradient summed in LDS
//                                  ACROSS the planes (see the kernel)
//
// KParams carries the alpha planes in its volume fields: rgba = alpha [M,D,1,Ht,Wt], s_mpi / s_plane / s_row its strides, s_chan = 0 (so that the
// 4-channel helpers that only want the alpha sample -- total_transmittance -- read the alpha plane four times instead of leaving it).
#include "gmpi_backward.hpp"
#include "gmpi_shared.hpp"

namespace gmpi {

// ---- forward: render_gather_kernel with the colour taken from one image -------------------------------------------------------------------------
template <typename TexT, bool AC, bool STRICT>
__global__ __launch_bounds__(256) void render_shared_kernel(const KParams p, const SharedK sh) {
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
    const TexT* __restrict__ alpha = static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(m) * p.s_mpi;
    const TexT* __restrict__ rgb = static_cast<const TexT*>(sh.rgb) + static_cast<int64_t>(m) * sh.rs_mpi;
    const TexT* __restrict__ bgi = sh.bg ? static_cast<const TexT*>(sh.bg) + static_cast<int64_t>(m) * sh.bs_mpi : nullptr;

    Accum A;
    for (int k = 0; k < p.D; ++k) {
        float ix, iy, s, u, v;
        plane_coord<AC>(vw.dhw[3 * k] - vw.ez, vw.dhw[3 * k + 1], vw.dhw[3 * k + 2], vw.ex, vw.ey, rx, ry, rz, vw.cx, vw.cy, ix, iy, s, u, v);
        // (leaves_last_plane's test on the u, v the loop has anyway: after the loop it costs the strict bf16 instances 2 VGPRs)
        if (check_last && k == p.D - 1 && outside_pm1(u, v)) bad |= GMPI_STATUS_OUT_OF_LAST_PLANE;
        const Taps t = make_taps(ix, iy, Ht, Wt);
        const bool last_bg = bgi != nullptr && k == p.D - 1;   // uniform
        float smp[4];
        shared_sample<TexT, STRICT>(alpha + static_cast<int64_t>(k) * p.s_plane, p.s_row, last_bg ? bgi : rgb, last_bg ? sh.bs_chan : sh.rs_chan,
                                    last_bg ? sh.bs_row : sh.rs_row, t, check_range, bad, smp);
        blend<STRICT>(A, smp[0], smp[1], smp[2], smp[3], s, dot);
    }
    store_pixel<STRICT>(p, n, HW, pix, A, dot, active);
    report_status(p.status, bad);
}

// where the colour gradient of plane k goes: the shared image, or the background on the last plane (nullptr: nobody wants it)
struct ColTarget {
    float* base;
    int64_t s_chan, s_row;
};
__device__ __forceinline__ ColTarget colour_target(const SharedK& sh, const SharedG& g, int m, int k, int D) {
    if (sh.bg != nullptr && k == D - 1) return ColTarget{g.g_bg ? g.g_bg + static_cast<int64_t>(m) * g.gb_mpi : nullptr, g.gb_chan, g.gb_row};
    return ColTarget{g.g_rgb ? g.g_rgb + static_cast<int64_t>(m) * g.gr_mpi : nullptr, g.gr_chan, g.gr_row};
}
// one value scattered to the four texels of a footprint (weights of taps outside the texture are zero: those are never written)
__device__ __forceinline__ void scatter4(float* __restrict__ ch, int64_t s_row, const Footprint& f, float d) {
    const int64_t oa = static_cast<int64_t>(f.y0) * s_row + f.x0, ob = oa + s_row;
    if (f.nw != 0.0f) atomicAdd(ch + oa, d * f.nw);
    if (f.ne != 0.0f) atomicAdd(ch + oa + 1, d * f.ne);
    if (f.sw != 0.0f) atomicAdd(ch + ob, d * f.sw);
    if (f.se != 0.0f) atomicAdd(ch + ob + 1, d * f.se);
}

// ---- backward, one pixel per lane: render_backward_kernel's sweep, three destinations --------------------------------------------------------
template <typename TexT, bool AC>
__global__ __launch_bounds__(256) void render_shared_backward_kernel(const KParams p, const SharedK sh, const SharedG g) {
    const int n = blockIdx.z;
    const int px = blockIdx.x * 64 + threadIdx.x;
    const int py = blockIdx.y * 4 + threadIdx.y;
    if (px >= p.W || py >= p.H) return;
    uint32_t unused = 0;
    const BwdView vw = bwd_view<AC>(p, n);
    const int m = vw.m;
    const int Ht = p.Ht, Wt = p.Wt;
    const TexT* __restrict__ alpha = static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(m) * p.s_mpi;
    const TexT* __restrict__ rgb = static_cast<const TexT*>(sh.rgb) + static_cast<int64_t>(m) * sh.rs_mpi;
    const TexT* __restrict__ bgi = sh.bg ? static_cast<const TexT*>(sh.bg) + static_cast<int64_t>(m) * sh.bs_mpi : nullptr;
    float* __restrict__ ga = g.g_alpha ? g.g_alpha + static_cast<int64_t>(m) * g.ga_mpi : nullptr;

    BwdPixel bp;
    bwd_pixel_setup<TexT, AC, false>(bp, p, vw, n, px, py, true, g.g_out, g.g_depth, g.g_T, alpha);
    for (int k = p.D - 1; k >= 0; --k) {
        float ix, iy, s;
        pixel_plane_coord<AC>(vw, bp, k, ix, iy, s);
        const Taps t = make_taps(ix, iy, Ht, Wt);
        const bool last_bg = bgi != nullptr && k == p.D - 1;
        float smp[4], d_s[4];
        shared_sample<TexT, false>(alpha + static_cast<int64_t>(k) * p.s_plane, p.s_row, last_bg ? bgi : rgb, last_bg ? sh.bs_chan : sh.rs_chan,
                                   last_bg ? sh.bs_row : sh.rs_row, t, false, unused, smp);
        bp.plane(smp, s, d_s);
        const ColTarget ct = colour_target(sh, g, m, k, p.D);
        if (ct.base != nullptr) {
#pragma unroll
            for (int c = 0; c < 3; ++c) scatter4(ct.base + c * ct.s_chan, ct.s_row, t.f, d_s[c]);
        }
        if (ga != nullptr) scatter4(ga + static_cast<int64_t>(k) * g.ga_plane, g.ga_row, t.f, d_s[3]);
    }
}

// ---- backward, one workgroup per pixel tile ------------------------------------------------------------------------------------------------
// A 32 x 16 pixel tile touches a small texel box on every plane (tile_box, gmpi_backward.hpp).  The frame -- tile order, box table, the moving window and
// its flush, the fixed-point scale and adds -- is "the cross-plane tile frame" of gmpi_backward.hpp; the tap prefetch is fetch_taps (gmpi_shared.hpp).
//
// ALPHA: as the volume kernels do it -- the 4 adds of a pixel go to a copy of the plane's box in LDS (64-bit fixed point, scaled per plane to the
// tile's largest |d alpha|: that gradient holds S / om and has no bound known in advance), the box is flushed with one global atomic per texel.
// Two boxes alternate, so that the flush of plane t + 1 and the scatter of plane t need no barrier between them: ONE barrier per plane, and that
// barrier orders LDS only (lds_barrier); the taps of plane t - 1 are fetched before plane t is scattered.
//
// COLOUR, the point of this kernel: every plane's colour gradient belongs to the same image, so it is summed in LDS across ALL planes, in a
// MovingWindow of 3 channels.  The window does NOT hold the union of the tile's per-plane boxes: the boxes drift over the planes by parallax -- with
// the FFHQ geometry (planes 0.2473 wide) 1.1 / 1.7 / 3.3 texels per plane in x and 0.5 / 1.1 / 2.3 in y on average at 256^2 / 512^2 / 1024^2, 30-100 texels
// over 32 planes against 29 x 13 texels of slack around a 35 x 19 box; and the last plane is a larger background plane whose box lies elsewhere.  So the
// window moves (MovingWindow's re-anchor rule).  Colour flushes per tile (tools/shared_window_replay.py, 32 planes, the poses tools/time_shared_color.py
// draws): 2.8 / 3.9 / 6.1 on average at 256^2 / 512^2 / 1024^2 (max 4 / 7 / 13) instead of 32 per-plane flushes; at the 2-sigma corner of the pose range
// 6.6 / 10.8 / 18.1 (max 31 at 1024^2: one per plane).  A plane whose own box does not fit the alpha box (strong minification, degenerate rays)
// scatters straight to global memory, both gradients, as in render_backward.hip.
// A colour flush empties all the window holds, so its row range is reset after EVERY flush, the background's included.  The per-plane barrier is also the
// one a colour flush relies on (every add of the planes behind is complete); one more follows the flush, before the next add.
//
// FIXED POINT of the colour window.  The scale cannot follow the planes; it is fixed per tile before the sweep from M = max over the tile's pixels
// of max(|gR|, |gG|, |gB|) (OUT_PM1's factor 2 included).  A term is gC w_k weight with w_k = a_k T_k <= 1 (alpha in [0, 1]: T_k <= (1 + 1e-10)^k) and a
// bilinear weight <= 1, so |term| <= M < 2^(e + 1), e = floor(log2 M).  Scaled by 2^(40 - e) a term is below 2^41.  Terms that can meet in one cell: a pixel
// adds each plane's sample to four DIFFERENT texels, so at most one term per pixel, plane and channel: 512 D <= 2^9 x 2^7 = 2^16 (D <= 128 here).
// |sum| < 2^57: 6 bits to spare in a signed 64-bit word.  The spare bits matter: a volume outside [0, 1] (range check off) can have w_k > 1; a lane whose
// scaled gradient reaches 2^42 -- or is not finite -- therefore scatters that plane's colour straight to global memory, which keeps every staged
// term below 2^42 and the sum below 2^58 whatever the inputs.  Resolution: 2^-41 M per add (round to nearest) -- finer than one fp32 atomic add's 2^-24 of
// the running sum.  Integer sums are exact and order-independent; the only fp32 rounding of the staged part is the conversion at the flush.
// (Plain fp32 LDS adds were not shipped: ds_add_f32 retires ~0.2 T lane-adds/s against ~9 T for ds_add_u64 on this part -- tools/ubench/lds_atomic_rate.hip,
// render_backward.hip.)
constexpr int kSAP = 56, kSAR = 27;   // alpha box: pitch, rows (64-bit words; two boxes of 11.8 KB); also the largest box whose plane is staged at all

template <typename TexT, bool AC>
__global__ __launch_bounds__(kTileThreads) void render_shared_tile_kernel(const KParams p, const SharedK sh, const SharedG g, const int tiles_x) {
    __shared__ int4 box[kTilePlanes];        // bx0, by0, nx (<= 0: not staged), ny
    __shared__ uint32_t gmax[kTilePlanes];   // per plane: largest |d alpha| of the tile, fp32 bits
    __shared__ uint32_t cmax;                // largest |gC| of the tile, fp32 bits
    __shared__ unsigned long long acc_a[2][kSAP * kSAR];
    __shared__ unsigned long long acc_c[3 * kCW * kCH];
    const int tid = threadIdx.x;
    const int n = blockIdx.y;
    const TileFrame tf = tile_frame(p, tiles_x);
    if (tf.tile < 0) return;
    const bool active = tf.active;
    const BwdView vw = bwd_view<AC>(p, n);
    const int m = vw.m, D = p.D;
    const int Ht = p.Ht, Wt = p.Wt;
    const TexT* __restrict__ alpha = static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(m) * p.s_mpi;
    const TexT* __restrict__ rgb = static_cast<const TexT*>(sh.rgb) + static_cast<int64_t>(m) * sh.rs_mpi;
    const TexT* __restrict__ bgi = sh.bg ? static_cast<const TexT*>(sh.bg) + static_cast<int64_t>(m) * sh.bs_mpi : nullptr;
    float* __restrict__ ga = g.g_alpha ? g.g_alpha + static_cast<int64_t>(m) * g.ga_mpi : nullptr;
    BwdPixel bp;
    bwd_pixel_setup<TexT, AC, true>(bp, p, vw, n, tf.px, tf.py, active, g.g_out, g.g_depth, g.g_T, alpha);

    for (int i = tid; i < 2 * kSAP * kSAR; i += kTileThreads) (&acc_a[0][0])[i] = 0ull;
    for (int i = tid; i < 3 * kCW * kCH; i += kTileThreads) acc_c[i] = 0ull;
    if (tid == 0) cmax = 0u;
    for (int k = tid; k < D; k += kTileThreads) {
        box[k] = tile_frame_box<AC>(p, vw, tf, k, kSAP, kSAR);
        gmax[k] = 0u;
    }
    __syncthreads();   // zero fills, tables, cmax = 0
    {   // the tile's largest |gC|: one LDS atomic per wave
        const uint32_t wm = wave_max_bits(max(abs_bits(bp.gr), max(abs_bits(bp.gg), abs_bits(bp.gb))));
        if ((tid & 63) == 0 && wm != 0u) atomicMax(&cmax, wm);
    }

    struct Grad { float d[4]; Footprint f; };
    auto fetch = [&](int k, Tap& tp) { fetch_taps<AC>(tp, active, p, vw, bp, k, sh, rgb, bgi, alpha, p.s_plane, p.s_row); };
    // second half: bilinear samples (tap_sample's arithmetic), BwdPixel::plane, the tile maximum of |d alpha|
    auto grads = [&](int k, const Tap& tp, Grad& G) {
        G.d[0] = G.d[1] = G.d[2] = G.d[3] = 0.0f;
        G.f = tp.f;
        if (active) {
            float smp[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) smp[c] = bilerp<false>(tp.v[4 * c + 0], tp.v[4 * c + 1], tp.v[4 * c + 2], tp.v[4 * c + 3], tp.f);
            bp.plane(smp, tp.s, G.d);
        }
        const uint32_t wm = wave_max_bits(abs_bits(G.d[3]));
        if ((tid & 63) == 0 && wm != 0u) atomicMax(&gmax[k], wm);
    };

    MovingWindow win;   // the colour window
    FixScale cs{false, 0.0f, 0.0f};
    // window -> global memory (one atomic per texel and channel) and reset
    auto flush_colour = [&](const ColTarget& ct) {
        if (ct.base != nullptr)
            win.flush(acc_c, tid, 3, Ht, Wt, [&](int c, int gx, int gy, float v) {
                atomicAdd(ct.base + c * ct.s_chan + static_cast<int64_t>(gy) * ct.s_row + gx, v * cs.inv);
            });
        win.reset_rows();
    };
    // scatter of one plane: alpha into its box (per-plane scale), colour into the window (tile scale); what is not staged goes straight to global memory
    auto scatter = [&](int k, const Grad& G, const ColTarget& ct, bool col_staged) {
        const int4 bb = box[k];
        const uint32_t mb = gmax[k];
        const Footprint& f = G.f;
        const bool any_w = f.nw != 0.0f || f.ne != 0.0f || f.sw != 0.0f || f.se != 0.0f;
        const int lx = f.x0 - bb.x, ly = f.y0 - bb.y;
        const bool in_box = bb.z > 0 && lx >= 0 && ly >= 0 && lx + 1 < bb.z && ly + 1 < bb.w;
        if (ga != nullptr && mb != 0u && any_w) {
            const FixScale as = fix_scale(mb, kFixBits);
            if (in_box && as.stage) {
                lds_add_taps(&acc_a[k & 1][ly * kSAP + lx], kSAP, G.d[3], f.nw, f.ne, f.sw, f.se, as.scale);
            } else {
                scatter4(ga + static_cast<int64_t>(k) * g.ga_plane, g.ga_row, f, G.d[3]);
            }
        }
        if (ct.base != nullptr && any_w) {
            const float dm = fmaxf(fmaxf(fabsf(G.d[0]), fabsf(G.d[1])), fabsf(G.d[2]));
            // (dm * scale < 2^42 is false for NaN; in_box implies the footprint lies inside the window, holds() keeps wild coordinates out)
            const bool staged = col_staged && in_box && win.holds(f) && (dm * cs.scale < 4398046511104.0f);
            if (staged) {
#pragma unroll
                for (int c = 0; c < 3; ++c) lds_add_taps(acc_c + c * (kCH * kCW) + win.cell(f), kCW, G.d[c], f.nw, f.ne, f.sw, f.se, cs.scale);
            } else if (dm != 0.0f) {
#pragma unroll
                for (int c = 0; c < 3; ++c) scatter4(ct.base + c * ct.s_chan, ct.s_row, f, G.d[c]);
            }
        }
    };
    // box of plane k -> global memory and reset (the plane's own scale)
    auto flush_alpha = [&](int k) {
        const int4 bb = box[k];
        const FixScale as = fix_scale(gmax[k], kFixBits);
        if (!(ga != nullptr && bb.z > 0 && as.stage)) return;
        float* __restrict__ gp = ga + static_cast<int64_t>(k) * g.ga_plane;
        for (int i = tid; i < bb.w * kSAP; i += kTileThreads) {
            const int row = i / kSAP, x = i - row * kSAP;
            unsigned long long* __restrict__ src = &acc_a[k & 1][i];
            const long long v = static_cast<long long>(*src);
            const int gx = bb.x + x, gy = bb.y + row;
            if (v != 0) {
                *src = 0ull;
                if (gx >= 0 && gx < Wt && gy >= 0 && gy < Ht)
                    atomicAdd(gp + static_cast<int64_t>(gy) * g.ga_row + gx, static_cast<float>(static_cast<double>(v)) * as.inv);
            }
        }
    };

    // ---- back-to-front sweep, software-pipelined by one plane -----------------------------------------------------------------------------------
    Grad G;
    Tap tp;
    fetch(D - 1, tp);
    grads(D - 1, tp, G);
    __syncthreads();   // cmax, gmax[D - 1] complete
    cs = fix_scale(cmax, kFixBits);
    const int4 box_front = box[0];
    for (int k = D - 1; k >= 0; --k) {
        const ColTarget ct = colour_target(sh, g, m, k, D);
        const int4 bb = box[k];
        const bool want_window = cs.stage && ct.base != nullptr && bb.z > 0;   // uniform
        if (want_window) {
            if (!win.covers(bb)) {
                if (win.open) {   // the previous planes' adds are complete (the barrier that ended the last iteration)
                    flush_colour(colour_target(sh, g, m, k + 1, D));
                    lds_barrier();
                }
                win.anchor(bb, box_front);
            }
            win.grow(bb);
        }
        if (k > 0) fetch(k - 1, tp);   // (in flight across the scatter)
        scatter(k, G, ct, want_window);
        if (k > 0) grads(k - 1, tp, G);
        if (k + 1 < D) flush_alpha(k + 1);
        lds_barrier();   // plane k's adds and gmax[k - 1] complete; box (k + 1) & 1 is clean for plane k - 1
        // the last plane's colour belongs to the background image: its own flush (the window stays where it is)
        if (k == D - 1 && bgi != nullptr && win.open && D > 1) {
            flush_colour(ct);
            lds_barrier();
        }
    }
    flush_alpha(0);
    if (win.open) flush_colour(colour_target(sh, g, m, 0, D));
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------
template <typename TexT>
static hipError_t launch_shared_t(const KParams& p, const SharedK& sh, hipStream_t stream) {
    const dim3 block(64, 4);
    const dim3 grid((p.W + 63) / 64, (p.H + 3) / 4, p.N);
    dispatch_ac_strict(p.flags, [&](auto AC, auto STRICT) {
        hipLaunchKernelGGL((render_shared_kernel<TexT, decltype(AC)::value, decltype(STRICT)::value>), grid, block, 0, stream, p, sh);
    });
    return hipGetLastError();
}

hipError_t launch_shared(const KParams& p, int dtype, const SharedK& sh, hipStream_t stream) {
    return dispatch_dtype(dtype, [&](auto t) { return launch_shared_t<typename decltype(t)::type>(p, sh, stream); });
}

bool shared_tile_supports(const KParams& p) { return tile_planes_fit(p); }

template <typename TexT>
static hipError_t launch_shared_backward_t(const KParams& p, const SharedK& sh, const SharedG& g, bool tiles, hipStream_t stream) {
    const bool ac = p.flags & GMPI_FLAG_ALIGN_CORNERS;
    if (tiles) {
        const TileGrid tg = tile_grid(p);
        dispatch_bool(ac, [&](auto AC) { hipLaunchKernelGGL((render_shared_tile_kernel<TexT, decltype(AC)::value>), tg.grid, dim3(kTileThreads), 0, stream, p, sh, g, tg.tiles_x); });
    } else {
        const dim3 block(64, 4);
        const dim3 grid((p.W + 63) / 64, (p.H + 3) / 4, p.N);
        dispatch_bool(ac, [&](auto AC) { hipLaunchKernelGGL((render_shared_backward_kernel<TexT, decltype(AC)::value>), grid, block, 0, stream, p, sh, g); });
    }
    return hipGetLastError();
}

hipError_t launch_shared_backward(const KParams& p, int dtype, const SharedK& sh, const SharedG& g, bool tiles, hipStream_t stream) {
    tiles = tiles && shared_tile_supports(p);
    return dispatch_dtype(dtype, [&](auto t) { return launch_shared_backward_t<typename decltype(t)::type>(p, sh, g, tiles, stream); });
}

}  // namespace gmpi
