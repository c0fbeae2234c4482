// render_depth_window.hip -- the window forward of the depth-alpha layout (gmpi_mpi_render_depth_window_launch, include/gmpi_render.h).
//
//   render_depth_window_kernel   forward, one workgroup of 512 threads per 32 x 16 pixel tile, one pixel per thread, planes front to back; every tap
//                                comes from ONE window of R, G, B and depth texels in LDS that moves with the tile's texel boxes
//
// The arithmetic is render_depth_kernel's (render_depth.hip), term for term: plane_coord, the last-plane test, make_taps, depth_ramp on the four depth
// taps, bilerp, the `a != 0` skip, three colour samples, blend, store_pixel, report_status.  What differs is where the taps come from.  In this layout
// all four channels are single images shared by every plane, so nothing new has to be read per plane: a tile's texel boxes (tile_box, gmpi_device.hpp)
// only drift by parallax, and one window of kCW x kCH texels (the tile backward's, here fp32 texels [row][channel][x]: 32 KiB) serves many planes.
//
// WINDOW.  When the next staged plane's box is not inside the window, the window is re-anchored with that box at the end it drifts away from (the
// direction is taken from the next staged box of the box-table chunk), so that the whole slack lies ahead, and reloaded as a whole: thread -> (row, item
// of 4 texels) fixed, one 16-byte load (8 bytes of 16-bit storage, converted on the way in) per channel.  The anchor column is a multiple of 4 texels, so
// that every item is aligned: a box is staged when, widened to whole items, it fits the window.  Texels outside the texture are stored as zeros and the
// weights of taps outside the texture are zeroed as make_taps zeroes them.  On plane D - 1 with a background the three colour channels are reloaded from
// background[m] (the depth channel has one source and stays).
//
// FALL-BACKS.  A (tile, plane) whose box does not fit the window or whose corners are not finite, and a single pixel whose 2 x 2 footprint is not
// inside the window (no pinhole ray field, a NaN ray), take render_depth_kernel's taps from global memory: clamped addresses, the same weights.  The
// result of a pixel does not depend on the path, with one exception the other staged forward shares: a tap OUTSIDE the texture reads a zero here and the
// clamped border texel there -- the same bits times a zero weight unless that border texel is not finite, and no range bit for it.
//
// TILE-LEVEL PLANE SKIP.  While the window is loaded its in-texture depth texels are reduced to their minimum dmin and to "any NaN".  A staged plane k
// with RN(plane_z[k] - dmin) <= z_lo and no NaN has every alpha tap of the window exactly 0 (fp32 subtraction is monotonic: d >= dmin gives
// RN(plane_z[k] - d) <= RN(plane_z[k] - dmin) <= z_lo), and the one-pixel kernel skips such a plane for every pixel whose taps lie in the window.  That
// is every pixel of a pinhole ray field; it is PROVED per pixel, once, before the plane loop: a pixel is `tame` when its ray slopes rx / rz, ry / rz lie
// between those of the tile's four corner pixels -- x_k = ex + (rx / rz) zdiff_k is monotonic in the slope on every plane, so the pixel's coordinates
// lie between the corners' and its footprint inside the box.  Only tame pixels skip; any other pixel runs every plane.  The plane on which
// GMPI_FLAG_CHECK_LAST_PLANE is evaluated runs its coordinate chain and skips only the sampling.
//
// BARRIERS.  Two per box-table chunk (kWChunk planes) and one before and one after every reload, none per plane.  Every condition that leads to a barrier
// is computed from the box table, the reduced window minimum and launch constants: workgroup-uniform.  Lanes outside the image shadow the last row /
// column of the image and pass every barrier.
#include "gmpi_backward.hpp"
#include "gmpi_shared.hpp"

namespace gmpi {

constexpr int kWTPI = 4, kWItems = kCW / kWTPI;   // texels per loader item, items per window row and channel
constexpr int kWLine = 4 * kCW;                   // floats per window row: [row][channel][x]
constexpr int kWChunk = 64;                       // planes per box-table refill
static_assert(kWItems * kCH == kTileThreads, "one loader item per thread and channel");
static_assert(kCH * kWLine * 4 + kWChunk * 16 + 128 <= 53 * 1024, "3 workgroups per CU");

template <typename TexT, bool AC, bool STRICT>
__global__ __launch_bounds__(kTileThreads) void render_depth_window_kernel(const KParams p, const SharedK sh, const DepthK dk, const int tiles_x,
                                                                            const int tiles_y, const int n_tiles) {
    using I4 = Item4<TexT>;
    using Raw = typename I4::Raw;
    __shared__ int4 box[kWChunk];   // bx0, by0, nx (0: not staged), ny
    __shared__ float wave_min[kTileThreads / 64];
    __shared__ int wave_nan[kTileThreads / 64];
    __shared__ __attribute__((aligned(16))) float win[kCH * kWLine];

    // ---- blockIdx -> tile, this lane's pixel, the tile's corner pixels: the tile frame of gmpi_device.hpp -----------------------------------------
    const int tid = threadIdx.x;
    FwdTile ft;
    if (!fwd_tile(p, fwd_tile_id(p, blockIdx.x, tiles_x, tiles_y, n_tiles), tiles_x, tiles_y, n_tiles, ft)) return;
    const int n = ft.n;

    uint32_t bad = 0;
    const View vw = view_setup<AC>(p, n, bad);
    check_camera_behind(p, vw, ft.rem == 0 && tid == 0);   // once per view
    const int D = p.D, Ht = p.Ht, Wt = p.Wt, H = p.H, W = p.W;
    const bool check_range = (p.flags & GMPI_FLAG_CHECK_RANGE) != 0;
    const bool check_last = (p.flags & GMPI_FLAG_CHECK_LAST_PLANE) != 0;
    const int64_t HW = vw.HW;
    const float* __restrict__ rdv = vw.rays;
    const TexT* __restrict__ depth = static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(vw.m) * p.s_mpi;
    const TexT* __restrict__ rgb = static_cast<const TexT*>(sh.rgb) + static_cast<int64_t>(vw.m) * sh.rs_mpi;
    const TexT* __restrict__ bgi = sh.bg ? static_cast<const TexT*>(sh.bg) + static_cast<int64_t>(vw.m) * sh.bs_mpi : nullptr;
    const float* __restrict__ pz = dk.plane_z + static_cast<int64_t>(vw.m) * dk.pz_stride;

    const TileLane tl = tile_lane<kTileW, kTileH>(ft.txi, ft.tyi, tid, W, H);
    const int64_t pix = tl.pix;
    const float rx = rdv[pix], ry = rdv[HW + pix], rz = rdv[2 * HW + pix];
    const float dot = ray_dot(vw, rx, ry, rz);
    const TileCorners tc = tile_corners<kTileW, kTileH>(ft.txi, ft.tyi, W, H);
    const int cx0 = tc.cx0, cx1 = tc.cx1, cy0 = tc.cy0, cy1 = tc.cy1;
    // tame: the ray's slopes lie between the four corner pixels' (a few ulp of tolerance: far below the box's 1/64 texel); false for NaN
    bool tame;
    {
        float lox = __builtin_inff(), hix = -__builtin_inff(), loy = lox, hiy = hix;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t q = static_cast<int64_t>((c & 2) ? cy1 : cy0) * W + ((c & 1) ? cx1 : cx0);
            const float cz = rdv[2 * HW + q], sx = rdv[q] / cz, sy = rdv[HW + q] / cz;
            lox = fminf(lox, sx), hix = fmaxf(hix, sx), loy = fminf(loy, sy), hiy = fmaxf(hiy, sy);
        }
        const float sx = rx / rz, sy = ry / rz;
        const float tx = 5e-7f * fmaxf(fabsf(lox), fabsf(hix)), ty = 5e-7f * fmaxf(fabsf(loy), fabsf(hiy));
        tame = sx >= lox - tx && sx <= hix + tx && sy >= loy - ty && sy <= hiy + ty && fabsf(hix - lox) < 1e30f && fabsf(hiy - loy) < 1e30f;
    }

    // ---- loader role: item lcol of window row lrow, the same for the four channels ----------------------------------------------------------------
    const int lrow = tid / kWItems, lcol = tid - lrow * kWItems;
    const bool ragged = (Wt % kWTPI) != 0;   // the last item of a texture row holds texels past its end (read from the row's padding, zeroed below)

    // the window: anchor texel, loaded or not, which image its colour channels hold, and what its depth texels reduce to (all workgroup-uniform)
    int wx0 = 0, wy0 = 0;
    bool open = false, holds_bg = false, any_nan = false;
    int dirx = 0, diry = 0;   // where the boxes drift: < 0 towards smaller coordinates
    float dmin = __builtin_inff();

    // channels [0, 3) from `col`, and channel 3 from the depth image when with_depth, for the window anchored at (wx0, wy0)
    auto reload = [&](bool with_depth, bool from_bg) {
        const int gx = wx0 + kWTPI * lcol, gy = wy0 + lrow;
        const bool ok = gx >= 0 && gx < Wt && gy >= 0 && gy < Ht;   // (gx is a multiple of 4: an item lies left of the texture as a whole or not at all)
        const int left = Wt - gx;                                   // texels of this item inside the texture row
        const TexT* __restrict__ col = from_bg ? bgi : rgb;
        const int64_t c_chan = from_bg ? sh.bs_chan : sh.rs_chan, c_row = from_bg ? sh.bs_row : sh.rs_row;
        Raw L[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) L[c] = Raw(0u);
        if (ok) {
#pragma unroll
            for (int c = 0; c < 3; ++c) L[c] = *reinterpret_cast<const Raw*>(col + c * c_chan + static_cast<int64_t>(gy) * c_row + gx);
            if (with_depth) L[3] = *reinterpret_cast<const Raw*>(depth + static_cast<int64_t>(gy) * p.s_row + gx);
        }
        float* __restrict__ dst = win + lrow * kWLine + kWTPI * lcol;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c == 3 && !with_depth) break;
            float4 q = I4::cvt(L[c]);
            if (ragged) {
                if (left < 2) q.y = 0.0f;
                if (left < 3) q.z = 0.0f;
                if (left < 4) q.w = 0.0f;
            }
            *reinterpret_cast<float4*>(dst + c * kCW) = q;
            if (c == 3) {   // the in-texture depth texels of this item -> the wave's minimum and NaN flag
                float m = __builtin_inff();
                bool nan = false;
                if (ok) {
                    m = q.x, nan = q.x != q.x;
                    if (left >= 2) m = fminf(m, q.y), nan |= q.y != q.y;
                    if (left >= 3) m = fminf(m, q.z), nan |= q.z != q.z;
                    if (left >= 4) m = fminf(m, q.w), nan |= q.w != q.w;
                    if (m != m) m = __builtin_inff();   // (fminf drops a NaN operand; a leading one is dropped here: the flag carries it)
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
                const int wn = __any(nan) ? 1 : 0;
                if ((tid & 63) == 0) wave_min[tid >> 6] = m, wave_nan[tid >> 6] = wn;
            }
        }
    };

    Accum A;
    for (int kc = 0; kc < D; kc += kWChunk) {
        const int kn = min(kWChunk, D - kc);
        __syncthreads();   // the previous chunk's table is no longer read
        if (tid < kn) {
            const int k = kc + tid;
            int4 bb = tile_box<AC>(p, vw, rdv, vw.dhw[3 * k] - vw.ez, vw.dhw[3 * k + 1], vw.dhw[3 * k + 2], cx0, cx1, cy0, cy1, kCW, kCH);
            // widened to whole loader items it must still fit the window
            if (bb.z > 0 && ((bb.x + bb.z + kWTPI - 1) & ~(kWTPI - 1)) - (bb.x & ~(kWTPI - 1)) > kCW) bb.z = 0;
            box[tid] = bb;
        }
        __syncthreads();   // table published

        for (int t = 0; t < kn; ++t) {
            const int k = kc + t;
            int4 bb = box[t];
            bb.x = __builtin_amdgcn_readfirstlane(bb.x), bb.y = __builtin_amdgcn_readfirstlane(bb.y);
            bb.z = __builtin_amdgcn_readfirstlane(bb.z), bb.w = __builtin_amdgcn_readfirstlane(bb.w);
            const bool staged = bb.z > 0;                        // uniform
            const bool last_bg = bgi != nullptr && k == D - 1;   // uniform
            if (staged) {
                const bool inside = open && bb.x >= wx0 && bb.y >= wy0 && bb.x + bb.z <= wx0 + kCW && bb.y + bb.w <= wy0 + kCH;
                if (!inside || last_bg != holds_bg) {
                    __syncthreads();   // every tap of the planes before has been read
                    if (!inside) {
                        // the drift: from this box to the next staged box of the chunk, centres compared (none, or equal: as it was).  Not the
                        // chunk's LAST box: plane D - 1 of the presets is enlarged, and its box says nothing about its neighbours' drift.
                        for (int u = t + 1; u < kn; ++u) {
                            const int4 nb = box[u];
                            if (__builtin_amdgcn_readfirstlane(nb.z) > 0) {
                                const int ddx = __builtin_amdgcn_readfirstlane(2 * nb.x + nb.z) - (2 * bb.x + bb.z);
                                const int ddy = __builtin_amdgcn_readfirstlane(2 * nb.y + nb.w) - (2 * bb.y + bb.w);
                                dirx = ddx != 0 ? ddx : dirx, diry = ddy != 0 ? ddy : diry;
                                break;
                            }
                        }
                        // the box at the end it drifts away from, so that the window's whole slack lies ahead
                        wx0 = dirx < 0 ? ((bb.x + bb.z + kWTPI - 1) & ~(kWTPI - 1)) - kCW : (bb.x & ~(kWTPI - 1));
                        wy0 = diry < 0 ? bb.y + bb.w - kCH : bb.y;
                        open = true;
                    }
                    reload(!inside, last_bg);
                    holds_bg = last_bg;
                    __syncthreads();   // the window is loaded
                    if (!inside) {
                        float m = wave_min[0];
                        int wn = wave_nan[0];
#pragma unroll
                        for (int w = 1; w < kTileThreads / 64; ++w) m = fminf(m, wave_min[w]), wn |= wave_nan[w];
                        dmin = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, m)));
                        any_nan = __builtin_amdgcn_readfirstlane(wn) != 0;
                    }
                }
            }
            const float z = pz[k];
            // the whole window lies in front of the ramp on this plane: every alpha tap taken from it is exactly 0
            const bool skip = staged && !any_nan && (z - dmin) <= dk.lo && tame;
            const bool last_checked = check_last && k == D - 1;
            if (skip && !last_checked) continue;
            float ix, iy, s, u, v;
            plane_coord<AC>(vw.dhw[3 * k] - vw.ez, vw.dhw[3 * k + 1], vw.dhw[3 * k + 2], vw.ex, vw.ey, rx, ry, rz, vw.cx, vw.cy, ix, iy, s, u, v);
            if (last_checked && outside_pm1(u, v)) bad |= GMPI_STATUS_OUT_OF_LAST_PLANE;
            if (skip) continue;
            const Taps tp = make_taps(ix, iy, Ht, Wt);
            const int lx = tp.f.x0 - wx0, ly = tp.f.y0 - wy0;
            const bool inw = staged && lx >= 0 && ly >= 0 && lx + 1 < kCW && ly + 1 < kCH;   // per lane: the 2 x 2 footprint lies inside the window
            // the plane for this pixel, given its taps: taps_of(c, q) fills the taps nw, ne, sw, se of channel c (3: depth)
            auto plane = [&](auto&& taps_of) {
                float q[4];
                taps_of(3, q);
                RampTaps r;
#pragma unroll
                for (int i = 0; i < 4; ++i) r.a[i] = depth_ramp<STRICT>(z, q[i], dk, r.in[i]);
                if (check_range && !(in_unit(r.a[0]) && in_unit(r.a[1]) && in_unit(r.a[2]) && in_unit(r.a[3]))) bad |= GMPI_STATUS_RGBA_RANGE;   // (a NaN depth)
                const float a = bilerp<STRICT>(r.a[0], r.a[1], r.a[2], r.a[3], tp.f);
                if (a != 0.0f) {   // (true for NaN)
                    float smp[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        taps_of(c, q);
                        if (check_range && !(in_unit(q[0]) && in_unit(q[1]) && in_unit(q[2]) && in_unit(q[3]))) bad |= GMPI_STATUS_RGBA_RANGE;
                        smp[c] = bilerp<STRICT>(q[0], q[1], q[2], q[3], tp.f);
                    }
                    blend<STRICT>(A, smp[0], smp[1], smp[2], a, s, dot);
                }
            };
            if (__builtin_expect(inw, 1)) {   // from the window (an LDS pointer by type: the two sources must not be merged into flat loads)
                typedef const float __attribute__((address_space(3))) lds_cfloat;
                lds_cfloat* __restrict__ top = (lds_cfloat*)win + (ly * kWLine + lx);
                plane([&](int c, float (&q)[4]) {
                    q[0] = top[c * kCW], q[1] = top[c * kCW + 1], q[2] = top[kWLine + c * kCW], q[3] = top[kWLine + c * kCW + 1];
                });
            } else {   // render_depth_kernel's loads: clamped addresses
                const TexT* __restrict__ col = last_bg ? bgi : rgb;
                const int64_t c_chan = last_bg ? sh.bs_chan : sh.rs_chan, c_row = last_bg ? sh.bs_row : sh.rs_row;
                plane([&](int c, float (&q)[4]) {
                    const TexT* __restrict__ ch = c < 3 ? col + c * c_chan : depth;
                    const int64_t s_row = c < 3 ? c_row : p.s_row;
                    const int64_t oa = static_cast<int64_t>(tp.ya) * s_row, ob = static_cast<int64_t>(tp.yb) * s_row;
                    q[0] = to_f32(ch[oa + tp.xa]), q[1] = to_f32(ch[oa + tp.xb]), q[2] = to_f32(ch[ob + tp.xa]), q[3] = to_f32(ch[ob + tp.xb]);
                });
            }
        }
    }
    store_pixel<STRICT>(p, n, HW, pix, A, dot, tl.active);
    report_status(p.status, bad);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
// Loader items are 16 bytes (8 of 16-bit storage) at a multiple of 4 texels from a row's start: base pointers and the MPI / channel / row strides of
// the three images must be multiples of 16 bytes.  Any Wt: the last item of a ragged row reads the row's padding, which a row stride that is a
// multiple of 4 texels always holds -- except behind the last row of a tensor, which the caller must have allocated (gmpi_render.h).
bool depth_window_supports(const KParams& p, int dtype, const SharedK& sh) {
    const int64_t es = dtype == GMPI_DTYPE_F32 ? 4 : 2;
    auto aligned = [&](const void* base, int64_t s0, int64_t s1, int64_t s2) {
        return reinterpret_cast<uintptr_t>(base) % 16 == 0 && (s0 * es) % 16 == 0 && (s1 * es) % 16 == 0 && (s2 * es) % 16 == 0;
    };
    if (!aligned(p.rgba, p.s_mpi, 0, p.s_row) || !aligned(sh.rgb, sh.rs_mpi, sh.rs_chan, sh.rs_row)) return false;
    if (sh.bg != nullptr && !aligned(sh.bg, sh.bs_mpi, sh.bs_chan, sh.bs_row)) return false;
    const int64_t tiles = static_cast<int64_t>((p.W + kTileW - 1) / kTileW) * ((p.H + kTileH - 1) / kTileH) * p.N;
    return tiles + 8 * static_cast<int64_t>(p.views_per_mpi) < (int64_t(1) << 31);   // (tile indices are ints)
}

int depth_window_query(int what) {
    switch (what) {
        case 26: return kCW;
        case 27: return kCH;
        case 28: return kWChunk;
        default: return -1;
    }
}

template <typename TexT>
static hipError_t launch_depth_window_t(const KParams& p, const SharedK& sh, const DepthK& dk, hipStream_t stream) {
    const FwdTileGrid tg = fwd_tile_grid<kTileW, kTileH>(p);
    dispatch_ac_strict(p.flags, [&](auto AC, auto STRICT) {
        hipLaunchKernelGGL((render_depth_window_kernel<TexT, decltype(AC)::value, decltype(STRICT)::value>), tg.grid, dim3(kTileThreads), 0, stream, p, sh, dk, tg.tiles_x,
                           tg.tiles_y, tg.n_tiles);
    });
    return hipGetLastError();
}

// (the caller has asked depth_window_supports)
hipError_t launch_depth_window(const KParams& p, int dtype, const SharedK& sh, const DepthK& dk, hipStream_t stream) {
    return dispatch_dtype(dtype, [&](auto t) { return launch_depth_window_t<typename decltype(t)::type>(p, sh, dk, stream); });
}

}  // namespace gmpi
