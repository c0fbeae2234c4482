// render_shared_forward.hip -- GMPI_VARIANT_LDS of the shared-colour forward (gmpi_mpi_render_shared_launch): render_lds.hip's pixel tiles for the
// layout of render_shared.hip.  Tile decode, pixel, corner box and origin words are the tile frame of gmpi_device.hpp.
//
// One workgroup of 512 threads owns a 32 x 16 pixel tile (one pixel per thread) and walks the D planes front to back.  Per plane the texel box
// spanned by the tile's four corner pixels is copied to LDS as fp32 planes [row][channel][x] (56 texels x 27 rows, the tile kernel's buffer) and
// every pixel takes its 16 taps from there.  The one idea that is new here: a plane's box has the same origin and shape in the alpha plane and in
// the colour image, so ONE loader map serves four channel base pointers -- channels 0-2 are rgb[m] (background[m] on plane D - 1 when one is given:
// uniform per plane), channel 3 is alpha[m, k].  The alpha planes stream from HBM once; the colour box is re-read per plane and comes from the
// caches (one image per MPI: 12 MB fp32 at 1024^2).
//
// Loader: one item = 4 texels of one channel row (16 bytes of fp32, 8 bytes of 16-bit storage, converted to fp32 on the way into LDS), thread ->
// (row, item column) fixed at compile time (27 x 14 = 378 of the 512 threads), one raw buffer load per channel with one descriptor per channel image.
// Items outside the box or outside the texture get an offset the hardware range check rejects: they read as zeros without touching memory, which
// IS the "zeros" padding -- no exec masking, the four loads of plane k + 1 are in flight while plane k is composited.  Two buffers, one barrier per
// plane.
//
// A (tile, plane) whose box exceeds the buffer (texture much finer than the image, NaN / inf corners) takes the direct gather for that plane
// (shared_sample, gmpi_shared.hpp: render_shared_kernel's arithmetic); so does a single pixel whose footprint lies outside its tile's box (a ray
// field that is no pinhole camera's).  Weights of taps outside the texture are zeroed as the direct gather zeroes them (make_taps), so a pixel's
// result does not depend on the path, and strict-order mode is bit-identical to render_shared_kernel.
//
// GMPI_FLAG_CHECK_RANGE tests every staged texel (the sampled taps plus the items and box rows around them) and every tap of the direct gather.
#include "gmpi_staged_forward.hpp"

namespace gmpi {

static_assert(staged_forward_fits_lds(16 + 32), "3 workgroups per CU");   // table bytes per plane: box, org
// (Item4 -- one loader item, 4 texels of storage -> fp32 -- and f_out_of_unit live in gmpi_shared.hpp: render_depth_window.hip loads with them too)

template <typename TexT, bool AC, bool STRICT>
__global__ __launch_bounds__(kSFThreads, 6) void render_shared_forward_kernel(const KParams p, const SharedK sh, const int tiles_x, const int tiles_y,
                                                                            const int n_tiles) {
    using I4 = Item4<TexT>;
    using Raw = typename I4::Raw;
    constexpr uint32_t kEs = static_cast<uint32_t>(sizeof(TexT));
    // Per plane of the chunk, written once by one thread so that the 8 waves do not repeat the address arithmetic on their scalar units:
    //   box: qx0 (a multiple of 4), by0, items per row (0: not staged), rows
    //   org: byte address of the box origin (texel row by0, column qx0) in the channel images 0, 1 | 2, 3 = words 0, 1 of the four buffer descriptors.
    //        The origin may lie before its image: only lanes inside the texture pass the range test.
    __shared__ int4 box[kSFChunk];
    __shared__ int4 org[kSFChunk][2];
    __shared__ __attribute__((aligned(16))) float stage[2][kSFBufFloats];

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
    const TexT* __restrict__ alpha = static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(vw.m) * p.s_mpi;
    const TexT* __restrict__ rgb = static_cast<const TexT*>(sh.rgb) + static_cast<int64_t>(vw.m) * sh.rs_mpi;
    const TexT* __restrict__ bgi = sh.bg ? static_cast<const TexT*>(sh.bg) + static_cast<int64_t>(vw.m) * sh.bs_mpi : nullptr;

    // (this lane's pixel is formed again for the epilogue: nothing of it stays in a register across the plane loop)
    auto pixel_of = [&]() {
        int lane = tid;
        asm volatile("" : "+v"(lane));   // (opaque: or the two evaluations are merged and the first one's results kept)
        return tile_lane<kSFW, kSFH>(ft.txi, ft.tyi, lane, W, H);
    };
    float rx, ry, rz;
    {
        const int64_t pix = pixel_of().pix;
        rx = rdv[pix], ry = rdv[HW + pix], rz = rdv[2 * HW + pix];
    }
    const float dot = ray_dot(vw, rx, ry, rz);
    Accum A;
    const TileCorners tc = tile_corners<kSFW, kSFH>(ft.txi, ft.tyi, W, H);

    // ---- loader role: item column lcol of box row lrow, the same for the four channels; byte offsets from the box origin per row stride ---------
    const int lrow = tid / kSFCols, lcol = tid - lrow * kSFCols;
    const bool loader = lrow < kSFRows;
    const uint32_t off_a = (static_cast<uint32_t>(lrow) * static_cast<uint32_t>(p.s_row) + kSFTPI * lcol) * kEs;
    const uint32_t off_c = (static_cast<uint32_t>(lrow) * static_cast<uint32_t>(sh.rs_row) + kSFTPI * lcol) * kEs;   // (the background's: formed on its one plane)
    const bool ragged = (Wt % kSFTPI) != 0;   // the last item of a texture row holds texels past its end (read from the row's padding, zeroed below)

    for (int kc = 0; kc < D; kc += kSFChunk) {
        const int kn = min(kSFChunk, D - kc);
        __syncthreads();   // the previous chunk's table and buffers are no longer read
        for (int t = tid; t < kn; t += kSFThreads) {
            const int k = kc + t;
            const float zdiff = vw.dhw[3 * k] - vw.ez, ph = vw.dhw[3 * k + 1], pw = vw.dhw[3 * k + 2];
            bool fits;
            int4 bb = item_box<kSFTPI>(corner_extent<AC>(vw, rdv, W, zdiff, ph, pw, tc.cx0, tc.cx1, tc.cy0, tc.cy1), kSFCols, kSFRows, fits);
            if (!fits) bb.z = 0;
            box[t] = bb;
            const bool last_bg = bgi != nullptr && k == D - 1;
            const TexT* col = last_bg ? bgi : rgb;
            const int64_t c_chan = last_bg ? sh.bs_chan : sh.rs_chan, c_row = last_bg ? sh.bs_row : sh.rs_row;
            const uint64_t o0 = reinterpret_cast<uint64_t>(col) + static_cast<uint64_t>((bb.y * c_row + bb.x) * static_cast<int64_t>(kEs));
            const uint64_t oc = static_cast<uint64_t>(c_chan * static_cast<int64_t>(kEs));
            const uint64_t o1 = o0 + oc, o2 = o1 + oc;
            const uint64_t o3 = reinterpret_cast<uint64_t>(alpha) + static_cast<uint64_t>((static_cast<int64_t>(k) * p.s_plane + bb.y * p.s_row + bb.x) * static_cast<int64_t>(kEs));
            const int2 w0 = origin_words(o0), w1 = origin_words(o1), w2 = origin_words(o2), w3 = origin_words(o3);
            org[t][0] = make_int4(w0.x, w0.y, w1.x, w1.y);
            org[t][1] = make_int4(w2.x, w2.y, w3.x, w3.y);
        }
        __syncthreads();   // table published

        // the four loads of plane t of the chunk; past the end of the chunk, or for a box that is not staged, every offset is rejected.  Issued
        // unconditionally: with the same memory operations on every path the loads stay in flight across the compositing of the plane before.
        auto issue_loads = [&](int t, Raw (&L)[4]) {
            const int4 bb = box[min(t, kn - 1)];
            const int qx0 = __builtin_amdgcn_readfirstlane(bb.x), by0 = __builtin_amdgcn_readfirstlane(bb.y);
            const int nq = t < kn ? __builtin_amdgcn_readfirstlane(bb.z) : 0, nrows = __builtin_amdgcn_readfirstlane(bb.w);
            const bool last_bg = bgi != nullptr && kc + t == D - 1;   // uniform
            const int4 o01 = org[min(t, kn - 1)][0], o23 = org[min(t, kn - 1)][1];
            const int ow[8] = {o01.x, o01.y, o01.z, o01.w, o23.x, o23.y, o23.z, o23.w};
            const int gx = qx0 + kSFTPI * lcol, gy = by0 + lrow;
            // (bitwise on purpose: `&&` would be lowered to exec-mask control flow)
            const bool ok = (lcol < nq) & (lrow < nrows) & (gx >= 0) & (gx < Wt) & (gy >= 0) & (gy < Ht);
            uint32_t off_col = off_c;
            if (last_bg) off_col = (static_cast<uint32_t>(lrow) * static_cast<uint32_t>(sh.bs_row) + kSFTPI * lcol) * kEs;
            const uint32_t oc = ok ? off_col : 0x80000000u, oa = ok ? off_a : 0x80000000u;   // == num_records: rejected
#pragma unroll
            for (int c = 0; c < 4; ++c) L[c] = I4::load(origin_rsrc(ow[2 * c], ow[2 * c + 1]), c < 3 ? oc : oa);
        };
        // registers -> LDS: the box itself (texels of it outside the texture are the zeros the loads returned); lanes outside the box stay idle
        auto store_box = [&](int t, float* buf, const Raw (&L)[4]) {
            const int4 bb = box[t];
            const int qx0 = __builtin_amdgcn_readfirstlane(bb.x), nq = __builtin_amdgcn_readfirstlane(bb.z), nrows = __builtin_amdgcn_readfirstlane(bb.w);
            const bool in_box = loader & (lcol < nq) & (lrow < nrows);
            const int dst0 = lrow * (4 * kSFPitch) + kSFTPI * lcol;   // floats: line (lrow, channel 0)
            const int left = Wt - (qx0 + kSFTPI * lcol);   // texels of this item that lie inside the texture row (ragged textures)
            float4 q[4];
            uint32_t mx = 0;   // max of the fp32 bit patterns this lane staged (rejected items hold zeros)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                q[c] = I4::cvt(L[c]);
                if (ragged) {
                    if (left < 2) q[c].y = 0.0f;
                    if (left < 3) q[c].z = 0.0f;
                    if (left < 4) q[c].w = 0.0f;
                }
                if (in_box) *reinterpret_cast<float4*>(buf + dst0 + c * kSFPitch) = q[c];
                mx = max(max(mx, __float_as_uint(q[c].x)), max(max(__float_as_uint(q[c].y), __float_as_uint(q[c].z)), __float_as_uint(q[c].w)));
            }
            if (check_range && __builtin_expect(mx > 0x3f800000u, 0)) {   // (cold: the exact test, -0.0 is legal)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (f_out_of_unit(q[c].x) || f_out_of_unit(q[c].y) || f_out_of_unit(q[c].z) || f_out_of_unit(q[c].w)) bad |= GMPI_STATUS_RGBA_RANGE;
            }
        };
        auto composite = [&](int t, const float* __restrict__ buf) {
            const int k = kc + t;
            const int4 bb = box[t];
            const int qx0 = __builtin_amdgcn_readfirstlane(bb.x), by0 = __builtin_amdgcn_readfirstlane(bb.y);
            const int nq = __builtin_amdgcn_readfirstlane(bb.z), nrows = __builtin_amdgcn_readfirstlane(bb.w);
            float ix, iy, s, u, v;
            plane_coord<AC>(vw.dhw[3 * k] - vw.ez, vw.dhw[3 * k + 1], vw.dhw[3 * k + 2], vw.ex, vw.ey, rx, ry, rz, vw.cx, vw.cy, ix, iy, s, u, v);
            if (check_last && k == D - 1 && outside_pm1(u, v)) bad |= GMPI_STATUS_OUT_OF_LAST_PLANE;
            const Taps tp = make_taps(ix, iy, Ht, Wt);
            const bool last_bg = bgi != nullptr && k == D - 1;   // uniform
            float smp[4];
            bool direct = true;
            if (nq > 0) {   // uniform: the plane is staged
                const int lx = tp.f.x0 - qx0, ly = tp.f.y0 - by0;
                const bool inb = (lx >= 0) & (ly >= 0) & (lx + 1 < kSFTPI * nq) & (ly + 1 < nrows);
                const bool any_w = (tp.f.nw != 0.0f) | (tp.f.ne != 0.0f) | (tp.f.sw != 0.0f) | (tp.f.se != 0.0f);
                // a footprint outside the box with every weight zero (the sentinel corner of NaN / far-off coordinates) reads texel (0, 0) of the box
                const uint32_t idx = inb ? static_cast<uint32_t>(ly * (4 * kSFPitch) + lx) : 0u;
                // LDS byte addresses of the two texel rows, opaque to the optimiser so that the 8 tap-pair reads keep immediate offsets (render_lds.hip)
                typedef const float __attribute__((address_space(3))) lds_cfloat;
                uint32_t buf_addr = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_cfloat*)buf));
                asm volatile("" : "+s"(buf_addr));
                uint32_t a_top = buf_addr + 4u * idx, a_bot = a_top + 16u * kSFPitch;
                asm volatile("" : "+v"(a_top), "+v"(a_bot));
                lds_cfloat* __restrict__ top = reinterpret_cast<lds_cfloat*>(static_cast<uintptr_t>(a_top));
                lds_cfloat* __restrict__ bot = reinterpret_cast<lds_cfloat*>(static_cast<uintptr_t>(a_bot));
#pragma unroll
                for (int c = 0; c < 4; ++c) smp[c] = bilerp<STRICT>(top[c * kSFPitch], top[c * kSFPitch + 1], bot[c * kSFPitch], bot[c * kSFPitch + 1], tp.f);
                direct = (!inb) & any_w;   // per lane: a pixel whose taps the box does not hold (no pinhole ray field)
            }
            if (__builtin_expect(direct, 0))
                shared_sample<TexT, STRICT>(alpha + static_cast<int64_t>(k) * p.s_plane, p.s_row, last_bg ? bgi : rgb, last_bg ? sh.bs_chan : sh.rs_chan,
                                            last_bg ? sh.bs_row : sh.rs_row, tp, check_range, bad, smp);
            blend<STRICT>(A, smp[0], smp[1], smp[2], smp[3], s, dot);
        };

        Raw L[4];
        issue_loads(0, L);
        for (int t = 0; t < kn; ++t) {
            float* buf = stage[t & 1];
            store_box(t, buf, L);
            __syncthreads();          // box t visible; everybody is done reading box t - 1 (the other buffer)
            issue_loads(t + 1, L);    // in flight while plane t is composited
            composite(t, buf);
        }
    }
    const TileLane tl = pixel_of();
    store_pixel<STRICT>(p, n, HW, tl.pix, A, dot, tl.active);
    report_status(p.status, bad);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
// Loader items are 4 texels: every channel row of the three tensors must start on an item boundary, and the in-box byte offsets are kept in 32 bits.
bool shared_forward_supports(const KParams& p, int dtype, const SharedK& sh) {
    const int64_t es = dtype == GMPI_DTYPE_F32 ? 4 : 2;
    if (!staged_item_aligned(p.rgba, es, p.s_mpi, p.s_plane, p.s_row) || !staged_item_aligned(sh.rgb, es, sh.rs_mpi, sh.rs_chan, sh.rs_row)) return false;
    if (sh.bg != nullptr && !(staged_item_aligned(sh.bg, es, sh.bs_mpi, sh.bs_chan, sh.bs_row) && staged_offsets_fit(sh.bs_row, es))) return false;
    return staged_offsets_fit(p.s_row, es) && staged_offsets_fit(sh.rs_row, es);
}

int shared_forward_query(int what) {
    switch (what) {
        case 12: return kSFW;
        case 13: return kSFPitch;
        case 14: return kSFRows;
        default: return -1;
    }
}

template <typename TexT>
static hipError_t launch_shared_forward_t(const KParams& p, const SharedK& sh, hipStream_t stream) {
    const FwdTileGrid tg = fwd_tile_grid<kSFW, kSFH>(p);
    dispatch_ac_strict(p.flags, [&](auto AC, auto STRICT) {
        hipLaunchKernelGGL((render_shared_forward_kernel<TexT, decltype(AC)::value, decltype(STRICT)::value>), tg.grid, dim3(kSFThreads), 0, stream, p, sh, tg.tiles_x,
                           tg.tiles_y, tg.n_tiles);
    });
    return hipGetLastError();
}

hipError_t launch_shared_forward(const KParams& p, int dtype, const SharedK& sh, hipStream_t stream) {
    return dispatch_dtype(dtype, [&](auto t) { return launch_shared_forward_t<typename decltype(t)::type>(p, sh, stream); });
}

}  // namespace gmpi
