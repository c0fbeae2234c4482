// render_shaded.hip -- the shaded render of an RGBA volume (gmpi_mpi_render_shaded_launch / _backward_launch, include/gmpi_render.h): the reference's
// training configuration shades the generator's volume before it renders it (light_renderer.py:189-197: new_rgb = clip(rgb * shading[B,1,1,H,W], 0, 1),
// alpha passed through; train.py:535-541, 703-709).  The shading is ONE factor per texel, the same for every plane and channel, so the shaded volume
// need not exist: by definition the result is the render of light_apply_kernel's output (light_kernels.hip), and the multiply and the clip happen on the
// taps -- shade_texel, gmpi_device.hpp: that kernel's arithmetic, so the strict-order forward is bit-identical to render_gather.hip on the shaded volume.
//
//   render_shaded_kernel                 forward, one pixel per lane, any shape / stride / dtype / ray field, every flag (render_gather_kernel's shape)
//   render_shaded_forward_kernel         forward, staged: the tile frame of render_shared_forward.hip (see the kernel)
//   light_apply_backward_inplace_kernel  the chain rule through clip(rgb * s) per texel, IN PLACE on the gradient volume the render backward filled
//                                        (light_apply_backward_kernel without its aliasing promise, any gradient strides) + the shading's gradient
//
// The backward kernels are the shaded twins of render_backward.hip (its Shade policy).
#include "gmpi_staged_forward.hpp"

namespace gmpi {

template <typename TexT, bool AC, bool STRICT>
__global__ __launch_bounds__(256) void render_shaded_kernel(const KParams p, const ShadeK shade) {
    const int n = blockIdx.z;
    const int px = blockIdx.x * 64 + threadIdx.x;
    const int py = blockIdx.y * 4 + threadIdx.y;
    uint32_t bad = 0;
    const View vw = view_setup<AC>(p, n, bad);
    check_camera_behind(p, vw, blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0);  // one lane per view, as the gather kernel
    // edge tiles: out-of-image lanes shadow the last pixel (keeps the wave converged for the status reduce)
    const bool active = px < p.W && py < p.H;
    const int64_t HW = vw.HW;
    const int64_t pix = static_cast<int64_t>(min(py, p.H - 1)) * p.W + min(px, p.W - 1);
    const float rx = vw.rays[pix], ry = vw.rays[HW + pix], rz = vw.rays[2 * HW + pix];
    const float dot = ray_dot(vw, rx, ry, rz);
    const bool check_range = (p.flags & GMPI_FLAG_CHECK_RANGE) != 0;
    const TexT* __restrict__ vol = static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(vw.m) * p.s_mpi;
    const float* __restrict__ sh = shade.s + static_cast<int64_t>(vw.m) * shade.s_mpi;

    Accum A;
    for (int k = 0; k < p.D; ++k) {
        float ix, iy, s, u, v, smp[4];
        plane_coord<AC>(vw.dhw[3 * k] - vw.ez, vw.dhw[3 * k + 1], vw.dhw[3 * k + 2], vw.ex, vw.ey, rx, ry, rz, vw.cx, vw.cy, ix, iy, s, u, v);
        shaded_gather_sample<TexT, STRICT>(vol + static_cast<int64_t>(k) * p.s_plane, p.s_chan, p.s_row, sh, shade.s_row, p.Ht, p.Wt, ix, iy, check_range, bad, smp);
        blend<STRICT>(A, smp[0], smp[1], smp[2], smp[3], s, dot);
    }
    const LastPlane lp = last_plane(p, vw);
    if (leaves_last_plane<AC>(vw, lp, rx, ry, rz)) bad |= GMPI_STATUS_OUT_OF_LAST_PLANE;
    store_pixel<STRICT>(p, n, HW, pix, A, dot, active);
    report_status(p.status, bad);
}

// ---- forward, staged --------------------------------------------------------------------------------------------------------------------------
// render_shared_forward_kernel's frame (render_shared_forward.hip has the why of every piece): 32 x 16 pixel tiles, one pixel per thread, the tile frame
// of gmpi_device.hpp, fp32 LDS planes [row][channel][x] of 56 x 27 texels in two buffers, one barrier per plane, a box table per 64 planes, Item4<TexT>
// loaders whose rejected offsets read zeros.  What differs: the four channels are the volume's own (plane k: a table entry per plane holds their four
// origins), and a plane's box has the same origin and shape in the MPI's shading image, so every loader lane issues a FIFTH load per plane -- one fp32
// Item4 of the shading box, which the caches serve (one image per MPI) -- and store_box multiplies and clips ONCE per staged colour texel, not per tap.
// The compositor reads shaded texels and is the shared-colour kernel's.  An item outside the box or the texture reads zeros in both images (0 * 0 = 0:
// the zeros padding); the texels of a ragged last item (Wt % 4 != 0) are zeroed after the shading, as there.  A (tile, plane) whose box does not fit, and
// a pixel whose footprint lies outside its tile's box, take shaded_gather_sample -- render_shaded_kernel's sampling: a pixel's bits do not depend on the
// path.  GMPI_FLAG_CHECK_RANGE tests the staged alpha texels raw (and the alpha taps of the direct path); a shaded colour is in [0, 1] by construction.
static_assert(staged_forward_fits_lds(16 + 32 + 8), "3 workgroups per CU");   // table bytes per plane: box, org, orgs

template <typename TexT, bool AC, bool STRICT>
__global__ __launch_bounds__(kSFThreads, 6) void render_shaded_forward_kernel(const KParams p, const ShadeK shade, const int tiles_x, const int tiles_y,
                                                                             const int n_tiles) {
    using I4 = Item4<TexT>;
    using Raw = typename I4::Raw;
    using S4 = Item4<float>;
    using RawS = typename S4::Raw;
    constexpr uint32_t kEs = static_cast<uint32_t>(sizeof(TexT));
    // per plane of the chunk, written once by one thread: box = qx0 (a multiple of 4), by0, items per row (0: not staged), rows; org = the byte address
    // of the box origin in channels 0, 1 | 2, 3 of plane k; orgs = in the shading image (words 0, 1 of the buffer descriptors; an origin may lie before its
    // image: only lanes inside the texture pass the range test)
    __shared__ int4 box[kSFChunk];
    __shared__ int4 org[kSFChunk][2];
    __shared__ int2 orgs[kSFChunk];
    __shared__ __attribute__((aligned(16))) float stage[2][kSFBufFloats];

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
    const TexT* __restrict__ vol = static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(vw.m) * p.s_mpi;
    const float* __restrict__ sh = shade.s + static_cast<int64_t>(vw.m) * shade.s_mpi;

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

    // loader role: item column lcol of box row lrow, the same for the five images; byte offsets from the box origin per row stride
    const int lrow = tid / kSFCols, lcol = tid - lrow * kSFCols;
    const bool loader = lrow < kSFRows;
    const uint32_t off_v = (static_cast<uint32_t>(lrow) * static_cast<uint32_t>(p.s_row) + kSFTPI * lcol) * kEs;
    const uint32_t off_s = (static_cast<uint32_t>(lrow) * static_cast<uint32_t>(shade.s_row) + kSFTPI * lcol) * 4u;
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
            const uint64_t o0 = reinterpret_cast<uint64_t>(vol) + static_cast<uint64_t>((static_cast<int64_t>(k) * p.s_plane + bb.y * p.s_row + bb.x) * static_cast<int64_t>(kEs));
            const uint64_t oc = static_cast<uint64_t>(p.s_chan * static_cast<int64_t>(kEs));
            const uint64_t o1 = o0 + oc, o2 = o1 + oc, o3 = o2 + oc;
            const uint64_t os = reinterpret_cast<uint64_t>(sh) + static_cast<uint64_t>((bb.y * shade.s_row + bb.x) * static_cast<int64_t>(4));
            const int2 w0 = origin_words(o0), w1 = origin_words(o1), w2 = origin_words(o2), w3 = origin_words(o3);
            org[t][0] = make_int4(w0.x, w0.y, w1.x, w1.y);
            org[t][1] = make_int4(w2.x, w2.y, w3.x, w3.y);
            orgs[t] = origin_words(os);
        }
        __syncthreads();   // table published

        // the five loads of plane t of the chunk; past the end of the chunk, or for a box that is not staged, every offset is rejected.  Issued
        // unconditionally: with the same memory operations on every path the loads stay in flight across the compositing of the plane before.
        auto issue_loads = [&](int t, Raw (&L)[4], RawS& LS) {
            const int ti = min(t, kn - 1);
            const int4 bb = box[ti];
            const int qx0 = __builtin_amdgcn_readfirstlane(bb.x), by0 = __builtin_amdgcn_readfirstlane(bb.y);
            const int nq = t < kn ? __builtin_amdgcn_readfirstlane(bb.z) : 0, nrows = __builtin_amdgcn_readfirstlane(bb.w);
            const int4 o01 = org[ti][0], o23 = org[ti][1];
            const int2 o4 = orgs[ti];
            const int ow[8] = {o01.x, o01.y, o01.z, o01.w, o23.x, o23.y, o23.z, o23.w};
            const int gx = qx0 + kSFTPI * lcol, gy = by0 + lrow;
            // (bitwise on purpose: `&&` would be lowered to exec-mask control flow)
            const bool ok = loader & (lcol < nq) & (lrow < nrows) & (gx >= 0) & (gx < Wt) & (gy >= 0) & (gy < Ht);
            const uint32_t ov = ok ? off_v : 0x80000000u, os = ok ? off_s : 0x80000000u;   // == num_records: rejected
#pragma unroll
            for (int c = 0; c < 4; ++c) L[c] = I4::load(origin_rsrc(ow[2 * c], ow[2 * c + 1]), ov);
            LS = S4::load(origin_rsrc(o4.x, o4.y), os);
        };
        // registers -> LDS: the shaded box (texels of it outside the texture are the zeros the loads returned); lanes outside the box stay idle
        auto store_box = [&](int t, float* buf, const Raw (&L)[4], const RawS& LS) {
            const int4 bb = box[t];
            const int qx0 = __builtin_amdgcn_readfirstlane(bb.x), nq = __builtin_amdgcn_readfirstlane(bb.z), nrows = __builtin_amdgcn_readfirstlane(bb.w);
            const bool in_box = loader & (lcol < nq) & (lrow < nrows);
            const int dst0 = lrow * (4 * kSFPitch) + kSFTPI * lcol;   // floats: line (lrow, channel 0)
            const int left = Wt - (qx0 + kSFTPI * lcol);   // texels of this item that lie inside the texture row (ragged textures)
            const float4 qs = S4::cvt(LS);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float4 q = I4::cvt(L[c]);
                if (c < 3) q = make_float4(shade_texel(q.x, qs.x), shade_texel(q.y, qs.y), shade_texel(q.z, qs.z), shade_texel(q.w, qs.w));
                if (ragged) {
                    if (left < 2) q.y = 0.0f;
                    if (left < 3) q.z = 0.0f;
                    if (left < 4) q.w = 0.0f;
                }
                if (in_box) *reinterpret_cast<float4*>(buf + dst0 + c * kSFPitch) = q;
                if (c == 3 && check_range && (f_out_of_unit(q.x) || f_out_of_unit(q.y) || f_out_of_unit(q.z) || f_out_of_unit(q.w))) bad |= GMPI_STATUS_RGBA_RANGE;
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
                shaded_gather_sample<TexT, STRICT>(vol + static_cast<int64_t>(k) * p.s_plane, p.s_chan, p.s_row, sh, shade.s_row, Ht, Wt, ix, iy, check_range, bad, smp);
            blend<STRICT>(A, smp[0], smp[1], smp[2], smp[3], s, dot);
        };

        Raw L[4];
        RawS LS;
        issue_loads(0, L, LS);
        for (int t = 0; t < kn; ++t) {
            float* buf = stage[t & 1];
            store_box(t, buf, L, LS);
            __syncthreads();              // box t visible; everybody is done reading box t - 1 (the other buffer)
            issue_loads(t + 1, L, LS);    // in flight while plane t is composited
            composite(t, buf);
        }
    }
    const TileLane tl = pixel_of();
    store_pixel<STRICT>(p, n, HW, tl.pix, A, dot, tl.active);
    report_status(p.status, bad);
}

// g holds dL/d shaded on entry and dL/d rgba on exit: g_rgb = g s [0 <= rgb s <= 1] (the closed mask: where torch.clip passes a gradient; a NaN product
// passes none), alpha untouched; g_shading = sum over planes and colour channels of g rgb [...], written (nullptr: not wanted).  A thread owns VEC
// consecutive texels of a row through all planes: it reads and writes its own cells only, so in place is safe -- and g is NOT __restrict__.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void light_apply_backward_inplace_kernel(const T* __restrict__ rgba, int64_t sb, int64_t sd, int64_t sc, int64_t sr,
                                                                           const float* __restrict__ shading, int64_t hb, int64_t hr, float* g, int64_t gb,
                                                                           int64_t gd, int64_t gc, int64_t gr, float* __restrict__ g_shading, int64_t qb, int64_t qr,
                                                                           int D, int H, int W) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * VEC, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    struct alignas(sizeof(T) * VEC) TV { T v[VEC]; };
    struct alignas(sizeof(float) * VEC) FV { float v[VEC]; };
    const FV s = *reinterpret_cast<const FV*>(shading + b * hb + static_cast<int64_t>(y) * hr + x);
    FV gs;
#pragma unroll
    for (int i = 0; i < VEC; ++i) gs.v[i] = 0.0f;
    for (int k = 0; k < D; ++k) {
        const T* __restrict__ src = rgba + b * sb + k * sd + static_cast<int64_t>(y) * sr + x;
        float* gk = g + b * gb + k * gd + static_cast<int64_t>(y) * gr + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const TV v = *reinterpret_cast<const TV*>(src + c * sc);
            const FV gv = *reinterpret_cast<const FV*>(gk + c * gc);
            FV r;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float vf = to_f32(v.v[i]), t = vf * s.v[i];
                const bool pass = t >= 0.0f && t <= 1.0f;
                r.v[i] = pass ? gv.v[i] * s.v[i] : 0.0f;
                gs.v[i] += pass ? gv.v[i] * vf : 0.0f;
            }
            *reinterpret_cast<FV*>(gk + c * gc) = r;
        }
    }
    if (g_shading != nullptr) *reinterpret_cast<FV*>(g_shading + b * qb + static_cast<int64_t>(y) * qr + x) = gs;
}

// an image [M,1,Ht,Wt] with MPI and row strides set to zero (the shading's gradient before the shading-only backward adds into it)
__global__ __launch_bounds__(256) void zero_image_kernel(float* __restrict__ img, int64_t s_mpi, int64_t s_row, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < W) img[blockIdx.z * s_mpi + static_cast<int64_t>(blockIdx.y) * s_row + x] = 0.0f;
}
hipError_t launch_zero_image(float* img, const int64_t* st, int M, int Ht, int Wt, hipStream_t stream) {
    hipLaunchKernelGGL(zero_image_kernel, dim3((Wt + 255) / 256, Ht, M), dim3(256), 0, stream, img, st[0], st[1], Wt);
    return hipGetLastError();
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------
template <typename TexT>
static hipError_t launch_shaded_t(const KParams& p, const ShadeK& sh, hipStream_t stream) {
    const dim3 block(64, 4);
    const dim3 grid((p.W + 63) / 64, (p.H + 3) / 4, p.N);
    dispatch_ac_strict(p.flags, [&](auto AC, auto STRICT) {
        hipLaunchKernelGGL((render_shaded_kernel<TexT, decltype(AC)::value, decltype(STRICT)::value>), grid, block, 0, stream, p, sh);
    });
    return hipGetLastError();
}
hipError_t launch_shaded(const KParams& p, int dtype, const ShadeK& sh, hipStream_t stream) {
    return dispatch_dtype(dtype, [&](auto t) { return launch_shaded_t<typename decltype(t)::type>(p, sh, stream); });
}

// Loader items are 4 texels: every channel row of the volume and every row of the shading image must start on an item boundary, and the in-box byte
// offsets are kept in 32 bits (shared_forward_supports' rules, extended to the shading image).
bool shaded_forward_supports(const KParams& p, int dtype, const ShadeK& sh) {
    const int64_t es = dtype == GMPI_DTYPE_F32 ? 4 : 2;
    if (!staged_item_aligned(p.rgba, es, p.s_mpi, p.s_plane, p.s_chan, p.s_row) || !staged_item_aligned(sh.s, 4, sh.s_mpi, sh.s_row)) return false;
    return staged_offsets_fit(p.s_row, es) && staged_offsets_fit(sh.s_row, 4);
}

template <typename TexT>
static hipError_t launch_shaded_forward_t(const KParams& p, const ShadeK& sh, hipStream_t stream) {
    const FwdTileGrid tg = fwd_tile_grid<kSFW, kSFH>(p);
    dispatch_ac_strict(p.flags, [&](auto AC, auto STRICT) {
        hipLaunchKernelGGL((render_shaded_forward_kernel<TexT, decltype(AC)::value, decltype(STRICT)::value>), tg.grid, dim3(kSFThreads), 0, stream, p, sh, tg.tiles_x,
                           tg.tiles_y, tg.n_tiles);
    });
    return hipGetLastError();
}
hipError_t launch_shaded_forward(const KParams& p, int dtype, const ShadeK& sh, hipStream_t stream) {
    return dispatch_dtype(dtype, [&](auto t) { return launch_shaded_forward_t<typename decltype(t)::type>(p, sh, stream); });
}

// gst: the 5 element strides of the gradient volume; qst: MPI and row stride of g_shading (unused when it is nullptr).  M <= 65535 (grid.z), Ht <= 65535.
hipError_t launch_shaded_chain_rule(const KParams& p, int dtype, const ShadeK& sh, float* g, const int64_t* gst, float* g_shading, const int64_t* qst,
                                    hipStream_t stream) {
    const int64_t qb = g_shading ? qst[0] : 0, qr = g_shading ? qst[1] : 0;
    const int es = dtype == GMPI_DTYPE_F32 ? 4 : 2;
    auto mult4 = [](int64_t v) { return v % 4 == 0; };
    const bool vec = p.Wt % 4 == 0 && mult4(p.s_mpi) && mult4(p.s_plane) && mult4(p.s_chan) && mult4(p.s_row) && mult4(sh.s_mpi) && mult4(sh.s_row) &&
                     mult4(gst[0]) && mult4(gst[1]) && mult4(gst[2]) && mult4(gst[3]) && mult4(qb) && mult4(qr) &&
                     reinterpret_cast<uintptr_t>(p.rgba) % (4 * es) == 0 && reinterpret_cast<uintptr_t>(sh.s) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(g) % 16 == 0 && reinterpret_cast<uintptr_t>(g_shading) % 16 == 0;
    const dim3 block(256), grid(((vec ? p.Wt / 4 : p.Wt) + 255) / 256, p.Ht, p.M);
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        dispatch_bool(vec, [&](auto VEC) {
            hipLaunchKernelGGL((light_apply_backward_inplace_kernel<T, decltype(VEC)::value ? 4 : 1>), grid, block, 0, stream, static_cast<const T*>(p.rgba), p.s_mpi,
                               p.s_plane, p.s_chan, p.s_row, sh.s, sh.s_mpi, sh.s_row, g, gst[0], gst[1], gst[2], gst[3], g_shading, qb, qr, p.D, p.Ht, p.Wt);
        });
    });
    return hipGetLastError();
}

}  // namespace gmpi
