// render_u8.hip -- GMPI_VARIANT_LDS for GMPI_DTYPE_U8 volumes: the tile kernel's frame over 8-bit texels.
//
// A code c in 0..255 stands for the fp32 value c / 255 (to_f32(u8_t), gmpi_device.hpp): rendering the volume is by definition rendering that fp32
// volume.  One workgroup of 512 threads owns a 32 x 16 pixel tile (one pixel per thread) and walks the D planes front to back; per plane the texel
// box spanned by the tile's four corner pixels is staged in LDS, two buffers, one barrier per plane, the loads of plane k + 1 in flight while
// plane k is composited (render_lds.hip has the why of all that; tile decode, pixel, corner box and origin words are the tile frame of gmpi_device.hpp).
//
// What is new is the LDS image: the RAW texels, interleaved, one dword (R | G << 8 | B << 16 | A << 24) per texel, 64 texels x 32 rows.
//  * A pixel's 2 x 2 footprint is two ds_read2_b32 (texels x, x + 1 of rows y and y + 1) instead of the fp32 planes' eight.
//  * Row pitch 64 dwords: ds_read2_b32 banks by (a / 4) mod 32 per 32-lane half, and a half wave is one pixel row of the tile.  Its lanes read
//    consecutive texels (the warp is near-identity), and where a tilted row crosses from texel row y to y + 1 the two runs keep distinct x: with a
//    pitch that is a multiple of the 32 banks they do not collide as long as the row spans at most 32 texels.  (More than one texel per pixel
//    wraps around the banks in any one-dword-per-texel layout: a tilted camera's 47-texel boxes do.  That conflict rate has not been measured.)
//  * The volume is planar.  One loader item = 4 texels of one channel row = one dword load from each of the four channel images through the
//    plane's buffer descriptor (scalar offset = channel), 8 v_perm_b32 to interleave them, one 16-byte LDS store: 16 items per box row, 32 rows,
//    exactly one item per thread, the thread -> item map fixed at compile time.  A 16-byte item (16 texels) would need Wt, the base pointer and
//    every stride to be multiples of 16 bytes and the box origin rounded down to 16 texels (up to 15 dead columns of the 64); the 4-texel item asks
//    for multiples of 4 only, keeps more volumes on the staged path, and is what the tile kernel does for 16-bit texel pairs.
//  * Items outside the box or outside the texture take the offset the hardware range check rejects: they come back as zeros without touching
//    memory, which IS padding_mode="zeros"; nothing is exec-masked.
//  * The prefetch does not cross a chunk of the per-plane table (64 planes): the load issued behind a chunk's last plane is rejected as a whole,
//    and the next chunk's first plane is loaded after the table rebuild -- one exposed load latency per chunk (twice at D = 96).
//
// Arithmetic.  GMPI_FLAG_STRICT_ORDER: every tap is converted first (c / 255, three VALU ops) and the sample is gather_sample's sum: bit-identical
// to the gather kernel and to the oracle on the fp32 volume.  Default: the CODES are interpolated (v_cvt_f32_ubyte0..3 are exact) and the sample is
// scaled by RN(1/255) once per channel: 4 multiplies instead of 16 conversions; the error is a few ulp of 255, divided by 255: about 2e-7.
//
// A (tile, plane) whose box exceeds the buffer (texture much finer than the image, NaN / inf corners) takes gather_plane for that plane, and so does
// a single pixel whose footprint lies outside its tile's box (a ray field that is no pinhole camera's).  Weights of taps outside the texture are
// zeroed as gather_sample zeroes them, so in strict-order mode a pixel's bits do not depend on the path; in default mode gather_plane converts per
// tap, which differs from the staged sample by the 2e-7 above.  GMPI_FLAG_CHECK_RANGE has nothing to test: every code is in [0, 1].
//
// Sparse volumes (opt-in: gmpi_mpi_render_u8_sparse_launch).  A stored MPI is mostly empty, and at 8 bits "empty" is the exact alpha code 0, whose composite
// changes nothing: w = 0 T, C += 0 rgb, Z += 0 depth, T (1 - 0 + 1e-10) = T 1.0f.  u8_occupancy_kernel reduces a volume's alpha bytes to the largest code per
// 16 x 16 texel block; the Occ = OccK instances of the body below look a plane's box up in that map while they fill the plane table and, where it holds code 0
// alone, neither load nor stage nor sample it -- the same bits, for any ray field (composite's EMPTY branch has the argument).  Occ = NoOcc is the dense text.
#include "gmpi_device.hpp"

namespace gmpi {

constexpr int kUW = 32, kUH = 16, kUThreads = kUW * kUH;   // pixel tile, one pixel per thread
constexpr int kUPitch = 64, kURows = 32;                   // staging buffer: texels (dwords) per row, rows
constexpr int kUTPI = 4, kUCols = kUPitch / kUTPI;         // texels per loader item, items per row
constexpr int kUBufWords = kURows * kUPitch;               // 2048 dwords = 8 KB
constexpr int kUChunk = 64;                                // planes per table refill
static_assert(kURows * kUCols == kUThreads, "one loader item per thread");
static_assert(kUPitch % 32 == 0, "row pitch: a multiple of the 32 banks of ds_read2_b32");
static_assert(2 * kUBufWords * 4 + kUChunk * 48 <= 40 * 1024, "4 workgroups per CU");

// TexT = u8_t: the planar volume above.  TexT = rgba8_t: a channels-last volume (texel stride 4 bytes, gmpi_device.hpp), whose memory image IS the LDS
// image: one loader item = 4 texels = one 16-byte buffer load and one 16-byte LDS store, no v_perm; strides and offsets count bytes, a box row is one
// run of 16 bytes per item.  The item's dword alignment is what u8_variant_supports asks for.  Everything behind the LDS image is the same code:
// the kernel body is this one function, the two kernels below are its instances (the planar one keeps its name and its template arguments).
// Carry = CarryK: the instances of a plane-chunked render (gmpi_mpi_render_chunk_launch): the Accum enters from state_in and leaves to state_out.
// Occ = OccK: the sparse instances (gmpi_mpi_render_u8_sparse_launch; "the occupancy map" below): a (tile, plane) whose texel box holds alpha code 0
// alone is neither loaded nor staged nor sampled.  Occ = NoOcc (the default) is the text as it was: the one-shot and carry kernels do not change.
struct OccK {
    const uint8_t* map;   // [M, D, ceil(Ht / 16), ceil(Wt / 16)]: the largest alpha code of each 16 x 16 texel block
    uint32_t* stats;      // nullable: [0] += (tile, plane) pairs skipped, [1] += pairs staged
};
struct NoOcc {};
constexpr int kOccBlock = 16, kOccShift = 4;   // texels per side of a block of the map

// Does the box (x0 = bb.x, y0 = bb.y, bb.z items of kUTPI texels, bb.w rows) of plane k of MPI m hold alpha code 0 alone?  Texels outside the texture are
// the zero padding: only the part inside is looked up, in the blocks it overlaps -- at most 5 x 3 of them (64 texels from a multiple of 4, 32 rows).
__device__ __forceinline__ bool box_is_empty(const uint8_t* __restrict__ map, int m, int k, int D, const int4& bb, int Ht, int Wt) {
    const int x0 = max(bb.x, 0), x1 = min(bb.x + kUTPI * bb.z, Wt) - 1, y0 = max(bb.y, 0), y1 = min(bb.y + bb.w, Ht) - 1;   // (inclusive)
    if (x0 > x1 || y0 > y1) return true;
    const int nbx = (Wt + kOccBlock - 1) >> kOccShift, nby = (Ht + kOccBlock - 1) >> kOccShift;
    const uint8_t* __restrict__ mp = map + (static_cast<int64_t>(m) * D + k) * nby * nbx;
    // (5 x 3 loads whatever the box, the indices clamped into its blocks: fifteen independent loads and one wait -- a loop over the blocks that exist waits for
    //  every byte in turn, with the whole workgroup at the barrier behind the table)
    static_assert(kUPitch + kOccBlock - kUTPI <= 5 * kOccBlock && kURows + kOccBlock - 1 <= 3 * kOccBlock, "a staged box overlaps at most 5 x 3 blocks");
    const int bx0 = x0 >> kOccShift, bx1 = x1 >> kOccShift, by0 = y0 >> kOccShift, by1 = y1 >> kOccShift;
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 5; ++i) any |= mp[min(by0 + j, by1) * nbx + min(bx0 + i, bx1)];
    return any == 0;
}

template <typename TexT, bool AC, bool STRICT, typename Carry = NoCarry, typename Occ = NoOcc>
__device__ __forceinline__ void render_u8_tile(const KParams& p, const int tiles_x, const int tiles_y, const int n_tiles, const Carry& carry = Carry{},
                                               const Occ& occ = Occ{}) {
    constexpr bool kSparse = std::is_same_v<Occ, OccK>;
    // Per plane of the chunk, written once by one thread so that the 8 waves do not repeat the address arithmetic on their scalar units:
    //   box:  qx0 (a multiple of 4), by0, items per row (0: not staged), rows
    //   org:  byte address of the box origin (texel row by0, column qx0 of channel 0) = words 0, 1 of the plane's buffer descriptor, RN(1 / hh);
    //         the sparse instances: 1 where the staged box holds alpha code 0 alone (box_is_empty), else 0.
    //         The origin may lie before the image: only lanes inside the texture pass the range test.
    //   geo:  zdiff = d - eye_z, hw = w / 2, hh = h / 2, RN(1 / hw)
    __shared__ int4 box[kUChunk];
    __shared__ int4 org[kUChunk];
    __shared__ float4 geo[kUChunk];
    __shared__ __attribute__((aligned(16))) uint32_t stage[2][kUBufWords];

    // ---- blockIdx -> tile, this lane's pixel, the tile's corner pixels: the tile frame of gmpi_device.hpp -----------------------------------------
    const int tid = threadIdx.x;
    FwdTile ft;
    if (!fwd_tile(p, fwd_tile_id(p, blockIdx.x, tiles_x, tiles_y, n_tiles), tiles_x, tiles_y, n_tiles, ft)) return;
    const int n = ft.n;

    uint32_t bad = 0;
    const View vw = view_setup<AC>(p, n, bad);
    check_camera_behind(p, vw, ft.rem == 0 && tid == 0);   // once per view
    const int D = p.D, Ht = p.Ht, Wt = p.Wt, H = p.H, W = p.W;
    const int64_t HW = vw.HW;
    const float* __restrict__ rdv = vw.rays;
    constexpr bool kPacked = std::is_same_v<TexT, rgba8_t>;
    constexpr int kTexelBytes = kPacked ? 4 : 1;   // bytes from one texel of a row to the next
    const TexT* __restrict__ vol = tex_offset(static_cast<const TexT*>(p.rgba), static_cast<int64_t>(vw.m) * p.s_mpi);

    const TileLane tl = tile_lane<kUW, kUH>(ft.txi, ft.tyi, tid, W, H);
    const int64_t pix = tl.pix;
    const float rx = rdv[pix], ry = rdv[HW + pix], rz = rdv[2 * HW + pix];
    const float dot = ray_dot(vw, rx, ry, rz);
    const float rcp_rz = 1.0f / rz;   // correctly rounded; hoisted out of the plane loop (div_by_recip)
    Accum A = load_carry(carry, n, HW, pix);
    const TileCorners tc = tile_corners<kUW, kUH>(ft.txi, ft.tyi, W, H);

    // ---- loader role: item column lcol of box row lrow; byte offset from the box origin (one byte per texel and channel) ---------------------------
    const int lrow = tid / kUCols, lcol = tid - lrow * kUCols;
    const uint32_t l_off = static_cast<uint32_t>(lrow) * static_cast<uint32_t>(p.s_row) + kTexelBytes * kUTPI * lcol;
    const int chan_bytes = __builtin_amdgcn_readfirstlane(static_cast<int>(p.s_chan));   // (planar only)

    [[maybe_unused]] int n_skipped = 0, n_staged = 0;   // (the sparse instances: this tile's planes of either kind)
    for (int kc = 0; kc < D; kc += kUChunk) {
        const int kn = min(kUChunk, D - kc);
        __syncthreads();   // the previous chunk's table and buffers are no longer read
        for (int t = tid; t < kn; t += kUThreads) {
            const int k = kc + t;
            const float zdiff = vw.dhw[3 * k] - vw.ez, ph = vw.dhw[3 * k + 1], pw = vw.dhw[3 * k + 2];
            bool fits;
            int4 bb = item_box<kUTPI>(corner_extent<AC>(vw, rdv, W, zdiff, ph, pw, tc.cx0, tc.cx1, tc.cy0, tc.cy1), kUCols, kURows, fits);
            if (!fits) bb = make_int4(0, 0, 0, 0);
            box[t] = bb;
            const float hw = pw * 0.5f, hh = ph * 0.5f;   // exact halves: (2x) / w == x / (w / 2)
            const int2 o = origin_words(reinterpret_cast<uint64_t>(vol) + static_cast<uint64_t>(static_cast<int64_t>(k) * p.s_plane + bb.y * p.s_row + kTexelBytes * bb.x));
            int empty = 0;
            if constexpr (kSparse) empty = (bb.z > 0 && box_is_empty(occ.map, vw.m, k, D, bb, Ht, Wt)) ? 1 : 0;
            org[t] = make_int4(o.x, o.y, __float_as_int(1.0f / hh), empty);
            geo[t] = make_float4(zdiff, hw, hh, 1.0f / hw);
        }
        __syncthreads();   // table published

        // the four loads of plane t of the chunk; past the end of the chunk, or for a box that is not staged, every offset is rejected.  Issued
        // unconditionally: with the same memory operations on every path the loads stay in flight across the compositing of the plane before.
        auto issue_loads = [&](int t, uint32_t (&L)[4]) {
            const int4 bb = box[min(t, kn - 1)];
            const int4 oo = org[min(t, kn - 1)];
            const int qx0 = __builtin_amdgcn_readfirstlane(bb.x), by0 = __builtin_amdgcn_readfirstlane(bb.y);
            const int nq = t < kn ? __builtin_amdgcn_readfirstlane(bb.z) : 0, nrows = __builtin_amdgcn_readfirstlane(bb.w);
            const __amdgpu_buffer_rsrc_t rsrc = origin_rsrc(oo.x, oo.y);
            const int gx = qx0 + kUTPI * lcol, gy = by0 + lrow;   // (Wt is a multiple of 4: an item lies inside the texture row or outside it)
            // (bitwise on purpose: `&&` would be lowered to exec-mask control flow)
            const bool ok = (lcol < nq) & (lrow < nrows) & (gx >= 0) & (gx < Wt) & (gy >= 0) & (gy < Ht);
            const uint32_t off = ok ? l_off : 0x80000000u;   // == num_records: rejected, reads as zero
            if constexpr (kPacked) {   // four texels as they lie in memory
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 q = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0));
                L[0] = q.x, L[1] = q.y, L[2] = q.z, L[3] = q.w;
            } else {
                L[0] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0);
                L[1] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, chan_bytes, 0);
                L[2] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 2 * chan_bytes, 0);
                L[3] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 3 * chan_bytes, 0);
            }
        };
        // registers -> LDS: (r0 r1 r2 r3), (g0 ..), (b0 ..), (a0 ..) -> four texels (r g b a); lanes outside the box stay idle
        auto store_box = [&](int t, uint32_t* buf, const uint32_t (&L)[4]) {
            const int4 bb = box[t];
            const int nq = __builtin_amdgcn_readfirstlane(bb.z), nrows = __builtin_amdgcn_readfirstlane(bb.w);
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            u32x4 o;
            if constexpr (kPacked) {
                o.x = L[0], o.y = L[1], o.z = L[2], o.w = L[3];
            } else {
                const uint32_t rg_lo = __builtin_amdgcn_perm(L[1], L[0], 0x05010400u);   // g1 r1 g0 r0
                const uint32_t rg_hi = __builtin_amdgcn_perm(L[1], L[0], 0x07030602u);   // g3 r3 g2 r2
                const uint32_t ba_lo = __builtin_amdgcn_perm(L[3], L[2], 0x05010400u);   // a1 b1 a0 b0
                const uint32_t ba_hi = __builtin_amdgcn_perm(L[3], L[2], 0x07030602u);
                o.x = __builtin_amdgcn_perm(ba_lo, rg_lo, 0x05040100u);   // texel x:     a0 b0 g0 r0
                o.y = __builtin_amdgcn_perm(ba_lo, rg_lo, 0x07060302u);   // texel x + 1
                o.z = __builtin_amdgcn_perm(ba_hi, rg_hi, 0x05040100u);
                o.w = __builtin_amdgcn_perm(ba_hi, rg_hi, 0x07060302u);
            }
            if ((lcol < nq) & (lrow < nrows)) *reinterpret_cast<u32x4*>(buf + lrow * kUPitch + kUTPI * lcol) = o;
        };
        // EMPTY (the sparse instances, a staged box of alpha code 0 alone): the same coordinates and the same box test, no tap is read -- every alpha tap is
        // code 0 and every weight is finite (footprint), so the alpha sample is +0 and w = 0 T: the colour taps do not reach the Accum.
        auto composite = [&](int t, const uint32_t* __restrict__ buf, auto EMPTY) {
            const int k = kc + t;
            const int4 bb = box[t];
            const int qx0 = __builtin_amdgcn_readfirstlane(bb.x), by0 = __builtin_amdgcn_readfirstlane(bb.y);
            const int nq = __builtin_amdgcn_readfirstlane(bb.z), nrows = __builtin_amdgcn_readfirstlane(bb.w);
            const float4 g = geo[t];
            if (nq == 0) {   // uniform: the box does not fit -- everybody takes the direct gather (exact doublings of the table's halves)
                gather_plane<TexT, AC, STRICT>(p, vw, vol, k, g.x, g.z + g.z, g.y + g.y, rx, ry, rz, dot, false, bad, A);
                return;
            }
            float ix, iy, s;
            if (STRICT) {
                float u, v;
                plane_coord<AC>(g.x, g.z + g.z, g.y + g.y, vw.ex, vw.ey, rx, ry, rz, vw.cx, vw.cy, ix, iy, s, u, v);
            } else {   // the same quotients through hoisted reciprocals (div_by_recip: correctly rounded, so ix, iy, s are the same bits)
                plane_coord_recip<AC>(g.x, g.y, g.z, g.w, __int_as_float(org[t].z), vw.ex, vw.ey, rx, ry, rz, rcp_rz, vw.cx, vw.cy, ix, iy, s);
            }
            // gather_sample's footprint: weights of taps outside the texture are zero (the box holds zeros there anyway: same products, same bits)
            Footprint f = footprint(ix, iy, Ht, Wt);
            const bool x0in = f.x0 >= 0 && f.x0 <= Wt - 1, x1in = f.x0 >= -1 && f.x0 <= Wt - 2;
            const bool y0in = f.y0 >= 0 && f.y0 <= Ht - 1, y1in = f.y0 >= -1 && f.y0 <= Ht - 2;
            if (!(x0in && y0in)) f.nw = 0.0f;
            if (!(x1in && y0in)) f.ne = 0.0f;
            if (!(x0in && y1in)) f.sw = 0.0f;
            if (!(x1in && y1in)) f.se = 0.0f;
            const int lx = f.x0 - qx0, ly = f.y0 - by0;
            const bool inb = (lx >= 0) & (ly >= 0) & (lx + 1 < kUTPI * nq) & (ly + 1 < nrows);
            const bool any_w = (f.nw != 0.0f) | (f.ne != 0.0f) | (f.sw != 0.0f) | (f.se != 0.0f);
            if (__builtin_expect((!inb) & any_w, 0)) {   // per lane: a pixel whose taps the box does not hold (no pinhole ray field)
                gather_plane<TexT, AC, STRICT>(p, vw, vol, k, g.x, g.z + g.z, g.y + g.y, rx, ry, rz, dot, false, bad, A);
                return;
            }
            if constexpr (decltype(EMPTY)::value) {
                blend<STRICT>(A, 0.0f, 0.0f, 0.0f, 0.0f, s, dot);
                return;
            }
            // a footprint outside the box with every weight zero (the sentinel corner of NaN / far-off coordinates) reads texel (0, 0) of the box
            const uint32_t idx = inb ? static_cast<uint32_t>(ly * kUPitch + lx) : 0u;
            const uint32_t t_nw = buf[idx], t_ne = buf[idx + 1], t_sw = buf[idx + kUPitch], t_se = buf[idx + kUPitch + 1];   // two ds_read2_b32
            float smp[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float c_nw = static_cast<float>((t_nw >> (8 * c)) & 0xffu), c_ne = static_cast<float>((t_ne >> (8 * c)) & 0xffu);
                const float c_sw = static_cast<float>((t_sw >> (8 * c)) & 0xffu), c_se = static_cast<float>((t_se >> (8 * c)) & 0xffu);
                if (STRICT) smp[c] = bilerp<true>(unorm8_to_f32(c_nw), unorm8_to_f32(c_ne), unorm8_to_f32(c_sw), unorm8_to_f32(c_se), f);
                else smp[c] = bilerp<false>(c_nw, c_ne, c_sw, c_se, f) * kInv255;
            }
            blend<STRICT>(A, smp[0], smp[1], smp[2], smp[3], s, dot);
        };

        uint32_t L[4];
        if constexpr (kSparse) {
            // The chunk's empty planes as one wave-uniform 64-bit mask (lane l of every wave reads row l of the table).  Empty planes pass no barrier and
            // take no buffer: the two buffers alternate over the other planes alone (ns), and the prefetch goes to the next of THOSE, so that a store
            // still lands in the buffer that every wave has left at the barrier before.
            static_assert(kUChunk <= 64, "one bit per plane of the chunk");
            const int ln = tid & 63;
            const bool l_empty = ln < kn && org[min(ln, kn - 1)].w != 0;
            const uint64_t empty = __ballot(l_empty);
            const uint64_t staged = __ballot(ln < kn && !l_empty && box[min(ln, kn - 1)].z > 0);
            const uint64_t live = ~empty & (kn >= 64 ? ~uint64_t(0) : (uint64_t(1) << kn) - 1);
            n_skipped += __popcll(empty), n_staged += __popcll(staged);
            int ns = 0;
            issue_loads(live ? __ffsll(static_cast<unsigned long long>(live)) - 1 : kn, L);
            for (int t = 0; t < kn; ++t) {
                if ((empty >> t) & 1) {   // uniform
                    composite(t, nullptr, std::true_type{});
                    continue;
                }
                uint32_t* buf = stage[ns & 1];
                ++ns;
                store_box(t, buf, L);
                __syncthreads();          // this box visible; everybody is done reading the box staged before it (the other buffer)
                const uint64_t rest = t >= 63 ? uint64_t(0) : (live >> (t + 1)) << (t + 1);
                issue_loads(rest ? __ffsll(static_cast<unsigned long long>(rest)) - 1 : kn, L);   // in flight while plane t is composited
                composite(t, buf, std::false_type{});
            }
        } else {
            issue_loads(0, L);
            for (int t = 0; t < kn; ++t) {
                uint32_t* buf = stage[t & 1];
                store_box(t, buf, L);
                __syncthreads();          // box t visible; everybody is done reading box t - 1 (the other buffer)
                issue_loads(t + 1, L);    // in flight while plane t is composited
                composite(t, buf, std::false_type{});
            }
        }
    }
    if constexpr (kSparse) {
        if (occ.stats != nullptr && tid == 0) {
            atomicAdd(occ.stats, static_cast<uint32_t>(n_skipped));
            atomicAdd(occ.stats + 1, static_cast<uint32_t>(n_staged));
        }
    }
    const LastPlane lp = last_plane(p, vw);
    if (leaves_last_plane<AC>(vw, lp, rx, ry, rz)) bad |= GMPI_STATUS_OUT_OF_LAST_PLANE;
    store_pixel<STRICT>(p, n, HW, pix, A, dot, tl.active, carry);
    report_status(p.status, bad);
}

// (strict-order instances: 6 waves per SIMD -- at 8 the 16 per-tap conversions push one of them 12 bytes into scratch)
template <bool AC, bool STRICT>
__global__ __launch_bounds__(kUThreads, STRICT ? 6 : 8) void render_u8_kernel(const KParams p, const int tiles_x, const int tiles_y, const int n_tiles) {
    render_u8_tile<u8_t, AC, STRICT>(p, tiles_x, tiles_y, n_tiles);
}
// (the packed loader holds fewer registers: at 7 waves per SIMD asked for, the strict-order instances take 61 / 63 VGPRs without scratch -- 8 waves;
//  with 6 asked for the allocator spreads to 73 / 75 -- 6 waves)
template <bool AC, bool STRICT>
__global__ __launch_bounds__(kUThreads, STRICT ? 7 : 8) void render_rgba8_kernel(const KParams p, const int tiles_x, const int tiles_y, const int n_tiles) {
    render_u8_tile<rgba8_t, AC, STRICT>(p, tiles_x, tiles_y, n_tiles);
}

// (the carry instances: the state's five loads and stores lie outside the plane loop; same bounds as their one-shot twins)
template <bool AC, bool STRICT>
__global__ __launch_bounds__(kUThreads, STRICT ? 6 : 8) void render_u8_chunk_kernel(const KParams p, const CarryK carry, const int tiles_x, const int tiles_y, const int n_tiles) {
    render_u8_tile<u8_t, AC, STRICT>(p, tiles_x, tiles_y, n_tiles, carry);
}
template <bool AC, bool STRICT>
__global__ __launch_bounds__(kUThreads, STRICT ? 7 : 8) void render_rgba8_chunk_kernel(const KParams p, const CarryK carry, const int tiles_x, const int tiles_y, const int n_tiles) {
    render_u8_tile<rgba8_t, AC, STRICT>(p, tiles_x, tiles_y, n_tiles, carry);
}

// (the sparse instances: the bounds of their dense twins)
template <bool AC, bool STRICT>
__global__ __launch_bounds__(kUThreads, STRICT ? 6 : 8) void render_u8_sparse_kernel(const KParams p, const OccK occ, const int tiles_x, const int tiles_y, const int n_tiles) {
    render_u8_tile<u8_t, AC, STRICT>(p, tiles_x, tiles_y, n_tiles, NoCarry{}, occ);
}
template <bool AC, bool STRICT>
__global__ __launch_bounds__(kUThreads, STRICT ? 7 : 8) void render_rgba8_sparse_kernel(const KParams p, const OccK occ, const int tiles_x, const int tiles_y, const int n_tiles) {
    render_u8_tile<rgba8_t, AC, STRICT>(p, tiles_x, tiles_y, n_tiles, NoCarry{}, occ);
}

// ---- the occupancy map: map[m, k, by, bx] = the largest alpha code among the texels of block (by, bx) of plane k of MPI m that exist (border blocks are
//      partial).  One lane per texel column, 16 rows each, a maximum over 16 lanes; 256 columns per workgroup.  Only the alpha bytes are read: `a_off` is the
//      alpha channel's byte offset inside a plane (3 s_chan; 3 for channels-last texels), `xs` the bytes from one texel of a row to the next (1 / 4). ------
constexpr int kOccThreads = 256;
__global__ __launch_bounds__(kOccThreads) void u8_occupancy_kernel(const uint8_t* __restrict__ vol, const int64_t s_mpi, const int64_t s_plane, const int64_t s_row,
                                                                   const int64_t a_off, const int xs, const int D, const int Ht, const int Wt, const int gx,
                                                                   uint8_t* __restrict__ map) {
    const int nbx = (Wt + kOccBlock - 1) >> kOccShift, nby = (Ht + kOccBlock - 1) >> kOccShift;
    int64_t b = blockIdx.x;
    const int cx = static_cast<int>(b % gx);
    b /= gx;
    const int by = static_cast<int>(b % nby);
    b /= nby;
    const int k = static_cast<int>(b % D);
    const int64_t m = b / D;
    const int x = cx * kOccThreads + static_cast<int>(threadIdx.x);
    uint32_t v = 0;
    if (x < Wt) {
        const uint8_t* __restrict__ col = vol + m * s_mpi + k * s_plane + a_off + static_cast<int64_t>(x) * xs;
        for (int r = 0; r < kOccBlock; ++r) {
            const int y = by * kOccBlock + r;
            if (y < Ht) v = max(v, static_cast<uint32_t>(col[y * s_row]));
        }
    }
#pragma unroll
    for (int o = kOccBlock / 2; o > 0; o >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), o)));   // (every lane is here: no early exit above)
    const int bx = x >> kOccShift;
    if ((threadIdx.x & (kOccBlock - 1)) == 0 && bx < nbx) map[((m * D + k) * nby + by) * nbx + bx] = static_cast<uint8_t>(v);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
// The analogue of volume_stages_in_items for one-byte texels and 4-texel items: an item of a box that touches the border does not straddle it
// (Wt % 4), every item is a naturally aligned dword (base pointer and strides in BYTES), and the in-box byte offsets are kept in 32 bits.
bool u8_variant_supports(const KParams& p) {
    if (u8_interleaved(p)) {   // the same rule in bytes: an item is 4 texels = 16 bytes at dword alignment, a box row at most 64 texels = 256 bytes
        if (p.Wt % kUTPI != 0 || reinterpret_cast<uintptr_t>(p.rgba) % 4 != 0) return false;
        if (p.s_row % 4 != 0 || p.s_plane % 4 != 0 || p.s_mpi % 4 != 0) return false;
        return (kURows + 1) * p.s_row + 4 * kUPitch + 128 < (int64_t(1) << 31);
    }
    if (p.Wt % kUTPI != 0 || reinterpret_cast<uintptr_t>(p.rgba) % kUTPI != 0) return false;
    if (p.s_row % kUTPI != 0 || p.s_chan % kUTPI != 0 || p.s_plane % kUTPI != 0 || p.s_mpi % kUTPI != 0) return false;
    return 3 * p.s_chan + (kURows + 1) * p.s_row + 128 < (int64_t(1) << 31);
}

int u8_variant_query(int what) {
    switch (what) {
        case 16: return kUW;
        case 17: return kUPitch;
        case 18: return kURows;
        case 20: return 1;   // the channels-last instances (rgba8_t) are built in
        case 53: return kOccBlock;   // texels per side of a block of the occupancy map
        default: return -1;
    }
}

hipError_t launch_u8(const KParams& p, hipStream_t stream) {
    const FwdTileGrid tg = fwd_tile_grid<kUW, kUH>(p);
    const dim3 block(kUThreads);
    const bool packed = u8_interleaved(p);
    dispatch_ac_strict(p.flags, [&](auto AC, auto STRICT) {
        if (packed) hipLaunchKernelGGL((render_rgba8_kernel<decltype(AC)::value, decltype(STRICT)::value>), tg.grid, block, 0, stream, p, tg.tiles_x, tg.tiles_y, tg.n_tiles);
        else hipLaunchKernelGGL((render_u8_kernel<decltype(AC)::value, decltype(STRICT)::value>), tg.grid, block, 0, stream, p, tg.tiles_x, tg.tiles_y, tg.n_tiles);
    });
    return hipGetLastError();
}
hipError_t launch_u8_sparse(const KParams& p, const uint8_t* map, uint32_t* stats, hipStream_t stream) {
    const FwdTileGrid tg = fwd_tile_grid<kUW, kUH>(p);
    const dim3 block(kUThreads);
    const bool packed = u8_interleaved(p);
    const OccK occ{map, stats};
    dispatch_ac_strict(p.flags, [&](auto AC, auto STRICT) {
        if (packed) hipLaunchKernelGGL((render_rgba8_sparse_kernel<decltype(AC)::value, decltype(STRICT)::value>), tg.grid, block, 0, stream, p, occ, tg.tiles_x, tg.tiles_y, tg.n_tiles);
        else hipLaunchKernelGGL((render_u8_sparse_kernel<decltype(AC)::value, decltype(STRICT)::value>), tg.grid, block, 0, stream, p, occ, tg.tiles_x, tg.tiles_y, tg.n_tiles);
    });
    return hipGetLastError();
}
// The map of a volume of M x D planes of Ht x Wt texels: its bytes, and the launch that fills it (byte strides of the alpha channel, see the kernel).
uint64_t u8_occupancy_bytes(int M, int D, int Ht, int Wt) {
    return static_cast<uint64_t>(M) * D * ((Ht + kOccBlock - 1) / kOccBlock) * ((Wt + kOccBlock - 1) / kOccBlock);
}
hipError_t launch_u8_occupancy(const void* vol, int64_t s_mpi, int64_t s_plane, int64_t s_row, int64_t a_off, int xs, int M, int D, int Ht, int Wt, uint8_t* map,
                               hipStream_t stream) {
    const int gx = (Wt + kOccThreads - 1) / kOccThreads;
    const int64_t groups = static_cast<int64_t>(M) * D * ((Ht + kOccBlock - 1) / kOccBlock) * gx;
    if (groups > 0x7fffffff) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(u8_occupancy_kernel, dim3(static_cast<uint32_t>(groups)), dim3(kOccThreads), 0, stream, static_cast<const uint8_t*>(vol), s_mpi, s_plane, s_row,
                       a_off, xs, D, Ht, Wt, gx, map);
    return hipGetLastError();
}
hipError_t launch_u8_chunk(const KParams& p, const CarryK& carry, hipStream_t stream) {
    const FwdTileGrid tg = fwd_tile_grid<kUW, kUH>(p);
    const dim3 block(kUThreads);
    const bool packed = u8_interleaved(p);
    dispatch_ac_strict(p.flags, [&](auto AC, auto STRICT) {
        if (packed) hipLaunchKernelGGL((render_rgba8_chunk_kernel<decltype(AC)::value, decltype(STRICT)::value>), tg.grid, block, 0, stream, p, carry, tg.tiles_x, tg.tiles_y, tg.n_tiles);
        else hipLaunchKernelGGL((render_u8_chunk_kernel<decltype(AC)::value, decltype(STRICT)::value>), tg.grid, block, 0, stream, p, carry, tg.tiles_x, tg.tiles_y, tg.n_tiles);
    });
    return hipGetLastError();
}

}  // namespace gmpi
