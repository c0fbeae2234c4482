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
#include "gmpi_backward.hpp"

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

template <typename TexT>
__device__ __forceinline__ void gather_taps(const TexT* __restrict__ pl, int64_t s_chan, int64_t s_row, int Ht, int Wt, float ix, float iy, Taps& q) {
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    q.wx1 = ix - fx0, q.wx0 = (fx0 + 1.0f) - ix;
    q.wy1 = iy - fy0, q.wy0 = (fy0 + 1.0f) - iy;
    const int x0 = (fx0 >= -2.0f && fx0 <= static_cast<float>(Wt)) ? static_cast<int>(fx0) : -2;   // (NaN / huge coordinates: out of range)
    const int y0 = (fy0 >= -2.0f && fy0 <= static_cast<float>(Ht)) ? static_cast<int>(fy0) : -2;
    const bool x0in = x0 >= 0 && x0 <= Wt - 1, x1in = x0 >= -1 && x0 <= Wt - 2;
    const bool y0in = y0 >= 0 && y0 <= Ht - 1, y1in = y0 >= -1 && y0 <= Ht - 2;
    const int xa = min(max(x0, 0), Wt - 1), xb = min(max(x0 + 1, 0), Wt - 1);
    const int ya = min(max(y0, 0), Ht - 1), yb = min(max(y0 + 1, 0), Ht - 1);
    const int64_t oa = static_cast<int64_t>(ya) * s_row, ob = static_cast<int64_t>(yb) * s_row;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const TexT* __restrict__ ch = pl + c * s_chan;
        const float nw = to_f32(ch[oa + xa]), ne = to_f32(ch[oa + xb]), sw = to_f32(ch[ob + xa]), se = to_f32(ch[ob + xb]);
        q.t[c][0] = (x0in && y0in) ? nw : 0.0f;
        q.t[c][1] = (x1in && y0in) ? ne : 0.0f;
        q.t[c][2] = (x0in && y1in) ? sw : 0.0f;
        q.t[c][3] = (x1in && y1in) ? se : 0.0f;
    }
}

// Slab layout (floats): component j of tile t of view n at ws[(j * N + n) * T + t];  j = 0..2 eye, 3..5 z_dir, 6 + 3k + (0, 1, 2) = plane k's
// (d, h, w).  Every slot is written by exactly one workgroup.
template <typename TexT, bool AC, bool STRICT, bool DHW>
__global__ __launch_bounds__(kGT) void geometry_pixel_kernel(const KParams p, const BwdParams b, float* __restrict__ g_ray, float* __restrict__ slab,
                                                             const int tiles_x, const int n_tiles) {
    __shared__ float4 pcA[kGChunk];                    // zdiff, w, h, RN(2/w)
    __shared__ float pcB[kGChunk];                     // RN(2/h)
    __shared__ float red[DHW ? kGWaves * kGChunk * 3 : 1];   // per wave and plane: (d, h, w) partial sums
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
    const TexT* __restrict__ vol = static_cast<const TexT*>(p.rgba) + static_cast<int64_t>(vw.m) * p.s_mpi;
    BwdPixel bp;
    bwd_pixel_setup<TexT, AC, true>(bp, p, vw, n, px, py, active, b.g_rgb, b.g_depth, b.g_T, vol);
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
            gather_taps<TexT>(vol + static_cast<int64_t>(kc + t) * p.s_plane, p.s_chan, p.s_row, Ht, Wt, ix, iy, q);
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
                float vd = g_s * rrz, vh = -0.5f * g_y * y * rh, vw = -0.5f * g_x * x * rw;   // d(2x/w)/dw = -(2/w)(x/w)
                vd = active ? vd : 0.0f, vh = active ? vh : 0.0f, vw = active ? vw : 0.0f;
                vd = wave_sum(vd), vh = wave_sum(vh), vw = wave_sum(vw);
                if (lane == 0) {
                    float* o = red + (wave * kGChunk + t) * 3;
                    o[0] = vd, o[1] = vh, o[2] = vw;
                }
            }
        }
        if (DHW && slab != nullptr) {   // this chunk's plane sums: the waves in order, one slot per (component, plane)
            __syncthreads();
            for (int i = tid; i < 3 * kn; i += kGT) {
                const int t = i / 3, j = i - 3 * t;
                float v = red[t * 3 + j];
#pragma unroll
                for (int wv = 1; wv < kGWaves; ++wv) v += red[(wv * kGChunk + t) * 3 + j];
                slab[(6 + 3 * static_cast<int64_t>(kc + t) + j) * ncomp_stride + static_cast<int64_t>(n) * n_tiles + tile] = v;
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

static int tiles_x_of(const KParams& p) { return (p.W + kGTW - 1) / kGTW; }
static int tiles_of(const KParams& p) { return tiles_x_of(p) * ((p.H + kGTH - 1) / kGTH); }

}  // namespace bwgeo

uint64_t geometry_backward_workspace_bytes(const KParams& p, bool want_dhw) {
    const uint64_t comps = 6u + (want_dhw ? 3u * static_cast<uint64_t>(p.D) : 0u);
    return (comps * p.N * static_cast<uint64_t>(bwgeo::tiles_of(p)) * sizeof(float) + 255) / 256 * 256;
}

// g_ray [N,3,H,W], g_eye / g_z [N,3], g_dhw [M,D,3]: overwritten; nullptr = not wanted.  p.ws must hold geometry_backward_workspace_bytes(p,
// g_dhw != nullptr) bytes when any of g_eye, g_z, g_dhw is wanted (checked by the caller).
hipError_t launch_backward_geometry(const KParams& p, int dtype, const float* g_rgb, const float* g_depth, const float* g_T, float* g_ray, float* g_eye,
                                    float* g_z, float* g_dhw, hipStream_t stream) {
    BwdParams b{};
    b.g_rgb = g_rgb, b.g_depth = g_depth, b.g_T = g_T;
    const bool want_dhw = g_dhw != nullptr;
    float* slab = (g_eye || g_z || g_dhw) ? static_cast<float*>(p.ws) : nullptr;
    {
        using namespace bwgeo;
        const int tx = tiles_x_of(p), nt = tiles_of(p);
        const dim3 grid(xcd_grid_per_group(nt, nt), p.N);
        dispatch_dtype(dtype, [&](auto t) {
            dispatch_bool(p.flags & GMPI_FLAG_ALIGN_CORNERS, [&](auto AC) {
                dispatch_bool(p.flags & GMPI_FLAG_STRICT_ORDER, [&](auto STRICT) {
                    dispatch_bool(want_dhw, [&](auto DHW) {
                        hipLaunchKernelGGL((geometry_pixel_kernel<typename decltype(t)::type, decltype(AC)::value, decltype(STRICT)::value, decltype(DHW)::value>),
                                           grid, dim3(kGT), 0, stream, p, b, g_ray, slab, tx, nt);
                    });
                });
            });
        });
    }
    if (slab != nullptr) {
        const dim3 grid(6 + (want_dhw ? 3 * p.D : 0), std::max(p.N, p.M));
        hipLaunchKernelGGL(bwgeo::geometry_reduce_kernel, grid, dim3(bwgeo::kGRed), 0, stream, p, slab, bwgeo::tiles_of(p), g_eye, g_z, g_dhw);
    }
    return hipGetLastError();
}

}  // namespace gmpi
