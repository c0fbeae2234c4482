// gmpi_abi.hip -- the extern "C" entry points declared in include/gmpi_render.h, plus the small
// auxiliary kernels (diagnostics, exhaustive range check, uint8 frame epilogue).
#include "gmpi_device.hpp"
#include "gmpi_shared.hpp"

#include "../../include/gmpi_render.h"

#include <atomic>
#include <cstdlib>

namespace gmpi {

hipError_t launch_gather(const KParams& p, int dtype, hipStream_t stream);  // render_gather.hip
hipError_t launch_lds(const KParams& p, int dtype, int tune, hipStream_t stream);  // render_lds.hip
hipError_t launch_gather_chunk(const KParams& p, const CarryK& carry, int dtype, hipStream_t stream);   // render_gather.hip
hipError_t launch_lds_chunk(const KParams& p, const CarryK& carry, int dtype, hipStream_t stream);      // render_lds.hip
hipError_t launch_u8_chunk(const KParams& p, const CarryK& carry, hipStream_t stream);                  // render_u8.hip
hipError_t launch_backward_chunk(const KParams& p, int dtype, const float* g_rgb, const float* g_depth, const float* g_T, const float* T_in, const float* S_in,
                                 float* S_out, float* g_rgba, const int64_t* gstride, bool tiles, hipStream_t stream);   // render_backward.hip
hipError_t launch_backward(const KParams& p, int dtype, const float* g_rgb, const float* g_depth, const float* g_T, float* g_rgba,
                           const int64_t* gstride, bool tiles, hipStream_t stream);  // render_backward.hip
bool lds_variant_supports(const KParams& p, int dtype);                     // render_lds.hip
int lds_variant_query(int what);                                            // render_lds.hip
hipError_t launch_wave(const KParams& p, int dtype, int tune, hipStream_t stream);  // render_wave.hip
bool wave_variant_supports(const KParams& p, int dtype);                    // render_wave.hip
hipError_t launch_band(const KParams& p, int dtype, int tune, hipStream_t stream);  // render_band.hip
bool band_variant_supports(const KParams& p, int dtype);                    // render_band.hip
hipError_t launch_band_chunk(const KParams& p, const CarryK& carry, int dtype, hipStream_t stream);   // render_band.hip
bool band_takes_tensors(const KParams& p, int dtype);                       // render_band.hip (band_variant_supports without its workspace clause)
bool band_workspace_ok(const KParams& p, int dtype);                        // render_band.hip
uint64_t band_workspace_bytes(const KParams& p, int dtype);                 // render_band.hip
uint32_t* band_gate_words(const KParams& p, int dtype);                     // render_band.hip
int band_pixels_wide(int dtype);                                            // render_band.hip
uint64_t backward_gather_workspace_bytes(const KParams& p, int dtype);      // render_backward_gather.hip
uint64_t geometry_backward_workspace_bytes(const KParams& p, bool want_dhw, bool want_plane_z = false);   // render_backward_geometry.hip
uint64_t layout_gather_workspace_bytes(const KParams& p, bool depth);       // render_backward_gather.hip
int layout_gather_runs(const KParams& p);                                   // render_backward_gather.hip
void layout_gather_force_runs(int runs);                                    // render_backward_gather.hip
hipError_t launch_layout_backward_gather(const KParams& p, int dtype, const SharedK& sh, const DepthK* dk, const SharedG& g, bool overwrite,
                                         hipStream_t stream);               // render_backward_gather.hip
hipError_t launch_shared(const KParams& p, int dtype, const SharedK& sh, hipStream_t stream);   // render_shared.hip
hipError_t launch_shared_backward(const KParams& p, int dtype, const SharedK& sh, const SharedG& g, bool tiles, hipStream_t stream);   // render_shared.hip
hipError_t launch_shared_forward(const KParams& p, int dtype, const SharedK& sh, hipStream_t stream);   // render_shared_forward.hip
bool shared_forward_supports(const KParams& p, int dtype, const SharedK& sh);   // render_shared_forward.hip
int shared_forward_query(int what);                                         // render_shared_forward.hip
hipError_t launch_shaded(const KParams& p, int dtype, const ShadeK& sh, hipStream_t stream);   // render_shaded.hip
bool shaded_forward_supports(const KParams& p, int dtype, const ShadeK& sh);   // render_shaded.hip
hipError_t launch_shaded_forward(const KParams& p, int dtype, const ShadeK& sh, hipStream_t stream);   // render_shaded.hip
hipError_t launch_shaded_chain_rule(const KParams& p, int dtype, const ShadeK& sh, float* g, const int64_t* gst, float* g_shading, const int64_t* qst,
                                    hipStream_t stream);   // render_shaded.hip
hipError_t launch_zero_image(float* img, const int64_t* st, int M, int Ht, int Wt, hipStream_t stream);   // render_shaded.hip
hipError_t launch_backward_shading_only(const KParams& p, int dtype, const ShadeK& sh, const float* g_rgb, const float* g_depth, const float* g_T, float* g_shading,
                                        const int64_t* qst, hipStream_t stream);   // render_backward.hip
hipError_t launch_backward_shaded(const KParams& p, int dtype, const ShadeK& sh, const float* g_rgb, const float* g_depth, const float* g_T, float* g_rgba,
                                  const int64_t* gstride, bool tiles, hipStream_t stream);   // render_backward.hip
hipError_t launch_depth(const KParams& p, int dtype, const SharedK& sh, const DepthK& dk, hipStream_t stream);   // render_depth.hip
hipError_t launch_depth_backward(const KParams& p, int dtype, const SharedK& sh, const DepthK& dk, const SharedG& g, hipStream_t stream);   // render_depth.hip
hipError_t launch_depth_backward_tile(const KParams& p, int dtype, const SharedK& sh, const DepthK& dk, const SharedG& g, hipStream_t stream);   // render_depth_tile.hip
bool depth_tile_supports(const KParams& p);                                 // render_depth_tile.hip
int depth_tile_planes();                                                    // render_depth_tile.hip
hipError_t launch_depth_window(const KParams& p, int dtype, const SharedK& sh, const DepthK& dk, hipStream_t stream);   // render_depth_window.hip
bool depth_window_supports(const KParams& p, int dtype, const SharedK& sh);   // render_depth_window.hip
int depth_window_query(int what);                                           // render_depth_window.hip
hipError_t launch_u8(const KParams& p, hipStream_t stream);                 // render_u8.hip
bool u8_variant_supports(const KParams& p);                                 // render_u8.hip
int u8_variant_query(int what);                                             // render_u8.hip
hipError_t launch_u8_sparse(const KParams& p, const uint8_t* map, uint32_t* stats, hipStream_t stream);   // render_u8.hip
uint64_t u8_occupancy_bytes(int M, int D, int Ht, int Wt);                   // render_u8.hip
hipError_t launch_u8_occupancy(const void* vol, int64_t s_mpi, int64_t s_plane, int64_t s_row, int64_t a_off, int xs, int M, int D, int Ht, int Wt, uint8_t* map,
                               hipStream_t stream);                         // render_u8.hip
hipError_t launch_gather_layers(const KParams& p, int dtype, hipStream_t stream);   // render_gather.hip
hipError_t launch_layers(const KParams& p, int dtype, hipStream_t stream);  // render_layers.hip
bool layers_variant_supports(const KParams& p, int dtype);                  // render_layers.hip
hipError_t launch_backward_layers(const KParams& p, int dtype, const float* g_rgb, const float* g_depth, const float* g_T, float* g_layers, const int64_t* gstride,
                                  bool tiles, hipStream_t stream);   // render_backward.hip
bool backward_layers_tile_supports(const KParams& p, int dtype, const int64_t* gstride);   // render_backward.hip
hipError_t launch_backward_geometry(const KParams& p, int dtype, const float* g_rgb, const float* g_depth, const float* g_T, float* g_ray, float* g_eye,
                                    float* g_z, float* g_dhw, hipStream_t stream);   // render_backward_geometry.hip
hipError_t launch_backward_geometry_inplace(const KParams& p, int dtype, bool layers, const float* g_rgb, const float* g_depth, const float* g_T, float* g_ray,
                                            float* g_eye, float* g_z, float* g_dhw, hipStream_t stream);   // render_backward_geometry.hip
hipError_t launch_backward_geometry_layout(const KParams& p, int dtype, const SharedK& sh, const DepthK* dk, const float* g_rgb, const float* g_depth,
                                           const float* g_T, float* g_ray, float* g_eye, float* g_z, float* g_dhw, float* g_pz, hipStream_t stream);   // render_backward_geometry.hip

// ---- min/max of the normalised grid on the last plane (mpi.py:103-109 diagnostics) --------------
template <bool AC>
__global__ __launch_bounds__(256) void last_plane_uv_kernel(const KParams p, float* __restrict__ uv) {
    const int n = blockIdx.x;
    uint32_t bad_index = 0;  // (the forward reports a bad view index; here it is only clamped)
    const int m = view_mpi(p, n, bad_index);
    const float* dhw = p.dhw + (static_cast<int64_t>(m) * p.D + (p.D - 1)) * 3;
    const float d = dhw[0], ph = dhw[1], pw = dhw[2];
    const float ex = p.eye_pos[3 * n + 0], ey = p.eye_pos[3 * n + 1], ez = p.eye_pos[3 * n + 2];
    const float zdiff = d - ez;
    const int64_t HW = static_cast<int64_t>(p.H) * p.W;
    const float* rd = p.ray_dir + static_cast<int64_t>(n) * 3 * HW;
    const float inf = __builtin_inff();
    float mnu = inf, mxu = -inf, mnv = inf, mxv = -inf;
    bool nan = false;
    for (int64_t i = threadIdx.x; i < HW; i += blockDim.x) {
        float ix, iy, s, u, v;
        plane_coord<AC>(zdiff, ph, pw, ex, ey, rd[i], rd[HW + i], rd[2 * HW + i], 1.0f, 1.0f, ix, iy, s, u, v);
        nan |= (u != u) || (v != v);
        mnu = fminf(mnu, u), mxu = fmaxf(mxu, u), mnv = fminf(mnv, v), mxv = fmaxf(mxv, v);
    }
    __shared__ float red[4][256];
    __shared__ int red_nan;
    if (threadIdx.x == 0) red_nan = 0;
    red[0][threadIdx.x] = mnu, red[1][threadIdx.x] = mxu, red[2][threadIdx.x] = mnv, red[3][threadIdx.x] = mxv;
    __syncthreads();
    if (nan) atomicOr(&red_nan, 1);
    for (int o = 128; o > 0; o >>= 1) {
        if (static_cast<int>(threadIdx.x) < o) {
            red[0][threadIdx.x] = fminf(red[0][threadIdx.x], red[0][threadIdx.x + o]);
            red[1][threadIdx.x] = fmaxf(red[1][threadIdx.x], red[1][threadIdx.x + o]);
            red[2][threadIdx.x] = fminf(red[2][threadIdx.x], red[2][threadIdx.x + o]);
            red[3][threadIdx.x] = fmaxf(red[3][threadIdx.x], red[3][threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) {
        const float q = __builtin_nanf("");
        uv[4 * n + threadIdx.x] = red_nan ? q : red[threadIdx.x][0];  // torch.min/max propagate NaN
    }
}

// ---- exhaustive [0,1] check (the reference's full min/max passes) ----------------------------------
template <typename T>
__global__ __launch_bounds__(256) void range_check_kernel(const T* __restrict__ v, int64_t count, uint32_t* status) {
    bool bad = false;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride)
        bad |= !in_unit(to_f32(v[i]));
    report_status(status, bad ? GMPI_STATUS_RGBA_RANGE : 0u);
}

// 16-byte vectorised body for contiguous, aligned volumes
template <typename T, int PER>
__global__ __launch_bounds__(256) void range_check_vec_kernel(const uint4* __restrict__ v, int64_t nvec,
                                                              uint32_t* status) {
    // A pure streaming read: non-temporal loads (7.0-7.4 TB/s against 6.3 for cached loads, profiles/r03_calibration.txt), four 16-byte
    // loads per lane in flight.
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4* __restrict__ vv = reinterpret_cast<const u32x4*>(v);
    bool bad = false;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    auto test = [&](const u32x4& q) {
        const T* e = reinterpret_cast<const T*>(&q);
#pragma unroll
        for (int j = 0; j < PER; ++j) bad |= !in_unit(to_f32(e[j]));
    };
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        const u32x4 q0 = __builtin_nontemporal_load(vv + i), q1 = __builtin_nontemporal_load(vv + i + stride);
        const u32x4 q2 = __builtin_nontemporal_load(vv + i + 2 * stride), q3 = __builtin_nontemporal_load(vv + i + 3 * stride);
        test(q0), test(q1), test(q2), test(q3);
    }
    for (; i < nvec; i += stride) test(__builtin_nontemporal_load(vv + i));
    report_status(status, bad ? GMPI_STATUS_RGBA_RANGE : 0u);
}

// ---- diagnostic: a pure streaming read (the ceiling bench.py quotes next to the render kernel's rate) -------------------------------
// Non-temporal 4-byte loads, 32 per lane in flight, 2 workgroups per CU: the fastest read pattern of profiles/r03_calibration.txt
// (7.0-7.4 TB/s on MI355X; cached loads and 16-byte loads stream at 6.3-7.1).
__global__ __launch_bounds__(256) void stream_probe_kernel(const uint32_t* __restrict__ v, int64_t nwords, uint32_t* sink) {
    uint32_t acc = 0;
    const int64_t trip = static_cast<int64_t>(256) * 32, stride = static_cast<int64_t>(gridDim.x) * trip;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * trip + threadIdx.x; i + 31 * 256 < nwords; i += stride) {
#pragma unroll
        for (int u = 0; u < 32; ++u) acc |= __builtin_nontemporal_load(v + i + u * 256);
    }
    if (acc == 0x9e3779b9u && sink != nullptr) sink[0] = acc;  // (keeps the loads alive; a volume of [0, 1] values never has this OR)
}

// ---- driver epilogue: float frames -> uint8 (render_video.py:118-126) -------------------------------
__global__ __launch_bounds__(256) void frames_to_uint8_kernel(const float* __restrict__ rgb, const float* __restrict__ dep,
                                                              int64_t HW, int64_t total, float dnear, float span,
                                                              uint8_t* __restrict__ img8, uint8_t* __restrict__ dep8) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;  // over N*H*W
    if (i >= total) return;
    const int64_t n = i / HW, q = i - n * HW;
    if (img8) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = rgb[(n * 3 + c) * HW + q];
            v = v + 1.0f;    // img = (img + 1) / 2.0
            v = v / 2.0f;
            v = v * 255.0f;  // (img * 255).astype(np.uint8): C truncation toward zero
            // astype(uint8) of an out-of-range float is UB in numpy; compositing keeps v in [0,255], clamp for safety
            v = fminf(fmaxf(v, 0.0f), 255.0f);
            img8[i * 3 + c] = static_cast<uint8_t>(static_cast<int>(v));
        }
    }
    if (dep8) {
        float v = dep[i];
        v = v - dnear;
        v = v / span;
        v = fminf(fmaxf(v, 0.0f), 1.0f);  // np.clip
        v = v * 255.0f;
        dep8[i] = static_cast<uint8_t>(static_cast<int>(v));
    }
}

// ---- rays of N views: R @ unit_dirs with the CPU sgemm's FMA order (camera.py:189-211) -----------------------
__global__ __launch_bounds__(256) void generate_rays_kernel(const float* __restrict__ c2w, const float* __restrict__ dirs,
                                                            int64_t HW, float* __restrict__ ray, float* __restrict__ eye,
                                                            float* __restrict__ zdir) {
    const int n = blockIdx.y;
    const float* m = c2w + 16 * n;
    const float r00 = m[0], r01 = m[1], r02 = m[2], r10 = m[4], r11 = m[5], r12 = m[6], r20 = m[8], r21 = m[9], r22 = m[10];
    if (blockIdx.x == 0 && threadIdx.x < 3) {
        eye[3 * n + threadIdx.x] = m[4 * threadIdx.x + 3];
        zdir[3 * n + threadIdx.x] = m[4 * threadIdx.x + 2];
    }
    const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    const float d0 = dirs[p], d1 = dirs[HW + p], d2 = dirs[2 * HW + p];
    float* o = ray + static_cast<int64_t>(n) * 3 * HW + p;
    o[0] = __builtin_fmaf(r02, d2, __builtin_fmaf(r01, d1, r00 * d0));
    o[HW] = __builtin_fmaf(r12, d2, __builtin_fmaf(r11, d1, r10 * d0));
    o[2 * HW] = __builtin_fmaf(r22, d2, __builtin_fmaf(r21, d1, r20 * d0));
}

// ---- LightRenderer.compute_depth (light_renderer.py:82-100): composite plane depths with the un-warped alphas ----
template <typename T>
__global__ __launch_bounds__(256) void alpha_depth_kernel(const T* __restrict__ alpha, int64_t sb, int64_t sd, int64_t sr,
                                                          const float* __restrict__ ds, int D, int H, int W,
                                                          float* __restrict__ depth, float* __restrict__ tout) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const T* a = alpha + b * sb + y * sr + x;
    float Tr = 1.0f, Z = 0.0f;
    alpha_depth_composite(D, ds, [&](int k) { return to_f32(a[k * sd]); }, Tr, Z);   // (gmpi_shared.hpp: one text with ramp_depth_kernel)
    const int64_t o = (static_cast<int64_t>(b) * H + y) * W + x;
    depth[o] = Z;
    if (tout) tout[o] = Tr;
}

// ---- self-test of div_by_recip (gmpi_device.hpp): q = n / d through RN(1/d) against the IEEE division --------------
// Operand classes: 0 = zdiff / ray_z (plane distance minus eye height over the z component of a unit ray), 1 = x / (w/2)
// (in-plane position over a plane half extent), 2 = full-range significands and exponents within +-20, 3 = divisors of the
// one significand pattern the correction step's proof treats separately, d = 2^k (2 - 2^-23).
__device__ __forceinline__ uint32_t mix32(uint32_t x) {  // lowbias32
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float unit_float(uint32_t h) { return __uint_as_float(0x3f800000u | (h >> 9)) - 1.0f; }  // [0, 1)
__global__ __launch_bounds__(256) void selftest_division_kernel(uint64_t pairs, uint32_t seed, unsigned long long* mism) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    unsigned int bad[4] = {0, 0, 0, 0};
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < pairs; i += stride) {
        const uint32_t lo = static_cast<uint32_t>(i), hi = static_cast<uint32_t>(i >> 32);
        // (the seed enters b non-bijectively: with a = mix32(lo ^ seed) alone two seeds would test permutations of the SAME operand pairs)
        const uint32_t a = mix32(lo ^ seed), b = mix32(a + mix32(seed + 0x5bd1e995u) * 0x9e3779b9u + hi * 0x85ebca6bu + 0x85ebca6bu), c = mix32(b ^ 0xc2b2ae35u);
        const int cls = static_cast<int>(c & 3u);
        float n, d;
        if (cls == 0) {
            n = (unit_float(a) - 0.5f) * 4.0f;             // zdiff in [-2, 2)
            d = 0.35f + 0.65f * unit_float(b);             // ray_z of a unit ray inside a < 70 degree cone
            if (c & 4u) d = -d;
        } else if (cls == 1) {
            n = (unit_float(a) - 0.5f) * 2.0f;             // x in [-1, 1)
            d = 0.02f + 2.0f * unit_float(b);              // half extent of a plane
        } else if (cls == 2) {
            n = __uint_as_float((a & 0x807fffffu) | ((107u + (a >> 23) % 41u) << 23));   // exponent in [-20, 20]
            d = __uint_as_float((b & 0x807fffffu) | ((107u + (b >> 23) % 41u) << 23));
        } else {
            n = __uint_as_float((a & 0x807fffffu) | ((107u + (a >> 23) % 41u) << 23));
            d = __uint_as_float(0x007fffffu | ((107u + (b >> 23) % 41u) << 23) | (b & 0x80000000u));  // 2^k (2 - 2^-23)
        }
        const float r = 1.0f / d;
        const float q = div_by_recip(n, d, r);
        const float q_ref = n / d;
        if (__float_as_uint(q) != __float_as_uint(q_ref) && !(q == 0.0f && q_ref == 0.0f)) bad[cls]++;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned int v = bad[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(mism + k, static_cast<unsigned long long>(v));
    }
}

// takes_u8: the entry has kernels for GMPI_DTYPE_U8 (the forward launch and its workspace query); every other caller refuses the type here.
static int to_kparams(const GmpiRenderParams* q, KParams& p, bool need_outputs, bool need_volume = false, bool takes_u8 = false) {
    if (q == nullptr) return GMPI_E_NULL;
    if (q->struct_size != sizeof(GmpiRenderParams)) return GMPI_E_ABI;
    bool interleaved = false;
    if (q->flags & ~static_cast<uint32_t>(GMPI_FLAG_ALL)) return GMPI_E_FLAGS;  // undefined bits never reach a kernel
    if (q->N < 0 || q->M <= 0 || q->D <= 0 || q->Ht <= 0 || q->Wt <= 0 || q->H <= 0 || q->W <= 0) return GMPI_E_SHAPE;
    if (q->view_to_mpi == nullptr) {
        if (q->views_per_mpi < 1) return GMPI_E_SHAPE;
        if (q->N > static_cast<int64_t>(q->M) * q->views_per_mpi) return GMPI_E_SHAPE;
    }
    if (q->dhw == nullptr || q->ray_dir == nullptr || q->eye_pos == nullptr) return GMPI_E_NULL;
    if (need_outputs && (q->rgb_out == nullptr || q->depth_out == nullptr)) return GMPI_E_NULL;
    if (need_outputs || need_volume) {
        if (q->rgba == nullptr || q->z_dir == nullptr) return GMPI_E_NULL;
        if (q->rgba_dtype < GMPI_DTYPE_F32 || q->rgba_dtype > (takes_u8 ? GMPI_DTYPE_U8 : GMPI_DTYPE_F16)) return GMPI_E_DTYPE;
        // channels-last codes: texel stride 4 with channel stride 1, for GMPI_DTYPE_U8 at the entries that take the type -- and nothing else with [4] != 1
        interleaved = takes_u8 && q->rgba_dtype == GMPI_DTYPE_U8 && q->rgba_stride[4] == 4 && q->rgba_stride[2] == 1;
        if (q->rgba_stride[4] != 1 && !interleaved) return GMPI_E_STRIDE;
        for (int i = 0; i < 4; ++i)
            if (q->rgba_stride[i] < 0) return GMPI_E_STRIDE;
        if (q->rgba_stride[3] < (interleaved ? 4 : 1) * static_cast<int64_t>(q->Wt) || q->rgba_stride[2] == 0 || q->rgba_stride[1] == 0) return GMPI_E_STRIDE;
    }
    p.rgba = q->rgba;
    p.view_to_mpi = q->view_to_mpi;
    p.dhw = q->dhw;
    p.ray_dir = q->ray_dir;
    p.eye_pos = q->eye_pos;
    p.z_dir = q->z_dir;
    p.rgb_out = q->rgb_out;
    p.depth_out = q->depth_out;
    p.T_out = q->transmittance_out;
    p.status = q->status;
    p.s_mpi = q->rgba_stride[0];
    p.s_plane = q->rgba_stride[1];
    p.s_chan = interleaved ? 0 : q->rgba_stride[2];   // (0: u8_interleaved, gmpi_device.hpp -- the other strides then count bytes)
    p.s_row = q->rgba_stride[3];
    p.N = q->N, p.M = q->M, p.D = q->D, p.Ht = q->Ht, p.Wt = q->Wt, p.H = q->H, p.W = q->W;
    p.views_per_mpi = q->view_to_mpi ? 1 : q->views_per_mpi;
    p.flags = q->flags;
    p.ws = q->workspace;
    p.ws_bytes = q->workspace != nullptr ? q->workspace_bytes : 0;
    p.gate = nullptr, p.gate_gen = 0, p.gate_sense = 0;
    p.band_cols = 1, p.band_rot = 0, p.band_split = 1, p.band_tail = 0;
    return GMPI_OK;
}

// bf16 / fp16: bands (of 256 x 8 pixels) from which AUTO takes the band kernel.  Round 5: 256 = one workgroup on every CU (rounds 3-4: 512 = two).
// At 256 bands (two views of 512^2, eight of 256^2) the band kernel takes 0.115-0.125 ms where the strip / tile kernels take 0.140-0.146, whatever the
// frontal hint says; at 128 bands it loses (0.122-0.133 against 0.078): profiles/r05_small_launches.txt.
constexpr int64_t kAutoBandMin = 256;
constexpr int64_t kAutoBandMinF32 = 1024;  // fp32: bands of 128 x 8 pixels (at 512 -- config 2 -- the strip kernel is as fast: profiles/r03_band_variants.txt)
// The 256-band threshold was measured in DEFAULT mode with frontal-to-moderate cameras (profiles/r05_small_launches.txt).  Two kinds of 16-bit launches keep
// rounds 3-4's threshold of 512 bands: strict-order launches (never measured below it: the strip kernel keeps its 2^18..2^19-pixel range) and launches whose
// caller says that some camera is tilted beyond 0.53 rad (a view the band kernel cannot stage then costs a table kernel and an empty band launch on top).
constexpr int64_t kAutoBandMinUnmeasured = 512;
constexpr int64_t kAutoBandMinShared = 1024, kAutoBandMinSharedF32 = 2048;   // views that share MPIs (config 4's launch, the size that was measured)

// does GMPI_VARIANT_AUTO consider the band kernel for this launch (given a workspace and the band kernel's alignment preconditions)?
static int64_t band_count(const KParams& p, int dtype) {
    const int bw = band_pixels_wide(dtype);
    return static_cast<int64_t>(p.N) * ((p.W + bw - 1) / bw) * ((p.H + 7) / 8);
}
static bool auto_takes_band(const KParams& p, int dtype) {
    if (dtype != GMPI_DTYPE_BF16 && dtype != GMPI_DTYPE_F32 && dtype != GMPI_DTYPE_F16) return false;
    // Views that share one MPI (views_per_mpi > 1: the video paths).  Rounds 3-5 kept them on the tile kernel after a measurement -- config 4 through the band
    // kernel + gate: 1.14 ms against 0.545 -- that was an artefact of the gated tile kernel's loop stride (kGatedGrid, render_lds.hip).  Both kernels interleave
    // such views per band / tile position and read the volume from HBM about once per group; with every view fitting, the band kernel is faster: 8 views of one
    // 512^2 x 96 MPI, yaw within +-0.25 rad: 0.521 -> 0.474 ms (fp32), 0.427 -> 0.340 (bf16); +-0.35: 0.528 -> 0.495, 0.427 -> 0.346.  A group with a view that
    // does NOT fit goes to the tile kernel as a whole (the table kernel gates every view of the group: two small tile launches next to a thinned band launch
    // lose, 0.78 against 0.545) -- which a caller that knows its cameras spares the launch by saying so (GMPI_FLAG_HINT_OBLIQUE / _TILTED).
    if (p.view_to_mpi == nullptr && p.views_per_mpi > 1) {
        if ((p.flags & (GMPI_FLAG_HINT_OBLIQUE | GMPI_FLAG_HINT_TILTED)) != 0) return false;
#ifdef GMPI_TUNE
        static const int env_shared = [] { const char* e = getenv("GMPI_TUNE_SHARED"); return e ? atoi(e) : 1; }();   // (0: the old routing, for A/B runs)
        if (env_shared == 0) return false;
#endif
    }
    const int bw = band_pixels_wide(dtype);
    const int64_t cols = (p.W + bw - 1) / bw, rows = (p.H + 7) / 8;
    // (an image that fills less than 3/4 of its bands -- narrower than a band, a ragged last column -- wastes the idle lanes' issue slots:
    //  the tile kernel's 32 x 16 tiles fit such images better)
    if (static_cast<int64_t>(p.W) * 4 < cols * bw * 3 || static_cast<int64_t>(p.H) * 4 < rows * 8 * 3) return false;
    int64_t need = dtype == GMPI_DTYPE_F32 ? kAutoBandMinF32 : kAutoBandMin;
    // (views that share MPIs: only launches of the size that was measured, config 4's -- 8 views of 512^2: 1024 bands of 256 x 8 pixels / 2048 of 128 x 8.  Small
    //  shared launches belong to the tile kernel, whose interleaved tiles keep the one volume in the L2s: 8 views of 256^2 or 2 of 512^2 over a bf16 volume, 256 bands:
    //  0.118 ms against the band kernel's 0.129 (frontal) / 0.143 (0.3 rad of yaw))
    if (p.view_to_mpi == nullptr && p.views_per_mpi > 1) need = dtype == GMPI_DTYPE_F32 ? kAutoBandMinSharedF32 : kAutoBandMinShared;
    // (round 6: GMPI_FLAG_HINT_OBLIQUE counts like _TILTED here -- a camera beyond 0.35 rad is one the band kernel cannot stage at these sizes: 2 views of 512^2 / 8 of
    //  256^2 at 0.45 rad of yaw went through the table kernel, an empty band launch and the gated tile launch, 0.168-0.174 ms against the tile kernel's 0.141-0.145)
    if (dtype != GMPI_DTYPE_F32 && (p.flags & (GMPI_FLAG_STRICT_ORDER | GMPI_FLAG_HINT_TILTED | GMPI_FLAG_HINT_OBLIQUE)) != 0) need = kAutoBandMinUnmeasured;
    return band_count(p, dtype) >= need;
}

// The generation of a two-kernel launch's view gate (KParams::gate_gen): one counter for every entry that stamps gate words into a workspace.
static uint32_t next_gate_gen() {
    static std::atomic<uint32_t> gate_counter{0x6d2b79f5u};
    return gate_counter.fetch_add(1u, std::memory_order_relaxed);
}

static int hip_rc(hipError_t e) { return e == hipSuccess ? GMPI_OK : GMPI_E_LAUNCH - static_cast<int>(e); }

// Channels-last layers (gmpi_mpi_render_layers_launch, gmpi_render_layers_supports): rgba_stride = [s_M, s_D, 1, s_row, 4] in elements, s_row >= 4 Wt, s_M and
// s_D >= 0.  Anything else is GMPI_E_STRIDE, before any other field is looked at.
static int layers_strides_ok(const GmpiRenderParams* q) {
    if (q->rgba_stride[2] != 1 || q->rgba_stride[4] != 4) return GMPI_E_STRIDE;
    if (q->rgba_stride[0] < 0 || q->rgba_stride[1] < 0 || q->rgba_stride[3] < 4 * static_cast<int64_t>(q->Wt)) return GMPI_E_STRIDE;
    return GMPI_OK;
}
// The float layers of *q as the texel instances read them: everything but the strides validated by to_kparams (over a planar stand-in for them), the strides
// in BYTES, s_chan unused.  GMPI_DTYPE_U8 does not come here: the callers forward it to the entries that have the type (the backward refuses it).
// backward: the layers' backward entries -- the volume is needed, the forward's outputs are not.
static int to_kparams_layers(const GmpiRenderParams* q, KParams& p, bool backward = false) {
    GmpiRenderParams planar = *q;
    planar.rgba_stride[0] = planar.rgba_stride[1] = planar.rgba_stride[2] = 1, planar.rgba_stride[3] = q->Wt, planar.rgba_stride[4] = 1;
    const int rc = to_kparams(&planar, p, !backward, backward);
    if (rc != GMPI_OK) return rc;
    const int64_t esize = q->rgba_dtype == GMPI_DTYPE_F32 ? 4 : 2;
    p.s_mpi = q->rgba_stride[0] * esize, p.s_plane = q->rgba_stride[1] * esize, p.s_row = q->rgba_stride[3] * esize, p.s_chan = 0;
    return GMPI_OK;
}
// What gmpi_mpi_render_layers_backward_launch and gmpi_render_layers_backward_supports check alike, in this order: the struct, the layers' strides, the
// type (float layers only), every other field, then the gradient's strides -- [gs_M, gs_D, 1, gs_row, 4] in elements, gs_row >= 4 Wt, gs_M and gs_D positive
// (gs_M = 0 for one MPI).  Fills p (strides in bytes) on GMPI_OK.
static int layers_backward_args(const GmpiRenderParams* q, const int64_t* gst, KParams& p) {
    if (q == nullptr) return GMPI_E_NULL;
    if (q->struct_size != sizeof(GmpiRenderParams)) return GMPI_E_ABI;
    const int rs = layers_strides_ok(q);
    if (rs != GMPI_OK) return rs;
    if (q->rgba_dtype == GMPI_DTYPE_U8) return GMPI_E_DTYPE;   // no gradient flows to codes
    const int rc = to_kparams_layers(q, p, true);
    if (rc != GMPI_OK) return rc;
    if (gst == nullptr) return GMPI_E_NULL;
    if (gst[2] != 1 || gst[4] != 4 || gst[3] < 4 * static_cast<int64_t>(q->Wt)) return GMPI_E_STRIDE;
    if (gst[1] <= 0 || (gst[0] <= 0 && !(gst[0] == 0 && q->M == 1))) return GMPI_E_STRIDE;
    return GMPI_OK;
}

}  // namespace gmpi

using namespace gmpi;

extern "C" {

int gmpi_mpi_render_launch(const GmpiRenderParams* params, void* stream) {
    if (params != nullptr && params->struct_size == sizeof(GmpiRenderParams) && params->N == 0) return GMPI_OK;  // no views
    KParams p;
    const int rc = to_kparams(params, p, true, false, true);
    if (rc != GMPI_OK) return rc;
    if (p.N == 0) return GMPI_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int variant = params->variant;
    if (params->rgba_dtype == GMPI_DTYPE_U8) {
        // 8-bit volumes: one staged kernel and the gather kernel.  AUTO is the staged kernel wherever it can take the tensors -- no threshold, and the
        // camera hints change nothing; nothing below this block sees the type.
        const bool staged = u8_variant_supports(p);
        if (variant == GMPI_VARIANT_AUTO) variant = staged ? GMPI_VARIANT_LDS : GMPI_VARIANT_GATHER;
        if (variant == GMPI_VARIANT_GATHER) {
            if (p.N > 65535) return GMPI_E_SHAPE;  // the gather kernel puts the view index in grid.z
            return hip_rc(launch_gather(p, GMPI_DTYPE_U8, st));
        }
        if (variant == GMPI_VARIANT_LDS && staged) return hip_rc(launch_u8(p, st));
        return GMPI_E_VARIANT;  // WAVE, BAND: not built for this type; LDS: these tensors are not aligned for its loader
    }
    if (variant == GMPI_VARIANT_AUTO) {
        // Measured on MI355X at steady clocks (profiles/r02_variants.txt, "small launches"): the tile kernel wins on large
        // launches (configs 3-5: 32 waves per CU hide its latencies, its shared 32x16 boxes tolerate tilted cameras); the strip
        // kernel wins where the launch under-fills the chip: up to 512 strips of 32x8 pixels (its waves split the planes 6-way),
        // 16-bit volumes up to 1024 strips (3-way), and fp32 volumes between 1537 and 2048 strips (config 2, 8 views of 256^2:
        // the tile kernel needs a second round of workgroups there, 3 x 53 KB of LDS per CU).  Strict-order mode has no plane
        // split: there only launches of 2^18 .. 2^19 pixels go to the strip kernel.
        const int64_t pixels = static_cast<int64_t>(p.N) * p.H * p.W;
        const int64_t strips = static_cast<int64_t>(p.N) * ((p.W + 31) / 32) * ((p.H + 7) / 8);
        const bool strict = (p.flags & GMPI_FLAG_STRICT_ORDER) != 0;
        const bool lds_ok = lds_variant_supports(p, params->rgba_dtype), wave_ok = wave_variant_supports(p, params->rgba_dtype);
        // 16-bit volumes between 513 and 2048 strips: the strip kernel wins by 4-7 % under a frontal camera, the tile kernel by 3-10 % (and
        // more above 1024 strips) from 0.3 rad of yaw on (profiles/r03_pose_sweep.txt) -- the caller's GMPI_FLAG_HINT_FRONTAL decides;
        // without it: tilted.
        const bool frontal = (p.flags & GMPI_FLAG_HINT_FRONTAL) != 0;
        // ... and beyond 0.53 rad of tilt (GMPI_FLAG_HINT_TILTED) the strip kernel's wave-private boxes overflow into half strips and the direct
        // gather: config 2 takes 0.25-0.77 ms instead of 0.16 where the tile kernel stays at 0.21 (profiles/r04_pose_distribution.txt)
        const bool tilted = (p.flags & GMPI_FLAG_HINT_TILTED) != 0;
        // ... and views that SHARE MPIs (round 6): the tile kernel interleaves them per tile, the volume comes from HBM once per group -- 16-bit volumes, 8 views of
        // 256^2 or 2 of 512^2 (2048 strips) under a frontal camera: 0.118 ms against the strip kernel's 0.145 (fp32 volumes: the strip kernel stays ahead, 0.130 / 0.152)
        const bool shared = p.view_to_mpi == nullptr && p.views_per_mpi > 1;
        const bool small = strict ? (pixels <= (int64_t(1) << 19) && pixels > (int64_t(1) << 18))
                         : params->rgba_dtype == GMPI_DTYPE_F32 ? (strips <= 512 || (strips > 1536 && strips <= 2048 && !tilted))
                                                                : (strips <= 512 || (strips <= 2048 && frontal && !shared));
        variant = (wave_ok && (small || !lds_ok)) ? GMPI_VARIANT_WAVE : lds_ok ? GMPI_VARIANT_LDS : GMPI_VARIANT_GATHER;
        // (a launch the band kernel takes -- below -- is not "small", whatever the hints say: 16-bit volumes reach the band threshold at exactly the
        //  2048 strips up to which a frontal hint would pick the strip kernel)
        // (auto_takes_band keeps 16-bit launches of 256-511 bands off the band path in strict-order mode and when the caller says that some camera is
        //  tilted beyond 0.53 rad: a view the band kernel cannot stage goes to the tile kernel behind a table kernel and an empty band launch, ~18 us
        //  that such a small launch feels -- two views of 512^2 at 0.45 rad of yaw: 0.158 ms against the tile kernel's 0.140; the frontal ones 0.120 against 0.143)
        const bool band_path = lds_ok && auto_takes_band(p, params->rgba_dtype) && band_variant_supports(p, params->rgba_dtype);
        if (band_path) variant = GMPI_VARIANT_LDS;
        // Large launches over bf16 / fp32 volumes, when the caller lends a workspace: the band kernel (256 x 8 / 128 x 8 pixel bands, LDS-DMA;
        // 0.81 ms on BASELINE config 3 where the tile kernel takes 1.02, 1.21 against 1.33 with an fp32 volume) -- for the views it can stage.  Whether a view's texel boxes fit the band
        // kernel's buffers depends on the camera (tilt shears the boxes) and is only known on the device, so AUTO launches BOTH kernels and
        // lets the band kernel's table kernel share out the views through a gate word per view (KParams::gate): views with a box that does
        // not fit fall to the tile kernel, the others' tile workgroups exit at once (an empty second launch costs a few microseconds).
        if (band_path) {
            const uint32_t gen = next_gate_gen();
            KParams pb = p;
            pb.gate = band_gate_words(p, params->rgba_dtype), pb.gate_gen = gen, pb.gate_sense = 0u;
            const hipError_t e = launch_band(pb, params->rgba_dtype, 0, st);
            if (e != hipSuccess) return hip_rc(e);
            pb.gate_sense = 1u;
            return hip_rc(launch_lds(pb, params->rgba_dtype, 0, st));
        }
    }
    if (variant == GMPI_VARIANT_GATHER) {
        if (p.N > 65535) return GMPI_E_SHAPE;  // the gather kernel puts the view index in grid.z
        return hip_rc(launch_gather(p, params->rgba_dtype, st));
    }
    int tune = 0;
#ifdef GMPI_TUNE  // profiling builds only (make EXTRA=-DGMPI_TUNE): experiment knobs from the environment
    static const int env_tune = [] { const char* e = getenv("GMPI_TUNE_WAVE"); return e ? atoi(e) : 0; }();
    tune = env_tune;
#endif
    if (variant == GMPI_VARIANT_WAVE) {
        if (!wave_variant_supports(p, params->rgba_dtype)) return GMPI_E_VARIANT;
        return hip_rc(launch_wave(p, params->rgba_dtype, tune, st));
    }
    if (variant == GMPI_VARIANT_LDS) {
        if (!lds_variant_supports(p, params->rgba_dtype)) return GMPI_E_VARIANT;
        return hip_rc(launch_lds(p, params->rgba_dtype, tune, st));
    }
    if (variant == GMPI_VARIANT_BAND) {
        if (!band_variant_supports(p, params->rgba_dtype)) return GMPI_E_VARIANT;
        return hip_rc(launch_band(p, params->rgba_dtype, tune, st));
    }
    // (GMPI_VARIANT_DMA -- round 3's LDS-DMA loader inside the 32 x 16 tile decomposition, the A/B that separated the loader from the
    //  decomposition -- was retired in round 4: the band kernel is that loader's home.  The value stays reserved and is refused.)
    return GMPI_E_VARIANT;
}

int gmpi_render_layers_supports(const GmpiRenderParams* params) {
    if (params == nullptr) return GMPI_E_NULL;
    if (params->struct_size != sizeof(GmpiRenderParams)) return GMPI_E_ABI;
    const int rs = layers_strides_ok(params);
    if (rs != GMPI_OK) return rs;
    KParams p;
    if (params->rgba_dtype == GMPI_DTYPE_U8) {   // the existing uint8 path's rule
        const int rc = to_kparams(params, p, true, false, true);
        return rc != GMPI_OK ? rc : (u8_variant_supports(p) ? 1 : 0);
    }
    const int rc = to_kparams_layers(params, p);
    return rc != GMPI_OK ? rc : (layers_variant_supports(p, params->rgba_dtype) ? 1 : 0);
}

int gmpi_mpi_render_layers_launch(const GmpiRenderParams* params, void* stream) {
    if (params == nullptr) return GMPI_E_NULL;
    if (params->struct_size != sizeof(GmpiRenderParams)) return GMPI_E_ABI;
    if (params->N == 0) return GMPI_OK;  // no views
    const int rs = layers_strides_ok(params);
    if (rs != GMPI_OK) return rs;
    if (params->rgba_dtype == GMPI_DTYPE_U8) return gmpi_mpi_render_launch(params, stream);   // channels-last codes: the kernels that exist, the same bits
    KParams p;
    const int rc = to_kparams_layers(params, p);
    if (rc != GMPI_OK) return rc;
    int variant = params->variant;
    if (variant != GMPI_VARIANT_AUTO && variant != GMPI_VARIANT_GATHER && variant != GMPI_VARIANT_LDS) return GMPI_E_VARIANT;   // WAVE, BAND, DMA: not built for the layout
    // AUTO is the staged kernel wherever it can take the tensors: no threshold, the camera hints change nothing, no workspace
    const bool staged = layers_variant_supports(p, params->rgba_dtype);
    if (variant == GMPI_VARIANT_AUTO) variant = staged ? GMPI_VARIANT_LDS : GMPI_VARIANT_GATHER;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (variant == GMPI_VARIANT_GATHER) {
        if (p.N > 65535) return GMPI_E_SHAPE;  // the gather kernel puts the view index in grid.z
        return hip_rc(launch_gather_layers(p, params->rgba_dtype, st));
    }
    if (!staged) return GMPI_E_VARIANT;   // LDS by name over tensors its 16-byte items cannot take
    return hip_rc(launch_layers(p, params->rgba_dtype, st));
}

int gmpi_render_layers_backward_supports(const GmpiRenderParams* params, const int64_t* grad_layers_stride) {
    KParams p;
    const int rc = layers_backward_args(params, grad_layers_stride, p);
    return rc != GMPI_OK ? rc : (backward_layers_tile_supports(p, params->rgba_dtype, grad_layers_stride) ? 1 : 0);
}

int gmpi_mpi_render_layers_backward_launch(const GmpiRenderParams* params, const float* grad_rgb, const float* grad_depth, const float* grad_transmittance,
                                           float* grad_layers, const int64_t* grad_layers_stride, void* stream) {
    if (params != nullptr && params->struct_size == sizeof(GmpiRenderParams) && params->N == 0) return GMPI_OK;  // no views
    KParams p;
    const int rc = layers_backward_args(params, grad_layers_stride, p);
    if (rc != GMPI_OK) return rc;
    if (grad_rgb == nullptr || grad_layers == nullptr) return GMPI_E_NULL;
    // GATHER: the one-pixel kernel; anything else: the 64 x 8 tile kernel where its guards allow (launch_backward_layers), else the one-pixel kernel
    return hip_rc(launch_backward_layers(p, params->rgba_dtype, grad_rgb, grad_depth, grad_transmittance, grad_layers, grad_layers_stride,
                                         params->variant != GMPI_VARIANT_GATHER, static_cast<hipStream_t>(stream)));
}

uint64_t gmpi_render_workspace_bytes(const GmpiRenderParams* params) {
    KParams p;
    if (to_kparams(params, p, true, false, true) != GMPI_OK || p.N == 0) return 0;
    if (params->rgba_dtype == GMPI_DTYPE_U8) return 0;  // neither of its kernels wants scratch
    if (params->variant == GMPI_VARIANT_BAND) return band_workspace_bytes(p, params->rgba_dtype);
    if (params->variant == GMPI_VARIANT_AUTO && auto_takes_band(p, params->rgba_dtype)) return band_workspace_bytes(p, params->rgba_dtype);
    return 0;
}

uint64_t gmpi_render_backward_workspace_bytes(const GmpiRenderParams* params) {
    KParams p;
    if (to_kparams(params, p, false, true) != GMPI_OK || p.N == 0) return 0;
    if (params->variant == GMPI_VARIANT_GATHER) return 0;   // the all-atomic cross-check kernel
    return backward_gather_workspace_bytes(p, params->rgba_dtype);
}

int gmpi_mpi_render_backward_launch(const GmpiRenderParams* params, const float* grad_rgb, const float* grad_depth,
                                    float* grad_rgba, const int64_t* grad_rgba_stride, void* stream) {
    return gmpi_mpi_render_backward_ex_launch(params, grad_rgb, grad_depth, nullptr, grad_rgba, grad_rgba_stride, stream);
}

int gmpi_mpi_render_backward_ex_launch(const GmpiRenderParams* params, const float* grad_rgb, const float* grad_depth,
                                       const float* grad_transmittance, float* grad_rgba, const int64_t* grad_rgba_stride, void* stream) {
    if (params != nullptr && params->struct_size == sizeof(GmpiRenderParams) && params->N == 0) return GMPI_OK;
    KParams p;
    const int rc = to_kparams(params, p, false, true);
    if (rc != GMPI_OK) return rc;
    if (grad_rgb == nullptr || grad_rgba == nullptr || grad_rgba_stride == nullptr) return GMPI_E_NULL;
    if (p.N > 65535) return GMPI_E_SHAPE;  // both backward kernels put the view index in grid.y / grid.z: split the batch
    if (grad_rgba_stride[4] != 1) return GMPI_E_STRIDE;
    for (int i = 0; i < 4; ++i)
        if (grad_rgba_stride[i] <= 0 && !(i == 0 && params->M == 1)) return GMPI_E_STRIDE;
    return hip_rc(launch_backward(p, params->rgba_dtype, grad_rgb, grad_depth, grad_transmittance, grad_rgba, grad_rgba_stride,
                                  params->variant != GMPI_VARIANT_GATHER, static_cast<hipStream_t>(stream)));
}

// ---- the plane-chunked render: one chunk of the stack per launch, the per-pixel state (forward: Accum; backward: T and S) handed from launch to launch ----
int gmpi_mpi_render_chunk_launch(const GmpiRenderParams* params, const GmpiCarry* carry, void* stream) {
    if (params != nullptr && params->struct_size == sizeof(GmpiRenderParams) && params->N == 0) return GMPI_OK;  // no views
    KParams p;
    const int rc = to_kparams(params, p, false, true, true);
    if (rc != GMPI_OK) return rc;
    if (carry == nullptr) return GMPI_E_NULL;
    if (carry->struct_size != sizeof(GmpiCarry)) return GMPI_E_ABI;
    int variant = params->variant;
    if (variant == GMPI_VARIANT_WAVE || variant == GMPI_VARIANT_BAND) return GMPI_E_VARIANT;   // (the strip kernel splits the plane axis itself; the band kernel: gmpi_mpi_render_chunk_band_launch)
    if (variant != GMPI_VARIANT_AUTO && variant != GMPI_VARIANT_GATHER && variant != GMPI_VARIANT_LDS) return GMPI_E_VARIANT;
    if (carry->state_out == nullptr && p.rgb_out == nullptr && p.depth_out == nullptr && p.T_out == nullptr) return GMPI_E_NULL;   // nothing to write
    const CarryK ck{carry->state_in, carry->state_out};
    p.ws = nullptr, p.ws_bytes = 0;   // no kernel of this entry wants scratch
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool u8 = params->rgba_dtype == GMPI_DTYPE_U8;
    const bool staged = u8 ? u8_variant_supports(p) : lds_variant_supports(p, params->rgba_dtype);
    if (variant == GMPI_VARIANT_AUTO) variant = staged ? GMPI_VARIANT_LDS : GMPI_VARIANT_GATHER;
    if (variant == GMPI_VARIANT_GATHER) {
        if (p.N > 65535) return GMPI_E_SHAPE;  // the gather kernel puts the view index in grid.z
        return hip_rc(launch_gather_chunk(p, ck, params->rgba_dtype, st));
    }
    if (!staged) return GMPI_E_VARIANT;   // LDS: these tensors are not aligned for its loader
    return hip_rc(u8 ? launch_u8_chunk(p, ck, st) : launch_lds_chunk(p, ck, params->rgba_dtype, st));
}

// ---- ... through the band kernel's carry instances.  What the three entries ask alike once the struct is read: the variant (BAND, or AUTO = BAND and the tile
// kernel's carry instances behind the view gate), a float storage type, tensors the band kernel -- for AUTO the tile kernel too -- can take.  The workspace is the
// launch's own question.
static bool chunk_band_takes(const KParams& p, const GmpiRenderParams* params) {
    if (params->variant != GMPI_VARIANT_BAND && params->variant != GMPI_VARIANT_AUTO) return false;
    if (params->rgba_dtype == GMPI_DTYPE_U8) return false;   // (the band kernel is not built for the type)
    if (!band_takes_tensors(p, params->rgba_dtype)) return false;
    return params->variant == GMPI_VARIANT_BAND || lds_variant_supports(p, params->rgba_dtype);
}

int gmpi_render_chunk_band_supports(const GmpiRenderParams* params) {
    KParams p;
    const int rc = to_kparams(params, p, false, true, true);
    return rc != GMPI_OK ? rc : (chunk_band_takes(p, params) ? 1 : 0);
}

uint64_t gmpi_render_chunk_band_workspace_bytes(const GmpiRenderParams* params) {
    KParams p;
    if (to_kparams(params, p, false, true, true) != GMPI_OK || p.N == 0 || !chunk_band_takes(p, params)) return 0;
    return band_workspace_bytes(p, params->rgba_dtype);   // the table of the chunk's own D planes
}

int gmpi_mpi_render_chunk_band_launch(const GmpiRenderParams* params, const GmpiCarry* carry, void* stream) {
    if (params != nullptr && params->struct_size == sizeof(GmpiRenderParams) && params->N == 0) return GMPI_OK;  // no views
    KParams p;
    const int rc = to_kparams(params, p, false, true, true);
    if (rc != GMPI_OK) return rc;
    if (carry == nullptr) return GMPI_E_NULL;
    if (carry->struct_size != sizeof(GmpiCarry)) return GMPI_E_ABI;
    if (params->variant != GMPI_VARIANT_BAND && params->variant != GMPI_VARIANT_AUTO) return GMPI_E_VARIANT;
    if (carry->state_out == nullptr && p.rgb_out == nullptr && p.depth_out == nullptr && p.T_out == nullptr) return GMPI_E_NULL;   // nothing to write
    if (!chunk_band_takes(p, params)) return GMPI_E_VARIANT;
    if (!band_workspace_ok(p, params->rgba_dtype)) return GMPI_E_WORKSPACE;
    const CarryK ck{carry->state_in, carry->state_out};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (params->variant == GMPI_VARIANT_BAND) return hip_rc(launch_band_chunk(p, ck, params->rgba_dtype, st));   // bands whose boxes do not fit: the in-kernel direct gather
    // AUTO: the pair of gmpi_mpi_render_launch's band path -- the table kernel stamps the gate word of every view with a box that does not fit, the band carry kernel
    // renders the others, the tile kernel's carry instances render the stamped ones: every view's state passes through exactly one of the two.  No size threshold and
    // no camera hints: the caller opted in.
    KParams pb = p;
    pb.gate = band_gate_words(p, params->rgba_dtype), pb.gate_gen = next_gate_gen(), pb.gate_sense = 0u;
    const hipError_t e = launch_band_chunk(pb, ck, params->rgba_dtype, st);
    if (e != hipSuccess) return hip_rc(e);
    pb.gate_sense = 1u;
    return hip_rc(launch_lds_chunk(pb, ck, params->rgba_dtype, st));
}

// ---- sparse 8-bit volumes (render_u8.hip): the occupancy map of a volume, and the staged uint8 kernel's instances that skip the boxes it says are empty.
// The map entries read the volume description alone: the strides by the rules of to_kparams, nothing of the views.  On GMPI_OK: the alpha channel's byte
// offset inside a plane and the bytes from one texel of a row to the next.
static int occupancy_volume(const GmpiRenderParams* q, int64_t& a_off, int& xs) {
    if (q == nullptr) return GMPI_E_NULL;
    if (q->struct_size != sizeof(GmpiRenderParams)) return GMPI_E_ABI;
    if (q->M <= 0 || q->D <= 0 || q->Ht <= 0 || q->Wt <= 0) return GMPI_E_SHAPE;
    if (q->rgba == nullptr) return GMPI_E_NULL;
    if (q->rgba_dtype != GMPI_DTYPE_U8) return GMPI_E_DTYPE;
    const bool interleaved = q->rgba_stride[4] == 4 && q->rgba_stride[2] == 1;
    if (q->rgba_stride[4] != 1 && !interleaved) return GMPI_E_STRIDE;
    for (int i = 0; i < 4; ++i)
        if (q->rgba_stride[i] < 0) return GMPI_E_STRIDE;
    if (q->rgba_stride[3] < (interleaved ? 4 : 1) * static_cast<int64_t>(q->Wt) || q->rgba_stride[2] == 0 || q->rgba_stride[1] == 0) return GMPI_E_STRIDE;
    a_off = 3 * q->rgba_stride[2], xs = interleaved ? 4 : 1;
    return GMPI_OK;
}

uint64_t gmpi_u8_occupancy_bytes(const GmpiRenderParams* params) {
    int64_t a_off;
    int xs;
    return occupancy_volume(params, a_off, xs) == GMPI_OK ? u8_occupancy_bytes(params->M, params->D, params->Ht, params->Wt) : 0;
}

int gmpi_u8_occupancy_launch(const GmpiRenderParams* params, uint8_t* map, void* stream) {
    int64_t a_off;
    int xs;
    const int rc = occupancy_volume(params, a_off, xs);
    if (rc != GMPI_OK) return rc;
    if (map == nullptr) return GMPI_E_NULL;
    return hip_rc(launch_u8_occupancy(params->rgba, params->rgba_stride[0], params->rgba_stride[1], params->rgba_stride[3], a_off, xs, params->M, params->D,
                                      params->Ht, params->Wt, map, static_cast<hipStream_t>(stream)));
}

// What the sparse launch and its query check alike, in this order: the struct, the type, the map, its block size, then the variant and the tensors.
static int u8_sparse_args(const GmpiRenderParams* params, const GmpiOccupancy* occ, KParams& p) {
    const int rc = to_kparams(params, p, true, false, true);
    if (rc != GMPI_OK) return rc;
    if (params->rgba_dtype != GMPI_DTYPE_U8) return GMPI_E_DTYPE;
    if (occ == nullptr || occ->map == nullptr) return GMPI_E_NULL;
    if (occ->block != u8_variant_query(53)) return GMPI_E_SHAPE;
    if (params->variant != GMPI_VARIANT_AUTO && params->variant != GMPI_VARIANT_LDS) return GMPI_E_VARIANT;
    return u8_variant_supports(p) ? GMPI_OK : GMPI_E_VARIANT;
}

int gmpi_render_u8_sparse_supports(const GmpiRenderParams* params, const GmpiOccupancy* occ) {
    KParams p;
    const int rc = u8_sparse_args(params, occ, p);
    return rc == GMPI_OK ? 1 : rc == GMPI_E_VARIANT ? 0 : rc;
}

int gmpi_mpi_render_u8_sparse_launch(const GmpiRenderParams* params, const GmpiOccupancy* occ, void* stream) {
    if (params != nullptr && params->struct_size == sizeof(GmpiRenderParams) && params->N == 0) return GMPI_OK;  // no views
    KParams p;
    const int rc = u8_sparse_args(params, occ, p);
    if (rc != GMPI_OK) return rc;
    return hip_rc(launch_u8_sparse(p, occ->map, occ->stats, static_cast<hipStream_t>(stream)));
}

int gmpi_mpi_render_chunk_backward_launch(const GmpiRenderParams* params, const float* grad_rgb, const float* grad_depth, const float* grad_transmittance,
                                          const float* T_in, const float* S_in, float* S_out, float* grad_rgba, const int64_t* grad_rgba_stride, void* stream) {
    if (params != nullptr && params->struct_size == sizeof(GmpiRenderParams) && params->N == 0) return GMPI_OK;
    KParams p;
    const int rc = to_kparams(params, p, false, true);   // (GMPI_DTYPE_U8: GMPI_E_DTYPE)
    if (rc != GMPI_OK) return rc;
    if (grad_rgb == nullptr || grad_rgba == nullptr || grad_rgba_stride == nullptr) return GMPI_E_NULL;
    if (p.N > 65535) return GMPI_E_SHAPE;  // both backward kernels put the view index in grid.y / grid.z: split the batch
    if (grad_rgba_stride[4] != 1) return GMPI_E_STRIDE;
    for (int i = 0; i < 4; ++i)
        if (grad_rgba_stride[i] <= 0 && !(i == 0 && params->M == 1)) return GMPI_E_STRIDE;
    return hip_rc(launch_backward_chunk(p, params->rgba_dtype, grad_rgb, grad_depth, grad_transmittance, T_in, S_in, S_out, grad_rgba, grad_rgba_stride,
                                        params->variant != GMPI_VARIANT_GATHER, static_cast<hipStream_t>(stream)));
}

uint64_t gmpi_render_geometry_backward_workspace_bytes(const GmpiRenderParams* params, int want_dhw) {
    KParams p;
    if (to_kparams(params, p, false, true) != GMPI_OK || p.N == 0) return 0;
    return geometry_backward_workspace_bytes(p, want_dhw != 0);
}

int gmpi_mpi_render_geometry_backward_launch(const GmpiRenderParams* params, const float* grad_rgb, const float* grad_depth, float* grad_ray_dir,
                                             float* grad_eye_pos, float* grad_z_dir, float* grad_dhw, void* stream) {
    return gmpi_mpi_render_geometry_backward_ex_launch(params, grad_rgb, grad_depth, nullptr, grad_ray_dir, grad_eye_pos, grad_z_dir, grad_dhw,
                                                       stream);
}

// What the geometry backward entries check once their structs are read: GMPI_OK with *launch = false when there is nothing to do.  grad_plane_z: the
// depth-alpha layout's _pz entry alone.
static int geometry_backward_args(const KParams& p, const float* grad_rgb, float* grad_ray_dir, float* grad_eye_pos, float* grad_z_dir, float* grad_dhw,
                                  bool* launch, float* grad_plane_z = nullptr) {
    *launch = false;
    if (grad_rgb == nullptr) return GMPI_E_NULL;
    if (p.N > 65535 || p.M > 65535 || 6 + 3 * static_cast<int64_t>(p.D) > (int64_t(1) << 31) - 1) return GMPI_E_SHAPE;   // grid.y: views / MPIs, grid.x: components
    if (grad_ray_dir == nullptr && grad_eye_pos == nullptr && grad_z_dir == nullptr && grad_dhw == nullptr && grad_plane_z == nullptr) return GMPI_OK;
    if (grad_eye_pos != nullptr || grad_z_dir != nullptr || grad_dhw != nullptr || grad_plane_z != nullptr) {   // the slabs of the per-view / per-plane sums
        const uint64_t need = geometry_backward_workspace_bytes(p, grad_dhw != nullptr, grad_plane_z != nullptr);
        if (p.ws == nullptr || p.ws_bytes < need || reinterpret_cast<uintptr_t>(p.ws) % 256 != 0) return GMPI_E_WORKSPACE;
    }
    *launch = true;
    return GMPI_OK;
}

int gmpi_mpi_render_geometry_backward_ex_launch(const GmpiRenderParams* params, const float* grad_rgb, const float* grad_depth,
                                                const float* grad_transmittance, float* grad_ray_dir, float* grad_eye_pos, float* grad_z_dir,
                                                float* grad_dhw, void* stream) {
    if (params != nullptr && params->struct_size == sizeof(GmpiRenderParams) && params->N == 0) return GMPI_OK;
    KParams p;
    int rc = to_kparams(params, p, false, true);
    if (rc != GMPI_OK) return rc;
    bool launch;
    rc = geometry_backward_args(p, grad_rgb, grad_ray_dir, grad_eye_pos, grad_z_dir, grad_dhw, &launch);
    if (!launch) return rc;
    return hip_rc(launch_backward_geometry(p, params->rgba_dtype, grad_rgb, grad_depth, grad_transmittance, grad_ray_dir, grad_eye_pos, grad_z_dir, grad_dhw,
                                           static_cast<hipStream_t>(stream)));
}

// ---- the geometry backward over the volume as STORED, read in place: 8-bit codes (planar, or channels-last: told by the strides, as the forward tells
// them) and channels-last float layers.  Entries of their own: the two above keep refusing GMPI_DTYPE_U8 and the layers' strides.  The argument checks
// after the struct are geometry_backward_args'; the workspace is the volume entry's size (N, H, W, D only), asked for through the query below.
int gmpi_mpi_render_u8_geometry_backward_launch(const GmpiRenderParams* params, const float* grad_rgb, const float* grad_depth, const float* grad_transmittance,
                                                float* grad_ray_dir, float* grad_eye_pos, float* grad_z_dir, float* grad_dhw, void* stream) {
    if (params == nullptr) return GMPI_E_NULL;
    if (params->struct_size != sizeof(GmpiRenderParams)) return GMPI_E_ABI;
    if (params->N == 0) return GMPI_OK;  // no views
    if (params->rgba_dtype != GMPI_DTYPE_U8) return GMPI_E_DTYPE;   // (the float types: gmpi_mpi_render_geometry_backward_ex_launch)
    KParams p;
    int rc = to_kparams(params, p, false, true, true);
    if (rc != GMPI_OK) return rc;
    bool launch;
    rc = geometry_backward_args(p, grad_rgb, grad_ray_dir, grad_eye_pos, grad_z_dir, grad_dhw, &launch);
    if (!launch) return rc;
    // The sweep divides the transmittance it starts from by ITS alpha samples (per tap c / 255, then the fma chain).  Without GMPI_FLAG_STRICT_ORDER the
    // staged 8-bit forward (render_u8.hip) samples the CODES and scales the sum by RN(1 / 255): where all four taps are 255 -- exactly opaque texels, the
    // common case of a stored MPI -- its om = (1 - a) + 1e-10 and the sweep's differ in the last bits of a, i.e. by orders of magnitude in om (1e-10
    // against 6e-8), and so would every T in front of that plane.  Where that kernel may have written transmittance_out (the forward's own routing: not
    // GATHER, tensors it can stage; some of its planes fall back to per-tap sampling, which cannot be told from here) the value is NOT used: every pixel
    // walks the alpha texels with the sweep's arithmetic, as it does where the forward's value has underflowed.  The strict-order forwards and the gather
    // kernel sample per tap: their value is the sweep's own product and is used.
    if ((p.flags & GMPI_FLAG_STRICT_ORDER) == 0 && params->variant != GMPI_VARIANT_GATHER && u8_variant_supports(p)) p.T_out = nullptr;
    return hip_rc(launch_backward_geometry_inplace(p, GMPI_DTYPE_U8, false, grad_rgb, grad_depth, grad_transmittance, grad_ray_dir, grad_eye_pos, grad_z_dir,
                                                   grad_dhw, static_cast<hipStream_t>(stream)));
}

int gmpi_mpi_render_layers_geometry_backward_launch(const GmpiRenderParams* params, const float* grad_rgb, const float* grad_depth,
                                                    const float* grad_transmittance, float* grad_ray_dir, float* grad_eye_pos, float* grad_z_dir,
                                                    float* grad_dhw, void* stream) {
    if (params == nullptr) return GMPI_E_NULL;
    if (params->struct_size != sizeof(GmpiRenderParams)) return GMPI_E_ABI;
    if (params->N == 0) return GMPI_OK;  // no views
    const int rs = layers_strides_ok(params);   // (the order of layers_backward_args: the strides, the type, every other field)
    if (rs != GMPI_OK) return rs;
    if (params->rgba_dtype == GMPI_DTYPE_U8) return GMPI_E_DTYPE;   // (codes: gmpi_mpi_render_u8_geometry_backward_launch)
    KParams p;
    int rc = to_kparams_layers(params, p, true);
    if (rc != GMPI_OK) return rc;
    bool launch;
    rc = geometry_backward_args(p, grad_rgb, grad_ray_dir, grad_eye_pos, grad_z_dir, grad_dhw, &launch);
    if (!launch) return rc;
    return hip_rc(launch_backward_geometry_inplace(p, params->rgba_dtype, true, grad_rgb, grad_depth, grad_transmittance, grad_ray_dir, grad_eye_pos, grad_z_dir,
                                                   grad_dhw, static_cast<hipStream_t>(stream)));
}

// gmpi_render_geometry_backward_workspace_bytes for the params of the two entries above (that query answers 0 for GMPI_DTYPE_U8 and for the layers'
// strides, and stays so): the same size -- it depends on N, H, W and D only -- for 8-bit volumes in either order, float layers, and planar float volumes.
uint64_t gmpi_render_geometry_inplace_workspace_bytes(const GmpiRenderParams* params, int want_dhw) {
    if (params == nullptr || params->struct_size != sizeof(GmpiRenderParams)) return 0;
    KParams p;
    int rc;
    if (params->rgba_dtype == GMPI_DTYPE_U8) rc = to_kparams(params, p, false, true, true);
    else if (layers_strides_ok(params) == GMPI_OK) rc = to_kparams_layers(params, p, true);
    else rc = to_kparams(params, p, false, true);
    if (rc != GMPI_OK || p.N == 0) return 0;
    return geometry_backward_workspace_bytes(p, want_dhw != 0);
}

// shared-colour entries: params->rgba = the alpha planes (rgba_stride[2] ignored); checks of to_kparams + the GmpiSharedColor struct.
// forward: the forward launch and its support query, which know GMPI_VARIANT_LDS; the backward knows AUTO and GATHER only.
static int to_shared(const GmpiRenderParams* params, const GmpiSharedColor* shared, bool forward, KParams& p, SharedK& sh) {
    if (params == nullptr || shared == nullptr) return GMPI_E_NULL;
    if (params->struct_size != sizeof(GmpiRenderParams) || shared->struct_size != sizeof(GmpiSharedColor)) return GMPI_E_ABI;
    GmpiRenderParams q = *params;
    q.rgba_stride[2] = 1;   // (ignored: the alpha tensor has one channel)
    const int rc = to_kparams(&q, p, forward, true);   // (the forward needs the output pointers)
    if (rc != GMPI_OK) return rc;
    if (params->variant != GMPI_VARIANT_AUTO && params->variant != GMPI_VARIANT_GATHER && !(forward && params->variant == GMPI_VARIANT_LDS)) return GMPI_E_VARIANT;
    if (shared->rgb == nullptr) return GMPI_E_NULL;
    for (int i = 0; i < 3; ++i)
        if (shared->rgb_stride[i] < 0 || (shared->background != nullptr && shared->background_stride[i] < 0)) return GMPI_E_STRIDE;
    if (shared->rgb_stride[2] < q.Wt || shared->rgb_stride[1] == 0) return GMPI_E_STRIDE;
    if (shared->background != nullptr && (shared->background_stride[2] < q.Wt || shared->background_stride[1] == 0)) return GMPI_E_STRIDE;
    p.s_chan = 0;   // (render_shared.hip: the 4-channel helpers read the alpha plane four times)
    sh.rgb = shared->rgb, sh.bg = shared->background;
    sh.rs_mpi = shared->rgb_stride[0], sh.rs_chan = shared->rgb_stride[1], sh.rs_row = shared->rgb_stride[2];
    sh.bs_mpi = sh.bg ? shared->background_stride[0] : 0, sh.bs_chan = sh.bg ? shared->background_stride[1] : 0, sh.bs_row = sh.bg ? shared->background_stride[2] : 0;
    return GMPI_OK;
}

int gmpi_mpi_render_shared_launch(const GmpiRenderParams* params, const GmpiSharedColor* shared, void* stream) {
    KParams p;
    SharedK sh;
    const int rc = to_shared(params, shared, true, p, sh);
    if (rc != GMPI_OK) return rc;
    if (p.N == 0) return GMPI_OK;
    if (params->variant == GMPI_VARIANT_LDS) {   // the staged kernel, only on request: AUTO and GATHER keep the one-pixel-per-lane kernel
        if (!shared_forward_supports(p, params->rgba_dtype, sh)) return GMPI_E_VARIANT;
        return hip_rc(launch_shared_forward(p, params->rgba_dtype, sh, static_cast<hipStream_t>(stream)));
    }
    if (p.N > 65535) return GMPI_E_SHAPE;   // the view index is grid.z
    return hip_rc(launch_shared(p, params->rgba_dtype, sh, static_cast<hipStream_t>(stream)));
}

int gmpi_render_shared_supports(const GmpiRenderParams* params, const GmpiSharedColor* shared) {
    KParams p;
    SharedK sh;
    const int rc = to_shared(params, shared, true, p, sh);
    if (rc != GMPI_OK) return rc;
    if (params->variant == GMPI_VARIANT_LDS) return shared_forward_supports(p, params->rgba_dtype, sh) ? 1 : 0;
    return p.N > 65535 ? GMPI_E_SHAPE : 1;
}

// The gradient arguments of the shared-colour and depth-alpha backward entries (grad_mid: the alpha planes, resp. the depth image) -> g.  A launch
// without views (p.N == 0) is GMPI_OK before any stride is looked at.
static int to_shared_grads(const GmpiRenderParams* params, const KParams& p, const SharedK& sh, const float* grad_rgb_out, const float* grad_depth,
                           const float* grad_transmittance, float* grad_shared_rgb, const int64_t* grad_shared_rgb_stride, float* grad_mid,
                           const int64_t* grad_mid_stride, float* grad_background, const int64_t* grad_background_stride, SharedG& g) {
    if (grad_rgb_out == nullptr) return GMPI_E_NULL;
    if (grad_shared_rgb == nullptr && grad_mid == nullptr && grad_background == nullptr) return GMPI_E_NULL;
    if (grad_background != nullptr && sh.bg == nullptr) return GMPI_E_NULL;
    if ((grad_shared_rgb != nullptr && grad_shared_rgb_stride == nullptr) || (grad_mid != nullptr && grad_mid_stride == nullptr) ||
        (grad_background != nullptr && grad_background_stride == nullptr))
        return GMPI_E_NULL;
    if (p.N == 0) return GMPI_OK;
    if (p.N > 65535) return GMPI_E_SHAPE;
    g.g_out = grad_rgb_out, g.g_depth = grad_depth, g.g_T = grad_transmittance;
    g.g_rgb = grad_shared_rgb, g.g_alpha = grad_mid, g.g_bg = grad_background;
    auto ok3 = [&](const int64_t* s, int64_t rows_of) {   // MPI stride may be 0 only for one MPI; rows must not overlap
        return (s[0] > 0 || params->M == 1) && s[0] >= 0 && s[1] > 0 && s[2] >= rows_of;
    };
    if (g.g_rgb) {
        if (!ok3(grad_shared_rgb_stride, p.Wt)) return GMPI_E_STRIDE;
        g.gr_mpi = grad_shared_rgb_stride[0], g.gr_chan = grad_shared_rgb_stride[1], g.gr_row = grad_shared_rgb_stride[2];
    }
    if (g.g_alpha) {
        if (!ok3(grad_mid_stride, p.Wt)) return GMPI_E_STRIDE;
        g.ga_mpi = grad_mid_stride[0], g.ga_plane = grad_mid_stride[1], g.ga_row = grad_mid_stride[2];
    }
    if (g.g_bg) {
        if (!ok3(grad_background_stride, p.Wt)) return GMPI_E_STRIDE;
        g.gb_mpi = grad_background_stride[0], g.gb_chan = grad_background_stride[1], g.gb_row = grad_background_stride[2];
    }
    return GMPI_OK;
}

int gmpi_mpi_render_shared_backward_launch(const GmpiRenderParams* params, const GmpiSharedColor* shared, const float* grad_rgb_out, const float* grad_depth,
                                           const float* grad_transmittance, float* grad_shared_rgb, const int64_t* grad_shared_rgb_stride, float* grad_alpha,
                                           const int64_t* grad_alpha_stride, float* grad_background, const int64_t* grad_background_stride, void* stream) {
    KParams p;
    SharedK sh;
    int rc = to_shared(params, shared, false, p, sh);
    if (rc != GMPI_OK) return rc;
    SharedG g{};
    rc = to_shared_grads(params, p, sh, grad_rgb_out, grad_depth, grad_transmittance, grad_shared_rgb, grad_shared_rgb_stride, grad_alpha, grad_alpha_stride,
                         grad_background, grad_background_stride, g);
    if (rc != GMPI_OK || p.N == 0) return rc;
    return hip_rc(launch_shared_backward(p, params->rgba_dtype, sh, g, params->variant != GMPI_VARIANT_GATHER, static_cast<hipStream_t>(stream)));
}

// ---- the shaded render of an RGBA volume: the checks of the volume entries (to_kparams; GMPI_DTYPE_U8 refused) + the GmpiShading struct --------------
static int to_shaded(const GmpiRenderParams* params, const GmpiShading* shading, bool forward, KParams& p, ShadeK& sh) {
    if (params == nullptr || shading == nullptr) return GMPI_E_NULL;
    if (params->struct_size != sizeof(GmpiRenderParams) || shading->struct_size != sizeof(GmpiShading)) return GMPI_E_ABI;
    p.N = 0;
    if (params->N == 0) return GMPI_OK;   // no views: the callers return at once
    const int rc = to_kparams(params, p, forward, true);
    if (rc != GMPI_OK) return rc;
    if (shading->shading == nullptr) return GMPI_E_NULL;
    if (shading->shading_stride[1] < p.Wt || shading->shading_stride[0] < 0 || (shading->shading_stride[0] == 0 && p.M != 1)) return GMPI_E_STRIDE;
    sh.s = shading->shading, sh.s_mpi = shading->shading_stride[0], sh.s_row = shading->shading_stride[1];
    p.ws = nullptr, p.ws_bytes = 0;   // no kernel of these entries wants scratch
    return GMPI_OK;
}

int gmpi_mpi_render_shaded_launch(const GmpiRenderParams* params, const GmpiShading* shading, void* stream) {
    KParams p;
    ShadeK sh;
    const int rc = to_shaded(params, shading, true, p, sh);
    if (rc != GMPI_OK) return rc;
    if (p.N == 0) return GMPI_OK;
    int variant = params->variant;
    if (variant != GMPI_VARIANT_AUTO && variant != GMPI_VARIANT_GATHER && variant != GMPI_VARIANT_LDS) return GMPI_E_VARIANT;
    const bool staged = shaded_forward_supports(p, params->rgba_dtype, sh);
    if (variant == GMPI_VARIANT_AUTO) variant = staged ? GMPI_VARIANT_LDS : GMPI_VARIANT_GATHER;
    if (variant == GMPI_VARIANT_LDS) {
        if (!staged) return GMPI_E_VARIANT;   // these tensors are not aligned for its loader
        return hip_rc(launch_shaded_forward(p, params->rgba_dtype, sh, static_cast<hipStream_t>(stream)));
    }
    if (p.N > 65535) return GMPI_E_SHAPE;  // the one-pixel kernel puts the view index in grid.z
    return hip_rc(launch_shaded(p, params->rgba_dtype, sh, static_cast<hipStream_t>(stream)));
}

int gmpi_render_shaded_supports(const GmpiRenderParams* params, const GmpiShading* shading) {
    KParams p;
    ShadeK sh;
    const int rc = to_shaded(params, shading, true, p, sh);
    if (rc != GMPI_OK) return rc;
    if (p.N == 0) return 0;
    return shaded_forward_supports(p, params->rgba_dtype, sh) ? 1 : 0;
}

int gmpi_mpi_render_shaded_backward_launch(const GmpiRenderParams* params, const GmpiShading* shading, const float* grad_rgb, const float* grad_depth,
                                           const float* grad_transmittance, float* grad_rgba, const int64_t* grad_rgba_stride, float* grad_shading,
                                           const int64_t* grad_shading_stride, void* stream) {
    KParams p;
    ShadeK sh;
    const int rc = to_shaded(params, shading, false, p, sh);
    if (rc != GMPI_OK) return rc;
    if (p.N == 0) return GMPI_OK;
    if (grad_rgb == nullptr || (grad_rgba == nullptr && grad_shading == nullptr)) return GMPI_E_NULL;   // either gradient may be NULL when the other is not
    if ((grad_rgba != nullptr && grad_rgba_stride == nullptr) || (grad_shading != nullptr && grad_shading_stride == nullptr)) return GMPI_E_NULL;
    if (p.N > 65535 || p.M > 65535 || p.Ht > 65535) return GMPI_E_SHAPE;  // the view index is grid.y / grid.z; the chain rule's grid is (columns, Ht, M)
    if (grad_rgba != nullptr) {
        if (grad_rgba_stride[4] != 1 || grad_rgba_stride[3] < p.Wt) return GMPI_E_STRIDE;
        for (int i = 0; i < 4; ++i)
            if (grad_rgba_stride[i] <= 0 && !(i == 0 && params->M == 1)) return GMPI_E_STRIDE;
    }
    if (grad_shading != nullptr && (grad_shading_stride[1] < p.Wt || grad_shading_stride[0] < 0 || (grad_shading_stride[0] == 0 && p.M != 1))) return GMPI_E_STRIDE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (grad_rgba == nullptr) {   // the shading's gradient alone: no volume buffer -- zero-fill, then the one-pixel kernel adds the chain rule's terms per tap
        const hipError_t z = launch_zero_image(grad_shading, grad_shading_stride, p.M, p.Ht, p.Wt, st);
        if (z != hipSuccess) return hip_rc(z);
        return hip_rc(launch_backward_shading_only(p, params->rgba_dtype, sh, grad_rgb, grad_depth, grad_transmittance, grad_shading, grad_shading_stride, st));
    }
    const hipError_t e = launch_backward_shaded(p, params->rgba_dtype, sh, grad_rgb, grad_depth, grad_transmittance, grad_rgba, grad_rgba_stride,
                                                params->variant != GMPI_VARIANT_GATHER, st);
    if (e != hipSuccess) return hip_rc(e);
    return hip_rc(launch_shaded_chain_rule(p, params->rgba_dtype, sh, grad_rgba, grad_rgba_stride, grad_shading, grad_shading_stride, st));
}

// depth-alpha entries: params->rgba = the depth image (rgba_stride[1], [2] ignored); the checks of to_shared (AUTO and GATHER only) + the GmpiDepthAlpha struct.
static int to_depth(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* da, bool forward, KParams& p, SharedK& sh, DepthK& dk) {
    if (params == nullptr || shared == nullptr || da == nullptr) return GMPI_E_NULL;
    if (params->struct_size != sizeof(GmpiRenderParams) || da->struct_size != sizeof(GmpiDepthAlpha)) return GMPI_E_ABI;
    GmpiRenderParams q = *params;
    q.rgba_stride[1] = 1;   // (ignored: the depth image has one plane)
    const int rc = to_shared(&q, shared, forward, p, sh);
    if (rc != GMPI_OK) return rc;
    if (params->variant == GMPI_VARIANT_LDS) return GMPI_E_VARIANT;   // (to_shared lets the shared-colour forward's staged kernel through)
    if (da->plane_z == nullptr) return GMPI_E_NULL;
    if (da->plane_z_stride < 0) return GMPI_E_STRIDE;
    if (!(da->z_lo < da->z_hi) || !(da->z_den > 0.0f)) return GMPI_E_SHAPE;
    p.s_plane = 0;
    dk.plane_z = da->plane_z, dk.pz_stride = da->plane_z_stride;
    dk.lo = da->z_lo, dk.hi = da->z_hi, dk.den = da->z_den, dk.rden = 1.0f / da->z_den;
    return GMPI_OK;
}

int gmpi_mpi_render_depth_launch(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* depth_alpha, void* stream) {
    KParams p;
    SharedK sh;
    DepthK dk;
    const int rc = to_depth(params, shared, depth_alpha, true, p, sh, dk);
    if (rc != GMPI_OK) return rc;
    if (p.N == 0) return GMPI_OK;
    if (p.N > 65535) return GMPI_E_SHAPE;   // the view index is grid.z
    return hip_rc(launch_depth(p, params->rgba_dtype, sh, dk, static_cast<hipStream_t>(stream)));
}

// The window forward (render_depth_window.hip), only through this entry: gmpi_mpi_render_depth_launch keeps its one kernel.  AUTO: the window kernel, where
// its loader can take the tensors; GATHER: the one-pixel-per-lane kernel.
int gmpi_mpi_render_depth_window_launch(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* depth_alpha, void* stream) {
    KParams p;
    SharedK sh;
    DepthK dk;
    const int rc = to_depth(params, shared, depth_alpha, true, p, sh, dk);
    if (rc != GMPI_OK) return rc;
    if (p.N == 0) return GMPI_OK;
    if (params->variant == GMPI_VARIANT_GATHER) {
        if (p.N > 65535) return GMPI_E_SHAPE;   // the view index is grid.z
        return hip_rc(launch_depth(p, params->rgba_dtype, sh, dk, static_cast<hipStream_t>(stream)));
    }
    if (!depth_window_supports(p, params->rgba_dtype, sh)) return GMPI_E_VARIANT;
    return hip_rc(launch_depth_window(p, params->rgba_dtype, sh, dk, static_cast<hipStream_t>(stream)));
}

int gmpi_render_depth_window_supports(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* depth_alpha) {
    KParams p;
    SharedK sh;
    DepthK dk;
    const int rc = to_depth(params, shared, depth_alpha, true, p, sh, dk);
    if (rc != GMPI_OK) return rc;
    if (params->variant == GMPI_VARIANT_GATHER) return p.N > 65535 ? GMPI_E_SHAPE : 1;
    return depth_window_supports(p, params->rgba_dtype, sh) ? 1 : 0;
}

// Both depth-alpha backward entries: one argument check, one marshalling; `tile`: the entry that may launch the tile kernel.
static int depth_backward(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* depth_alpha, const float* grad_rgb_out,
                          const float* grad_depth, const float* grad_transmittance, float* grad_shared_rgb, const int64_t* grad_shared_rgb_stride,
                          float* grad_depth_image, const int64_t* grad_depth_image_stride, float* grad_background, const int64_t* grad_background_stride,
                          void* stream, bool tile) {
    KParams p;
    SharedK sh;
    DepthK dk;
    int rc = to_depth(params, shared, depth_alpha, false, p, sh, dk);
    if (rc != GMPI_OK) return rc;
    int64_t gd_stride[3] = {0, 1, 0};   // (the depth image's channel stride is ignored)
    if (grad_depth_image != nullptr && grad_depth_image_stride != nullptr) gd_stride[0] = grad_depth_image_stride[0], gd_stride[2] = grad_depth_image_stride[2];
    SharedG g{};
    rc = to_shared_grads(params, p, sh, grad_rgb_out, grad_depth, grad_transmittance, grad_shared_rgb, grad_shared_rgb_stride, grad_depth_image,
                         grad_depth_image_stride != nullptr ? gd_stride : nullptr, grad_background, grad_background_stride, g);
    if (rc != GMPI_OK || p.N == 0) return rc;
    // the tile kernel's box table holds 128 planes (gmpi_query(23)): more take the one-pixel-per-lane kernel, and so does GATHER by name
    if (tile && params->variant != GMPI_VARIANT_GATHER && depth_tile_supports(p))
        return hip_rc(launch_depth_backward_tile(p, params->rgba_dtype, sh, dk, g, static_cast<hipStream_t>(stream)));
    return hip_rc(launch_depth_backward(p, params->rgba_dtype, sh, dk, g, static_cast<hipStream_t>(stream)));
}

int gmpi_mpi_render_depth_backward_launch(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* depth_alpha,
                                          const float* grad_rgb_out, const float* grad_depth, const float* grad_transmittance, float* grad_shared_rgb,
                                          const int64_t* grad_shared_rgb_stride, float* grad_depth_image, const int64_t* grad_depth_image_stride,
                                          float* grad_background, const int64_t* grad_background_stride, void* stream) {
    return depth_backward(params, shared, depth_alpha, grad_rgb_out, grad_depth, grad_transmittance, grad_shared_rgb, grad_shared_rgb_stride,
                          grad_depth_image, grad_depth_image_stride, grad_background, grad_background_stride, stream, false);
}

int gmpi_mpi_render_depth_backward_tile_launch(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* depth_alpha,
                                               const float* grad_rgb_out, const float* grad_depth, const float* grad_transmittance, float* grad_shared_rgb,
                                               const int64_t* grad_shared_rgb_stride, float* grad_depth_image, const int64_t* grad_depth_image_stride,
                                               float* grad_background, const int64_t* grad_background_stride, void* stream) {
    return depth_backward(params, shared, depth_alpha, grad_rgb_out, grad_depth, grad_transmittance, grad_shared_rgb, grad_shared_rgb_stride,
                          grad_depth_image, grad_depth_image_stride, grad_background, grad_background_stride, stream, true);
}

// The atomics-free pair over the two layouts (render_backward_gather.hip).  ONE predicate for the query and the launches: the layout's struct checks
// pass, the variant is AUTO and layout_gather_workspace_bytes is not 0 (the caller allocates on the strength of the query).  depth_alpha NULL:
// shared-colour.
static int to_layout(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* depth_alpha, bool depth, KParams& p, SharedK& sh,
                     DepthK& dk) {
    return depth ? to_depth(params, shared, depth_alpha, false, p, sh, dk) : to_shared(params, shared, false, p, sh);
}

uint64_t gmpi_render_layout_backward_gather_workspace_bytes(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* depth_alpha) {
    KParams p;
    SharedK sh;
    DepthK dk;
    if (to_layout(params, shared, depth_alpha, depth_alpha != nullptr, p, sh, dk) != GMPI_OK || p.N == 0) return 0;
    if (params->variant != GMPI_VARIANT_AUTO) return 0;
    return layout_gather_workspace_bytes(p, depth_alpha != nullptr);
}

int gmpi_render_layout_backward_gather_runs(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* depth_alpha) {
    if (gmpi_render_layout_backward_gather_workspace_bytes(params, shared, depth_alpha) == 0) return 0;
    KParams p;
    SharedK sh;
    DepthK dk;
    to_layout(params, shared, depth_alpha, depth_alpha != nullptr, p, sh, dk);
    return layout_gather_runs(p);
}

void gmpi_render_layout_backward_gather_set_runs(int32_t runs) { layout_gather_force_runs(runs); }

static int layout_backward_gather(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* depth_alpha, bool depth,
                                  const float* grad_rgb_out, const float* grad_depth, const float* grad_transmittance, float* grad_shared_rgb,
                                  const int64_t* grad_shared_rgb_stride, float* grad_mid, const int64_t* grad_mid_stride, float* grad_background,
                                  const int64_t* grad_background_stride, void* stream) {
    KParams p;
    SharedK sh;
    DepthK dk;
    int rc = to_layout(params, shared, depth_alpha, depth, p, sh, dk);
    if (rc != GMPI_OK) return rc;
    int64_t gd_stride[3] = {0, 1, 0};   // (depth-alpha: the depth image's channel stride is ignored)
    if (depth && grad_mid != nullptr && grad_mid_stride != nullptr) {
        gd_stride[0] = grad_mid_stride[0], gd_stride[2] = grad_mid_stride[2];
        grad_mid_stride = gd_stride;
    }
    SharedG g{};
    rc = to_shared_grads(params, p, sh, grad_rgb_out, grad_depth, grad_transmittance, grad_shared_rgb, grad_shared_rgb_stride, grad_mid, grad_mid_stride,
                         grad_background, grad_background_stride, g);
    if (rc != GMPI_OK || p.N == 0) return rc;
    if (params->variant != GMPI_VARIANT_AUTO) return GMPI_E_VARIANT;   // the pair has one form; the atomic kernels have entries of their own
    const uint64_t need = layout_gather_workspace_bytes(p, depth);
    if (need == 0) return GMPI_E_VARIANT;                              // a launch the pair does not take: never a quiet fall-back to atomics
    if (p.ws == nullptr || p.ws_bytes < need || reinterpret_cast<uintptr_t>(p.ws) % 256 != 0) return GMPI_E_WORKSPACE;
    return hip_rc(launch_layout_backward_gather(p, params->rgba_dtype, sh, depth ? &dk : nullptr, g, (p.flags & GMPI_FLAG_GRAD_OVERWRITE) != 0,
                                                static_cast<hipStream_t>(stream)));
}

int gmpi_mpi_render_shared_backward_gather_launch(const GmpiRenderParams* params, const GmpiSharedColor* shared, const float* grad_rgb_out,
                                                  const float* grad_depth, const float* grad_transmittance, float* grad_shared_rgb,
                                                  const int64_t* grad_shared_rgb_stride, float* grad_alpha, const int64_t* grad_alpha_stride,
                                                  float* grad_background, const int64_t* grad_background_stride, void* stream) {
    return layout_backward_gather(params, shared, nullptr, false, grad_rgb_out, grad_depth, grad_transmittance, grad_shared_rgb, grad_shared_rgb_stride,
                                  grad_alpha, grad_alpha_stride, grad_background, grad_background_stride, stream);
}

int gmpi_mpi_render_depth_backward_gather_launch(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* depth_alpha,
                                                 const float* grad_rgb_out, const float* grad_depth, const float* grad_transmittance,
                                                 float* grad_shared_rgb, const int64_t* grad_shared_rgb_stride, float* grad_depth_image,
                                                 const int64_t* grad_depth_image_stride, float* grad_background, const int64_t* grad_background_stride,
                                                 void* stream) {
    return layout_backward_gather(params, shared, depth_alpha, true, grad_rgb_out, grad_depth, grad_transmittance, grad_shared_rgb, grad_shared_rgb_stride,
                                  grad_depth_image, grad_depth_image_stride, grad_background, grad_background_stride, stream);
}

// The geometry backward over the two layouts: the layout's own struct checks (to_shared / to_depth, as its image backward), then the volume entry's.
int gmpi_mpi_render_shared_geometry_backward_launch(const GmpiRenderParams* params, const GmpiSharedColor* shared, const float* grad_rgb, const float* grad_depth,
                                                    const float* grad_transmittance, float* grad_ray_dir, float* grad_eye_pos, float* grad_z_dir,
                                                    float* grad_dhw, void* stream) {
    KParams p;
    SharedK sh;
    int rc = to_shared(params, shared, false, p, sh);
    if (rc != GMPI_OK || p.N == 0) return rc;
    bool launch;
    rc = geometry_backward_args(p, grad_rgb, grad_ray_dir, grad_eye_pos, grad_z_dir, grad_dhw, &launch);
    if (!launch) return rc;
    return hip_rc(launch_backward_geometry_layout(p, params->rgba_dtype, sh, nullptr, grad_rgb, grad_depth, grad_transmittance, grad_ray_dir, grad_eye_pos,
                                                  grad_z_dir, grad_dhw, nullptr, static_cast<hipStream_t>(stream)));
}

int gmpi_mpi_render_depth_geometry_backward_launch(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* depth_alpha,
                                                   const float* grad_rgb, const float* grad_depth, const float* grad_transmittance, float* grad_ray_dir,
                                                   float* grad_eye_pos, float* grad_z_dir, float* grad_dhw, void* stream) {
    return gmpi_mpi_render_depth_geometry_backward_pz_launch(params, shared, depth_alpha, grad_rgb, grad_depth, grad_transmittance, grad_ray_dir, grad_eye_pos,
                                                             grad_z_dir, grad_dhw, nullptr, stream);
}

// ... and w.r.t. plane_z (grad_plane_z NULL: the entry above, its kernels and its bits)
int gmpi_mpi_render_depth_geometry_backward_pz_launch(const GmpiRenderParams* params, const GmpiSharedColor* shared, const GmpiDepthAlpha* depth_alpha,
                                                      const float* grad_rgb, const float* grad_depth, const float* grad_transmittance, float* grad_ray_dir,
                                                      float* grad_eye_pos, float* grad_z_dir, float* grad_dhw, float* grad_plane_z, void* stream) {
    KParams p;
    SharedK sh;
    DepthK dk;
    int rc = to_depth(params, shared, depth_alpha, false, p, sh, dk);
    if (rc != GMPI_OK || p.N == 0) return rc;
    bool launch;
    rc = geometry_backward_args(p, grad_rgb, grad_ray_dir, grad_eye_pos, grad_z_dir, grad_dhw, &launch, grad_plane_z);
    if (!launch) return rc;
    return hip_rc(launch_backward_geometry_layout(p, params->rgba_dtype, sh, &dk, grad_rgb, grad_depth, grad_transmittance, grad_ray_dir, grad_eye_pos,
                                                  grad_z_dir, grad_dhw, grad_plane_z, static_cast<hipStream_t>(stream)));
}

uint64_t gmpi_render_depth_geometry_backward_workspace_bytes(const GmpiRenderParams* params, int want_dhw, int want_plane_z) {
    KParams p;
    if (to_kparams(params, p, false, true) != GMPI_OK || p.N == 0) return 0;
    return geometry_backward_workspace_bytes(p, want_dhw != 0, want_plane_z != 0);
}

int gmpi_last_plane_uv_minmax_launch(const GmpiRenderParams* params, float* uv_minmax, void* stream) {
    KParams p;
    const int rc = to_kparams(params, p, false);
    if (rc != GMPI_OK) return rc;
    if (uv_minmax == nullptr) return GMPI_E_NULL;
    if (p.N == 0) return GMPI_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (p.flags & GMPI_FLAG_ALIGN_CORNERS) hipLaunchKernelGGL(last_plane_uv_kernel<true>, dim3(p.N), dim3(256), 0, st, p, uv_minmax);
    else hipLaunchKernelGGL(last_plane_uv_kernel<false>, dim3(p.N), dim3(256), 0, st, p, uv_minmax);
    return hip_rc(hipGetLastError());
}

int gmpi_rgba_range_check_launch(const void* rgba, int32_t rgba_dtype, int64_t count, uint32_t* status, void* stream) {
    if (rgba == nullptr || status == nullptr) return GMPI_E_NULL;
    if (count < 0) return GMPI_E_SHAPE;
    if (rgba_dtype < GMPI_DTYPE_F32 || rgba_dtype > GMPI_DTYPE_F16) return GMPI_E_DTYPE;
    if (count == 0) return GMPI_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int esz = rgba_dtype == GMPI_DTYPE_F32 ? 4 : 2;
    const int per = 16 / esz;
    const bool aligned = (reinterpret_cast<uintptr_t>(rgba) % 16) == 0;
    const int64_t nvec = aligned ? count / per : 0;
    const int64_t tail = count - nvec * per;
    if (nvec > 0) {
        const int blocks = static_cast<int>(std::min<int64_t>((nvec + 255) / 256, 256 * 8));
        const uint4* v = static_cast<const uint4*>(rgba);
        dispatch_dtype(rgba_dtype, [&](auto t) {
            using T = typename decltype(t)::type;
            hipLaunchKernelGGL((range_check_vec_kernel<T, 16 / static_cast<int>(sizeof(T))>), dim3(blocks), dim3(256), 0, st, v, nvec, status);
        });
    }
    if (tail > 0) {
        const char* base = static_cast<const char*>(rgba) + nvec * 16;
        const int blocks = static_cast<int>(std::min<int64_t>((tail + 255) / 256, 256 * 8));
        dispatch_dtype(rgba_dtype, [&](auto t) {
            using T = typename decltype(t)::type;
            hipLaunchKernelGGL(range_check_kernel<T>, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const T*>(base), tail, status);
        });
    }
    return hip_rc(hipGetLastError());
}

int gmpi_frames_to_uint8_launch(const float* rgb_pm1, const float* depth, int32_t N, int32_t H, int32_t W, double depth_near,
                                double depth_far, uint8_t* img8, uint8_t* dep8, void* stream) {
    if (N < 0 || H <= 0 || W <= 0) return GMPI_E_SHAPE;
    if ((img8 && !rgb_pm1) || (dep8 && !depth)) return GMPI_E_NULL;
    if (N == 0 || (!img8 && !dep8)) return GMPI_OK;
    const int64_t HW = static_cast<int64_t>(H) * W, total = HW * N;
    const int64_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(frames_to_uint8_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       rgb_pm1, depth, HW, total, static_cast<float>(depth_near), static_cast<float>(depth_far - depth_near), img8,
                       dep8);
    return hip_rc(hipGetLastError());
}

int gmpi_generate_rays_launch(const float* c2w, const float* unit_dirs, int32_t N, int32_t H, int32_t W, float* ray_dir,
                              float* eye_pos, float* z_dir, void* stream) {
    if (N < 0 || H <= 0 || W <= 0) return GMPI_E_SHAPE;
    if (N == 0) return GMPI_OK;
    if (!c2w || !unit_dirs || !ray_dir || !eye_pos || !z_dir) return GMPI_E_NULL;
    const int64_t HW = static_cast<int64_t>(H) * W;
    const dim3 grid(static_cast<unsigned>((HW + 255) / 256), static_cast<unsigned>(N));
    hipLaunchKernelGGL(generate_rays_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), c2w, unit_dirs, HW, ray_dir,
                       eye_pos, z_dir);
    return hip_rc(hipGetLastError());
}

int gmpi_alpha_depth_launch(const void* alpha, int32_t alpha_dtype, int64_t stride_b, int64_t stride_d, int64_t stride_row,
                            const float* plane_ds, int32_t B, int32_t D, int32_t H, int32_t W, float* depth_out,
                            float* transmittance_out, void* stream) {
    if (B < 0 || D <= 0 || H <= 0 || W <= 0) return GMPI_E_SHAPE;
    if (B == 0) return GMPI_OK;
    if (!alpha || !plane_ds || !depth_out) return GMPI_E_NULL;
    if (alpha_dtype < GMPI_DTYPE_F32 || alpha_dtype > GMPI_DTYPE_F16) return GMPI_E_DTYPE;
    if (stride_b < 0 || stride_d <= 0 || stride_row < W) return GMPI_E_STRIDE;
    const dim3 grid((W + 255) / 256, H, B), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    dispatch_dtype(alpha_dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(alpha_depth_kernel<T>, grid, block, 0, st, static_cast<const T*>(alpha), stride_b, stride_d, stride_row, plane_ds, D, H, W, depth_out,
                           transmittance_out);
    });
    return hip_rc(hipGetLastError());
}

int gmpi_selftest_division_launch(uint64_t pairs, uint32_t seed, uint64_t* mismatches, void* stream) {
    if (mismatches == nullptr) return GMPI_E_NULL;
    if (pairs == 0) return GMPI_OK;
    const uint64_t want = (pairs + 255) / 256;
    const unsigned blocks = static_cast<unsigned>(want < 256u * 64u ? want : 256u * 64u);
    hipLaunchKernelGGL(selftest_division_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), pairs, seed,
                       reinterpret_cast<unsigned long long*>(mismatches));
    return hip_rc(hipGetLastError());
}

int gmpi_stream_probe_launch(const void* buf, uint64_t bytes, uint32_t* sink, void* stream) {
    if (buf == nullptr) return GMPI_E_NULL;
    if (reinterpret_cast<uintptr_t>(buf) % 4 != 0) return GMPI_E_STRIDE;
    if (bytes < 4) return GMPI_OK;
    hipLaunchKernelGGL(stream_probe_kernel, dim3(256 * 2), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint32_t*>(buf),
                       static_cast<int64_t>(bytes / 4), sink);
    return hip_rc(hipGetLastError());
}

int gmpi_query(int32_t what) {
    switch (what) {
        case 0: return GMPI_ABI_VERSION;
        case 1: return static_cast<int>(sizeof(GmpiRenderParams));
        case 2: return 950;
        case 3: case 4: case 5: return lds_variant_query(what);
        case 6: return 1;  // GMPI_VARIANT_WAVE is built in
        case 7: return 0;  // GMPI_VARIANT_DMA: retired in round 4 (reserved value, refused with GMPI_E_VARIANT)
        case 8: return 1;  // GMPI_VARIANT_BAND is built in
        case 9: return static_cast<int>(kAutoBandMin);
        case 10: return static_cast<int>(kAutoBandMinF32);
        case 11: return 1;  // the atomics-free backward (pixel pass + texel gather) is built in
        case 12: case 13: case 14: return shared_forward_query(what);
        case 16: case 17: case 18: case 20: return u8_variant_query(what);  // (15, 19: unused)
        case 22: return 1;  // the depth-alpha layout (gmpi_mpi_render_depth_launch) is built in  (21: unused)
        case 23: return depth_tile_planes();  // planes the depth-alpha tile backward takes (more: the one-pixel-per-lane kernel)
        case 25: return 1;  // the depth-alpha window forward (gmpi_mpi_render_depth_window_launch) is built in  (24: unused)
        case 26: case 27: case 28: return depth_window_query(what);
        case 30: return 1;  // the geometry backward of the shared-colour and depth-alpha layouts is built in  (29: unused)
        case 32: return 1;  // compute_depth of the depth-alpha layout (gmpi_ramp_depth_launch, light_kernels.hip) is built in  (31: unused)
        case 34: return 1;  // the atomics-free backward of the shared-colour and depth-alpha layouts (gmpi_mpi_render_*_backward_gather_launch) is built in  (33: unused)
        case 38: return 1;  // the shaded render of an RGBA volume (gmpi_mpi_render_shaded_launch, gmpi_mpi_render_shaded_backward_launch) is built in  (37: unused)
        case 40: return 1;  // the gradient w.r.t. plane_z of the depth-alpha layout (gmpi_mpi_render_depth_geometry_backward_pz_launch) is built in  (39: unused)
        case 42: return 1;  // channels-last float layers (gmpi_mpi_render_layers_launch, gmpi_render_layers_supports) are built in  (41: unused)
        case 44: return 1;  // the in-place backward of channels-last float layers (gmpi_mpi_render_layers_backward_launch, gmpi_render_layers_backward_supports) is built in  (43: unused)
        case 46: return 1;  // the backward of the shading augmentation's image-sized middle and the shade-images pair (gmpi_light_shading_backward_launch, gmpi_light_blur_backward_launch, gmpi_light_shade_images_launch, gmpi_light_shade_images_backward_launch) are built in  (45: unused)
        case 48: return 1;  // the geometry backward over 8-bit volumes and float layers in place (gmpi_mpi_render_u8_geometry_backward_launch, gmpi_mpi_render_layers_geometry_backward_launch, gmpi_render_geometry_inplace_workspace_bytes) is built in  (47: unused)
        case 50: return 1;  // the plane-chunked render through the band kernel (gmpi_mpi_render_chunk_band_launch, gmpi_render_chunk_band_workspace_bytes, gmpi_render_chunk_band_supports) is built in  (49: unused)
        case 52: return 1;  // the occupancy map and the sparse render of 8-bit volumes (gmpi_u8_occupancy_bytes, gmpi_u8_occupancy_launch, gmpi_mpi_render_u8_sparse_launch, gmpi_render_u8_sparse_supports) are built in  (51: unused)
        case 53: return u8_variant_query(what);  // the side of a block of that map, in texels
        case 36: return 1;  // the plane-chunked render (gmpi_mpi_render_chunk_launch, gmpi_mpi_render_chunk_backward_launch) is built in  (35: unused)
        default: return -1;
    }
}

const char* gmpi_version_string(void) { return "ml-gmpi_amd 0.3 (gfx950, ABI 2)"; }

}  // extern "C"
