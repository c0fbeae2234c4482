// light_kernels.hip -- the reference's shading augmentation (gmpi/core/light_renderer.py `LightRenderer.render`)
// after `compute_depth` (alpha_depth_kernel in gmpi_abi.hip):
//   gaussian_blur_kernel  = torchvision.transforms.GaussianBlur on the depth image (light_renderer.py:51-55, 109),
//   light_shading_kernel  = point cloud from the last plane's texel coordinates (compute_pcl :102-120), normals from
//                           the four neighbour cross products (get_normal :57-80), Lambert term and ka + kd*diffuse
//                           (:163-190) -> one shading factor per texel,
//   light_apply_kernel    = clip(rgb * shading, 0, 1), alpha passed through, over the whole volume (:193-198).
// The first two work on B*H*W images (tiny); the third streams the RGBA volume once (read + write).
#include "gmpi_device.hpp"
#include "gmpi_shared.hpp"

#include "../../include/gmpi_render.h"

namespace gmpi {

constexpr float kLightEps = 1e-8f;  // EPS of light_renderer.py:8

__device__ __forceinline__ int reflect_index(int i, int n) {  // padding_mode="reflect": -1 -> 1, n -> n-2
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

// out[b,y,x] = sum_{dy,dx} in[b, refl(y+dy-r), refl(x+dx-r)] * (k1d[dy] * k1d[dx])   (kernel2d = k1d^T k1d as torchvision)
__global__ __launch_bounds__(256) void gaussian_blur_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                            const float* __restrict__ k1d, int ksize) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const float* __restrict__ img = in + static_cast<int64_t>(blockIdx.z) * H * W;
    const int r = ksize / 2;
    float acc = 0.0f;
    for (int dy = 0; dy < ksize; ++dy) {
        const float* __restrict__ row = img + static_cast<int64_t>(reflect_index(y + dy - r, H)) * W;
        const float wy = k1d[dy];
        for (int dx = 0; dx < ksize; ++dx) acc += row[reflect_index(x + dx - r, W)] * (wy * k1d[dx]);
    }
    out[(static_cast<int64_t>(blockIdx.z) * H + y) * W + x] = acc;
}

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

__global__ __launch_bounds__(256) void light_shading_kernel(const float* __restrict__ depth, const float* __restrict__ xyz_last,
                                                            const float* __restrict__ light_dir, float ka, float kd, int H, int W,
                                                            float* __restrict__ shading) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    const float* __restrict__ d = depth + static_cast<int64_t>(b) * H * W;
    // normals exist for the interior and are replicate-padded to the border (light_renderer.py:73)
    const int yc = min(max(y, 1), H - 2), xc = min(max(x, 1), W - 2);
    auto pcl = [&](int yy, int xx) {
        const float* __restrict__ p = xyz_last + (static_cast<int64_t>(yy) * W + xx) * 3;
        const float scale = d[static_cast<int64_t>(yy) * W + xx] / (p[2] + kLightEps);
        return V3{p[0] * scale, p[1] * scale, p[2] * scale};
    };
    const V3 c = pcl(yc, xc), up = pcl(yc - 1, xc), down = pcl(yc + 1, xc), left = pcl(yc, xc - 1), right = pcl(yc, xc + 1);
    V3 n = cross(up - c, left - c) + cross(left - c, down - c);
    n = n + cross(down - c, right - c);
    n = n + cross(right - c, up - c);
    float len2 = n.x * n.x;
    len2 = len2 + n.y * n.y;
    len2 = len2 + n.z * n.z;
    const float len = sqrtf(len2) + kLightEps;
    n = {n.x / len, n.y / len, n.z / len};
    const float* __restrict__ l = light_dir + 3 * b;
    float dotv = n.x * l[0];
    dotv = dotv + n.y * l[1];
    dotv = dotv + n.z * l[2];
    const float diffuse = fmaxf(-1.0f * dotv, 0.0f);
    shading[(static_cast<int64_t>(b) * H + y) * W + x] = ka + diffuse * kd;
}

// VEC consecutive texels of a row per thread (4: 16-byte loads for fp32 / 8-byte for 16-bit storage, 16-byte stores)
template <typename T, int VEC>
__global__ __launch_bounds__(256) void light_apply_kernel(const T* __restrict__ rgba, int64_t sb, int64_t sd, int64_t sc, int64_t sr,
                                                          const float* __restrict__ shading, float* __restrict__ out, int D, int H,
                                                          int W) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * VEC, y = blockIdx.y;
    if (x >= W) return;
    const int b = blockIdx.z / D, k = blockIdx.z - b * D;
    struct alignas(sizeof(T) * VEC) TV { T v[VEC]; };
    struct alignas(sizeof(float) * VEC) FV { float v[VEC]; };
    const FV s = *reinterpret_cast<const FV*>(shading + (static_cast<int64_t>(b) * H + y) * W + x);
    const T* __restrict__ src = rgba + b * sb + k * sd + static_cast<int64_t>(y) * sr + x;
    float* __restrict__ dst = out + ((static_cast<int64_t>(blockIdx.z) * 4) * H + y) * W + x;
    const int64_t plane = static_cast<int64_t>(H) * W;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const TV t = *reinterpret_cast<const TV*>(src + c * sc);
        FV o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) o.v[i] = c < 3 ? fminf(fmaxf(to_f32(t.v[i]) * s.v[i], 0.0f), 1.0f) : to_f32(t.v[i]);
        *reinterpret_cast<FV*>(dst + c * plane) = o;
    }
}

template <typename T>
static void launch_light_apply(const void* rgba, const int64_t* st, const float* shading, float* out, int B, int D, int H, int W,
                               hipStream_t stream) {
    const T* src = static_cast<const T*>(rgba);
    const bool vec = W % 4 == 0 && st[0] % 4 == 0 && st[1] % 4 == 0 && st[2] % 4 == 0 && st[3] % 4 == 0 &&
                     reinterpret_cast<uintptr_t>(rgba) % (4 * sizeof(T)) == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(shading) % 16 == 0;
    if (vec) hipLaunchKernelGGL((light_apply_kernel<T, 4>), dim3((W / 4 + 255) / 256, H, B * D), dim3(256), 0, stream, src, st[0], st[1], st[2], st[3], shading, out, D, H, W);
    else hipLaunchKernelGGL((light_apply_kernel<T, 1>), dim3((W + 255) / 256, H, B * D), dim3(256), 0, stream, src, st[0], st[1], st[2], st[3], shading, out, D, H, W);
}

// ---- backward of the augmentation (the reference applies it inside the G-step, train.py:535-541, 703-709) -------------
// (1), (2): the two volume-sized ops.  The B*H*W middle (blur, point cloud, normals, Lambert) is differentiated by torch autograd in
// light.py by default, and by the kernels (3), (4) below with LightRenderer(middle="hip"); (5) are the image-sized ends of the
// shared-colour and depth-alpha layouts in that mode.
//
// (1) out = clip(rgb * s, 0, 1) | alpha:   g_rgb = g_out * s * [0 < rgb*s < 1],  g_alpha = g_out_alpha (more is added by (2)),
//     g_s[b,y,x] = sum_{k,c} g_out * rgb * [0 < rgb*s < 1].  One pixel column per thread, planes in a loop (coalesced in x).
//     torch.clip passes the gradient at the bounds themselves (min <= x <= max), so the mask is closed.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void light_apply_backward_kernel(const T* __restrict__ rgba, int64_t sb, int64_t sd, int64_t sc,
                                                                   int64_t sr, const float* __restrict__ shading,
                                                                   const float* __restrict__ g_out, float* __restrict__ g_rgba,
                                                                   float* __restrict__ g_shading, int D, int H, int W) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * VEC, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    struct alignas(sizeof(T) * VEC) TV { T v[VEC]; };
    struct alignas(sizeof(float) * VEC) FV { float v[VEC]; };
    const int64_t plane = static_cast<int64_t>(H) * W, pix = static_cast<int64_t>(y) * W + x;
    const FV s = *reinterpret_cast<const FV*>(shading + b * plane + pix);
    FV gs;
#pragma unroll
    for (int i = 0; i < VEC; ++i) gs.v[i] = 0.0f;
    for (int k = 0; k < D; ++k) {
        const T* __restrict__ src = rgba + b * sb + k * sd + static_cast<int64_t>(y) * sr + x;
        const int64_t o = (static_cast<int64_t>(b) * D + k) * 4 * plane + pix;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const TV v = *reinterpret_cast<const TV*>(src + c * sc);
            const FV g = *reinterpret_cast<const FV*>(g_out + o + c * plane);
            FV r;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float vf = to_f32(v.v[i]), t = vf * s.v[i];
                const bool pass = t >= 0.0f && t <= 1.0f;
                r.v[i] = pass ? g.v[i] * s.v[i] : 0.0f;
                gs.v[i] += pass ? g.v[i] * vf : 0.0f;
            }
            *reinterpret_cast<FV*>(g_rgba + o + c * plane) = r;
        }
        *reinterpret_cast<FV*>(g_rgba + o + 3 * plane) = *reinterpret_cast<const FV*>(g_out + o + 3 * plane);
    }
    *reinterpret_cast<FV*>(g_shading + b * plane + pix) = gs;
}

// (2) depth = sum_k a_k T_k d_k (compute_depth): dL/da_k = T_k q_k - S_k / om_k, q_k = g d_k, S_k = gT T_out + sum_{j>k} a_j T_j q_j,
//     back to front from the forward's final transmittance (same scheme as render_backward.hip: no cancellation behind opaque
//     planes; T carried as mantissa x 2^exponent).  g_depth and g_T (the gradient w.r.t. T_out = prod_k om_k: dT_out/da_k =
//     -T_out / om_k) may each be nullptr.  ADDS into g_alpha (the alpha channel of the volume gradient).
template <typename T>
__global__ __launch_bounds__(256) void alpha_depth_backward_kernel(const T* __restrict__ alpha, int64_t sb, int64_t sd, int64_t sr,
                                                                   const float* __restrict__ ds, const float* __restrict__ t_final,
                                                                   const float* __restrict__ g_depth, const float* __restrict__ g_T,
                                                                   float* __restrict__ g_alpha, int64_t gb, int64_t gd, int64_t gr, int D,
                                                                   int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    const T* __restrict__ a = alpha + b * sb + static_cast<int64_t>(y) * sr + x;
    float* __restrict__ ga = g_alpha + b * gb + static_cast<int64_t>(y) * gr + x;
    const int64_t o = (static_cast<int64_t>(b) * H + y) * W + x;
    alpha_depth_sweep(D, ds, t_final, g_depth, g_T, o, [&](int k) { return to_f32(a[k * sd]); }, [&](int k, float v) { ga[k * gd] += v; });
}

// ---- the same two passes for a depth-alpha MPI (GmpiDepthAlpha; depth_alpha.py): a_k is the ramp of plane_z[k] minus ONE depth texel, so the alpha
// planes are never read or written -- the texel sits in a register and the plane loop is register work (plane_z, plane_ds: wave-uniform reads).
// The ramp is depth_ramp (gmpi_shared.hpp) through the rounded reciprocal, which gives the IEEE quotient: the bits of alpha_depth_kernel on
// depth_alpha_planes(...).
template <typename T>
__global__ __launch_bounds__(256) void ramp_depth_kernel(const T* __restrict__ image, int64_t sb, int64_t sr, DepthK dk, const float* __restrict__ ds,
                                                         int D, int H, int W, float* __restrict__ depth, float* __restrict__ tout) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    const float d = to_f32(image[b * sb + static_cast<int64_t>(y) * sr + x]);
    const float* __restrict__ pz = dk.plane_z + b * dk.pz_stride;
    float Tr = 1.0f, Z = 0.0f;
    alpha_depth_composite(D, ds, [&](int k) { bool inside; return depth_ramp<false>(pz[k], d, dk, inside); }, Tr, Z);
    const int64_t o = (static_cast<int64_t>(b) * H + y) * W + x;
    depth[o] = Z;
    if (tout) tout[o] = Tr;
}

// d a_k / d depth = -1 / den where lo <= plane_z[k] - depth <= hi (bounds included: where torch.clamp passes a gradient), 0 elsewhere -- a NaN texel
// included.  One thread owns its texel: the sum over the planes is a register, ADDED to g_image by a plain load, add and store.
template <typename T>
__global__ __launch_bounds__(256) void ramp_depth_backward_kernel(const T* __restrict__ image, int64_t sb, int64_t sr, DepthK dk,
                                                                  const float* __restrict__ ds, const float* __restrict__ t_final,
                                                                  const float* __restrict__ g_depth, const float* __restrict__ g_T,
                                                                  float* __restrict__ g_image, int64_t gb, int64_t gr, int D, int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    const float d = to_f32(image[b * sb + static_cast<int64_t>(y) * sr + x]);
    const float* __restrict__ pz = dk.plane_z + b * dk.pz_stride;
    const int64_t o = (static_cast<int64_t>(b) * H + y) * W + x;
    bool inside = false;
    float acc = 0.0f;
    alpha_depth_sweep(D, ds, t_final, g_depth, g_T, o, [&](int k) { return depth_ramp<false>(pz[k], d, dk, inside); },
                      [&](int, float v) { acc += inside ? v : 0.0f; });
    float* __restrict__ gi = g_image + b * gb + static_cast<int64_t>(y) * gr + x;
    *gi += -acc / dk.den;
}

// ---- backward of the image-sized middle (LightRenderer(middle="hip"); the default differentiates a torch restatement) ---------------------------------
// Gather form throughout: one thread owns one texel of the gradient and writes it once; no atomics, the same bits on every run.
//
// (3) adjoint of light_shading_kernel.  A pixel takes the normal of its clamped interior cell, and everything after the normal is the same for all
//     replicas: the upstream gradient of an interior cell is the sum of grad_shading over the pixels that clamp to it -- the cell itself, and the
//     border row / column / corner next to it (a whole row, column or image where H == 3 or W == 3).
__device__ __forceinline__ float replica_sum(const float* __restrict__ gs, int cy, int cx, int H, int W) {
    const int y0 = cy == 1 ? 0 : cy, y1 = cy == H - 2 ? H - 1 : cy;
    const int x0 = cx == 1 ? 0 : cx, x1 = cx == W - 2 ? W - 1 : cx;
    float acc = 0.0f;
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) acc += gs[static_cast<int64_t>(yy) * W + xx];
    return acc;
}

//     Per cell, with n the forward's normal (the same operations in the same order, so the clamp's mask is the forward's): shading = ka + kd max(-nh.l, 0),
//     nh = n / (|n| + EPS)  ->  g_nh = -kd G l where -nh.l >= 0 (closed, as torch.clamp passes it), g_n = g_nh / (|n| + EPS) - nh (g_nh . nh) / |n|,
//     and 0 where |n| == 0 (torch's pow(0.5) yields NaN there).  The four cross products add up to n = (up - down) x (left - right): the centre
//     cancels, so a point p receives a gradient only from the (at most four) interior cells that have it as a neighbour:
//         as up: (left - right) x g_n,  as down: the negative;  as right: (up - down) x g_n,  as left: the negative
//     with the points of THAT cell.  Finally p = xyz d / (xyz_z + EPS): grad_blurred = g_p . xyz / (xyz_z + EPS).  13-point diamond read of the depth.
__global__ __launch_bounds__(256) void light_shading_backward_kernel(const float* __restrict__ depth, const float* __restrict__ xyz_last,
                                                                     const float* __restrict__ light_dir, float kd,
                                                                     const float* __restrict__ grad_shading, int H, int W,
                                                                     float* __restrict__ grad_blurred) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    const float* __restrict__ d = depth + static_cast<int64_t>(b) * H * W;
    const float* __restrict__ gs = grad_shading + static_cast<int64_t>(b) * H * W;
    const float* __restrict__ l = light_dir + 3 * b;
    auto pcl = [&](int yy, int xx) {
        const float* __restrict__ p = xyz_last + (static_cast<int64_t>(yy) * W + xx) * 3;
        const float scale = d[static_cast<int64_t>(yy) * W + xx] / (p[2] + kLightEps);
        return V3{p[0] * scale, p[1] * scale, p[2] * scale};
    };
    // g_n of the interior cell (cy, cx) and its two diagonals; false where the cell does not exist or passes nothing
    auto cell = [&](int cy, int cx, V3& gn, V3& ud, V3& lr) {
        if (cy < 1 || cy > H - 2 || cx < 1 || cx > W - 2) return false;
        const V3 c = pcl(cy, cx), up = pcl(cy - 1, cx), down = pcl(cy + 1, cx), left = pcl(cy, cx - 1), right = pcl(cy, cx + 1);
        V3 n = cross(up - c, left - c) + cross(left - c, down - c);
        n = n + cross(down - c, right - c);
        n = n + cross(right - c, up - c);
        float len2 = n.x * n.x;
        len2 = len2 + n.y * n.y;
        len2 = len2 + n.z * n.z;
        const float norm = sqrtf(len2), len = norm + kLightEps;
        const V3 nh = {n.x / len, n.y / len, n.z / len};
        float dotv = nh.x * l[0];
        dotv = dotv + nh.y * l[1];
        dotv = dotv + nh.z * l[2];
        if (!(-1.0f * dotv >= 0.0f) || !(norm > 0.0f)) return false;
        const float g_dot = -(kd * replica_sum(gs, cy, cx, H, W));
        const V3 g_nh = {g_dot * l[0], g_dot * l[1], g_dot * l[2]};
        const float along = (g_nh.x * nh.x + g_nh.y * nh.y + g_nh.z * nh.z) / norm;
        gn = {g_nh.x / len - nh.x * along, g_nh.y / len - nh.y * along, g_nh.z / len - nh.z * along};
        ud = up - down, lr = left - right;
        return true;
    };
    V3 g = {0.0f, 0.0f, 0.0f}, gn, ud, lr;
    if (cell(y + 1, x, gn, ud, lr)) g = g + cross(lr, gn);   // this texel is that cell's `up`
    if (cell(y - 1, x, gn, ud, lr)) g = g - cross(lr, gn);   // ... `down`
    if (cell(y, x + 1, gn, ud, lr)) g = g - cross(ud, gn);   // ... `left`
    if (cell(y, x - 1, gn, ud, lr)) g = g + cross(ud, gn);   // ... `right`
    const float* __restrict__ p = xyz_last + (static_cast<int64_t>(y) * W + x) * 3;
    grad_blurred[(static_cast<int64_t>(b) * H + y) * W + x] = (g.x * p[0] + g.y * p[1] + g.z * p[2]) / (p[2] + kLightEps);
}

// (4) adjoint of gaussian_blur_kernel.  Along one axis of length n, input i is read by output j through tap t wherever refl(j + t - r) == i.  The
//     unpadded sources with that image are s = i, s = -i (i != 0) and s = 2(n-1) - i (i != n-1), and j = s - t + r must lie in [0, n): taps
//     max(0, s + r - (n-1)) .. min(ksize-1, s + r), an empty range for a reflected source away from its border (both can be live when n is as small as
//     r + 1).  A row is summed first, then weighted: n_x + n_y roundings per texel instead of n_x n_y.
__device__ __forceinline__ bool blur_source(int a, int i, int n, int& s) {
    s = a == 0 ? i : a == 1 ? -i : 2 * (n - 1) - i;
    return a == 0 || (a == 1 ? i != 0 : i != n - 1);
}

__global__ __launch_bounds__(256) void gaussian_blur_backward_kernel(const float* __restrict__ grad_blurred, float* __restrict__ grad_depth, int H,
                                                                     int W, const float* __restrict__ k1d, int ksize) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const float* __restrict__ img = grad_blurred + static_cast<int64_t>(blockIdx.z) * H * W;
    const int r = ksize / 2;
    float acc = 0.0f;
    for (int ay = 0; ay < 3; ++ay) {
        int sy;
        if (!blur_source(ay, y, H, sy)) continue;
        for (int ty = max(0, sy + r - (H - 1)); ty <= min(ksize - 1, sy + r); ++ty) {
            const float* __restrict__ row = img + static_cast<int64_t>(sy - ty + r) * W;
            float racc = 0.0f;
            for (int ax = 0; ax < 3; ++ax) {
                int sx;
                if (!blur_source(ax, x, W, sx)) continue;
                for (int tx = max(0, sx + r - (W - 1)); tx <= min(ksize - 1, sx + r); ++tx) racc += k1d[tx] * row[sx - tx + r];
            }
            acc += k1d[ty] * racc;
        }
    }
    grad_depth[(static_cast<int64_t>(blockIdx.z) * H + y) * W + x] = acc;
}

// (5) the image-sized ends of the shared-colour and depth-alpha layouts: clip(c * shading, 0, 1) on the colour image and, where there is one, the
//     background image, and its backward.  The two images may differ in storage type and strides: the type is a wave-uniform switch, not an instance.
struct LightImage {
    const void* p;   // [B,3,H,W], innermost stride 1; nullptr: no such image
    int32_t dtype;
    int64_t sb, sc, sr;
};
__device__ __forceinline__ float load_image(const LightImage& im, int64_t off) {
    switch (im.dtype) {
        case GMPI_DTYPE_BF16: return to_f32(static_cast<const bf16_t*>(im.p)[off]);
        case GMPI_DTYPE_F16: return to_f32(static_cast<const f16_t*>(im.p)[off]);
        default: return static_cast<const float*>(im.p)[off];
    }
}

__global__ __launch_bounds__(256) void light_shade_images_kernel(LightImage rgb, LightImage bg, const float* __restrict__ shading,
                                                                 float* __restrict__ rgb_out, float* __restrict__ bg_out, int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    const int64_t plane = static_cast<int64_t>(H) * W, pix = static_cast<int64_t>(y) * W + x;
    const float s = shading[b * plane + pix];
#pragma unroll
    for (int c = 0; c < 3; ++c) {   // (a NaN colour shades to 0, as in light_apply_kernel)
        rgb_out[(static_cast<int64_t>(b) * 3 + c) * plane + pix] = fminf(fmaxf(load_image(rgb, b * rgb.sb + c * rgb.sc + y * rgb.sr + x) * s, 0.0f), 1.0f);
        if (bg.p) bg_out[(static_cast<int64_t>(b) * 3 + c) * plane + pix] = fminf(fmaxf(load_image(bg, b * bg.sb + c * bg.sc + y * bg.sr + x) * s, 0.0f), 1.0f);
    }
}

//     g_c = g * s * mask and g_shading = sum over the channels of both images of g * c * mask, mask = [0 <= c * s <= 1] (closed: light_apply_backward_kernel's).
//     An upstream gradient that is nullptr counts as zero; an output that is nullptr is not written.
__global__ __launch_bounds__(256) void light_shade_images_backward_kernel(LightImage rgb, LightImage bg, const float* __restrict__ shading,
                                                                          const float* __restrict__ g_rgb_out, const float* __restrict__ g_bg_out,
                                                                          float* __restrict__ g_rgb, float* __restrict__ g_bg,
                                                                          float* __restrict__ g_shading, int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    const int64_t plane = static_cast<int64_t>(H) * W, pix = static_cast<int64_t>(y) * W + x;
    const float s = shading[b * plane + pix];
    float gs = 0.0f;
    auto image = [&](const LightImage& im, const float* __restrict__ g_out, float* __restrict__ g_in) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t o = (static_cast<int64_t>(b) * 3 + c) * plane + pix;
            const float v = load_image(im, b * im.sb + c * im.sc + y * im.sr + x), t = v * s, g = g_out ? g_out[o] : 0.0f;
            const bool pass = t >= 0.0f && t <= 1.0f;
            if (g_in) g_in[o] = pass ? g * s : 0.0f;
            gs += pass ? g * v : 0.0f;
        }
    };
    image(rgb, g_rgb_out, g_rgb);
    if (bg.p) image(bg, g_bg_out, g_bg);
    if (g_shading) g_shading[b * plane + pix] = gs;
}

static int rc_of(hipError_t e) { return e == hipSuccess ? GMPI_OK : GMPI_E_LAUNCH - static_cast<int>(e); }

// The checks of one image operand of the two shade-images entries.
static int to_light_image(const void* p, int32_t dtype, const int64_t* stride, int32_t W, LightImage& im) {
    if (!stride) return GMPI_E_NULL;
    if (dtype < GMPI_DTYPE_F32 || dtype > GMPI_DTYPE_F16) return GMPI_E_DTYPE;
    if (stride[0] < 0 || stride[1] <= 0 || stride[2] < W) return GMPI_E_STRIDE;
    im = {p, dtype, stride[0], stride[1], stride[2]};
    return GMPI_OK;
}

}  // namespace gmpi

using namespace gmpi;

extern "C" {

int gmpi_light_blur_launch(const float* depth, float* blurred, int32_t B, int32_t H, int32_t W, const float* kernel1d,
                           int32_t ksize, void* stream) {
    if (B < 0 || H <= 0 || W <= 0 || ksize <= 0 || (ksize & 1) == 0) return GMPI_E_SHAPE;
    if (ksize / 2 >= H || ksize / 2 >= W) return GMPI_E_SHAPE;  // reflect padding needs pad < size
    if (B == 0) return GMPI_OK;
    if (!depth || !blurred || !kernel1d) return GMPI_E_NULL;
    hipLaunchKernelGGL(gaussian_blur_kernel, dim3((W + 255) / 256, H, B), dim3(256), 0, static_cast<hipStream_t>(stream), depth,
                       blurred, H, W, kernel1d, ksize);
    return rc_of(hipGetLastError());
}

int gmpi_light_shading_launch(const float* depth_blurred, const float* xyz_last, const float* light_dir, float ka, float kd,
                              int32_t B, int32_t H, int32_t W, float* shading, void* stream) {
    if (B < 0 || H < 3 || W < 3) return GMPI_E_SHAPE;
    if (B == 0) return GMPI_OK;
    if (!depth_blurred || !xyz_last || !light_dir || !shading) return GMPI_E_NULL;
    hipLaunchKernelGGL(light_shading_kernel, dim3((W + 255) / 256, H, B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       depth_blurred, xyz_last, light_dir, ka, kd, H, W, shading);
    return rc_of(hipGetLastError());
}

int gmpi_light_apply_launch(const void* rgba, int32_t rgba_dtype, const int64_t* rgba_stride, const float* shading, float* out,
                            int32_t B, int32_t D, int32_t H, int32_t W, void* stream) {
    if (B < 0 || D <= 0 || H <= 0 || W <= 0 || static_cast<int64_t>(B) * D > 65535) return GMPI_E_SHAPE;
    if (B == 0) return GMPI_OK;
    if (!rgba || !rgba_stride || !shading || !out) return GMPI_E_NULL;
    if (rgba_dtype < GMPI_DTYPE_F32 || rgba_dtype > GMPI_DTYPE_F16) return GMPI_E_DTYPE;
    if (rgba_stride[4] != 1 || rgba_stride[3] < W || rgba_stride[2] <= 0 || rgba_stride[1] <= 0 || rgba_stride[0] < 0) return GMPI_E_STRIDE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    dispatch_dtype(rgba_dtype, [&](auto t) { launch_light_apply<typename decltype(t)::type>(rgba, rgba_stride, shading, out, B, D, H, W, st); });
    return rc_of(hipGetLastError());
}

int gmpi_light_apply_backward_launch(const void* rgba, int32_t rgba_dtype, const int64_t* rgba_stride, const float* shading,
                                     const float* grad_out, float* grad_rgba, float* grad_shading, int32_t B, int32_t D, int32_t H,
                                     int32_t W, void* stream) {
    if (B < 0 || D <= 0 || H <= 0 || W <= 0) return GMPI_E_SHAPE;
    if (B == 0) return GMPI_OK;
    if (!rgba || !rgba_stride || !shading || !grad_out || !grad_rgba || !grad_shading) return GMPI_E_NULL;
    if (rgba_dtype < GMPI_DTYPE_F32 || rgba_dtype > GMPI_DTYPE_F16) return GMPI_E_DTYPE;
    if (rgba_stride[4] != 1 || rgba_stride[3] < W || rgba_stride[2] <= 0 || rgba_stride[1] <= 0 || rgba_stride[0] < 0) return GMPI_E_STRIDE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t sb = rgba_stride[0], sd = rgba_stride[1], sc = rgba_stride[2], sr = rgba_stride[3];
    const int es = rgba_dtype == GMPI_DTYPE_F32 ? 4 : 2;
    const bool vec = W % 4 == 0 && sb % 4 == 0 && sd % 4 == 0 && sc % 4 == 0 && sr % 4 == 0 && reinterpret_cast<uintptr_t>(rgba) % (4 * es) == 0 &&
                     reinterpret_cast<uintptr_t>(shading) % 16 == 0 && reinterpret_cast<uintptr_t>(grad_out) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(grad_rgba) % 16 == 0 && reinterpret_cast<uintptr_t>(grad_shading) % 16 == 0;
    const dim3 block(256), grid(((vec ? W / 4 : W) + 255) / 256, H, B);
    dispatch_dtype(rgba_dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        dispatch_bool(vec, [&](auto VEC) {
            hipLaunchKernelGGL((light_apply_backward_kernel<T, decltype(VEC)::value ? 4 : 1>), grid, block, 0, st, static_cast<const T*>(rgba), sb, sd, sc, sr, shading,
                               grad_out, grad_rgba, grad_shading, D, H, W);
        });
    });
    return rc_of(hipGetLastError());
}

int gmpi_alpha_depth_backward_ex_launch(const void* alpha, int32_t alpha_dtype, int64_t stride_b, int64_t stride_d, int64_t stride_row,
                                        const float* plane_ds, const float* transmittance, const float* grad_depth,
                                        const float* grad_transmittance, float* grad_alpha, int64_t gstride_b, int64_t gstride_d,
                                        int64_t gstride_row, int32_t B, int32_t D, int32_t H, int32_t W, void* stream) {
    if (B < 0 || D <= 0 || H <= 0 || W <= 0) return GMPI_E_SHAPE;
    if (B == 0) return GMPI_OK;
    if (!alpha || !plane_ds || !grad_alpha) return GMPI_E_NULL;
    if (alpha_dtype < GMPI_DTYPE_F32 || alpha_dtype > GMPI_DTYPE_F16) return GMPI_E_DTYPE;
    if (stride_b < 0 || stride_d <= 0 || stride_row < W || gstride_b <= 0 || gstride_d <= 0 || gstride_row < W) return GMPI_E_STRIDE;
    if (!grad_depth && !grad_transmittance) return GMPI_OK;   // (nothing to add)
    const dim3 grid((W + 255) / 256, H, B), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    dispatch_dtype(alpha_dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(alpha_depth_backward_kernel<T>, grid, block, 0, st, static_cast<const T*>(alpha), stride_b, stride_d, stride_row, plane_ds, transmittance,
                           grad_depth, grad_transmittance, grad_alpha, gstride_b, gstride_d, gstride_row, D, H, W);
    });
    return rc_of(hipGetLastError());
}

int gmpi_alpha_depth_backward_launch(const void* alpha, int32_t alpha_dtype, int64_t stride_b, int64_t stride_d, int64_t stride_row,
                                     const float* plane_ds, const float* transmittance, const float* grad_depth, float* grad_alpha,
                                     int64_t gstride_b, int64_t gstride_d, int64_t gstride_row, int32_t B, int32_t D, int32_t H,
                                     int32_t W, void* stream) {
    if (B > 0 && D > 0 && H > 0 && W > 0 && !grad_depth) return GMPI_E_NULL;
    return gmpi_alpha_depth_backward_ex_launch(alpha, alpha_dtype, stride_b, stride_d, stride_row, plane_ds, transmittance, grad_depth, nullptr,
                                               grad_alpha, gstride_b, gstride_d, gstride_row, B, D, H, W, stream);
}

// The checks the two ramp entries share, all before any launch; fills DepthK as the depth-alpha launchers fill it (to_depth, gmpi_abi.hip).
// GMPI_OK with B == 0 means: nothing to do.
static int to_ramp(const void* depth_image, int32_t depth_dtype, int64_t stride_b, int64_t stride_row, const GmpiDepthAlpha* ramp, const float* plane_ds,
                   int32_t B, int32_t D, int32_t H, int32_t W, DepthK& dk) {
    if (B < 0 || D <= 0 || H <= 0 || W <= 0 || B > 65535 || H > 65535) return GMPI_E_SHAPE;   // (rows and images are grid.y and grid.z)
    if (B == 0) return GMPI_OK;
    if (!depth_image || !ramp || !plane_ds) return GMPI_E_NULL;
    if (ramp->struct_size != sizeof(GmpiDepthAlpha)) return GMPI_E_ABI;
    if (!ramp->plane_z) return GMPI_E_NULL;
    if (depth_dtype < GMPI_DTYPE_F32 || depth_dtype > GMPI_DTYPE_F16) return GMPI_E_DTYPE;
    if (ramp->plane_z_stride < 0 || stride_b < 0 || stride_row < W) return GMPI_E_STRIDE;
    if (!(ramp->z_lo < ramp->z_hi) || !(ramp->z_den > 0.0f)) return GMPI_E_SHAPE;
    dk.plane_z = ramp->plane_z, dk.pz_stride = ramp->plane_z_stride;
    dk.lo = ramp->z_lo, dk.hi = ramp->z_hi, dk.den = ramp->z_den, dk.rden = 1.0f / ramp->z_den;
    return GMPI_OK;
}

int gmpi_ramp_depth_launch(const void* depth_image, int32_t depth_dtype, int64_t stride_b, int64_t stride_row, const GmpiDepthAlpha* ramp,
                           const float* plane_ds, int32_t B, int32_t D, int32_t H, int32_t W, float* depth_out, float* transmittance_out,
                           void* stream) {
    DepthK dk;
    const int rc = to_ramp(depth_image, depth_dtype, stride_b, stride_row, ramp, plane_ds, B, D, H, W, dk);
    if (rc != GMPI_OK || B == 0) return rc;
    if (!depth_out) return GMPI_E_NULL;
    const dim3 grid((W + 255) / 256, H, B), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    dispatch_dtype(depth_dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(ramp_depth_kernel<T>, grid, block, 0, st, static_cast<const T*>(depth_image), stride_b, stride_row, dk, plane_ds, D, H, W, depth_out,
                           transmittance_out);
    });
    return rc_of(hipGetLastError());
}

int gmpi_ramp_depth_backward_launch(const void* depth_image, int32_t depth_dtype, int64_t stride_b, int64_t stride_row, const GmpiDepthAlpha* ramp,
                                    const float* plane_ds, const float* transmittance, const float* grad_depth, const float* grad_transmittance,
                                    float* grad_depth_image, int64_t gstride_b, int64_t gstride_row, int32_t B, int32_t D, int32_t H, int32_t W,
                                    void* stream) {
    DepthK dk;
    const int rc = to_ramp(depth_image, depth_dtype, stride_b, stride_row, ramp, plane_ds, B, D, H, W, dk);
    if (rc != GMPI_OK || B == 0) return rc;
    if (!grad_depth_image) return GMPI_E_NULL;
    if (gstride_b <= 0 || gstride_row < W) return GMPI_E_STRIDE;
    if (!grad_depth && !grad_transmittance) return GMPI_OK;   // (nothing to add)
    const dim3 grid((W + 255) / 256, H, B), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    dispatch_dtype(depth_dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(ramp_depth_backward_kernel<T>, grid, block, 0, st, static_cast<const T*>(depth_image), stride_b, stride_row, dk, plane_ds, transmittance,
                           grad_depth, grad_transmittance, grad_depth_image, gstride_b, gstride_row, D, H, W);
    });
    return rc_of(hipGetLastError());
}

int gmpi_light_shading_backward_launch(const float* depth_blurred, const float* xyz_last, const float* light_dir, float kd, const float* grad_shading,
                                       int32_t B, int32_t H, int32_t W, float* grad_blurred, void* stream) {
    if (B < 0 || H < 3 || W < 3 || B > 65535 || H > 65535) return GMPI_E_SHAPE;   // (rows and images are grid.y and grid.z)
    if (B == 0) return GMPI_OK;
    if (!depth_blurred || !xyz_last || !light_dir || !grad_shading || !grad_blurred) return GMPI_E_NULL;
    hipLaunchKernelGGL(light_shading_backward_kernel, dim3((W + 255) / 256, H, B), dim3(256), 0, static_cast<hipStream_t>(stream), depth_blurred,
                       xyz_last, light_dir, kd, grad_shading, H, W, grad_blurred);
    return rc_of(hipGetLastError());
}

int gmpi_light_blur_backward_launch(const float* grad_blurred, float* grad_depth, int32_t B, int32_t H, int32_t W, const float* kernel1d,
                                    int32_t ksize, void* stream) {
    if (B < 0 || H <= 0 || W <= 0 || B > 65535 || H > 65535 || ksize <= 0 || (ksize & 1) == 0) return GMPI_E_SHAPE;
    if (ksize / 2 >= H || ksize / 2 >= W) return GMPI_E_SHAPE;  // the forward's limit: reflect padding needs pad < size
    if (B == 0) return GMPI_OK;
    if (!grad_blurred || !grad_depth || !kernel1d) return GMPI_E_NULL;
    hipLaunchKernelGGL(gaussian_blur_backward_kernel, dim3((W + 255) / 256, H, B), dim3(256), 0, static_cast<hipStream_t>(stream), grad_blurred,
                       grad_depth, H, W, kernel1d, ksize);
    return rc_of(hipGetLastError());
}

int gmpi_light_shade_images_launch(const void* rgb, int32_t rgb_dtype, const int64_t* rgb_stride, const void* background, int32_t background_dtype,
                                   const int64_t* background_stride, const float* shading, float* rgb_out, float* background_out, int32_t B,
                                   int32_t H, int32_t W, void* stream) {
    if (B < 0 || H <= 0 || W <= 0 || B > 65535 || H > 65535) return GMPI_E_SHAPE;
    if (B == 0) return GMPI_OK;
    if (!rgb || !shading || !rgb_out || (background && !background_out)) return GMPI_E_NULL;
    LightImage c{}, bg{};
    int rc = to_light_image(rgb, rgb_dtype, rgb_stride, W, c);
    if (rc == GMPI_OK && background) rc = to_light_image(background, background_dtype, background_stride, W, bg);
    if (rc != GMPI_OK) return rc;
    hipLaunchKernelGGL(light_shade_images_kernel, dim3((W + 255) / 256, H, B), dim3(256), 0, static_cast<hipStream_t>(stream), c, bg, shading, rgb_out,
                       background_out, H, W);
    return rc_of(hipGetLastError());
}

int gmpi_light_shade_images_backward_launch(const void* rgb, int32_t rgb_dtype, const int64_t* rgb_stride, const void* background,
                                            int32_t background_dtype, const int64_t* background_stride, const float* shading,
                                            const float* grad_rgb_out, const float* grad_background_out, float* grad_rgb, float* grad_background,
                                            float* grad_shading, int32_t B, int32_t H, int32_t W, void* stream) {
    if (B < 0 || H <= 0 || W <= 0 || B > 65535 || H > 65535) return GMPI_E_SHAPE;
    if (B == 0) return GMPI_OK;
    if (!rgb || !shading || (!grad_rgb && !grad_background && !grad_shading)) return GMPI_E_NULL;
    if (!background && (grad_background_out || grad_background)) return GMPI_E_NULL;
    LightImage c{}, bg{};
    int rc = to_light_image(rgb, rgb_dtype, rgb_stride, W, c);
    if (rc == GMPI_OK && background) rc = to_light_image(background, background_dtype, background_stride, W, bg);
    if (rc != GMPI_OK) return rc;
    hipLaunchKernelGGL(light_shade_images_backward_kernel, dim3((W + 255) / 256, H, B), dim3(256), 0, static_cast<hipStream_t>(stream), c, bg, shading,
                       grad_rgb_out, grad_background_out, grad_rgb, grad_background, grad_shading, H, W);
    return rc_of(hipGetLastError());
}

}  // extern "C"
