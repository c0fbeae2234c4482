// gmpi_device.hpp -- device-side arithmetic shared by the render kernels (gfx950 / CDNA4 only).
//
// The coordinate chain below must reproduce the reference's fp32 arithmetic EXACTLY
// (gmpi/core/mpi.py:74-99 followed by ATen's grid_sampler unnormalize): a 1-ulp difference in
// ray/plane intersection moves the sample position by up to 4e-4 texel at 1024^2 and the output by
// up to 5e-4 on white-noise textures (hard part 1).  Hence:
//   * this translation unit is compiled with -ffp-contract=off (and the pragma below): a*b+c is
//     v_mul_f32 + v_add_f32, never v_fma_f32, unless __builtin_fmaf is written out;
//   * a/b is the correctly rounded IEEE division (hipcc default
//     -fhip-fp32-correctly-rounded-divide-sqrt; never -ffast-math);
//   * fp32 denormals are on (gfx9 default).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/gmpi_render.h"  // GMPI_FLAG_* / GMPI_STATUS_*: device and launcher code names the bits, never writes them out

#pragma clang fp contract(off)

namespace gmpi {

constexpr float kNarrowScale = 0.95f;  // mpi.py:23 ALIGN_CORNERS_FALSE_NARROW_SCALE

// Kernel-side view of GmpiRenderParams (include/gmpi_render.h), passed by value.
struct KParams {
    const void* rgba;
    const int32_t* view_to_mpi;
    const float* dhw;
    const float* ray_dir;
    const float* eye_pos;
    const float* z_dir;
    float* rgb_out;
    float* depth_out;
    float* T_out;
    uint32_t* status;
    int64_t s_mpi, s_plane, s_chan, s_row;  // element strides of rgba [M,D,4,Ht,Wt] (col stride 1; rgba8_t and float-texel instances: bytes, texel stride 4 elements, s_chan unused)
    int32_t N, M, D, Ht, Wt, H, W, views_per_mpi;
    uint32_t flags;
    void* ws;           // caller's workspace (GmpiRenderParams.workspace): the band kernel's geometry table
    uint64_t ws_bytes;
    // View gate (GMPI_VARIANT_AUTO's two-kernel launches, gmpi_abi.hip): the band kernel's table kernel stamps gate[n] = gate_gen for every view
    // with a box that does not fit the band kernel's staging buffers; a render kernel takes view n iff (gate[n] == gate_gen) == (gate_sense != 0).
    // Whatever the workspace held before, exactly one of the two kernels renders each view.  gate == nullptr: every view.
    uint32_t* gate;
    uint32_t gate_gen, gate_sense;
    int32_t band_cols;  // band kernel: band columns per XCD window (render_band.hip band_pos; set by launch_band)
    int32_t band_rot, band_split;   // band kernel: per-view rotation of the XCD <-> run assignment, pieces per run (xcd_item_per_group)
    int32_t band_tail;              // band kernel: the last band_tail bands of every XCD's last run are handed out by tickets (render_band.hip)
};
// The carry of a plane-chunked render (gmpi_mpi_render_chunk_launch; load_carry / store_carry below): the Accum of every pixel in front of this launch's
// planes / behind them, [N, 5, H, W] fp32, either may be nullptr.  An argument of its own, of the carry instances of the gather, tile and 8-bit tile
// kernels alone: as two more members of KParams the pointers moved the band kernel's range-checking instances into scratch.
struct CarryK {
    const float* state_in;
    float* state_out;
};
struct NoCarry {};   // what the one-shot instances take in CarryK's place: nothing

// blockIdx -> work item (pixel tile / band), "per view group" form: XCD x = blockIdx % 8 (workgroups are dealt round-robin to the 8 XCDs)
// gets a contiguous run of the items of EVERY group of views that share an MPI, so that row-major neighbours meet in one L2 AND the XCDs walk
// the views together -- a launch that only renders some of the views (gate) still fills every XCD.  Returns n_items for "no item".
// `rot`: group g hands XCD x the run that XCD (x + g rot) % 8 would get in group 0.  The dispatcher deals workgroups to the XCDs round-robin and NO work moves
// between XCDs afterwards: a launch ends when the most loaded XCD is done.  With rot = 0 every XCD renders the same region of every view; regions differ in
// cost (the camera's keystone makes the texel boxes of some band rows taller: a third DMA pass), and what is expensive in one view tends to be expensive in the
// next: rotating the assignment per view averages that out (round 6, render_band.hip; measured per XCD with s_memtime stamps: profiles/r06_band_order.txt).
// `split` (1, 2, 4 or 8): an XCD's run of a group is cut into `split` pieces taken from regions 8 / split apart (piece s from region + s 8 / split): the XCD then
// renders pieces of opposite parts of the view -- whose costs complement each other -- already within ONE view.
__device__ __forceinline__ int xcd_item_per_group(int block, int group_items, int n_items, int rot = 0, int split = 1) {
    const int per_xcd = (group_items + 7) / 8, n_groups = (n_items + group_items - 1) / group_items;
    const int jb = block / 8, grp = jb / per_xcd, rr = jb - grp * per_xcd;
    const int piece = split > 1 ? rr * split / per_xcd : 0;
    const int in_group = ((block + grp * rot + piece * (8 / max(split, 1))) % 8) * per_xcd + rr;
    const int item = grp * group_items + in_group;
    return (grp >= n_groups || in_group >= group_items || item >= n_items) ? n_items : item;
}
inline __host__ unsigned xcd_grid_per_group(int group_items, int n_items) {
    return static_cast<unsigned>(((group_items + 7) / 8) * 8 * ((n_items + group_items - 1) / group_items));
}

__device__ __forceinline__ bool view_gated_out(const KParams& p, int n) {
    return p.gate != nullptr && ((p.gate[n] == p.gate_gen) != (p.gate_sense != 0u));
}

// MPI sampled by view n: view_to_mpi[n], or n / views_per_mpi.  An index outside [0, M) would address dhw and the volume
// out of bounds: it is clamped and reported (GMPI_STATUS_BAD_VIEW_INDEX) instead.
__device__ __forceinline__ int view_mpi(const KParams& p, int n, uint32_t& bad) {
    int m = p.view_to_mpi ? p.view_to_mpi[n] : n / p.views_per_mpi;
    if (m < 0 || m >= p.M) {
        bad |= GMPI_STATUS_BAD_VIEW_INDEX;
        m = min(max(m, 0), p.M - 1);
    }
    return m;
}

// Work item (pixel tile / strip band / band) -> view n and position `rem` inside the view, `per_view` items per view.  Views that share one MPI
// (video paths: views_per_mpi > 1) are interleaved per position, so that the workgroups that need (nearly) the same texels of a plane run next to
// each other in time and on the same XCD: the volume is then read from HBM about once per group of views instead of once per view.
__device__ __forceinline__ void item_to_view(const KParams& p, int item, int per_view, int& n, int& rem) {
    if (p.view_to_mpi == nullptr && p.views_per_mpi > 1) {
        const int group = item / (per_view * p.views_per_mpi);  // full groups come first
        const int first = group * p.views_per_mpi, size = min(p.views_per_mpi, p.N - first);
        const int r = item - first * per_view;
        rem = r / size;
        n = first + (r - rem * size);
    } else {
        n = item / per_view;
        rem = item - n * per_view;
    }
}

// ---- texel fetch: storage type -> fp32 (exact upcast, mpi_renderer.py:446) -----------------------
struct bf16_t { uint16_t bits; };
struct f16_t { _Float16 v; };

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(bf16_t v) { return __uint_as_float(static_cast<uint32_t>(v.bits) << 16); }
__device__ __forceinline__ float to_f32(f16_t v) { return static_cast<float>(v.v); }
// 8-bit storage (GMPI_DTYPE_U8): code c in 0..255 stands for the fp32 value c / 255, the correctly rounded quotient.  A bare c * RN(1/255) misses it for
// 126 of the 256 codes; one correction step (div_by_recip below, written out: the residual e is exact) gives it for all 256
// (tests/test_u8_storage_cpu.py restates this in numpy and checks every code).  Not an upcast any more: three VALU ops per texel.
struct u8_t { uint8_t code; };
constexpr float kInv255 = 1.0f / 255.0f;  // RN(1/255)
__device__ __forceinline__ float unorm8_to_f32(float c) {  // c: the code as a float (v_cvt_f32_ubyte0..3 are exact)
    const float q = c * kInv255;
    const float e = __builtin_fmaf(-q, 255.0f, c);
    return __builtin_fmaf(e, kInv255, q);
}
__device__ __forceinline__ float to_f32(u8_t v) { return unorm8_to_f32(static_cast<float>(v.code)); }
// The same codes, channels-last (GMPI_DTYPE_U8 with rgba_stride[2] == 1 and rgba_stride[4] == 4): one texel = the four bytes R, G, B, A.  A storage type of
// its own, so that no other instance carries a texel stride.  The strides of such a volume count BYTES (tex_offset); alignment 1: a base pointer may
// sit at any byte.
struct rgba8_t { uint8_t c[4]; };
// Channels-last FLOAT layers (gmpi_mpi_render_layers_launch: [M,D,Ht,Wt,4], channel stride 1, texel stride 4 elements): one texel = R, G, B, A of the
// element type, 16 bytes of fp32 or 8 bytes of 16-bit storage.  Storage types of their own, as rgba8_t: the instances over them learn the layout from
// the template argument, KParams carries no texel stride and no other instance changes.  Their strides count BYTES (tex_offset; the launcher
// converts the struct's element strides), s_chan is unused.  Alignment: the element's -- a texel may start at any element (a column slice).
struct rgba32f_t { float c[4]; };
struct rgba16h_t { f16_t c[4]; };
struct rgba16b_t { bf16_t c[4]; };
template <typename TexT> struct FloatTexel { static constexpr bool value = false; };
template <> struct FloatTexel<rgba32f_t> { static constexpr bool value = true; using elem = float; };
template <> struct FloatTexel<rgba16h_t> { static constexpr bool value = true; using elem = f16_t; };
template <> struct FloatTexel<rgba16b_t> { static constexpr bool value = true; using elem = bf16_t; };
template <typename TexT> constexpr bool is_float_texel = FloatTexel<TexT>::value;
template <typename TexT>
__device__ __forceinline__ const TexT* tex_offset(const TexT* p, int64_t n) {
    if constexpr (is_float_texel<TexT>) return reinterpret_cast<const TexT*>(reinterpret_cast<const uint8_t*>(p) + n);
    else return p + n;
}
__device__ __forceinline__ const rgba8_t* tex_offset(const rgba8_t* p, int64_t n) {
    return reinterpret_cast<const rgba8_t*>(reinterpret_cast<const uint8_t*>(p) + n);
}
// One texel as the dword R | G << 8 | B << 16 | A << 24: a single 4-byte load at byte alignment (the memcpy says so).
__device__ __forceinline__ uint32_t load_texel(const rgba8_t* p, int64_t byte_off) {
    uint32_t t;
    __builtin_memcpy(&t, reinterpret_cast<const uint8_t*>(p) + byte_off, 4);
    return t;
}
__device__ __forceinline__ float texel_code(uint32_t t, int c) { return static_cast<float>((t >> (8 * c)) & 0xffu); }   // v_cvt_f32_ubyte<c>: exact

// One whole texel in a single load (global_load_dwordx4 / dwordx2) at the ELEMENT's alignment: the memcpy from an element pointer says so.
template <typename TexT, std::enable_if_t<is_float_texel<TexT>, int> = 0>
__device__ __forceinline__ TexT load_texel(const TexT* p, int64_t byte_off) {
    using E = typename FloatTexel<TexT>::elem;
    TexT t;
    __builtin_memcpy(&t, __builtin_assume_aligned(reinterpret_cast<const uint8_t*>(p) + byte_off, alignof(E)), sizeof(TexT));
    return t;
}

// Host side: a run-time dtype (GMPI_DTYPE_F32 / _BF16 / _F16 = 0 / 1 / 2, validated by the C ABI) or flag picks the template instance.
// f is a generic lambda: it gets TypeTag<float | bf16_t | f16_t>{} (storage type: `typename decltype(t)::type`), resp. std::true_type{} /
// std::false_type{} (`decltype(b)::value`), and its result is passed on.
// The three floating-point storage types ONLY.  GMPI_DTYPE_U8 has instances of two forward kernels (render_gather.hip, render_u8.hip), whose
// launchers pick them before they come here; every other entry refuses the type with GMPI_E_DTYPE.  Should one forget to: nothing is launched
// and hipErrorInvalidValue comes back -- never another type's instance.
template <typename T> struct TypeTag { using type = T; };
template <typename F>
inline auto dispatch_dtype(int dtype, F&& f) {
    using R = decltype(f(TypeTag<float>{}));
    switch (dtype) {
        case GMPI_DTYPE_F32: return f(TypeTag<float>{});
        case GMPI_DTYPE_BF16: return f(TypeTag<bf16_t>{});
        case GMPI_DTYPE_F16: return f(TypeTag<f16_t>{});
        default:
            if constexpr (std::is_void_v<R>) return;
            else return static_cast<R>(hipErrorInvalidValue);
    }
}
template <typename F>
inline auto dispatch_bool(bool flag, F&& f) {
    return flag ? f(std::true_type{}) : f(std::false_type{});
}
// The two flags every forward kernel is instantiated over: f(AC, STRICT) for GMPI_FLAG_ALIGN_CORNERS, GMPI_FLAG_STRICT_ORDER.
template <typename F>
inline auto dispatch_ac_strict(uint32_t flags, F&& f) {
    return dispatch_bool(flags & GMPI_FLAG_ALIGN_CORNERS, [&](auto AC) { return dispatch_bool(flags & GMPI_FLAG_STRICT_ORDER, [&](auto STRICT) { return f(AC, STRICT); }); });
}
// Host side: a GMPI_DTYPE_U8 volume is channels-last (the rgba8_t instances).  to_kparams (gmpi_abi.hip) says so through s_chan = 0, which no planar
// volume has (its channel stride is validated to be non-zero); s_mpi, s_plane and s_row then count bytes.
inline __host__ bool u8_interleaved(const KParams& p) { return p.s_chan == 0; }
// Host side: the volume can be staged in 16-byte loader items -- items of a box that touches the border do not straddle it, and every item is aligned.
inline __host__ bool volume_stages_in_items(const KParams& p, int dtype) {
    const int tpi = 16 / (dtype == GMPI_DTYPE_F32 ? 4 : 2);  // texels per item
    return p.Wt % tpi == 0 && reinterpret_cast<uintptr_t>(p.rgba) % 16 == 0 && p.s_row % tpi == 0 && p.s_chan % tpi == 0 && p.s_plane % tpi == 0 &&
           p.s_mpi % tpi == 0;
}

// ---- ray/plane intersection -> unnormalised texture coordinates --------------------------------
// One rounding per line, in the reference's order.
//   zdiff = d - eye_z                (mpi.py:74)   computed by the caller (wave-uniform)
//   s     = zdiff / ray_z            (mpi.py:76)
//   x     = eye_x + ray_x * s        (mpi.py:79)
//   u     = (2 x) / w                (mpi.py:90)   2*x is exact
//   AC:   ix = (u + 1) * ((Wt-1)/2)  == ((u+1)/2)*(Wt-1) as a real number -> same single rounding
//   !AC:  u *= 0.95 if -1<=u<=1 (mpi.py:98-99); ix = ((u+1)*Wt - 1)/2   (GridSampler.h:27-35)
template <bool AC>
__device__ __forceinline__ void plane_coord(float zdiff, float ph, float pw, float ex, float ey, float rx, float ry,
                                            float rz, float cx, float cy, float& ix, float& iy, float& s, float& u,
                                            float& v) {
    s = zdiff / rz;
    const float tx = rx * s;
    const float ty = ry * s;
    const float x = ex + tx;
    const float y = ey + ty;
    const float x2 = 2.0f * x;
    const float y2 = 2.0f * y;
    u = x2 / pw;
    v = y2 / ph;
    if (AC) {
        const float u1 = u + 1.0f;
        const float v1 = v + 1.0f;
        ix = u1 * cx;  // cx = (Wt-1)/2
        iy = v1 * cy;  // cy = (Ht-1)/2
    } else {
        if (v >= -1.0f && v <= 1.0f) v = v * kNarrowScale;
        if (u >= -1.0f && u <= 1.0f) u = u * kNarrowScale;
        const float u1 = u + 1.0f;
        const float v1 = v + 1.0f;
        const float ux = u1 * cx;  // cx = Wt
        const float vy = v1 * cy;  // cy = Ht
        const float uxm = ux - 1.0f;
        const float vym = vy - 1.0f;
        ix = uxm * 0.5f;
        iy = vym * 0.5f;
    }
}

// ---- division through a correctly rounded reciprocal ------------------------------------------------
// q = n / d, correctly rounded, from r = RN(1/d):   q0 = RN(n*r);  e = n - d*q0 (exact, one FMA);
// q = RN(q0 + e*r).  This is Markstein's final-correction step ("IA-64 and Elementary Functions",
// thm. 8.2 / Cornea-Harrison-Tang): with r the CORRECTLY ROUNDED reciprocal and q0 within one ulp of
// n/d, the corrected quotient is the correctly rounded one (for normal-range operands and results;
// the single exceptional significand pattern d = 2^k*(2-2^-23) needs n*r to be faithful, which it
// is here).  r is an IEEE division itself (1.0f / d) but a loop-invariant one: per pixel for ray_z,
// per plane for the plane extents.  `gmpi_selftest_division_launch` (C ABI, gmpi_abi.hip) compares this
// against the hardware-correct `/` on 2^32 operand pairs drawn from the renderer's ranges and on the edge
// pattern (tests/test_hip_parity.py::test_division_through_reciprocal_is_exact runs it), and
// tests/test_hip_parity.py::test_default_mode_samples_the_strict_texels checks the texel indices of the
// default mode against the strict-order mode (compiler division) on fuzzed poses.
__device__ __forceinline__ float div_by_recip(float n, float d, float r) {
    const float q0 = n * r;
    const float e = __builtin_fmaf(-d, q0, n);
    return __builtin_fmaf(e, r, q0);
}

// Same chain as plane_coord(), with the three divisions taken through reciprocals:
//   rrz = RN(1/ray_z) (per pixel), rw = RN(1/hw), rh = RN(1/hh) with hw = w/2, hh = h/2 (per plane).
//   (2x)/w == x/(w/2) exactly (power-of-two scaling), so u = x/hw.
template <bool AC>
__device__ __forceinline__ void plane_coord_recip(float zdiff, float hw, float hh, float rw, float rh, float ex, float ey,
                                                  float rx, float ry, float rz, float rrz, float cx, float cy, float& ix,
                                                  float& iy, float& s) {
    s = div_by_recip(zdiff, rz, rrz);
    const float tx = rx * s;
    const float ty = ry * s;
    const float x = ex + tx;
    const float y = ey + ty;
    float u = div_by_recip(x, hw, rw);
    float v = div_by_recip(y, hh, rh);
    if (AC) {
        const float u1 = u + 1.0f;
        const float v1 = v + 1.0f;
        ix = u1 * cx;
        iy = v1 * cy;
    } else {
        if (v >= -1.0f && v <= 1.0f) v = v * kNarrowScale;
        if (u >= -1.0f && u <= 1.0f) u = u * kNarrowScale;
        const float u1 = u + 1.0f;
        const float v1 = v + 1.0f;
        const float ux = u1 * cx;
        const float vy = v1 * cy;
        const float uxm = ux - 1.0f;
        const float vym = vy - 1.0f;
        ix = uxm * 0.5f;
        iy = vym * 0.5f;
    }
}

// Bilinear footprint: integer corner (clamped so that NaN / huge coordinates stay out of range) and
// the four weights nw, ne, sw, se in ATen's order.
struct Footprint {
    int x0, y0;
    float nw, ne, sw, se;
};

__device__ __forceinline__ Footprint footprint(float ix, float iy, int Ht, int Wt) {
    Footprint f;
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const float fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
    const float wx1 = ix - fx0, wx0 = fx1 - ix;
    const float wy1 = iy - fy0, wy0 = fy1 - iy;
    f.nw = wx0 * wy0;
    f.ne = wx1 * wy0;
    f.sw = wx0 * wy1;
    f.se = wx1 * wy1;
    f.x0 = (fx0 >= -2.0f && fx0 <= static_cast<float>(Wt)) ? static_cast<int>(fx0) : -2;
    f.y0 = (fy0 >= -2.0f && fy0 <= static_cast<float>(Ht)) ? static_cast<int>(fy0) : -2;
    return f;
}

// Composite state per pixel (mpi.py:421-434): T = running cumprod, C/Z the weighted sums.
struct Accum {
    float T = 1.0f, r = 0.0f, g = 0.0f, b = 0.0f, z = 0.0f;
};

// STRICT: exactly the oracle's op sequence.  Otherwise the blend uses FMA (fewer roundings; the
// difference is below 1e-6, everything after ix/iy is benign -- SURVEY.md section 7).
template <bool STRICT>
__device__ __forceinline__ float bilerp(float t_nw, float t_ne, float t_sw, float t_se, const Footprint& f) {
    if (STRICT) {
        float acc = t_nw * f.nw;
        acc = acc + t_ne * f.ne;
        acc = acc + t_sw * f.sw;
        acc = acc + t_se * f.se;
        return acc;
    } else {
        float acc = t_nw * f.nw;
        acc = __builtin_fmaf(t_ne, f.ne, acc);
        acc = __builtin_fmaf(t_sw, f.sw, acc);
        acc = __builtin_fmaf(t_se, f.se, acc);
        return acc;
    }
}

template <bool STRICT>
__device__ __forceinline__ void blend(Accum& A, float r, float g, float b, float a, float s, float dot) {
    if (STRICT) {
        const float dep = s * dot;          // mpi.py:150
        const float disp = 1.0f / dep;      // mpi.py:151
        const float depk = 1.0f / disp;     // mpi.py:411
        const float w = a * A.T;            // mpi.py:423
        A.r = A.r + w * r;                  // mpi.py:430
        A.g = A.g + w * g;
        A.b = A.b + w * b;
        A.z = A.z + w * depk;               // mpi.py:434
        float om = 1.0f - a;                // mpi.py:421
        om = om + 1e-10f;
        A.T = A.T * om;
    } else {
        // depth_k = s*dot (1/(1/x) == x to within an ulp); dot is constant per pixel, so sum w*s and scale once
        // at the end (finish_depth) -- depth tolerance is 1e-5, this moves it by a few 1e-7
        const float w = a * A.T;
        A.r = __builtin_fmaf(w, r, A.r);
        A.g = __builtin_fmaf(w, g, A.g);
        A.b = __builtin_fmaf(w, b, A.b);
        A.z = __builtin_fmaf(w, s, A.z);
        // (T - a*T would save an instruction but cancels behind nearly opaque planes: 1 - a is exact, a*T is not)
        float om = 1.0f - a;
        om = om + 1e-10f;
        A.T = A.T * om;
    }
}

template <bool STRICT>
__device__ __forceinline__ float finish_depth(const Accum& A, float dot) {
    return STRICT ? A.z : A.z * dot;
}

__device__ __forceinline__ bool in_unit(float v) { return v >= 0.0f && v <= 1.0f; }

// Direct-from-global bilinear sample of the 4 channels of one plane (zeros padding): clamp the
// address, zero the weight of a tap that lies outside the texture.  `pl` points at channel 0.
template <typename TexT, bool STRICT>
__device__ __forceinline__ void gather_sample(const TexT* __restrict__ pl, int64_t s_chan, int64_t s_row, int Ht, int Wt,
                                              float ix, float iy, bool check_range, uint32_t& bad, float (&smp)[4]) {
    Footprint f = footprint(ix, iy, Ht, Wt);
    const bool x0in = f.x0 >= 0 && f.x0 <= Wt - 1, x1in = f.x0 >= -1 && f.x0 <= Wt - 2;
    const bool y0in = f.y0 >= 0 && f.y0 <= Ht - 1, y1in = f.y0 >= -1 && f.y0 <= Ht - 2;
    if (!(x0in && y0in)) f.nw = 0.0f;
    if (!(x1in && y0in)) f.ne = 0.0f;
    if (!(x0in && y1in)) f.sw = 0.0f;
    if (!(x1in && y1in)) f.se = 0.0f;
    const int xa = min(max(f.x0, 0), Wt - 1), xb = min(max(f.x0 + 1, 0), Wt - 1);
    const int ya = min(max(f.y0, 0), Ht - 1), yb = min(max(f.y0 + 1, 0), Ht - 1);
    const int64_t oa = static_cast<int64_t>(ya) * s_row, ob = static_cast<int64_t>(yb) * s_row;
    if constexpr (std::is_same_v<TexT, rgba8_t>) {   // one load per tap; every code is in [0, 1]: nothing for check_range to test
        const uint32_t t_nw = load_texel(pl, oa + 4 * xa), t_ne = load_texel(pl, oa + 4 * xb);
        const uint32_t t_sw = load_texel(pl, ob + 4 * xa), t_se = load_texel(pl, ob + 4 * xb);
#pragma unroll
        for (int c = 0; c < 4; ++c)   // to_f32(u8_t) per tap, as the planar instance: the same bits
            smp[c] = bilerp<STRICT>(unorm8_to_f32(texel_code(t_nw, c)), unorm8_to_f32(texel_code(t_ne, c)), unorm8_to_f32(texel_code(t_sw, c)),
                                    unorm8_to_f32(texel_code(t_se, c)), f);
    } else if constexpr (is_float_texel<TexT>) {   // float layers: one load per tap of the whole texel, then the planar instance's arithmetic per channel
        constexpr int64_t kTexel = sizeof(TexT);
        const TexT t_nw = load_texel(pl, oa + kTexel * xa), t_ne = load_texel(pl, oa + kTexel * xb);
        const TexT t_sw = load_texel(pl, ob + kTexel * xa), t_se = load_texel(pl, ob + kTexel * xb);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float c_nw = to_f32(t_nw.c[c]), c_ne = to_f32(t_ne.c[c]), c_sw = to_f32(t_sw.c[c]), c_se = to_f32(t_se.c[c]);
            if (check_range && !(in_unit(c_nw) && in_unit(c_ne) && in_unit(c_sw) && in_unit(c_se))) bad |= GMPI_STATUS_RGBA_RANGE;
            smp[c] = bilerp<STRICT>(c_nw, c_ne, c_sw, c_se, f);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const TexT* __restrict__ ch = pl + c * s_chan;
            const float t_nw = to_f32(ch[oa + xa]);
            const float t_ne = to_f32(ch[oa + xb]);
            const float t_sw = to_f32(ch[ob + xa]);
            const float t_se = to_f32(ch[ob + xb]);
            if (check_range && !(in_unit(t_nw) && in_unit(t_ne) && in_unit(t_sw) && in_unit(t_se))) bad |= GMPI_STATUS_RGBA_RANGE;
            smp[c] = bilerp<STRICT>(t_nw, t_ne, t_sw, t_se, f);
        }
    }
}

// ---- the Shade policy: the shaded render of an RGBA volume (GmpiShading, include/gmpi_render.h; render_shaded.hip) --------------------------------
// The kernels that take it sample the volume clip(rgb * shading, 0, 1) | alpha without anybody building it: every colour tap is shaded where it is
// fetched, with the shading texel of the SAME position (one image per MPI), the alpha tap is raw.  NoShade -- the default of every body that takes the
// policy (render_backward.hip) -- is a compile-time nothing: the kernels of old.  shade_texel is light_apply_kernel's arithmetic (one
// rounding for the product; fmaxf drops a NaN: a NaN colour texel is shaded to 0).
struct NoShade {};
struct ShadeK {
    const float* s;          // [M,1,Ht,Wt]
    int64_t s_mpi, s_row;
};
__device__ __forceinline__ float shade_texel(float t, float s) { return fminf(fmaxf(t * s, 0.0f), 1.0f); }

// gather_sample of the shaded volume: the same footprint, addresses, zeroed weights and bilerp, the 12 colour taps shaded with the four shading taps of
// the footprint.  check_range tests the alpha taps only: a shaded colour is in [0, 1] by construction.  sh: the MPI's shading image.
template <typename TexT, bool STRICT>
__device__ __forceinline__ void shaded_gather_sample(const TexT* __restrict__ pl, int64_t s_chan, int64_t s_row, const float* __restrict__ sh, int64_t sh_row,
                                                     int Ht, int Wt, float ix, float iy, bool check_range, uint32_t& bad, float (&smp)[4]) {
    Footprint f = footprint(ix, iy, Ht, Wt);
    const bool x0in = f.x0 >= 0 && f.x0 <= Wt - 1, x1in = f.x0 >= -1 && f.x0 <= Wt - 2;
    const bool y0in = f.y0 >= 0 && f.y0 <= Ht - 1, y1in = f.y0 >= -1 && f.y0 <= Ht - 2;
    if (!(x0in && y0in)) f.nw = 0.0f;
    if (!(x1in && y0in)) f.ne = 0.0f;
    if (!(x0in && y1in)) f.sw = 0.0f;
    if (!(x1in && y1in)) f.se = 0.0f;
    const int xa = min(max(f.x0, 0), Wt - 1), xb = min(max(f.x0 + 1, 0), Wt - 1);
    const int ya = min(max(f.y0, 0), Ht - 1), yb = min(max(f.y0 + 1, 0), Ht - 1);
    const int64_t oa = static_cast<int64_t>(ya) * s_row, ob = static_cast<int64_t>(yb) * s_row;
    const int64_t ha = static_cast<int64_t>(ya) * sh_row, hb = static_cast<int64_t>(yb) * sh_row;
    const float s_nw = sh[ha + xa], s_ne = sh[ha + xb], s_sw = sh[hb + xa], s_se = sh[hb + xb];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const TexT* __restrict__ ch = pl + c * s_chan;
        float t_nw = to_f32(ch[oa + xa]);
        float t_ne = to_f32(ch[oa + xb]);
        float t_sw = to_f32(ch[ob + xa]);
        float t_se = to_f32(ch[ob + xb]);
        if (c < 3) {
            t_nw = shade_texel(t_nw, s_nw), t_ne = shade_texel(t_ne, s_ne), t_sw = shade_texel(t_sw, s_sw), t_se = shade_texel(t_se, s_se);
        } else if (check_range && !(in_unit(t_nw) && in_unit(t_ne) && in_unit(t_sw) && in_unit(t_se))) {
            bad |= GMPI_STATUS_RGBA_RANGE;
        }
        smp[c] = bilerp<STRICT>(t_nw, t_ne, t_sw, t_se, f);
    }
}

// ---- the forward's frame: what every render kernel does around its plane loop.  A change here reaches all of them, and
//      the backward sweeps (gmpi_backward.hpp), which read the same view constants and the same dot product.  View / view_setup, check_camera_behind,
//      ray_dot, last_plane / leaves_last_plane, gather_plane, store_pixel; then the tile frame of the staged tile kernels: view_group_items, fwd_tile_id /
//      fwd_tile / fwd_tile_grid, tile_lane / tile_corners, corner_extent / item_box / tile_box, origin_words / origin_rsrc. ---------------------------
// What is uniform over view n.  Everything is forced inline: a field a kernel does not read costs it nothing.
struct View {
    int m;                          // the MPI the view samples
    const float* __restrict__ dhw;  // its plane table [D, 3]
    float ex, ey, ez;               // eye
    float zx, zy, zz;               // optical axis
    float cx, cy;                   // plane_coord's texture constants: (Wt - 1) / 2, (Ht - 1) / 2 (align_corners) or Wt, Ht
    int64_t HW;
    const float* __restrict__ rays; // ray_dir of the view: [3, H W]
};
template <bool AC>
__device__ __forceinline__ View view_setup(const KParams& p, int n, uint32_t& bad) {
    View vw;
    vw.m = view_mpi(p, n, bad);  // (an index outside [0, M) is clamped and reported)
    vw.dhw = p.dhw + static_cast<int64_t>(vw.m) * p.D * 3;
    vw.ex = p.eye_pos[3 * n + 0], vw.ey = p.eye_pos[3 * n + 1], vw.ez = p.eye_pos[3 * n + 2];
    vw.zx = p.z_dir[3 * n + 0], vw.zy = p.z_dir[3 * n + 1], vw.zz = p.z_dir[3 * n + 2];
    vw.cx = AC ? static_cast<float>(p.Wt - 1) * 0.5f : static_cast<float>(p.Wt);
    vw.cy = AC ? static_cast<float>(p.Ht - 1) * 0.5f : static_cast<float>(p.Ht);
    vw.HW = static_cast<int64_t>(p.H) * p.W;
    vw.rays = p.ray_dir + static_cast<int64_t>(n) * 3 * vw.HW;
    return vw;
}

// mpi.py:70-72 compares every plane distance of the view's MPI with eye_z of the FIRST view ("Camera must be placed closer...").  The caller
// says which one lane of the view runs it (`once`).
__device__ __forceinline__ void check_camera_behind(const KParams& p, const View& vw, bool once) {
    if (p.status != nullptr && once) {
        const float ez0 = p.eye_pos[2];
        bool behind = false;
        for (int k = 0; k < p.D; ++k) behind |= !(vw.dhw[3 * k] >= ez0);
        if (behind) atomicOr(p.status, GMPI_STATUS_CAMERA_BEHIND_PLANE);
    }
}

// ray . z_dir in the association of einsum("nchw,nc->nhw") (mpi.py:149): depth_k = s_k dot
__device__ __forceinline__ float ray_dot(const View& vw, float rx, float ry, float rz) {
    float dot = rx * vw.zx;
    dot = dot + ry * vw.zy;
    dot = dot + rz * vw.zz;
    return dot;
}

__device__ __forceinline__ bool outside_pm1(float u, float v) { return !(u >= -1.0f && u <= 1.0f && v >= -1.0f && v <= 1.0f); }

// assert_not_out_of_last_plane (mpi.py:381-395, 103-109), once per pixel in the epilogue: whether the launch asks for it (GMPI_FLAG_CHECK_LAST_PLANE)
// and plane D - 1, read once per thread; then per pixel whether its u, v on that plane leave [-1, 1].
struct LastPlane {
    bool check;
    float d, ph, pw;
};
__device__ __forceinline__ LastPlane last_plane(const KParams& p, const View& vw) {
    LastPlane lp{(p.flags & GMPI_FLAG_CHECK_LAST_PLANE) != 0, 0.0f, 1.0f, 1.0f};
    if (lp.check) lp.d = vw.dhw[3 * (p.D - 1) + 0], lp.ph = vw.dhw[3 * (p.D - 1) + 1], lp.pw = vw.dhw[3 * (p.D - 1) + 2];
    return lp;
}
template <bool AC>
__device__ __forceinline__ bool leaves_last_plane(const View& vw, const LastPlane& lp, float rx, float ry, float rz) {
    if (!lp.check) return false;
    float ix, iy, s, u, v;
    plane_coord<AC>(lp.d - vw.ez, lp.ph, lp.pw, vw.ex, vw.ey, rx, ry, rz, vw.cx, vw.cy, ix, iy, s, u, v);
    return outside_pm1(u, v);
}

// One plane for one pixel straight from global memory: the gather kernel's loop body and the staged kernels' last resort (a box that does not
// fit).  `vol` points at channel 0 of plane 0 of the view's MPI; (zdiff, ph, pw) = (d - eye_z, height, width) of plane k.  check_range: a bool, or std::bool_constant where
// the range check is a template parameter of the kernel (the band kernel: as a run-time value it moves that kernel's registers).
template <typename TexT, bool AC, bool STRICT, typename CheckT>
__device__ __forceinline__ void gather_plane(const KParams& p, const View& vw, const TexT* vol, int k, float zdiff, float ph, float pw,
                                             float rx, float ry, float rz, float dot, CheckT check_range, uint32_t& bad, Accum& A) {
    float ix, iy, s, u, v, smp[4];
    plane_coord<AC>(zdiff, ph, pw, vw.ex, vw.ey, rx, ry, rz, vw.cx, vw.cy, ix, iy, s, u, v);
    gather_sample<TexT, STRICT>(tex_offset(vol, static_cast<int64_t>(k) * p.s_plane), p.s_chan, p.s_row, p.Ht, p.Wt, ix, iy, check_range, bad, smp);
    blend<STRICT>(A, smp[0], smp[1], smp[2], smp[3], s, dot);
}

// The carry of a plane-chunked render: the composite is associative over the plane axis, and the raw Accum of a pixel after the planes so far -- channels
// r, g, b, z, T of state [N, 5, H, W]; colour in [0, 1], z in the mode's own form (STRICT: sum w depth_k; default: sum w s_k, before finish_depth's factor)
// -- is all that passes from one plane range to the next.  A launch that starts from the loaded Accum and runs blend() over its planes performs, per
// pixel, exactly the operations the one-shot launch performs over those planes: same bits.  A lane reads and writes only its own pixel, so state_in ==
// state_out is fine (a lane outside the image shadows a neighbour's pixel and may see it half-written: its result is never stored).
__device__ __forceinline__ Accum load_carry(NoCarry, int, int64_t, int64_t) { return Accum{}; }
__device__ __forceinline__ void store_carry(NoCarry, int, int64_t, int64_t, const Accum&, bool) {}
__device__ __forceinline__ Accum load_carry(const CarryK& c, int n, int64_t HW, int64_t pix) {
    Accum A;
    if (c.state_in != nullptr) {
        const float* s = c.state_in + static_cast<int64_t>(n) * 5 * HW + pix;
        A.r = s[0], A.g = s[HW], A.b = s[2 * HW], A.z = s[3 * HW], A.T = s[4 * HW];
    }
    return A;
}
__device__ __forceinline__ void store_carry(const CarryK& c, int n, int64_t HW, int64_t pix, const Accum& A, bool active) {
    if (c.state_out != nullptr && active) {
        float* s = c.state_out + static_cast<int64_t>(n) * 5 * HW + pix;
        s[0] = A.r, s[HW] = A.g, s[2 * HW] = A.b, s[3 * HW] = A.z, s[4 * HW] = A.T;
    }
}

// The pixel's results: colour ([0, 1], or 2 c - 1 with GMPI_FLAG_OUT_PM1: mpi_renderer.py:467), depth, transmittance if wanted.  (2 c - 1 is
// formed before the `active` test on purpose: the 16-bit tile kernels sit at their register cap and the other order moves their spills.)
// With a CarryK (the carry instances): the state goes out first, and rgb_out / depth_out may each be nullptr -- a chunk that is not the last wants neither.
template <bool STRICT, typename Carry = NoCarry>
__device__ __forceinline__ void store_pixel(const KParams& p, int n, int64_t HW, int64_t pix, const Accum& A, float dot, bool active, const Carry& carry = Carry{}) {
    constexpr bool CARRY = std::is_same_v<Carry, CarryK>;
    float r = A.r, g = A.g, b = A.b;
    if (p.flags & GMPI_FLAG_OUT_PM1) {
        r = 2.0f * r - 1.0f;
        g = 2.0f * g - 1.0f;
        b = 2.0f * b - 1.0f;
    }
    if constexpr (CARRY) {
        store_carry(carry, n, HW, pix, A, active);
        if (active && p.rgb_out != nullptr) {
            float* out = p.rgb_out + static_cast<int64_t>(n) * 3 * HW + pix;
            out[0] = r, out[HW] = g, out[2 * HW] = b;
        }
        if (active && p.depth_out != nullptr) p.depth_out[static_cast<int64_t>(n) * HW + pix] = finish_depth<STRICT>(A, dot);
        if (active && p.T_out != nullptr) p.T_out[static_cast<int64_t>(n) * HW + pix] = A.T;
        return;
    }
    if (active) {
        float* __restrict__ out = p.rgb_out + static_cast<int64_t>(n) * 3 * HW + pix;
        out[0] = r;
        out[HW] = g;
        out[2 * HW] = b;
        p.depth_out[static_cast<int64_t>(n) * HW + pix] = finish_depth<STRICT>(A, dot);
        if (p.T_out) p.T_out[static_cast<int64_t>(n) * HW + pix] = A.T;
    }
}

// ---- the tile frame: a workgroup of TW x TH lanes owns a TW x TH pixel tile, one pixel per lane, and stages per plane the texel box spanned by the
//      tile's four corner pixels (render_lds.hip has the why).  ONE text for the four forward tile kernels (render_lds, render_u8, render_shared_forward,
//      render_depth_window) and, through tile_lane / tile_corners / tile_box, for the tile backwards (gmpi_backward.hpp, render_backward.hip). ---------
// Work items of one group of views that share an MPI (xcd_item_per_group's group_items), `per_view` items per view.
inline __host__ __device__ int view_group_items(const KParams& p, int per_view) { return per_view * (p.view_to_mpi == nullptr ? p.views_per_mpi : 1); }

// blockIdx -> tile id: every XCD gets a contiguous run of the tiles of every group of views that share an MPI; n_tiles and above: a padding workgroup.
__device__ __forceinline__ int fwd_tile_id(const KParams& p, int block, int tiles_x, int tiles_y, int n_tiles, int rot = 0, int split = 1) {
    return xcd_item_per_group(block, view_group_items(p, tiles_x * tiles_y), n_tiles, rot, split);
}
// tile id -> view n, position `rem` inside the view (0: the tile that runs check_camera_behind), tile column and row; views that share one MPI are
// interleaved per tile position (item_to_view).  false: a padding workgroup, which returns as a whole.
struct FwdTile { int n, rem, txi, tyi; };
__device__ __forceinline__ bool fwd_tile(const KParams& p, int tile_id, int tiles_x, int tiles_y, int n_tiles, FwdTile& t) {
    if (tile_id >= n_tiles) return false;
    item_to_view(p, tile_id, tiles_x * tiles_y, t.n, t.rem);
    t.tyi = t.rem / tiles_x, t.txi = t.rem - t.tyi * tiles_x;
    return true;
}
// host side: what fwd_tile_id expects of the launch
struct FwdTileGrid { int tiles_x, tiles_y, n_tiles; dim3 grid; };
template <int TW, int TH>
inline FwdTileGrid fwd_tile_grid(const KParams& p) {
    const int tiles_x = (p.W + TW - 1) / TW, tiles_y = (p.H + TH - 1) / TH, n_tiles = tiles_x * tiles_y * p.N;
    return FwdTileGrid{tiles_x, tiles_y, n_tiles, dim3(xcd_grid_per_group(view_group_items(p, tiles_x * tiles_y), n_tiles))};
}

// The pixel of lane `lane` of tile (txi, tyi): lanes outside the image shadow the last row / column (pix is clamped, `active` says so).
struct TileLane { int px, py; bool active; int64_t pix; };
template <int TW, int TH>
__device__ __forceinline__ TileLane tile_lane(int txi, int tyi, int lane, int W, int H) {
    TileLane l;
    l.px = txi * TW + (lane % TW), l.py = tyi * TH + (lane / TW);
    l.active = l.px < W && l.py < H;
    l.pix = static_cast<int64_t>(min(l.py, H - 1)) * W + min(l.px, W - 1);
    return l;
}
// The tile's corner pixels, clamped into the image.
struct TileCorners { int cx0, cx1, cy0, cy1; };
template <int TW, int TH>
__device__ __forceinline__ TileCorners tile_corners(int txi, int tyi, int W, int H) {
    const int cx0 = txi * TW, cy0 = tyi * TH;
    return TileCorners{cx0, min(cx0 + TW - 1, W - 1), cy0, min(cy0 + TH - 1, H - 1)};
}

// The pixels (cx0, cy0), (cx1, cy0), (cx0, cy1), (cx1, cy1) map to (cix, ciy)[0..3] on one plane (the exact chain; rdv = the view's rays): their extent,
// and whether all of them are finite (below 1e6: false for NaN too).  A pinhole ray field maps pixel lines to lines, so every tap of the pixel rectangle
// lies in that extent grown by the 2 x 2 support.
struct CornerExtent { float mnx, mxx, mny, mxy; bool finite; };
template <bool AC>
__device__ __forceinline__ CornerExtent corner_extent(const View& vw, const float* __restrict__ rdv, int W, float zdiff, float ph, float pw, int cx0, int cx1,
                                                      int cy0, int cy1, float (&cix)[4], float (&ciy)[4]) {
    CornerExtent e{__builtin_inff(), -__builtin_inff(), __builtin_inff(), -__builtin_inff(), true};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int64_t q = static_cast<int64_t>((c & 2) ? cy1 : cy0) * W + ((c & 1) ? cx1 : cx0);
        float s, u, v;
        plane_coord<AC>(zdiff, ph, pw, vw.ex, vw.ey, rdv[q], rdv[vw.HW + q], rdv[2 * vw.HW + q], vw.cx, vw.cy, cix[c], ciy[c], s, u, v);
        e.finite = e.finite && (fabsf(cix[c]) < 1e6f) && (fabsf(ciy[c]) < 1e6f);
        e.mnx = fminf(e.mnx, cix[c]), e.mxx = fmaxf(e.mxx, cix[c]), e.mny = fminf(e.mny, ciy[c]), e.mxy = fmaxf(e.mxy, ciy[c]);
    }
    return e;
}
template <bool AC>
__device__ __forceinline__ CornerExtent corner_extent(const View& vw, const float* __restrict__ rdv, int W, float zdiff, float ph, float pw, int cx0, int cx1,
                                                      int cy0, int cy1) {
    float cix[4], ciy[4];
    return corner_extent<AC>(vw, rdv, W, zdiff, ph, pw, cx0, cx1, cy0, cy1, cix, ciy);
}
// Extent -> staged box (x0, y0, items per row, rows) in loader items of TPI texels: grown by kBoxSlack (the fp32 error of ix is < 1e-3 texel) and the
// 2 x 2 support, x0 aligned down to an item.  `fits`: within max_cols items x max_rows rows; how "not staged" is written is the caller's.  An extent
// that is not finite gives four zeros and does not fit.
constexpr float kBoxSlack = 1.0f / 64;
template <int TPI>
__device__ __forceinline__ int4 item_box(const CornerExtent& e, int max_cols, int max_rows, bool& fits) {
    int4 bb = make_int4(0, 0, 0, 0);
    fits = false;
    if (e.finite) {
        const int bx0 = static_cast<int>(floorf(e.mnx - kBoxSlack)), bx1 = static_cast<int>(floorf(e.mxx + kBoxSlack)) + 1;   // first and last texel column
        const int by0 = static_cast<int>(floorf(e.mny - kBoxSlack)), by1 = static_cast<int>(floorf(e.mxy + kBoxSlack)) + 1;
        bb.x = bx0 & ~(TPI - 1), bb.y = by0;
        bb.z = (bx1 - bb.x) / TPI + 1, bb.w = by1 - by0 + 1;
        fits = bb.z <= max_cols && bb.w <= max_rows;
    }
    return bb;
}
// Texel box of a pixel tile on one plane, in texels: (bx0, by0, nx, ny); nx = 0: not staged -- the corner images are not finite (all four fields 0) or
// the box exceeds pitch x rows.
template <bool AC>
__device__ __forceinline__ int4 tile_box(const KParams& p, const View& vw, const float* __restrict__ rdv, float zdiff, float ph, float pw, int cx0, int cx1,
                                         int cy0, int cy1, int pitch, int rows, float (&cix)[4], float (&ciy)[4]) {
    bool fits;
    int4 bb = item_box<1>(corner_extent<AC>(vw, rdv, p.W, zdiff, ph, pw, cx0, cx1, cy0, cy1, cix, ciy), pitch, rows, fits);
    if (!fits) bb.z = 0;
    return bb;
}
template <bool AC>
__device__ __forceinline__ int4 tile_box(const KParams& p, const View& vw, const float* __restrict__ rdv, float zdiff, float ph, float pw, int cx0, int cx1,
                                         int cy0, int cy1, int pitch, int rows) {
    float cix[4], ciy[4];
    return tile_box<AC>(p, vw, rdv, zdiff, ph, pw, cx0, cx1, cy0, cy1, pitch, rows, cix, ciy);
}

// A box origin's address in the per-plane table: two words (48 bits) = words 0, 1 of the plane's raw-buffer descriptor; and the descriptor rebuilt from
// them.  It must be PROVABLY wave-uniform or hipcc wraps every buffer op in a waterfall loop: its inputs go through readfirstlane.  num_records 2^31:
// only the explicit out-of-range offset 0x80000000 is rejected (reads as zero without touching memory).
__device__ __forceinline__ int2 origin_words(uint64_t a) { return make_int2(static_cast<int>(a & 0xffffffffu), static_cast<int>((a >> 32) & 0xffffu)); }
__device__ __forceinline__ __amdgpu_buffer_rsrc_t origin_rsrc(int lo, int hi) {
    const uint32_t b_lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(lo)), b_hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(hi));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>((static_cast<uint64_t>(b_hi) << 32) | b_lo), 0, static_cast<int>(0x80000000u), 0x00020000);
}

// floor(x) as an integer in one instruction (v_cvt_flr_i32_f32); NaN -> 0, saturating
__device__ __forceinline__ int floor_to_int(float x) {
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// OR a per-lane flag word into status[0] with at most one atomic per wave.
__device__ __forceinline__ void report_status(uint32_t* status, uint32_t bad) {
    if (status == nullptr) return;
    if (__any(bad != 0u)) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o);
        if ((threadIdx.x + threadIdx.y * blockDim.x) % 64 == 0) atomicOr(status, bad);
    }
}

}  // namespace gmpi
