/*
 * gmpi_render.h -- C ABI of the MI355X-native multiplane-image (MPI) renderer.
 *
 * This is the drop-in boundary for ONE path of apple/ml-gmpi: the gmpi/core renderer
 *   homography()          gmpi/core/mpi.py:26-153     (ray/plane intersection + F.grid_sample)
 *   MPI.forward()         gmpi/core/mpi.py:308-436    (front-to-back over-compositing, depth)
 *   MPIRenderer.render()  gmpi/core/mpi_renderer.py:387-469 (range asserts, [0,1] -> [-1,1])
 * The reference has no native entry point for this path (its only native code is the
 * generator's bias_act/upfirdn2d pybind plugins, gmpi/models/torch_utils/ops/bias_act.cpp:94-97,
 * whose convention -- one POD parameter struct, launch on the caller's stream -- is mirrored
 * here).  Everything below is plain C: pointers, sizes, no torch types.  A Python host binds it
 * with ctypes (ml-gmpi_amd/_lib.py); INTEGRATION.md shows the stub a reference maintainer adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller; the library never allocates or
 *     frees device memory and never synchronises the stream;
 *   - every entry point returns 0 or a negative GMPI_E_* code; it never throws and never exits
 *     (the reference's `sys.exit(1)` on a ray leaving the last plane, mpi.py:105-128, becomes a
 *     status bit the host turns into the same diagnostics);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - re-entrant; no global state that a result depends on (the only process-wide datum is an atomic launch counter that stamps the view
 *     gate words of GMPI_VARIANT_AUTO's two-kernel launches, so that a workspace never needs clearing).
 */
#ifndef GMPI_RENDER_H
#define GMPI_RENDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMPI_ABI_VERSION 2

/* storage type of the RGBA volume; arithmetic is always fp32 (mpi_renderer.py:446 `.float()`).
 * GMPI_DTYPE_U8: 8 bits per channel, code c in 0..255 stands for the fp32 value c / 255 (the correctly rounded quotient): rendering such a volume
 * is by definition rendering that fp32 volume.  gmpi_mpi_render_launch and gmpi_render_workspace_bytes take it; every other entry returns
 * GMPI_E_DTYPE for it (no gradients, no shared-colour layout, no shading, no range pass: every code is in [0, 1]). */
enum { GMPI_DTYPE_F32 = 0, GMPI_DTYPE_BF16 = 1, GMPI_DTYPE_F16 = 2, GMPI_DTYPE_U8 = 3 };

/* GmpiRenderParams.flags */
enum {
    GMPI_FLAG_ALIGN_CORNERS = 1 << 0,    /* MPI(align_corners=...)            mpi.py:157-159, 86-99    */
    GMPI_FLAG_OUT_PM1 = 1 << 1,          /* write 2*C-1 instead of C          mpi_renderer.py:467      */
    GMPI_FLAG_CHECK_LAST_PLANE = 1 << 2, /* assert_not_out_of_last_plane      mpi.py:381-395, 103-109  */
    GMPI_FLAG_CHECK_RANGE = 1 << 3,      /* rgba/alpha in [0,1] (mpi.py:185-187, mpi_renderer.py:447-449) on AT LEAST the texels the render
                                            SAMPLES (the taps with which some pixel forms its bilinear sample); a kernel may test more:
                                              band kernel (GMPI_VARIANT_BAND, AUTO's large launches): exactly the sampled taps (the landed tap
                                                registers are folded into a running maximum);
                                              tile / strip kernels (LDS, WAVE): every texel of the boxes they stage -- the sampled taps plus
                                                the 16-byte items and box rows around them;
                                              gather kernel: exactly the sampled taps.
                                            STATUS_RGBA_RANGE therefore never reports a texel in [0,1], always reports an out-of-range or
                                            NaN texel that some pixel samples, and MAY miss one that no pixel samples (outside every view's
                                            footprint: 10-16 % of a volume) -- which the reference, testing min/max of the whole tensor,
                                            reports.  The exhaustive test is gmpi_rgba_range_check_launch (one streaming pass); the Python
                                            host runs it with range_check="full" (install()'s default) once per unchanged volume.        */
    GMPI_FLAG_STRICT_ORDER = 1 << 4,     /* one rounding per reference op everywhere (bit-identical to
                                            oracle/mpi_oracle.c); default lets the blend use FMA       */
    GMPI_FLAG_HINT_FRONTAL = 1 << 5,     /* advisory: every view's camera axis (z_dir) is within 0.2 rad of the MPI normal (0,0,1).
                                            Only GMPI_VARIANT_AUTO reads it, and only to choose between kernels that render the
                                            same pixels: the strip kernel's narrow boxes win on small frontal launches, the tile
                                            kernel's shared boxes on tilted ones (profiles/r03_pose_sweep.txt).  Results never
                                            depend on it; without it AUTO assumes a tilted camera.                              */
    GMPI_FLAG_HINT_TILTED = 1 << 6,      /* advisory (round 4), the other end: SOME view's camera axis is more than 0.53 rad off the MPI normal
                                            (the 2-sigma corner of the FFHQ / MetFaces pose range).  The strip kernel's wave-private boxes
                                            overflow there -- config 2 takes 0.25-0.77 ms instead of 0.16 -- while the tile kernel stays at
                                            0.21 (profiles/r04_pose_distribution.txt): AUTO keeps such fp32 launches of 1537-2048 strips (the
                                            window that was measured: config 2) off the strip kernel, and (round 5) 16-bit launches of 256-511
                                            bands of 256 x 8 pixels off the band kernel's two-kernel path (a view it cannot stage costs such a
                                            small launch ~18 us of table kernel and empty launches); launches of up to 512 strips stay with the
                                            strip kernel whatever the hint (its 6-way plane split still wins there).  Like
                                            GMPI_FLAG_HINT_FRONTAL it never changes a result.                                                */
    GMPI_FLAG_GRAD_OVERWRITE = 1 << 7,   /* gmpi_mpi_render_backward_launch (round 6; and the layouts' _backward_gather_launch entries, which say what it
                                            means there): the caller does not need what grad_rgba holds.
                                            With the workspace gmpi_render_backward_workspace_bytes asks for, the launch then WRITES every element
                                            of grad_rgba (no zero-fill needed); without the flag it reads, adds and writes back.  On the tile-kernel
                                            path (no workspace, or a launch the gather path does not take) the flag changes nothing: that path only
                                            ever ADDS, and the caller zero-fills as before.                                                      */
    GMPI_FLAG_HINT_OBLIQUE = 1 << 8,     /* advisory (round 6), between the two: SOME view's camera axis is more than 0.35 rad off the MPI normal.  Read (a) like
                                            GMPI_FLAG_HINT_TILTED for 16-bit launches of 256-511 bands of 256 x 8 pixels (kept off the band kernel's two-kernel path), and (b) for
                                            launches whose views SHARE MPIs (views_per_mpi > 1: camera paths over one MPI) and that are large enough (from 1024 bands of 256 x 8 pixels
                                            over a 16-bit volume, 2048 of 128 x 8 over an fp32 one: 8 views of 512^2): without it GMPI_VARIANT_AUTO renders
                                            them with the band kernel -- 9 % (fp32) to 20 % (16-bit volumes) faster than the tile kernel when every view's texel
                                            boxes fit its buffers, which cameras up to 0.35 rad do at 512^2 (and further out on larger images) -- and, when the device finds a view that does not
                                            fit, hands that view's whole group of views to the tile kernel (a table kernel and an empty band launch, ~20 us, for
                                            nothing); with it such launches go to the tile kernel at once, as in rounds 1-5.  GMPI_FLAG_HINT_TILTED implies it.
                                            Never changes a result.                                                                                           */
    GMPI_FLAG_ALL = (1 << 9) - 1         /* every defined bit; any other bit -> GMPI_E_FLAGS            */
};

/* bits of status[0] (OR-accumulated across launches until the caller clears the word) */
enum {
    GMPI_STATUS_OUT_OF_LAST_PLANE = 1u << 0, /* mpi.py:106-109 would have failed                      */
    GMPI_STATUS_RGBA_RANGE = 1u << 1,        /* mpi.py:185-187 / mpi_renderer.py:447-449              */
    GMPI_STATUS_CAMERA_BEHIND_PLANE = 1u << 2, /* mpi.py:70-72 "Camera must be placed closer..."     */
    GMPI_STATUS_BAD_VIEW_INDEX = 1u << 3      /* view_to_mpi[n] outside [0, M): clamped and reported   */
};
#define GMPI_STATUS_WORDS 4

/* kernel selection (GmpiRenderParams.variant) */
enum {
    GMPI_VARIANT_AUTO = 0,
    GMPI_VARIANT_GATHER = 1, /* one pixel per lane, taps straight from global memory (any shape/stride) */
    GMPI_VARIANT_LDS = 2,    /* pixel tiles, texel boxes staged through LDS with 16-byte row loads      */
    GMPI_VARIANT_WAVE = 3,   /* wave-private 32x8 pixel strips, whole RGBA texels (fp32 / fp16) in LDS  */
    GMPI_VARIANT_DMA = 4,    /* RETIRED (round 4): reserved, refused with GMPI_E_VARIANT; gmpi_query(7) == 0            */
    GMPI_VARIANT_BAND = 5    /* 256 x 8 (bf16, fp16) / 128 x 8 (fp32) pixel bands, LDS-DMA loader; needs the workspace         */
};

enum {
    GMPI_OK = 0,
    GMPI_E_NULL = -1,        /* required pointer is NULL                      */
    GMPI_E_SHAPE = -2,       /* non-positive / inconsistent extent; N > 65535 views for the gather kernel
                                or the backward (split the batch)             */
    GMPI_E_DTYPE = -3,       /* unknown rgba_dtype, or one this entry does not take (GMPI_DTYPE_U8 anywhere but the forward) */
    GMPI_E_STRIDE = -4,      /* innermost rgba stride != 1 or negative stride */
    GMPI_E_ABI = -5,         /* struct_size does not match this library       */
    GMPI_E_VARIANT = -6,     /* requested kernel variant cannot run this shape */
    GMPI_E_FLAGS = -7,       /* a bit outside GMPI_FLAG_ALL is set            */
    GMPI_E_WORKSPACE = -8,   /* the workspace is missing, too small or not 256-byte aligned */
    GMPI_E_LAUNCH = -100     /* -100 - hipError_t of the failed launch        */
};

/*
 * One render call = MPI.forward (mpi.py:308-436) [+ the epilogue of MPIRenderer.render].
 *
 *   N views, M multiplane images, D planes per MPI (plane 0 nearest, mpi.py:413).
 *   View n samples MPI  view_to_mpi[n]  (or n / views_per_mpi when view_to_mpi is NULL); this
 *   replaces the reference's expand+cat of the volume per view (mpi.py:331-346) -- the volume is
 *   never replicated.
 */
typedef struct GmpiRenderParams {
    uint32_t struct_size; /* = sizeof(GmpiRenderParams) */
    uint32_t flags;       /* GMPI_FLAG_*                */
    int32_t variant;      /* GMPI_VARIANT_*             */
    int32_t rgba_dtype;   /* GMPI_DTYPE_*               */

    int32_t N, M, D;         /* views, MPIs, planes                                   */
    int32_t Ht, Wt;          /* texture height/width (texels)                          */
    int32_t H, W;            /* rendered image height/width (pixels)                   */
    int32_t views_per_mpi;   /* used when view_to_mpi == NULL (>=1)                    */

    const void *rgba;        /* [M, D, 4, Ht, Wt] planar RGBA in [0,1]                 */
    int64_t rgba_stride[5];  /* element strides; [4] must be 1; 0 allowed on [0] (expand).  One exception, for GMPI_DTYPE_U8 at the forward launch and
                                its workspace query: the channels-last ("interleaved") layout of 8-bit images, [M, D, Ht, Wt, 4] in memory seen as
                                [M, D, 4, Ht, Wt]: [2] == 1 and [4] == 4 with [3] >= 4 Wt (one RGBA texel = 4 consecutive bytes; the strides count
                                bytes; [0] and [1] as ever).  [4] == 4 with any other dtype or channel stride, and any other texel stride, is
                                GMPI_E_STRIDE.                                                                                                   */
    const int32_t *view_to_mpi; /* [N] or NULL                                          */
    const float *dhw;        /* [M, D, 3] (distance, height, width), contiguous         */
    const float *ray_dir;    /* [N, 3, H, W] unit ray directions, contiguous.  The LDS-staged variants (LDS, WAVE, BAND and therefore AUTO)
                                stage, per pixel tile and plane, the texel box spanned by the tile's four corner pixels: that contains every tap
                                of the tile iff the field is a pinhole camera's (straight pixel lines map to straight lines on every plane), which
                                is what Camera.generate_rays (camera.py:182-211) / gmpi_generate_rays_launch produce.  NaN / infinite rays are
                                handled (NaN pixels, no false status bit); an arbitrary smooth field needs GMPI_VARIANT_GATHER.               */
    const float *eye_pos;    /* [N, 3]                                                  */
    const float *z_dir;      /* [N, 3] optical axis                                     */

    float *rgb_out;          /* [N, 3, H, W]   colour, [0,1] (or [-1,1] with OUT_PM1)   */
    float *depth_out;        /* [N, 1, H, W]   expected depth (mpi.py:434)              */
    float *transmittance_out;/* [N, 1, H, W] or NULL: prod_k (1-a_k+1e-10) -- the cumprod
                                element the reference slices off at mpi.py:423            */
    uint32_t *status;        /* [GMPI_STATUS_WORDS] or NULL; word 0 is OR-ed with GMPI_STATUS_* */

    void *workspace;         /* device scratch owned by the caller, 256-byte aligned, or NULL.  GMPI_VARIANT_BAND keeps its
                                per-plane geometry table there (gmpi_render_workspace_bytes() says how much this call
                                wants); without it GMPI_VARIANT_AUTO uses the kernels that need none.  Contents are
                                scratch: nothing is carried from one call to the next, it need not be cleared, and calls
                                in flight at the same time (different streams) must not share one.                  */
    uint64_t workspace_bytes;
} GmpiRenderParams;

/* Bytes of workspace gmpi_mpi_render_launch can make use of for these parameters (0 when no kernel wants any). */
uint64_t gmpi_render_workspace_bytes(const GmpiRenderParams *params);

/* Enqueue the fused render on `stream`.  Replaces MPI.forward (mpi.py:308-436).
 * GMPI_VARIANT_AUTO picks the kernel from the launch shape; for large launches over bf16 / fp32 volumes with a workspace it enqueues
 * the band kernel and the tile kernel together and shares out the views on the device: the band kernel takes every view whose
 * texel boxes fit its staging buffers (mildly tilted cameras), the tile kernel the others.  An explicit variant that cannot
 * take the parameters returns GMPI_E_VARIANT.
 * GMPI_DTYPE_U8 volumes have two kernels: GATHER (the one-pixel-per-lane kernel: any shape, any stride) and LDS (render_u8.hip: 32 x 16 pixel tiles,
 * per plane a box of up to 64 x 32 raw RGBA texels in LDS, 4 bytes each; it loads 4 texels of a channel row at a time: Wt, the base pointer and the
 * row, channel, plane and MPI strides must be multiples of 4 bytes, else GMPI_E_VARIANT).  WAVE and BAND are GMPI_E_VARIANT; AUTO is LDS where
 * it can take the tensors, else GATHER, whatever the camera hints say.  No workspace.  GMPI_FLAG_CHECK_RANGE is accepted and never sets a bit.
 * With GMPI_FLAG_STRICT_ORDER both are bit-identical to the render of the fp32 volume c / 255; without it the LDS kernel interpolates the codes
 * and scales the sample by RN(1/255) once per channel (about 2e-7 from the strict result).
 * An interleaved GMPI_DTYPE_U8 volume (rgba_stride above) is read in place by the same two kernels, in instances of their own: GATHER loads one texel
 * (4 bytes, any alignment) per tap and takes any Wt; LDS loads 4 texels (16 bytes) at a time and wants Wt a multiple of 4 and the base pointer and the
 * row, plane and MPI strides multiples of 4 bytes, else GMPI_E_VARIANT; AUTO, WAVE, BAND, workspace and flags as for the planar layout.  Same codes, same
 * result: both kernels give the planar volume's bits, in both modes (gmpi_query(20) says whether the layout is built in). */
int gmpi_mpi_render_launch(const GmpiRenderParams *params, void *stream);

/*
 * gmpi_mpi_render_launch over channels-last FLOAT layers: rgba is [M, D, Ht, Wt, 4] in memory (what image files, numpy and channels-last networks
 * hold), described in the struct as the volume [M, D, 4, Ht, Wt] it is a view of -- rgba_dtype F32 / BF16 / F16 and rgba_stride, in elements as ever,
 * [s_M, s_D, 1, s_row, 4]: channel stride 1, texel stride 4, s_row >= 4 Wt (padded rows are fine), s_M and s_D >= 0 (0 on s_M: one MPI for every
 * view group).  Any other stride combination is GMPI_E_STRIDE: planar strides, a channel stride other than 1, a texel stride other than 4, rows
 * that overlap, a negative stride.  Every other field means what it means for gmpi_mpi_render_launch; the camera hints are accepted and ignored; no
 * workspace is used.  The layers are read in place by instances of their own over whole texels (16 bytes of fp32, 8 bytes of 16-bit storage):
 *   GMPI_VARIANT_GATHER  the one-pixel-per-lane kernel, one load per tap of the whole texel at the element's alignment: any Wt, any such strides.
 *                        The planar gather kernel's arithmetic behind the load: its bits, in both modes.
 *   GMPI_VARIANT_LDS     render_layers.hip: 32 x 16 pixel tiles, per plane a box of up to 64 x 32 raw texels in LDS, loaded 16 bytes at a time.
 *                        It takes the tensors gmpi_render_layers_supports() answers 1 for, else GMPI_E_VARIANT.  Bit-identical to GATHER (and to the
 *                        render of the planar copy of the same values) with GMPI_FLAG_STRICT_ORDER, within 1e-5 of it without.
 *                        GMPI_FLAG_CHECK_RANGE tests every staged texel (a superset of the sampled ones).  A (tile, plane) whose box exceeds the
 *                        buffer, and a pixel whose footprint leaves its tile's box (no pinhole ray field), are gathered from global memory.
 *   GMPI_VARIANT_AUTO    LDS where gmpi_render_layers_supports() says 1, else GATHER.
 *   WAVE, BAND, DMA and unknown values: GMPI_E_VARIANT.
 * GMPI_DTYPE_U8 with these strides is forwarded to gmpi_mpi_render_launch (the interleaved uint8 layout above: same kernels, same bits).
 * gmpi_mpi_render_launch and every other entry but gmpi_mpi_render_layers_backward_launch (below) keep refusing the layout for the float types
 * (GMPI_E_STRIDE); the geometry gradients have an entry of their own, gmpi_mpi_render_layers_geometry_backward_launch.  Not built for the layout: the
 * atomics-free backward pair, the chunked, shaded, shared-colour and depth-alpha forms, the strip and band kernels, texel strides other than 4.  gmpi_query(42) == 1 says the two entries are built in.
 */
int gmpi_mpi_render_layers_launch(const GmpiRenderParams *params, void *stream);

/* 1: GMPI_VARIANT_LDS of gmpi_mpi_render_layers_launch can stage these layers, 0: it cannot (AUTO runs GATHER, an explicit LDS is GMPI_E_VARIANT),
 * < 0: the error the launch would return for the struct.  The rule: every 16-byte loader item is a run of naturally aligned dwords that does not
 * straddle the texture's border --
 *   fp32    one texel per item: any Wt; the element's alignment is dword alignment, nothing more is asked;
 *   16-bit  two texels per item: Wt even, and the base pointer and the row, plane and MPI strides multiples of 4 bytes (2 elements);
 * and the byte offsets inside one staged box stay below 2^31: 33 rows of s_row bytes + 1152.  GMPI_DTYPE_U8: the rule of the interleaved uint8
 * layout (gmpi_mpi_render_launch).  Launches nothing. */
int gmpi_render_layers_supports(const GmpiRenderParams *params);

/*
 * Gradient of gmpi_mpi_render_layers_launch w.r.t. the float layers, IN PLACE: the layers are read where they lie and the gradient has their order --
 * no planar copy of either.  `params` describe the layers exactly as gmpi_mpi_render_layers_launch takes them (rgba_stride [s_M, s_D, 1, s_row, 4],
 * rgba_dtype F32 / BF16 / F16; planar or any other strides: GMPI_E_STRIDE; GMPI_DTYPE_U8: GMPI_E_DTYPE -- no gradient flows to codes); rgb_out,
 * depth_out and status may be NULL; transmittance_out, GMPI_FLAG_OUT_PM1, view_to_mpi / views_per_mpi, grad_rgb, grad_depth (or NULL) and
 * grad_transmittance (or NULL) mean what they mean for gmpi_mpi_render_backward_ex_launch.  grad_layers is fp32 [M, D, Ht, Wt, 4] and is ACCUMULATED
 * into (the caller zero-fills it); grad_layers_stride, in elements, is [gs_M, gs_D, 1, gs_row, 4] with gs_row >= 4 Wt, gs_D > 0 and gs_M > 0 (0 for
 * M == 1) -- anything else is GMPI_E_STRIDE.  A NULL grad_rgb, grad_layers or grad_layers_stride is GMPI_E_NULL.  N == 0 returns GMPI_OK; N is not
 * limited.  No workspace is read: the atomics-free pair has no texel form.  Two kernels, instances of the planar backward's two bodies over whole texels:
 *   GMPI_VARIANT_GATHER  one pixel per lane: one whole-texel load per tap, the planar one-pixel kernel's arithmetic behind it, 16 fp32 atomics per
 *                        pixel and plane at 64-bit offsets.  Any Wt, any such strides.
 *   any other variant    the 64 x 8 tile kernel (the fixed-point scatter staged in LDS, as for the planar layout: for equal inputs the staged sums
 *                        have the planar kernel's bits) where gmpi_render_layers_backward_supports() answers 1, else the one-pixel kernel -- the launch
 *                        never fails for that reason.  A tap pair (x, x + 1) of a row is one run of 32 bytes (16 for 16-bit storage) loaded at the
 *                        element's alignment; the flush walks box ROWS -- in the layers' order the 4 nx gradient dwords of a box row are contiguous
 *                        -- with one atomic per dword, consecutive lanes on consecutive dwords.
 * gmpi_query(44) == 1 says the two entries are built in.
 */
int gmpi_mpi_render_layers_backward_launch(const GmpiRenderParams *params, const float *grad_rgb, const float *grad_depth,
                                           const float *grad_transmittance /* or NULL */, float *grad_layers,
                                           const int64_t *grad_layers_stride /* [5], elements: [gs_M, gs_D, 1, gs_row, 4] */, void *stream);

/* 1: gmpi_mpi_render_layers_backward_launch runs its tile kernel on these tensors (unless the variant is GATHER, which this query does not look at),
 * 0: its one-pixel kernel, < 0: the error the launch would return for the struct and the gradient strides.  The tile kernel's guards: Wt >= 2 (pair
 * loads); N <= 65535 (the view index in grid.y); the byte offsets inside one plane of the layers fit 31 bits, (Ht s_row + 4 Wt) x the element size
 * < 2^31; the dword offsets inside one plane of the gradient do, Ht gs_row + 4 Wt < 2^31.  Launches nothing. */
int gmpi_render_layers_backward_supports(const GmpiRenderParams *params, const int64_t *grad_layers_stride);

/*
 * Gradient of the render w.r.t. the RGBA volume -- what autograd computes when the reference's G-step
 * back-propagates through MPIRenderer.render (gmpi/train.py:740-779; the sampling grid carries no gradient,
 * mpi.py:65).  `params` are the forward's parameters; rgb_out / depth_out may be NULL; transmittance_out, when not
 * NULL, must still hold what the forward wrote (the sweep runs back to front from it; without it every pixel first
 * re-walks the alpha channel).  variant GATHER selects the one-pixel-per-lane kernel (16 global atomics per
 * pixel*plane), anything else the tile kernel that stages the scatter in LDS.  grad_rgb [N,3,H,W] is the gradient
 * w.r.t. the colour the forward wrote (the OUT_PM1 factor 2 is applied inside when that flag is set); grad_depth
 * [N,1,H,W] or NULL; grad_rgba [M,D,4,Ht,Wt] fp32 with the given element strides (innermost 1) is ACCUMULATED into
 * (atomicAdd) -- the caller zero-fills it.
 * Round 6: when params->workspace holds at least gmpi_render_backward_workspace_bytes(params) bytes (256-byte aligned; N D H W 24 bytes for the
 * sample gradients and sample positions of every pixel and plane, plus one homography record per view and plane), the launch runs WITHOUT atomics: a pixel pass writes the sample gradients, a texel pass gathers them
 * through each plane's homography and writes every cell of grad_rgba once (deterministic; += without GMPI_FLAG_GRAD_OVERWRITE, = with it: then no
 * zero-fill is needed).  align_corners = True, uniform views_per_mpi (no view_to_mpi), Wt >= 2 and a volume whose offsets inside one plane fit 32 bits,
 * (3 rgba_stride[2] + Ht rgba_stride[3] + Wt) * sizeof(element) < 2^31 (the pixel pass addresses its taps so; grad_rgba may have any strides); other
 * launches take the tile kernels whatever the workspace, and the workspace query answers 0 for them.
 * `ray_dir` must be a pinhole ray field (straight pixel lines map to straight lines on every plane -- what `Camera.generate_rays` /
 * gmpi_generate_rays_launch produce) for the tile kernels' texel boxes and for the gather's candidate windows; GMPI_VARIANT_GATHER (one pixel per lane,
 * 16 atomics per pixel and plane: the cross-check) makes no such assumption and takes no workspace.
 */
int gmpi_mpi_render_backward_launch(const GmpiRenderParams *params, const float *grad_rgb, const float *grad_depth,
                                    float *grad_rgba, const int64_t *grad_rgba_stride, void *stream);
/*
 * The same with a gradient w.r.t. the final transmittance as well: grad_transmittance [N,1,H,W] fp32 or NULL (NULL: exactly
 * gmpi_mpi_render_backward_launch, bit for bit).  With om_k = (1 - a_k) + 1e-10, T_0 = 1, T_{k+1} = T_k om_k, T_out = T_D:
 *     dT_out/da_k = -T_out / om_k = -T_k prod_{j>k} om_j,    dT_out/drgb_k = 0,
 * so with q_k = <gC, rgb_k> + gZ depth_k the volume backward's recurrence  dL/da_k = T_k q_k - S_k / om_k  holds unchanged when the suffix sum
 * starts at gT T_out instead of 0:  S_k = gT T_out + sum_{j>k} w_j q_j  (T_out acts as a background colour every pixel sees through all
 * planes); dL/drgb_k does not change.  The sweep forms gT T_out from the transmittance it starts from (the forward's value, or the one it
 * rebuilds in mantissa x 2^exponent form when that value is below 1e-30): when T_out underflows fp32 the term flushes to zero, which loses
 * contributions below 1e-30 |gT| (four exactly opaque planes give T_out ~ 1e-40).  No scratch of its own: the workspace query is unchanged.
 */
int gmpi_mpi_render_backward_ex_launch(const GmpiRenderParams *params, const float *grad_rgb, const float *grad_depth,
                                       const float *grad_transmittance, float *grad_rgba, const int64_t *grad_rgba_stride,
                                       void *stream);
/* Bytes of caller-owned scratch with which the backward runs without atomics (0: this launch takes the tile kernels). */
uint64_t gmpi_render_backward_workspace_bytes(const GmpiRenderParams *params);

/*
 * The plane-chunked render: the stack [M, D, 4, Ht, Wt] never exists as one tensor (the reference's render_video.py:55-77 generates `chunk_n_planes` planes
 * at a time and has to torch.cat them only because MPI.forward cannot composite a stack piece by piece).  The composite is associative over the plane
 * axis: a partial (C, Z, T) per pixel is all that passes from one plane range to the next.  One launch renders ONE chunk, front chunks first.
 *   params   describes the chunk: D, rgba (+ strides) and dhw are the chunk's own -- the chunk's tensor and the chunk's rows [M, D, 3] of the plane table.
 *   carry    state_in: the state behind the planes in front of this chunk, [N, 5, H, W] fp32, or NULL: the stack starts here (T = 1, sums 0).
 *            state_out: [N, 5, H, W] fp32, or NULL: not wanted (the last chunk).  state_in == state_out is allowed: a lane reads and writes its own pixel.
 * The five channels are the kernels' raw accumulator after the planes so far: r, g, b, z, T.  Colour is in [0, 1] -- never GMPI_FLAG_OUT_PM1's form --, z is
 * in the launch mode's own form: with GMPI_FLAG_STRICT_ORDER sum w_k depth_k, without it sum w_k s_k, BEFORE the per-pixel factor ray . z_dir.  The state is
 * OPAQUE: do not interpret it, and consume a state in the mode (GMPI_FLAG_STRICT_ORDER set or not) that produced it.
 * rgb_out, depth_out and transmittance_out may each be NULL here.  When given they receive the FINISHED images of the stack so far (the epilogue of
 * gmpi_mpi_render_launch; GMPI_FLAG_OUT_PM1 applies only there): transmittance_out is the T behind the chunk, which the chunk backward wants.  state_out and all
 * three outputs NULL: GMPI_E_NULL.  GMPI_FLAG_CHECK_LAST_PLANE refers to the last plane of THIS launch: set it on the final chunk only.  Status bits
 * OR-accumulate as ever (GMPI_STATUS_CAMERA_BEHIND_PLANE looks at the chunk's planes).
 * Kernels: GMPI_VARIANT_GATHER and GMPI_VARIANT_LDS for fp32 / bf16 / fp16 and for GMPI_DTYPE_U8, planar and channels-last (the kernels and conditions of
 * gmpi_mpi_render_launch, in instances of their own); GMPI_VARIANT_AUTO is LDS where the tile kernel takes the tensors, else GATHER, whatever the launch
 * size and the camera hints; WAVE and BAND are GMPI_E_VARIANT (the strip kernel splits the plane axis itself; the band kernel's carry instances have an
 * entry of their own, gmpi_mpi_render_chunk_band_launch below, because they want a workspace).  No workspace is read.  With GMPI_FLAG_STRICT_ORDER the chunked render has the bits of the one-shot render of the concatenation with the same variant, however
 * the stack is cut; without it too, as long as the tile kernel stages the same planes.  gmpi_query(36) == 1 says the entries are built in.
 */
typedef struct GmpiCarry {
    uint32_t struct_size;    /* = sizeof(GmpiCarry) */
    uint32_t reserved;       /* 0 */
    const float *state_in;   /* [N,5,H,W] fp32 or NULL: the stack starts here (T = 1, sums 0) */
    float *state_out;        /* [N,5,H,W] fp32 or NULL: not wanted (the last chunk) */
} GmpiCarry;
int gmpi_mpi_render_chunk_launch(const GmpiRenderParams *params, const GmpiCarry *carry, void *stream);

/*
 * One chunk through the BAND kernel's carry instances (fp32 / bf16 / fp16 volumes; 256 x 8 / 128 x 8 pixel bands, LDS-DMA loader: what GMPI_VARIANT_AUTO of
 * gmpi_mpi_render_launch means for large launches).  `params` and `carry` are those of gmpi_mpi_render_chunk_launch in every respect: the state's layout and
 * format, the NULL rules, GMPI_FLAG_OUT_PM1 / GMPI_FLAG_CHECK_LAST_PLANE on the last chunk only, status bits OR-accumulated, state_in == state_out allowed (every
 * band is rendered exactly once; a lane outside the image may read a pixel that is being rewritten, and stores nothing).  The state is ONE format: a stack may be
 * carried from a chunk of gmpi_mpi_render_chunk_launch into a chunk of this entry and back, in the mode (GMPI_FLAG_STRICT_ORDER or not) that produced it.
 * params->workspace must hold gmpi_render_chunk_band_workspace_bytes(params) bytes, 256-byte aligned: the band table of the chunk's own D planes, rebuilt by
 * every launch (what it held before does not matter); missing, too small or misaligned: GMPI_E_WORKSPACE.
 *   GMPI_VARIANT_BAND  the band carry kernel renders every view; a band with a texel box that does not fit its staging buffers takes the direct gather inside
 *                      the kernel, with the same state.
 *   GMPI_VARIANT_AUTO  the pair of gmpi_mpi_render_launch's band path: views with a box that does not fit are handed, through a gate word per view in the
 *                      workspace, to the tile kernel's carry instances (a second launch); every view's state passes through exactly one of the two kernels.
 *                      No size threshold and no camera hints: the caller opted in by calling this entry.
 *   any other variant: GMPI_E_VARIANT.  GMPI_DTYPE_U8, and tensors the band kernel (for AUTO: the tile kernel too) cannot take -- the alignment rules of
 *   GMPI_VARIANT_BAND / GMPI_VARIANT_LDS above, Ht or Wt above 8192 --: GMPI_E_VARIANT; gmpi_render_chunk_band_supports() says so beforehand.
 * N == 0: GMPI_OK.  Every other error as at gmpi_mpi_render_chunk_launch.  With GMPI_FLAG_STRICT_ORDER the chunked render has the bits of the oracle and of the
 * one-shot GMPI_VARIANT_BAND render however the stack is cut; without it too wherever every box fits (the per-plane arithmetic does not know the chunk).
 * gmpi_query(50) == 1 says the three entries are built in.
 */
int gmpi_mpi_render_chunk_band_launch(const GmpiRenderParams *params, const GmpiCarry *carry, void *stream);
/* Bytes of workspace the launch above wants: gmpi_render_workspace_bytes of the same struct with variant = GMPI_VARIANT_BAND; 0 where it answers GMPI_E_VARIANT
 * or a struct error, and for N == 0. */
uint64_t gmpi_render_chunk_band_workspace_bytes(const GmpiRenderParams *params);
/* 1: gmpi_mpi_render_chunk_band_launch takes these parameters given its workspace, 0: it answers GMPI_E_VARIANT; a negative struct error as the launch. */
int gmpi_render_chunk_band_supports(const GmpiRenderParams *params);

/*
 * Sparse GMPI_DTYPE_U8 volumes: the staged uint8 kernel (GMPI_VARIANT_LDS above) skipping every (tile, plane) whose texel box holds alpha code 0 alone.
 *
 * Stored MPIs are mostly empty, and at 8 bits "empty" is the exact code 0.  An alpha sample of exactly 0 changes nothing: w = 0 T, C += 0 rgb,
 * Z += 0 depth, T (1 - 0 + 1e-10) = T 1.0f.  So such a pair needs no loads, no LDS store, no taps, no conversions and no bilerps -- and skipping them
 * moves no output bit and no status bit (codes cannot be out of range: GMPI_FLAG_CHECK_RANGE has nothing to miss).  The bits are those of
 * gmpi_mpi_render_launch with GMPI_VARIANT_LDS on the same parameters, in both modes and for both layouts, whatever the ray field: an empty plane still
 * computes each pixel's coordinates and its box test, a pixel whose footprint lies outside its tile's box takes the direct gather as ever, every other
 * pixel is blended with the all-zero sample and its own s and dot (so a non-finite s does to the depth what it did before).
 *
 * The occupancy map: uint8 map[M, D, ceil(Ht / B), ceil(Wt / B)], contiguous, B = gmpi_query(53) = 16; an entry is the largest alpha code among the texels
 * of its B x B block that exist (border blocks are partial).  gmpi_u8_occupancy_launch builds it from a planar or channels-last GMPI_DTYPE_U8 volume with
 * any outer strides (the stride rules of gmpi_mpi_render_launch; no alignment is asked for), reading the alpha bytes only; it uses nothing of *params but
 * the volume description: rgba, rgba_dtype, rgba_stride, M, D, Ht, Wt and struct_size.  gmpi_u8_occupancy_bytes is the map's size (0 for a struct the launch refuses).
 * A map describes the codes it was built from: after a write to the volume it must be rebuilt (a stale zero skips texels that are no longer empty).
 *
 * gmpi_mpi_render_u8_sparse_launch: params as gmpi_mpi_render_launch takes a GMPI_DTYPE_U8 volume, variant AUTO or LDS; occ->map the volume's map, occ->block =
 * gmpi_query(53); occ->stats NULL or two uint32 counters on the device, to which every workgroup adds (atomically) [0] the (tile, plane) pairs it skipped and
 * [1] those it staged -- a pair whose box does not fit the staging buffer takes the direct gather and is neither.  Per tile the thread that fills a plane's row of
 * the box table tests the box, clipped to the texture (outside is zero padding), against the at most 5 x 3 blocks it overlaps.
 * Refusals, nothing written: a struct error as gmpi_mpi_render_launch; another dtype: GMPI_E_DTYPE; occ or occ->map NULL: GMPI_E_NULL; occ->block !=
 * gmpi_query(53): GMPI_E_SHAPE; any other variant, or tensors the staged kernel cannot take (the alignment rules above): GMPI_E_VARIANT --
 * gmpi_render_u8_sparse_supports says 1 / 0 (GMPI_E_VARIANT) / a negative error beforehand.  N == 0: GMPI_OK.
 * Stream-ordered, allocate nothing, never synchronise.  Not built: float volumes, the carry instances of the chunked render, thresholds above code 0 (not
 * exact), early termination behind opaque planes; GMPI_VARIANT_AUTO of gmpi_mpi_render_launch never comes here.  gmpi_query(52) == 1 says the four entries are built in.
 */
typedef struct GmpiOccupancy {
    const uint8_t *map;   /* [M, D, ceil(Ht / block), ceil(Wt / block)], device memory                         */
    int32_t block;        /* gmpi_query(53)                                                                    */
    uint32_t *stats;      /* NULL, or uint32[2] on the device: [0] += pairs skipped, [1] += pairs staged       */
} GmpiOccupancy;
uint64_t gmpi_u8_occupancy_bytes(const GmpiRenderParams *params);
int gmpi_u8_occupancy_launch(const GmpiRenderParams *params, uint8_t *map, void *stream);
int gmpi_mpi_render_u8_sparse_launch(const GmpiRenderParams *params, const GmpiOccupancy *occ, void *stream);
int gmpi_render_u8_sparse_supports(const GmpiRenderParams *params, const GmpiOccupancy *occ);

/*
 * Gradient of a chunked render w.r.t. ONE chunk; chunks are swept from the last to the first.  `params` are the chunk's forward parameters;
 * params->transmittance_out is T BEHIND the chunk as the forward launch wrote it (NULL: rebuilt from T_in by a walk of the chunk's alpha).  grad_rgb,
 * grad_depth, grad_transmittance are the gradients w.r.t. the FINAL images (grad_depth NULL or given to every chunk; grad_transmittance to the LAST chunk
 * only, NULL elsewhere; the GMPI_FLAG_OUT_PM1 factor is applied as in gmpi_mpi_render_backward_launch when the flag is set in params -- set it for every
 * chunk of a stack whose final colour was written with it).
 *   T_in   [N,1,H,W] T in front of the chunk (the transmittance_out of the chunk in front), or NULL = 1 (the first chunk)
 *   S_in   [N,1,H,W] the suffix sum handed over by the chunk behind, or NULL = 0 (the last chunk)
 *   S_out  [N,1,H,W] or NULL: the suffix sum in front of this chunk's first plane.  S_in == S_out is allowed.
 * The sweep is gmpi_mpi_render_backward_ex_launch's, continued instead of started: T starts at the boundary value, S = S_in + gT T_behind, and
 * dL/da_k = T_k q_k - S_k / om_k, dL/drgb_k = g w_k hold unchanged with the GLOBAL T_k and S_k (every later plane is linear in the T that reaches it).
 * Underflow: where T behind the chunk is below 1e-30, T is rebuilt in mantissa x 2^exponent form by walking the chunk's alpha from T_in instead of from 1.
 * Where T_in is below 1e-30 too (zero and denormals included) the pixel contributes nothing from this chunk: its volume gradients are zero and
 * S_out = S_in.  The terms dropped are below 1e-20 D |q|.
 * variant GATHER selects the one-pixel-per-lane all-atomic kernel, anything else the 64 x 8 tile kernel; grad_rgba [M,D,4,Ht,Wt] of the CHUNK, fp32, is
 * accumulated into (the caller zero-fills it).  The atomics-free pair, the geometry backward and the two image layouts have no chunk form.
 * GMPI_DTYPE_U8: GMPI_E_DTYPE.  N == 0: GMPI_OK.  N > 65535: GMPI_E_SHAPE.
 */
int gmpi_mpi_render_chunk_backward_launch(const GmpiRenderParams *params, const float *grad_rgb, const float *grad_depth,
                                          const float *grad_transmittance, const float *T_in, const float *S_in, float *S_out,
                                          float *grad_rgba, const int64_t *grad_rgba_stride, void *stream);

/*
 * Gradient of the render w.r.t. the sample POSITIONS (an extension: the reference builds the grid under torch.no_grad(), mpi.py:65):
 * the rays, the eye positions, the optical axes and the plane geometry.  `params`, grad_rgb, grad_depth and transmittance_out as for
 * gmpi_mpi_render_backward_launch.  Per view n, pixel, plane k, with s = (d_k - ez)/rz, x = ex + rx s, y = ey + ry s, depth_k = s (r . z_dir),
 * d_s[c] the gradient w.r.t. sample channel c and G_k = gZ w_k (the volume backward's sweep), and the bilinear derivatives of the four taps
 * (zeros padding):  g_x = g_ix dix/dx, g_y = g_iy diy/dy, g_s = g_x rx + g_y ry + G_k dot; summed over the planes
 *     grad_ray_dir[n,:,p] = (g_x s, g_y s, -g_s s / rz) + G_k s z_dir         [N,3,H,W]
 *     grad_eye_pos[n]     = sum over pixels of (g_x, g_y, -g_s / rz)            [N,3]
 *     grad_z_dir[n]       = sum over pixels of G_k s r                          [N,3]
 *     grad_dhw[m,k]       = sum over pixels and every view of MPI m of (g_s / rz, -g_y y / h_k, -g_x x / w_k)   [M,D,3]
 * Outputs are OVERWRITTEN; NULL = not wanted.  Any view_to_mpi, any ray field.  The per-view and per-plane sums go through slabs in
 * params->workspace (at least gmpi_render_geometry_backward_workspace_bytes(params, grad_dhw != NULL) bytes, 256-byte aligned; otherwise
 * GMPI_E_WORKSPACE) and are summed in a fixed order: no atomics, every output bit-reproducible.  The coordinate chain is the forward's for
 * the launch's flags (GMPI_FLAG_STRICT_ORDER included), so the pass floors to the texels the forward sampled.
 */
int gmpi_mpi_render_geometry_backward_launch(const GmpiRenderParams *params, const float *grad_rgb, const float *grad_depth,
                                             float *grad_ray_dir, float *grad_eye_pos, float *grad_z_dir, float *grad_dhw,
                                             void *stream);
/* The same with grad_transmittance [N,1,H,W] fp32 or NULL (NULL: exactly gmpi_mpi_render_geometry_backward_launch).  The transmittance
 * term enters through the alpha sample gradient d_s[3] (the suffix sum starts at gT T_out, as in gmpi_mpi_render_backward_ex_launch) and
 * reaches the positions through g_ix and g_iy; G_k, the depth term, is untouched. */
int gmpi_mpi_render_geometry_backward_ex_launch(const GmpiRenderParams *params, const float *grad_rgb, const float *grad_depth,
                                                const float *grad_transmittance, float *grad_ray_dir, float *grad_eye_pos,
                                                float *grad_z_dir, float *grad_dhw, void *stream);
/* Bytes of workspace gmpi_mpi_render_geometry_backward_launch needs for the eye / z_dir sums, and with want_dhw != 0 the plane sums too. */
uint64_t gmpi_render_geometry_backward_workspace_bytes(const GmpiRenderParams *params, int want_dhw);

/*
 * gmpi_mpi_render_geometry_backward_ex_launch over the volume in the formats it is STORED in, read in place: the same four gradients, the same
 * tiles, slabs and fixed-order sums (no atomics: bit-reproducible), nothing the size of a volume is allocated, copied or written.  For equal values
 * the outputs have the bits of the volume entry over the planar float volume (GMPI_FLAG_STRICT_ORDER or not: the pass is one text over tap sources).
 *   gmpi_mpi_render_u8_geometry_backward_launch      params as gmpi_mpi_render_launch takes a GMPI_DTYPE_U8 volume -- planar codes, or channels-last
 *       texels (rgba_stride[2] == 1 and rgba_stride[4] == 4: one 4-byte load per tap, a base pointer at any byte): told by the strides, as the forward
 *       tells them.  Every tap is the correctly rounded c / 255, the value the forward reads.  Any other rgba_dtype: GMPI_E_DTYPE.  Without
 *       GMPI_FLAG_STRICT_ORDER, where the staged 8-bit forward may have written transmittance_out (variant not GATHER, tensors it can stage), that value
 *       is not read: the forward sums the CODES and scales once, and under exactly opaque texels (four taps of 255) its 1 - alpha differs from the
 *       sweep's by orders of magnitude; every pixel walks the alpha texels with the sweep's own arithmetic instead (one more pass over the taps).
 *   gmpi_mpi_render_layers_geometry_backward_launch  params as gmpi_mpi_render_layers_backward_launch takes them: channels-last float layers,
 *       rgba_stride [s_M, s_D, 1, s_row, 4], F32 / BF16 / F16 (one 16- / 8-byte load per tap at the element's alignment).  Planar or any other strides:
 *       GMPI_E_STRIDE; GMPI_DTYPE_U8: GMPI_E_DTYPE (the entry above takes channels-last codes).
 * Both: rgb_out, depth_out and status may be NULL; transmittance_out as for the volume entry (the sweep starts from it, or re-walks the alpha texels
 * where it has underflowed: runs of exactly opaque codes); grad_transmittance may be NULL.  A NULL grad_rgb is GMPI_E_NULL; with no output wanted
 * GMPI_OK and nothing is launched; N == 0 is GMPI_OK at once; N or M > 65535: GMPI_E_SHAPE.  The per-view and per-plane sums need
 * gmpi_render_geometry_inplace_workspace_bytes(params, grad_dhw != NULL) bytes in params->workspace (256-byte aligned; otherwise GMPI_E_WORKSPACE).
 * Nothing is written on any refusal.  No status bits are set.  gmpi_query(48) == 1 says the three entries are built in.
 */
int gmpi_mpi_render_u8_geometry_backward_launch(const GmpiRenderParams *params, const float *grad_rgb, const float *grad_depth,
                                                const float *grad_transmittance /* or NULL */, float *grad_ray_dir, float *grad_eye_pos,
                                                float *grad_z_dir, float *grad_dhw, void *stream);
int gmpi_mpi_render_layers_geometry_backward_launch(const GmpiRenderParams *params, const float *grad_rgb, const float *grad_depth,
                                                    const float *grad_transmittance /* or NULL */, float *grad_ray_dir, float *grad_eye_pos,
                                                    float *grad_z_dir, float *grad_dhw, void *stream);
/* gmpi_render_geometry_backward_workspace_bytes for the params of the two entries above (that query keeps answering 0 for GMPI_DTYPE_U8 and for the
 * layers' strides): the same size -- it depends on N, H, W and D only --, also for a planar float volume.  0 for params neither entry would take. */
uint64_t gmpi_render_geometry_inplace_workspace_bytes(const GmpiRenderParams *params, int want_dhw);

/*
 * Shared-colour layout: what GMPI's generator produces before it concatenates (networks_cond_on_pos_enc.py:950-975 with gmpi.yml:137-145) -- ONE
 * colour image per MPI, D alpha planes and, optionally, a separate colour image for the last plane.  By definition the result is the render of the
 * expanded volume  rgba[m,k,0:3] = rgb[m]  (k = D-1: background[m] when one is given),  rgba[m,k,3] = alpha[m,k,0]  -- per plane and channel the
 * arithmetic is the one of gmpi_mpi_render_launch (GMPI_FLAG_STRICT_ORDER: bit-identical to it), the volume is never materialised.
 * All three tensors have the storage type params->rgba_dtype and innermost stride 1.
 */
typedef struct GmpiSharedColor {
    uint32_t struct_size;         /* = sizeof(GmpiSharedColor)                                         */
    const void *rgb;              /* [M, 3, Ht, Wt] colour of every plane (but the last, with a background) */
    int64_t rgb_stride[3];        /* element strides: MPI, channel, row; 0 allowed on [0] (expand)     */
    const void *background;       /* [M, 3, Ht, Wt] colour of plane D-1, or NULL                       */
    int64_t background_stride[3]; /* MPI, channel, row (ignored without a background)                  */
} GmpiSharedColor;

/*
 * The fused render over a shared-colour MPI.  `params` as for gmpi_mpi_render_launch, except: params->rgba points at the ALPHA planes
 * [M, D, 1, Ht, Wt] -- rgba_stride[0], [1], [3] are its MPI, plane and row strides, rgba_stride[2] is ignored, rgba_stride[4] must be 1 -- so the
 * strided view rgba[:, :, 3:] of an ordinary volume is a valid alpha tensor.  Every flag, view_to_mpi / views_per_mpi, transmittance_out and the status
 * bits mean what they mean there; GMPI_FLAG_CHECK_RANGE covers the alpha, colour and background texels the render samples.  D == 1 with a background is
 * legal (the one plane is the background).  params->variant:
 *   AUTO, GATHER  one pixel per lane, taps from global memory (any shape, any stride, any ray field); the same kernel for both;
 *   LDS           one workgroup per 32 x 16 pixel tile: per plane the texel box spanned by the tile's four corner pixels is staged in LDS for the four
 *                 channels at once (the box has the same origin in the alpha plane and in the colour image; alpha streams from HBM, the colour box
 *                 is re-read per plane from the caches).  A (tile, plane) whose box exceeds the 56 x 27 texel buffer, and a pixel whose footprint
 *                 lies outside its tile's box (a ray field that is no pinhole camera's), take the direct gather: results do not depend on the path,
 *                 and with GMPI_FLAG_STRICT_ORDER they are bit-identical to AUTO's.  GMPI_FLAG_CHECK_RANGE then covers every staged texel.  It
 *                 loads items of 4 texels: the three base pointers and their MPI, channel / plane and row strides must be multiples of 4 texels
 *                 (16 bytes of fp32, 8 bytes of 16-bit storage; any Wt), else GMPI_E_VARIANT -- gmpi_render_shared_supports() says so beforehand.
 *                 With Wt % 4 != 0 the last item of a texel row reaches up to 3 texels past Wt (they are read and replaced by zeros): inside the
 *                 row stride for every row but the LAST row of each tensor, behind which that many elements must be readable memory -- the
 *                 caller's duty, neither the launch nor the query can see the allocation (the Python layer checks the storage and falls back);
 *   anything else GMPI_E_VARIANT.
 * No workspace.  Stream-ordered, allocates nothing, never synchronises.
 */
int gmpi_mpi_render_shared_launch(const GmpiRenderParams *params, const GmpiSharedColor *shared, void *stream);

/* Whether gmpi_mpi_render_shared_launch can run these parameters with params->variant: 1 yes, 0 no (the launch would return GMPI_E_VARIANT only
 * because this variant's kernel cannot take them: another variant can), negative GMPI_E_* for what the launch refuses whatever the kernel.  For
 * GMPI_VARIANT_LDS it is 1 whenever the three base pointers and all their outer strides are multiples of 16 bytes.  Launches nothing. */
int gmpi_render_shared_supports(const GmpiRenderParams *params, const GmpiSharedColor *shared);

/*
 * Gradient of gmpi_mpi_render_shared_launch w.r.t. the three tensors:  d rgb = sum over the planes that use rgb of d rgba[:, k, 0:3],
 * d background = d rgba[:, D-1, 0:3],  d alpha = d rgba[:, :, 3:]  of gmpi_mpi_render_backward_ex_launch on the expanded volume.  grad_rgb_out
 * [N,3,H,W], grad_depth [N,1,H,W] or NULL, grad_transmittance [N,1,H,W] or NULL as there; params->transmittance_out as there.
 * grad_shared_rgb [M,3,Ht,Wt], grad_alpha [M,D,1,Ht,Wt] and grad_background [M,3,Ht,Wt] are fp32, caller-zeroed and ADDED into (atomicAdd); each has
 * three element strides (MPI, channel or plane, row; innermost 1); each may be NULL and is then skipped (all three NULL: GMPI_E_NULL; a
 * grad_background without a background: GMPI_E_NULL).
 * variant GATHER: one pixel per lane, 16 global atomics per pixel and plane.  AUTO: one workgroup per 32 x 16 pixel tile; the alpha gradient
 * is staged in LDS and flushed per plane, the colour gradient is summed in LDS ACROSS the planes in a window of 64 x 32 texels, which is flushed
 * whenever the tile's texel boxes have drifted out of it and at the end of the tile: with the FFHQ geometry and 32 planes 2.8 / 3.9 / 6.1 flushes per
 * tile on average at 256^2 / 512^2 / 1024^2 (instead of 32 per-plane flushes of the colour channels; up to one per plane for strongly tilted cameras
 * at 1024^2 -- DESIGN.md 3.3c has the counts).  D > 128 (more planes than the tile kernel's tables hold) takes the one-pixel-per-lane kernel, several
 * times slower.  The tile kernel's texel boxes assume a pinhole ray field (see ray_dir above); this is NOT checked: a pixel whose taps fall outside its
 * tile's box adds them straight to global memory, so any ray field gives correct gradients, an irregular one at the one-pixel-per-lane kernel's speed.
 * Any other variant is GMPI_E_VARIANT: GMPI_VARIANT_LDS names a forward kernel only (the backward of a forward launched with it is AUTO's).
 */
int gmpi_mpi_render_shared_backward_launch(const GmpiRenderParams *params, const GmpiSharedColor *shared, const float *grad_rgb_out,
                                           const float *grad_depth, const float *grad_transmittance, float *grad_shared_rgb,
                                           const int64_t *grad_shared_rgb_stride, float *grad_alpha, const int64_t *grad_alpha_stride,
                                           float *grad_background, const int64_t *grad_background_stride, void *stream);

/*
 * Depth-alpha layout: what GMPI's "depth2alpha" generator produces (torgba_cond_on_pos_enc: "depth2alpha", networks_vanilla_depth2alpha.py:650-663) --
 * ONE colour image and ONE depth image per MPI and, optionally, a colour image for the last plane; no alpha planes.  The alpha of texel x on plane k is
 *     t = plane_z[k] - depth[x];   t = min(max(t, z_lo), z_hi);   alpha = (t - z_lo) / z_den
 * in fp32, one rounding per step, the division IEEE (depth stored in 16 bits is upcast first: exact).  By definition the result is the render of the
 * volume with these alphas and GmpiSharedColor's colours (expand_depth_alpha in the Python package is the executable definition); with
 * GMPI_FLAG_STRICT_ORDER it is bit-identical to gmpi_mpi_render_launch on that volume, which is never materialised.  The caller rounds the constants:
 * z_lo = (float)lo, z_hi = (float)hi, z_den = (float)(hi - lo + 1e-8) with the sum formed in double (the reference divides by z_hi - z_lo + 1e-8).
 */
typedef struct GmpiDepthAlpha {
    uint32_t struct_size;   /* = sizeof(GmpiDepthAlpha)                                              */
    const float *plane_z;   /* [D], or [M, D]: the (normalised) depth of every plane, device memory   */
    int64_t plane_z_stride; /* elements from one MPI's table to the next; 0 = one table for all MPIs  */
    float z_lo, z_hi;       /* the ramp's bounds, z_lo < z_hi                                         */
    float z_den;            /* the ramp's divisor, > 0                                                */
} GmpiDepthAlpha;

/*
 * The fused render over a depth-alpha MPI.  `params` as for gmpi_mpi_render_launch, except: params->rgba points at the DEPTH image seen as
 * [M, 1, 1, Ht, Wt] -- rgba_stride[0] and [3] are its MPI and row strides, [1] and [2] are ignored, [4] must be 1; params->D is the number of planes
 * (of dhw and plane_z).  `shared` carries rgb and background as for gmpi_mpi_render_shared_launch; the three images have the storage type
 * params->rgba_dtype (GMPI_DTYPE_U8: GMPI_E_DTYPE).  Every flag, view_to_mpi / views_per_mpi, transmittance_out and the status bits mean what they mean
 * there.  GMPI_FLAG_CHECK_RANGE covers every computed alpha tap (a NaN depth sets GMPI_STATUS_RGBA_RANGE) and the colour texels that are read: a plane
 * whose alpha sample is exactly 0 is skipped, colour taps and blend (with a = 0 the blend is the identity in fp32: w = 0, (1 - 0) + 1e-10 rounds to 1
 * -- for finite colour texels and a finite plane depth 1/(1/(s dot)); a NaN or infinite one gives NaN on the volume path, 0 * x, and nothing here; and
 * the colour texels under an alpha sample of 0 are not range-checked, which they are on the volume path).
 * One kernel, one pixel per lane, taps from global memory (any shape, any stride, any ray field): GMPI_VARIANT_AUTO and GMPI_VARIANT_GATHER run
 * it, any other variant is GMPI_E_VARIANT.  z_lo >= z_hi or z_den <= 0 (or a NaN among them): GMPI_E_SHAPE; a negative plane_z_stride:
 * GMPI_E_STRIDE; NULL params, shared, depth_alpha, plane_z, rgb or depth image: GMPI_E_NULL.  No workspace.  Stream-ordered, allocates nothing,
 * never synchronises.  A window forward has an entry of its own (gmpi_mpi_render_depth_window_launch, below: this entry keeps its one kernel and
 * still refuses GMPI_VARIANT_LDS).  Gradients w.r.t. the geometry: gmpi_mpi_render_depth_geometry_backward_launch (gmpi_query(30)).  The expected depth of the un-warped stack, for the
 * shading augmentation (LightRenderer): gmpi_ramp_depth_launch (gmpi_query(32)).  W.r.t. plane_z:
 * gmpi_mpi_render_depth_geometry_backward_pz_launch (gmpi_query(40)).  Not built: 8-bit storage, gradients w.r.t. the ramp's bounds (gmpi_query(22) says whether the layout itself is built in).
 */
int gmpi_mpi_render_depth_launch(const GmpiRenderParams *params, const GmpiSharedColor *shared, const GmpiDepthAlpha *depth_alpha, void *stream);

/*
 * gmpi_mpi_render_depth_launch with a window kernel: same arguments, same checks, same error codes, THE SAME BITS in both modes (default and
 * GMPI_FLAG_STRICT_ORDER), the same status words.  One workgroup per 32 x 16 pixel tile, planes front to back; every tap is read from one window of
 * gmpi_query(26) x gmpi_query(27) = 64 x 32 texels x 4 channels (R, G, B, depth; fp32) in LDS, which is reloaded whenever the tile's texel boxes have
 * drifted out of it (and, with a background, its colour channels once more before the last plane).  The box table is refilled every gmpi_query(28)
 * planes: any D.  While a window is loaded its depth texels are reduced to their minimum: a plane that lies in front of the ramp for the whole
 * window (RN(plane_z[k] - min) <= z_lo, no NaN among the texels) is skipped for every pixel whose ray lies between the tile's corner rays -- exactly
 * the planes the one-pixel kernel skips pixel by pixel.  Routing: GMPI_VARIANT_AUTO launches the window kernel, GMPI_VARIANT_GATHER the
 * one-pixel-per-lane kernel of gmpi_mpi_render_depth_launch; any other variant is GMPI_E_VARIANT.  The loader reads items of 16 bytes: base pointers and
 * the MPI / channel / row strides of the three images must be multiples of 16 bytes, or AUTO is GMPI_E_VARIANT too (ask
 * gmpi_render_depth_window_supports).  Any Wt: the last item of a row whose width is no multiple of 4 texels reads up to 3 texels of the row's
 * padding; behind the LAST row of each image that padding must be allocated -- the caller's duty, neither the launch nor the query can see the
 * allocation (the Python layer checks the storage and falls back).  The texel boxes assume a pinhole ray field (see ray_dir above); this is NOT
 * checked: a pixel whose taps fall outside the window reads them from global memory, and so does a tile whose box on a plane exceeds the window
 * (strong minification, corners that are not finite) -- any input gives the one-pixel kernel's pixels, an irregular one at its speed.  One
 * difference: a tap OUTSIDE the texture reads a zero from the window where the one-pixel kernel reads the clamped border texel; both multiply it by a
 * zero weight, so results and range bit differ only where that border texel is not finite resp. not in [0, 1].
 */
int gmpi_mpi_render_depth_window_launch(const GmpiRenderParams *params, const GmpiSharedColor *shared, const GmpiDepthAlpha *depth_alpha,
                                        void *stream);

/* 1: gmpi_mpi_render_depth_window_launch takes these arguments (for GMPI_VARIANT_AUTO: with the window kernel), 0: GMPI_VARIANT_AUTO and the
 * loader cannot take the tensors (alignment), negative: the error code the launch would return.  Launches nothing. */
int gmpi_render_depth_window_supports(const GmpiRenderParams *params, const GmpiSharedColor *shared, const GmpiDepthAlpha *depth_alpha);

/*
 * Gradient of gmpi_mpi_render_depth_launch w.r.t. the three images -- torch autograd's through expand_depth_alpha: the clamp passes the gradient
 * where z_lo <= plane_z[k] - depth <= z_hi (bounds included), d alpha / d depth = -1 / z_den there and 0 elsewhere, so the gradient of all D alpha
 * planes lands in ONE depth image; the colours as in gmpi_mpi_render_shared_backward_launch.  grad_rgb_out, grad_depth, grad_transmittance and
 * params->transmittance_out as there.  Behind the surface every plane is (almost) exactly opaque, so the forward's transmittance underflows for most
 * pixels: the kernel then re-walks the ramp samples front to back in mantissa x 2^exponent form before its back-to-front sweep -- the common path of
 * this layout, not the rare one.  grad_shared_rgb [M,3,Ht,Wt], grad_depth_image [M,1,Ht,Wt] and grad_background [M,3,Ht,Wt] are fp32, caller-zeroed
 * and ADDED into (atomicAdd); each has three element strides (MPI, channel, row; innermost 1; the depth image's channel stride is ignored); each may
 * be NULL and is then skipped (all three NULL: GMPI_E_NULL; a grad_background without a background: GMPI_E_NULL).  No atomic is issued for a term that
 * is exactly zero (planes of weight 0, clamped taps, zero bilinear weights).  One kernel, one pixel per lane (AUTO and GATHER; anything else
 * GMPI_E_VARIANT); N <= 65535.
 */
int gmpi_mpi_render_depth_backward_launch(const GmpiRenderParams *params, const GmpiSharedColor *shared, const GmpiDepthAlpha *depth_alpha,
                                          const float *grad_rgb_out, const float *grad_depth, const float *grad_transmittance,
                                          float *grad_shared_rgb, const int64_t *grad_shared_rgb_stride, float *grad_depth_image,
                                          const int64_t *grad_depth_image_stride, float *grad_background, const int64_t *grad_background_stride,
                                          void *stream);

/*
 * gmpi_mpi_render_depth_backward_launch with a tile kernel: same arguments, same checks, same error codes, same gradients up to the order of the
 * adds.  One workgroup per 32 x 16 pixel tile; the gradients of the colour image AND of the depth image are summed in LDS across the planes, in one
 * window of 64 x 32 texels x 4 channels (64-bit fixed point), which is flushed -- one atomicAdd per non-zero texel -- whenever the tile's texel boxes
 * have drifted out of it, and at the end of the tile; with a background, the colour channels once more after the last plane.  There is no per-plane
 * flush: all D alpha planes have one destination.  Routing: GMPI_VARIANT_GATHER launches the one-pixel-per-lane kernel of
 * gmpi_mpi_render_depth_backward_launch; so does D > gmpi_query(23) = 128 (more planes than the tile kernel's table holds), several times slower with
 * a wide ramp; everything else (GMPI_VARIANT_AUTO) launches the tile kernel.  Any other variant is GMPI_E_VARIANT.  The texel boxes assume a pinhole
 * ray field (see ray_dir above); this is NOT checked: a pixel whose taps fall outside its tile's box adds them straight to global memory, and so
 * does a tile whose box on a plane exceeds the window (strong minification) and a value outside the fixed-point range (colours far outside [0, 1],
 * non-finite gradients): any input gives the one-pixel kernel's gradients, an irregular one at its speed.
 */
int gmpi_mpi_render_depth_backward_tile_launch(const GmpiRenderParams *params, const GmpiSharedColor *shared, const GmpiDepthAlpha *depth_alpha,
                                               const float *grad_rgb_out, const float *grad_depth, const float *grad_transmittance,
                                               float *grad_shared_rgb, const int64_t *grad_shared_rgb_stride, float *grad_depth_image,
                                               const int64_t *grad_depth_image_stride, float *grad_background,
                                               const int64_t *grad_background_stride, void *stream);

/*
 * The image backward of the two layouts WITHOUT atomics: gmpi_mpi_render_shared_backward_launch / gmpi_mpi_render_depth_backward_launch as the pair of
 * gmpi_mpi_render_backward_launch's workspace path -- a pixel pass that writes one record per view, plane and pixel (the exact sample position from the
 * forward's coordinate chain and dL/d(r, g, b, alpha sample): 24 bytes; the sweep is the layout's one-pixel-per-lane kernel's, term for term), then a
 * texel gather through each plane's inverse homography in which every gradient cell has ONE owner and is written once, in a fixed order: two launches
 * give the same bits.  The colour sums run ACROSS the planes that use rgb (plane D-1's go to grad_background when there is one); grad_alpha is stored per
 * plane; the depth-alpha layout adds plane k's sum to a cell's depth gradient where z_lo <= plane_z[k] - depth <= z_hi for that texel and divides by
 * -z_den once per cell.  A workgroup owns a 64 x 16 texel tile of one MPI over a RUN of planes: one run when that fills the chip (at least 1024
 * workgroups), else the planes per run are halved until it does, each run writes its partial colour / depth sums to a slab of the workspace and a small
 * kernel adds the runs up in run order.  The number of runs is a function of M, D, Ht and Wt alone.
 * Arguments, checks and error codes: those of the layout's image backward, except
 *   - params->workspace must hold gmpi_render_layout_backward_gather_workspace_bytes(params, shared, depth_alpha) bytes, 256-byte aligned:
 *     GMPI_E_WORKSPACE otherwise;
 *   - the pair takes GMPI_FLAG_ALIGN_CORNERS launches with uniform views_per_mpi (no view_to_mpi), Wt >= 2, N, M, D <= 65535 and H W < 2^31; any D, any
 *     stride, fp32 / bf16 / fp16 storage.  Every other launch, and every variant but GMPI_VARIANT_AUTO, is GMPI_E_VARIANT: these entries run the pair or
 *     return an error, they never fall back to the atomic kernels (which have entries of their own);
 *   - with GMPI_FLAG_GRAD_OVERWRITE every cell inside [Ht, Wt] of each wanted gradient is WRITTEN (no zero-fill needed); without it every such cell is
 *     read, added to and written back by its owner.  Cells of the padding between rows, channels or MPIs are never touched.
 * A term is added only where its bilinear weight is not zero: a pixel whose upstream gradient is not finite reaches the cells of its own footprints
 * only.  The candidate windows assume a pinhole ray field (see ray_dir above); a (view, plane) without a usable homography looks at every pixel.
 * gmpi_query(34) == 1 says that the entries are built in.
 */
int gmpi_mpi_render_shared_backward_gather_launch(const GmpiRenderParams *params, const GmpiSharedColor *shared, const float *grad_rgb_out,
                                                  const float *grad_depth, const float *grad_transmittance, float *grad_shared_rgb,
                                                  const int64_t *grad_shared_rgb_stride, float *grad_alpha, const int64_t *grad_alpha_stride,
                                                  float *grad_background, const int64_t *grad_background_stride, void *stream);
int gmpi_mpi_render_depth_backward_gather_launch(const GmpiRenderParams *params, const GmpiSharedColor *shared, const GmpiDepthAlpha *depth_alpha,
                                                 const float *grad_rgb_out, const float *grad_depth, const float *grad_transmittance,
                                                 float *grad_shared_rgb, const int64_t *grad_shared_rgb_stride, float *grad_depth_image,
                                                 const int64_t *grad_depth_image_stride, float *grad_background,
                                                 const int64_t *grad_background_stride, void *stream);

/* Bytes of workspace the two entries above want for this launch (depth_alpha NULL: the shared-colour entry): the homography records, 24 bytes per view,
 * plane and pixel, and the run slabs, rounded to 256.  0: the pair cannot take the launch -- exactly where the launch returns GMPI_E_VARIANT or an
 * argument error.  Launches nothing. */
uint64_t gmpi_render_layout_backward_gather_workspace_bytes(const GmpiRenderParams *params, const GmpiSharedColor *shared,
                                                            const GmpiDepthAlpha *depth_alpha);

/* The plane runs per texel tile the pair uses for this launch (0 where the query above answers 0), and a hook for tests: a positive `runs` replaces the
 * rule for every later launch and query of this process (rounded to what D allows: ceil(D / ceil(D / runs)) runs), 0 restores it. */
int gmpi_render_layout_backward_gather_runs(const GmpiRenderParams *params, const GmpiSharedColor *shared, const GmpiDepthAlpha *depth_alpha);
void gmpi_render_layout_backward_gather_set_runs(int32_t runs);

/*
 * gmpi_mpi_render_geometry_backward_ex_launch over the two layouts: the gradient of gmpi_mpi_render_shared_launch / gmpi_mpi_render_depth_launch w.r.t.
 * the sample POSITIONS -- by definition that of the volume entry on the expanded volume, which is never materialised.  `params`, `shared` and
 * `depth_alpha` as for the layout's image backward (params->rgba = the alpha planes, resp. the depth image; AUTO and GATHER run the same kernel, any
 * other variant is GMPI_E_VARIANT; GMPI_DTYPE_U8: GMPI_E_DTYPE; a NULL struct: GMPI_E_NULL; their stride codes); grad_rgb [N,3,H,W], grad_depth and
 * grad_transmittance [N,1,H,W] or NULL, and the four outputs as for the volume entry: OVERWRITTEN, NULL = not wanted (all four NULL: GMPI_OK, nothing is
 * launched).  The workspace is the volume entry's: gmpi_render_geometry_backward_workspace_bytes(params, grad_dhw != NULL) bytes (it depends on N, H, W
 * and D only), 256-byte aligned, else GMPI_E_WORKSPACE when grad_eye_pos, grad_z_dir or grad_dhw is wanted.  The formulas are the volume entry's; only
 * the source of the four taps per channel and of the sweep's starting transmittance differs:
 *   shared-colour  channels 0-2 from rgb[m] (background[m] on plane D-1 when given), channel 3 from alpha[m,k]; the start is transmittance_out, with
 *                  the re-walk over the alpha planes when it underflowed;
 *   depth-alpha    channel 3's taps are the ramp of each depth tap -- the forward's correctly rounded quotient for the launch's mode, 0 outside the
 *                  texture -- so the alpha sample and its position derivative are those of the expanded volume with zeros padding; the start is the
 *                  re-walk over the ramp samples (the common path of this layout).  A plane whose four ramp taps are all exactly 0 is skipped for that
 *                  pixel, colour taps included (a NaN colour texel under such a region reaches no gradient); a zero alpha SAMPLE alone does not skip.
 * plane_z as [D] or [M,D], any view_to_mpi / views_per_mpi, GMPI_FLAG_OUT_PM1, GMPI_FLAG_STRICT_ORDER (the forward's chain for the flags), fp32 / bf16 /
 * fp16 storage.  No atomics: every output is bit-reproducible.  No status bit is set.  The gradient w.r.t. plane_z has an entry of its own
 * (gmpi_mpi_render_depth_geometry_backward_pz_launch, below); none w.r.t. the ramp's bounds.  gmpi_query(30) == 1 says that both entries are built in.
 */
int gmpi_mpi_render_shared_geometry_backward_launch(const GmpiRenderParams *params, const GmpiSharedColor *shared, const float *grad_rgb,
                                                    const float *grad_depth, const float *grad_transmittance, float *grad_ray_dir,
                                                    float *grad_eye_pos, float *grad_z_dir, float *grad_dhw, void *stream);
int gmpi_mpi_render_depth_geometry_backward_launch(const GmpiRenderParams *params, const GmpiSharedColor *shared, const GmpiDepthAlpha *depth_alpha,
                                                   const float *grad_rgb, const float *grad_depth, const float *grad_transmittance,
                                                   float *grad_ray_dir, float *grad_eye_pos, float *grad_z_dir, float *grad_dhw, void *stream);

/*
 * gmpi_mpi_render_depth_geometry_backward_launch with the gradient w.r.t. plane_z: same arguments, same checks, same error codes, and grad_plane_z
 * before `stream` -- fp32, contiguous, [M, D] when depth_alpha->plane_z_stride != 0, [D] when it is 0 (ONE table for all MPIs: summed over all
 * views in view order); OVERWRITTEN; NULL = not wanted: the entry above, its kernels and its bits.  The alpha of plane k is a ramp of plane_z[m,k] -
 * depth, so a plane depth acts twice: through dhw[..., 0], where the ray meets the plane (grad_dhw), and through plane_z, how opaque the plane is
 * there (this gradient).  By definition torch autograd's through expand_depth_alpha -- for view n of MPI m, pixel p, plane k, taps i = nw, ne, sw, se:
 *     grad_plane_z[m,k] = (1 / z_den) sum_{n: mpi(n) = m} sum_p  dL/d(alpha sample)(n,p,k)  sum_i w_i in_i tex_i
 * w_i the bilinear weights, in_i: z_lo <= f32(plane_z - d_i) <= z_hi (bounds included, as torch.clamp passes the gradient), tex_i: tap i lies inside
 * the texture; term by term minus plane k's share of the depth image's gradient.  With grad_plane_z a plane is skipped for a pixel only when its
 * four ramp taps are exactly 0 AND none of them lies on the ramp (a tap exactly on the lower bound has alpha 0 and a plane_z term).  The sums go
 * through the workspace like grad_dhw's, one more slab component per plane: gmpi_render_depth_geometry_backward_workspace_bytes(params, grad_dhw !=
 * NULL, grad_plane_z != NULL) bytes, 256-byte aligned, else GMPI_E_WORKSPACE.  No atomics: bit-reproducible.  The other outputs are, bit for bit,
 * those of a launch without grad_plane_z.  gmpi_query(40) == 1 says that the entry is built in.
 */
int gmpi_mpi_render_depth_geometry_backward_pz_launch(const GmpiRenderParams *params, const GmpiSharedColor *shared, const GmpiDepthAlpha *depth_alpha,
                                                      const float *grad_rgb, const float *grad_depth, const float *grad_transmittance,
                                                      float *grad_ray_dir, float *grad_eye_pos, float *grad_z_dir, float *grad_dhw, float *grad_plane_z,
                                                      void *stream);

/* Bytes of workspace gmpi_mpi_render_depth_geometry_backward_pz_launch needs: 6 + 3 D [want_dhw] + D [want_plane_z] floats per 64 x 4 pixel tile and
 * view.  want_plane_z == 0: gmpi_render_geometry_backward_workspace_bytes(params, want_dhw). */
uint64_t gmpi_render_depth_geometry_backward_workspace_bytes(const GmpiRenderParams *params, int want_dhw, int want_plane_z);

/*
 * ---- the shaded render of an RGBA volume ---------------------------------------------------------------------------------------------------------
 * The shading augmentation (LightRenderer: gmpi_light_apply_launch) multiplies the colour of every plane by ONE factor per texel and clips:
 *     shaded[m,k,c] = clip(rgba[m,k,c] * shading[m,0], 0, 1) for c < 3 (fp32, one rounding for the product),  shaded[m,k,3] = rgba[m,k,3].
 * By definition these entries render / back-propagate through THAT volume (apply_shading in the Python package is the executable definition)
 * without building it: the multiply and the clip happen on the taps.  A NaN colour texel is shaded to 0, as gmpi_light_apply_launch's
 * fminf(fmaxf(.)) makes it.  shading: fp32 [M,1,Ht,Wt]; shading_stride = {MPI stride, row stride} in elements, innermost stride 1, row stride >= Wt,
 * an MPI stride of 0 only for M == 1.
 */
typedef struct GmpiShading {
    uint32_t struct_size;         /* = sizeof(GmpiShading)                                             */
    const float *shading;         /* [M,1,Ht,Wt] fp32                                                  */
    int64_t shading_stride[2];    /* MPI, row                                                          */
} GmpiShading;

/*
 * Forward.  params as for gmpi_mpi_render_launch (same outputs, flags and status bits; GMPI_FLAG_CHECK_RANGE tests the alpha taps raw -- the shaded
 * colour is in [0, 1] by construction).  Variants: GMPI_VARIANT_GATHER = the one-pixel-per-lane kernel (render_shaded.hip: any shape, stride, ray
 * field); GMPI_VARIANT_AUTO = the staged kernel where gmpi_render_shaded_supports says 1, else the one-pixel kernel; GMPI_VARIANT_LDS = the staged
 * kernel, GMPI_E_VARIANT where it cannot run; WAVE / BAND: GMPI_E_VARIANT.  GMPI_DTYPE_U8: GMPI_E_DTYPE.  The staged kernel is the shared-colour
 * forward's frame (32 x 16 pixel tiles, texel boxes through LDS) with a fifth loader item per plane for the shading box; gmpi_render_shaded_supports
 * says 1 when its loader can take the tensors: the volume's base pointer and outer strides multiples of 4 texels, the shading's base pointer a
 * multiple of 16 bytes and its strides multiples of 4 (0, or a negative error code the launch would return, otherwise).  For a texture width that is
 * no multiple of 4 the loader reads up to 3 elements past the end of a row: behind the LAST row of each tensor they must be allocated.  In
 * strict-order mode the result is bit-identical to gmpi_mpi_render_launch on the shaded volume, whatever the kernel.  N == 0: GMPI_OK.
 */
int gmpi_mpi_render_shaded_launch(const GmpiRenderParams *params, const GmpiShading *shading, void *stream);
int gmpi_render_shaded_supports(const GmpiRenderParams *params, const GmpiShading *shading);

/*
 * Backward.  As gmpi_mpi_render_backward_ex_launch (grad_depth, grad_transmittance may be NULL; transmittance_out is the forward's T), followed on the
 * same stream by the per-texel chain rule through clip(rgb * s) IN PLACE on grad_rgba:
 *     g_rgb = g * s * [0 <= rgb * s <= 1],   grad_shading[m,0,y,x] = sum over planes and colour channels of g * rgb * [0 <= rgb * s <= 1],
 * alpha untouched (the closed mask: where torch.clip passes a gradient).  grad_rgba: fp32 [M,D,4,Ht,Wt], zero-filled by the caller and added into
 * (grad_rgba_stride: 5 element strides, innermost 1); it first holds the gradient w.r.t. the SHADED texels, and after the call the gradient w.r.t.
 * rgba.  grad_shading: fp32 [M,1,Ht,Wt], WRITTEN (grad_shading_stride: MPI and row stride).  Either of the two may be NULL when the other is not (both
 * NULL: GMPI_E_NULL).  With grad_rgba NULL no volume-sized buffer is involved: the entry zero-fills grad_shading and the one-pixel-per-lane kernel adds
 * the chain rule's terms per tap (4 atomics per pixel and plane; whatever the variant).  Otherwise the kernels are: the one-pixel-per-lane backward (GMPI_VARIANT_GATHER, and every launch the 64 x 8 tile backward's guards refuse: Wt < 2, plane offsets beyond 32 bits)
 * or the 64 x 8 tile backward, both with the taps shaded as the forward shades them.  Never the atomics-free pair; no workspace is read.
 * gmpi_query(38) == 1 says these entries are built in.
 */
int gmpi_mpi_render_shaded_backward_launch(const GmpiRenderParams *params, const GmpiShading *shading, const float *grad_rgb, const float *grad_depth,
                                           const float *grad_transmittance, float *grad_rgba, const int64_t *grad_rgba_stride, float *grad_shading,
                                           const int64_t *grad_shading_stride, void *stream);

/*
 * Diagnostics for a tripped GMPI_STATUS_OUT_OF_LAST_PLANE: min_u, max_u, min_v, max_v of the
 * normalised grid on the LAST plane per view (what mpi.py:106-109 print).  uv_minmax: [N,4] float.
 * Uses N, M, D, H, W, flags(ALIGN_CORNERS), view_to_mpi/views_per_mpi, dhw, ray_dir, eye_pos.
 */
int gmpi_last_plane_uv_minmax_launch(const GmpiRenderParams *params, float *uv_minmax, void *stream);

/*
 * Exhaustive range check over `count` contiguous elements (the reference's two full min/max
 * passes, mpi.py:185-187 and mpi_renderer.py:447-449): ORs GMPI_STATUS_RGBA_RANGE into status[0]
 * when any value is outside [0,1] or NaN.
 */
int gmpi_rgba_range_check_launch(const void *rgba, int32_t rgba_dtype, int64_t count, uint32_t *status,
                                 void *stream);

/*
 * Per-view epilogue of the reference's drivers (render_video.py:118-126, prepare_fake_data.py):
 *   img8  [N,H,W,3] = uint8( ((rgb_pm1 + 1) / 2) * 255 )           (C truncation, as numpy astype)
 *   dep8  [N,H,W,1] = uint8( clip((depth - near) / (far - near), 0, 1) * 255 )
 * rgb is the OUT_PM1 colour [N,3,H,W]; either output may be NULL.  near/far are the Python floats
 * `ray_start`/`ray_end`; as in numpy the subtraction uses float32(near) and the division uses
 * float32(far - near) (difference taken in double).
 */
int gmpi_frames_to_uint8_launch(const float *rgb_pm1, const float *depth, int32_t N, int32_t H, int32_t W,
                                double depth_near, double depth_far, uint8_t *img8, uint8_t *dep8, void *stream);

/*
 * World-space rays of N pinhole views (gmpi/core/camera.py:182-211 `_generate_rays_torch`, called per view
 * from mpi_renderer.py:320-335): for view n with camera-to-world matrix c2w[n] (row-major 4x4, fp32) and the
 * camera-frame unit directions unit_dirs [3, H*W] (camera.py:98-118),
 *     ray_dir[n,c,p] = fma(R[c][2], d2[p], fma(R[c][1], d1[p], R[c][0] * d0[p]))      R = c2w[n][:3,:3]
 *     eye_pos[n]     = c2w[n][:3,3]            z_dir[n] = R[:,2]
 * The FMA order is the one of the reference's CPU `torch.matmul` (3x3 @ 3xN sgemm): it reproduces the rays of
 * the CPU reference bit for bit (tests/test_host_geometry.py, tests/test_hip_parity.py), which the reference's
 * own GPU path (rocBLAS) does not.  All pointers are device pointers.
 */
int gmpi_generate_rays_launch(const float *c2w, const float *unit_dirs, int32_t N, int32_t H, int32_t W,
                              float *ray_dir, float *eye_pos, float *z_dir, void *stream);

/*
 * Expected depth of the UN-WARPED multiplane image (gmpi/core/light_renderer.py:82-100 `LightRenderer.compute_depth`,
 * the same cumprod weights as mpi.py:421-423 with the identity warp):
 *     depth[b,y,x] = sum_k a_k * T_k * plane_ds[k],   T_0 = 1,  T_{k+1} = T_k * ((1 - a_k) + 1e-10)
 * alpha: [B, D, 1, H, W] view (typically channel 3 of the RGBA volume): element strides for B, D and rows are given,
 * the innermost stride is 1.  depth_out [B,1,H,W]; transmittance_out [B,1,H,W] or NULL.  Streaming kernel: one read
 * of the alpha planes.
 */
int gmpi_alpha_depth_launch(const void *alpha, int32_t alpha_dtype, int64_t stride_b, int64_t stride_d, int64_t stride_row,
                            const float *plane_ds, int32_t B, int32_t D, int32_t H, int32_t W, float *depth_out,
                            float *transmittance_out, void *stream);

/*
 * The rest of the reference's shading augmentation (gmpi/core/light_renderer.py `LightRenderer.render`), after
 * gmpi_alpha_depth_launch:
 *  - gmpi_light_blur_launch: torchvision GaussianBlur of the depth images [B,H,W] (light_renderer.py:51-55,109):
 *    reflect padding, 2-D kernel = outer product of `kernel1d` [ksize] (ksize odd, ksize/2 < H, W).
 *  - gmpi_light_shading_launch: point cloud of the blurred depth along the last plane's texel rays (compute_pcl
 *    :102-120; xyz_last [H,W,3] contiguous), normals from the four neighbour cross products with replicate padding
 *    (get_normal :57-80), Lambert term against light_dir [B,3] (unit vectors), shading[b,y,x] = ka + kd * max(-n.l, 0).
 *  - gmpi_light_apply_launch: out[b,k,0:3] = clip(rgba[b,k,0:3] * shading[b], 0, 1), out[b,k,3] = rgba[b,k,3]
 *    (:193-198).  rgba [B,D,4,H,W] with element strides (innermost 1), any storage dtype; out fp32 contiguous.
 */
int gmpi_light_blur_launch(const float *depth, float *blurred, int32_t B, int32_t H, int32_t W, const float *kernel1d,
                           int32_t ksize, void *stream);
int gmpi_light_shading_launch(const float *depth_blurred, const float *xyz_last, const float *light_dir, float ka, float kd,
                              int32_t B, int32_t H, int32_t W, float *shading, void *stream);
int gmpi_light_apply_launch(const void *rgba, int32_t rgba_dtype, const int64_t *rgba_stride, const float *shading, float *out,
                            int32_t B, int32_t D, int32_t H, int32_t W, void *stream);

/*
 * Backward of the two volume-sized ops of the augmentation (the reference runs it inside the G-step with autograd,
 * train.py:535-541):
 *  - gmpi_light_apply_backward_launch: grad_out [B,D,4,H,W] fp32 contiguous -> grad_rgba [B,D,4,H,W] fp32 contiguous
 *    (rgb: grad*shading where 0 <= rgb*shading <= 1, alpha: passed through) and grad_shading [B,H,W].
 *  - gmpi_alpha_depth_backward_launch: gradient of gmpi_alpha_depth_launch w.r.t. alpha, ADDED to grad_alpha (an fp32
 *    [B,D,1,H,W] view with the given element strides, e.g. channel 3 of grad_rgba).  `transmittance` is the forward's
 *    transmittance_out or NULL.
 *  - gmpi_alpha_depth_backward_ex_launch: the same for both outputs: grad_depth and grad_transmittance ([B,1,H,W] fp32)
 *    may each be NULL (both NULL: nothing is added).  dL/da_k = T_k q_k - S_k / om_k with q_k = gZ d_k and
 *    S_k = gT T_out + sum_{j>k} a_j T_j q_j (the derivation of gmpi_mpi_render_backward_ex_launch, same numerics).
 */
int gmpi_light_apply_backward_launch(const void *rgba, int32_t rgba_dtype, const int64_t *rgba_stride, const float *shading,
                                     const float *grad_out, float *grad_rgba, float *grad_shading, int32_t B, int32_t D,
                                     int32_t H, int32_t W, void *stream);
int gmpi_alpha_depth_backward_launch(const void *alpha, int32_t alpha_dtype, int64_t stride_b, int64_t stride_d,
                                     int64_t stride_row, const float *plane_ds, const float *transmittance,
                                     const float *grad_depth, float *grad_alpha, int64_t gstride_b, int64_t gstride_d,
                                     int64_t gstride_row, int32_t B, int32_t D, int32_t H, int32_t W, void *stream);
int gmpi_alpha_depth_backward_ex_launch(const void *alpha, int32_t alpha_dtype, int64_t stride_b, int64_t stride_d,
                                        int64_t stride_row, const float *plane_ds, const float *transmittance,
                                        const float *grad_depth, const float *grad_transmittance, float *grad_alpha,
                                        int64_t gstride_b, int64_t gstride_d, int64_t gstride_row, int32_t B, int32_t D,
                                        int32_t H, int32_t W, void *stream);

/*
 * Backward of the image-sized middle of the augmentation (gmpi_light_blur_launch, gmpi_light_shading_launch), and the image-sized ends of the
 * shared-colour and depth-alpha layouts: what LightRenderer(middle="hip") of the Python package runs instead of torch autograd over a torch
 * restatement.  All four are gathers: one thread owns one cell of each gradient and writes it once.  No atomics: two runs give the same bits.
 * Stream-ordered, allocate nothing, never synchronise.  gmpi_query(46) == 1 says that they are built in.
 *  - gmpi_light_shading_backward_launch: grad_shading [B,H,W] -> grad_blurred [B,H,W] (both fp32 contiguous), the adjoint of
 *    gmpi_light_shading_launch w.r.t. depth_blurred (none w.r.t. xyz_last or light_dir; ka does not enter).  The upstream gradient of an interior
 *    cell is the sum of grad_shading over the pixels that take its normal (replicate padding: 1, 2 or 4 pixels; a whole row, column or image
 *    where H == 3 or W == 3); the clamp passes it where -n.l >= 0, zero included, as torch.clamp does; the normal is the forward's, bit for bit.
 *    Where the un-normalised normal is exactly 0 (a zero depth image, say) the cell contributes 0: torch autograd over the same formula yields NaN
 *    there (pow(0.5) at 0).  H, W >= 3 as in the forward.
 *  - gmpi_light_blur_backward_launch: grad_blurred [B,H,W] -> grad_depth [B,H,W], the adjoint (transpose) of gmpi_light_blur_launch's
 *    reflect-padded separable blur; the same limits: ksize odd, ksize/2 < H, W.
 *  - gmpi_light_shade_images_launch: rgb_out = clip(rgb * shading, 0, 1) and, with a background, background_out likewise.  rgb and background are
 *    [B,3,H,W] in fp32 / bf16 / fp16 (each its own dtype) with element strides {MPI, channel, row} (innermost 1; MPI >= 0, channel > 0, row >= W);
 *    background may be NULL (background_dtype / background_stride / background_out are then ignored); shading [B,H,W] and the outputs [B,3,H,W]
 *    are fp32 contiguous.  A NaN colour shades to 0, as in gmpi_light_apply_launch.
 *  - gmpi_light_shade_images_backward_launch: grad_rgb = grad_rgb_out * shading * mask, grad_background likewise, and
 *    grad_shading[b,y,x] = sum over the channels of BOTH images of grad_*_out * colour * mask, in one launch; mask = [0 <= colour * shading <= 1],
 *    bounds included (gmpi_light_apply_backward_launch's).  A NULL grad_rgb_out / grad_background_out counts as zero; each of the three outputs
 *    may be NULL and is then not written (all three NULL: GMPI_E_NULL; grad_background_out or grad_background without a background: GMPI_E_NULL).
 * Errors, all before any launch: B < 0, H or W <= 0 (< 3 for the shading backward), B or H > 65535, the ksize limits: GMPI_E_SHAPE; B == 0:
 * GMPI_OK; a required pointer NULL: GMPI_E_NULL; a dtype outside fp32 / bf16 / fp16: GMPI_E_DTYPE; a stride outside the above: GMPI_E_STRIDE.
 */
int gmpi_light_shading_backward_launch(const float *depth_blurred, const float *xyz_last, const float *light_dir, float kd,
                                       const float *grad_shading, int32_t B, int32_t H, int32_t W, float *grad_blurred, void *stream);
int gmpi_light_blur_backward_launch(const float *grad_blurred, float *grad_depth, int32_t B, int32_t H, int32_t W,
                                    const float *kernel1d, int32_t ksize, void *stream);
int gmpi_light_shade_images_launch(const void *rgb, int32_t rgb_dtype, const int64_t *rgb_stride, const void *background,
                                   int32_t background_dtype, const int64_t *background_stride, const float *shading, float *rgb_out,
                                   float *background_out, int32_t B, int32_t H, int32_t W, void *stream);
int gmpi_light_shade_images_backward_launch(const void *rgb, int32_t rgb_dtype, const int64_t *rgb_stride, const void *background,
                                            int32_t background_dtype, const int64_t *background_stride, const float *shading,
                                            const float *grad_rgb_out, const float *grad_background_out, float *grad_rgb,
                                            float *grad_background, float *grad_shading, int32_t B, int32_t H, int32_t W, void *stream);

/*
 * gmpi_alpha_depth_launch and gmpi_alpha_depth_backward_ex_launch for a depth-alpha MPI, WITHOUT the alpha planes (what the shading augmentation
 * needs of this layout: LightRenderer.render_depth in the Python package).  By definition gmpi_ramp_depth_launch equals gmpi_alpha_depth_launch on
 *     a_k = (min(max(plane_z[k] - depth, z_lo), z_hi) - z_lo) / z_den       (GmpiDepthAlpha above: fp32, one rounding per step, the IEEE quotient),
 * bit for bit in depth_out and transmittance_out ([B,1,H,W] fp32; transmittance_out may be NULL); the planes are never materialised: one thread
 * holds one depth texel in a register and walks the planes there.  depth_image: [B,1,H,W] in fp32 / bf16 / fp16 (GMPI_DTYPE_U8: GMPI_E_DTYPE),
 * innermost stride 1, stride_row >= W, stride_b >= 0 (an expanded batch, the channel view of an RGB-D tensor).  ramp->plane_z is [D] or [B,D]
 * through plane_z_stride; plane_ds [D] are the metric plane distances (another table than plane_z).
 * The backward gives the gradient w.r.t. the depth image through both outputs (grad_depth, grad_transmittance: [B,1,H,W] fp32, each may be NULL;
 * both NULL: nothing is added): dL/da_k as gmpi_alpha_depth_backward_ex_launch computes it (same numerics; `transmittance` is the forward's
 * transmittance_out or NULL), and plane k contributes -dL/da_k / z_den to its texel where z_lo <= plane_z[k] - depth <= z_hi, bounds included,
 * nothing elsewhere.  The sum is ADDED to grad_depth_image (fp32 [B,1,H,W] view: gstride_b > 0, gstride_row >= W, innermost stride 1; zeroed by
 * the caller) with a plain load, add and store: one thread owns a texel, there are no atomics.
 * Errors, all before any launch: D, H, W <= 0, B < 0, B or H > 65535: GMPI_E_SHAPE; B == 0: GMPI_OK; a NULL depth_image, ramp, ramp->plane_z,
 * plane_ds, depth_out / grad_depth_image: GMPI_E_NULL; ramp->struct_size: GMPI_E_ABI; z_lo >= z_hi or z_den <= 0 (or a NaN among them):
 * GMPI_E_SHAPE; a stride outside the above: GMPI_E_STRIDE.  Stream-ordered, allocate nothing, never synchronise.  gmpi_query(32) == 1 says that
 * both entries are built in.
 */
int gmpi_ramp_depth_launch(const void *depth_image, int32_t depth_dtype, int64_t stride_b, int64_t stride_row,
                           const GmpiDepthAlpha *ramp, const float *plane_ds, int32_t B, int32_t D, int32_t H, int32_t W,
                           float *depth_out, float *transmittance_out, void *stream);
int gmpi_ramp_depth_backward_launch(const void *depth_image, int32_t depth_dtype, int64_t stride_b, int64_t stride_row,
                                    const GmpiDepthAlpha *ramp, const float *plane_ds, const float *transmittance,
                                    const float *grad_depth, const float *grad_transmittance, float *grad_depth_image,
                                    int64_t gstride_b, int64_t gstride_row, int32_t B, int32_t D, int32_t H, int32_t W,
                                    void *stream);

/*
 * Self-test of the default mode's division: the coordinate chain (mpi.py:76, 89-90) divides through correctly rounded
 * reciprocals hoisted out of the plane loop (q0 = n*r, e = fma(-d, q0, n), q = fma(e, r, q0) with r = RN(1/d)); this entry
 * compares that against the IEEE division on `pairs` pseudo-random operand pairs (classes: 0 zdiff/ray_z, 1 x/(w/2),
 * 2 full-range significands with exponents within +-20, 3 divisors 2^k (2 - 2^-23)) and ADDS the number of pairs whose
 * quotients differ in any bit to mismatches[class] (device memory, 4 x uint64, zero-filled by the caller).
 */
int gmpi_selftest_division_launch(uint64_t pairs, uint32_t seed, uint64_t *mismatches, void *stream);

/*
 * Diagnostic: one read-only pass over `bytes` of device memory with the fastest read pattern measured on gfx950 (non-temporal dword loads,
 * profiles/r03_calibration.txt).  bench.py times it over the render's own volume and quotes the rate as `roofline.stream_read_gbs`: what a
 * kernel that did nothing but read the volume would reach on this box.  `sink` (4 bytes, may be NULL) only keeps the loads alive.
 */
int gmpi_stream_probe_launch(const void *buf, uint64_t bytes, uint32_t *sink, void *stream);

/* what: 0 ABI version, 1 sizeof(GmpiRenderParams), 2 target arch number (950), 3 LDS bytes the
 * LDS variant uses per workgroup, 4 pixel-tile width, 5 pixel-tile height, 6 whether
 * GMPI_VARIANT_WAVE is built in, 7 GMPI_VARIANT_DMA (retired: 0), 8 GMPI_VARIANT_BAND, 9 the number of 256 x 8 pixel bands from which
 * GMPI_VARIANT_AUTO uses the band kernel on bf16 volumes, 10 the number of 128 x 8 pixel bands on fp32 volumes, 11 whether the atomics-free
 * backward is built in; the staged shared-colour forward (gmpi_mpi_render_shared_launch with GMPI_VARIANT_LDS): 12 its pixel-tile width (a tile
 * is 512 / width pixels high), 13 the texels per row and 14 the rows its staging buffer holds per plane (a box's first column is rounded down to
 * a multiple of 4 texels before it is held against 13); 15 is unused (-1); the staged kernel for GMPI_DTYPE_U8 volumes: 16 its pixel-tile width (a tile
 * is 512 / width pixels high), 17 the texels per row and 18 the rows its staging buffer holds per plane (first column rounded down to a multiple of 4
 * texels, as for 13); 19 is unused (-1); 20 whether the interleaved GMPI_DTYPE_U8 layout (GmpiRenderParams.rgba_stride) is built in; 21 is unused (-1);
 * 22 whether the depth-alpha layout (gmpi_mpi_render_depth_launch) is built in; 23 the number of planes the depth-alpha tile backward
 * (gmpi_mpi_render_depth_backward_tile_launch) takes: more go to the one-pixel-per-lane kernel; 24 is unused (-1); the depth-alpha window forward
 * (gmpi_mpi_render_depth_window_launch): 25 whether it is built in, 26 / 27 the width / height of its window in texels, 28 the planes per refill of
 * its box table; 29 is unused (-1); 30 whether the geometry backward of the shared-colour and depth-alpha layouts (gmpi_mpi_render_shared_geometry_backward_launch,
 * gmpi_mpi_render_depth_geometry_backward_launch) is built in; 31 is unused (-1); 32 whether compute_depth of the depth-alpha layout
 * (gmpi_ramp_depth_launch, gmpi_ramp_depth_backward_launch) is built in; 33 is unused (-1); 34 whether the atomics-free backward of the shared-colour
 * and depth-alpha layouts (gmpi_mpi_render_shared_backward_gather_launch, gmpi_mpi_render_depth_backward_gather_launch) is built in; 35 is unused (-1); 36 whether the plane-chunked render (gmpi_mpi_render_chunk_launch,
 * gmpi_mpi_render_chunk_backward_launch) is built in; 37 is unused (-1); 38 whether the shaded render of an RGBA volume (gmpi_mpi_render_shaded_launch,
 * gmpi_mpi_render_shaded_backward_launch) is built in; 39 is unused (-1); 40 whether the gradient w.r.t. plane_z of the depth-alpha layout
 * (gmpi_mpi_render_depth_geometry_backward_pz_launch) is built in; 41 is unused (-1); 42 whether channels-last float layers
 * (gmpi_mpi_render_layers_launch, gmpi_render_layers_supports) are built in; 43 is unused (-1); 44 whether their in-place backward
 * (gmpi_mpi_render_layers_backward_launch, gmpi_render_layers_backward_supports) is built in; 45 is unused (-1); 46 whether the backward of the shading augmentation's image-sized middle and
 * the shade-images pair (gmpi_light_shading_backward_launch, gmpi_light_blur_backward_launch, gmpi_light_shade_images_launch,
 * gmpi_light_shade_images_backward_launch) are built in; 47 is unused (-1); 48 whether the geometry backward over 8-bit volumes and float layers in place
 * (gmpi_mpi_render_u8_geometry_backward_launch, gmpi_mpi_render_layers_geometry_backward_launch, gmpi_render_geometry_inplace_workspace_bytes) is built in;
 * 49 is unused (-1); 50 whether the plane-chunked render through the band kernel (gmpi_mpi_render_chunk_band_launch, gmpi_render_chunk_band_workspace_bytes,
 * gmpi_render_chunk_band_supports) is built in; 51 is unused (-1); 52 whether the occupancy map and the sparse render of GMPI_DTYPE_U8 volumes
 * (gmpi_u8_occupancy_bytes, gmpi_u8_occupancy_launch, gmpi_mpi_render_u8_sparse_launch, gmpi_render_u8_sparse_supports) are built in; 53 the side of a block of
 * that map in texels (16).
 * Unknown -> -1.  */
int gmpi_query(int32_t what);

const char *gmpi_version_string(void);

#ifdef __cplusplus
}
#endif
#endif /* GMPI_RENDER_H */
