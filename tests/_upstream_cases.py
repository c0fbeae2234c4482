"""Upstream gradients other than dense N(0,1), and the small scenes they are run on: tests/test_upstream_cases_cpu.py checks on the CPU, on the
references alone, the conditions that make the GPU comparisons mean something; tests/test_hip_upstream_gradients.py runs every backward kernel on
exactly these inputs.  CPU only (numpy / torch), never imported by the product.

The staged backwards are data-dependent on the upstream gradients: the fixed-point scale of a tile and plane comes from the largest |sample
gradient| (render_backward.hip `gmax`), the headroom `hbits` from how many taps can meet in one texel, a non-finite maximum un-stages the plane, an
all-zero tile returns early.  One family per hazard (`FAMILIES`), on the frame of `_deep_cases.TWIN_*` (20 x 150 pixels: three ragged columns of
64-pixel tiles, rows of 8; D = 5, M = 2, `_cam(..., tilt=0.3)`, `_dhw`) with alphas in [0.05, 0.6], over textures chosen by the box and area
arithmetic of `tile_box` restated here (`tile_paths`): one per path of the default 64 x 8 tile backward."""
import functools

import numpy as np
import torch

import oracle
from test_hip_edge_cases import _cam, _dhw

H, W, D, M = 20, 150, 5, 2
FAMILIES = ("normal", "down40", "up40", "same_sign", "sparse", "two_scale", "inf_pixel", "nan_pixel")
FINITE = FAMILIES[:6]
# name -> (Ht, Wt) and the path every plane and tile of view 0 takes in render_backward_tile2_body (asserted by tests/test_upstream_cases_cpu.py):
#   twin    the twins' own texture: staged, one word per cell
#   broad   the widest texture whose boxes still fit (80 columns x 19 rows): staged, few taps per texel; the footprints of a dozen pixels cover a
#           few percent of a plane, which `sparse` needs for its `far` mask to leave out at most a tenth (on `twin` they cover an eighth)
#   coarse  ~7 to 30 pixels per texel: staged, one word per cell, hbits 7-8
#   wide    a few texels per tile: staged, two words per cell (the `wide` path), hbits >= 9
#   fine    no box fits: every plane scatters straight to global memory
TEXTURES = {"twin": (36, 52), "broad": (42, 170), "coarse": (14, 28), "wide": (6, 18), "fine": (260, 48)}
PATHS = {"twin": "narrow", "broad": "narrow", "coarse": "narrow", "wide": "wide", "fine": "direct"}
LAST_EXTENT = {"coarse": 0.25}   # the last plane as large as the others (`_dhw`'s default doubles it, which quadruples its pixels per texel: no one
                                 # texture then keeps every plane between 2^6 and 2^8 taps)
HBITS = {"twin": (5, 7), "broad": (4, 5), "coarse": (7, 8), "wide": (9, 11)}
# the textures on which the `far` mask of a family leaves out at most a tenth of a slab (a pixel's footprint is up to 5 x 5 texels): a quality
# gate of the CPU test.  The GPU tests apply the mask on every texture: smaller on the coarse ones, never empty
FAR_TEXTURES = {"sparse": ("broad", "fine"), "inf_pixel": ("twin", "broad", "coarse", "fine"), "nan_pixel": ("twin", "broad", "coarse", "fine")}
# `same_sign` asks the headroom of the STAGED paths its worst case; there the fp32 chain is within 1e-5 of float64 per slab.  On `broad` and `fine`
# the sample coordinates reach 170 and 260: their fp32 rounding (2^-17, 2^-16 of a texel) is 2 to 3e-5 of a bilinear weight, whatever sums them
SAME_SIGN_TIGHT = ("twin", "coarse", "wide")
POISON = (0, 11, 75)   # (view n0, py, px): off the tile seams of both tile shapes, near the image centre (its samples move little from plane to plane)
# `sparse`: (py, px, which of colour / depth / T carry a value).  The four corners, both sides of the 64- and the 32-pixel seams in x and of the 8-
# and the 16-pixel seams in y, and two interior pixels, each alone in its 64 x 8 tile, one with a depth gradient only and one with a T gradient
# only: the tile's colour maximum is 0 while its alpha maximum is not.  (Ten pixels: with twelve the footprints of all planes together cover more
# than a tenth of `broad`, which the images the two layouts share between their planes must not lose to the `far` mask.)
SPARSE_PIXELS = [(0, 0, "cdT"), (0, W - 1, "cdT"), (H - 1, 0, "cdT"), (H - 1, W - 1, "cdT"), (7, 63, "cdT"), (8, 64, "cdT"), (15, 31, "cdT"),
                 (16, 32, "cdT"), (12, 130, "d"), (18, 80, "T")]
SPARSE_ZERO_VIEW = 1
TWO_SCALE_X = 64


def upstream(name, N, H, W, seed):
    """(gc [N,3,H,W], gd [N,1,H,W], gT [N,1,H,W]) float32 of family `name`, all built from one N(0,1) draw."""
    g = np.random.default_rng(seed)
    g0 = [g.standard_normal((N, c, H, W)).astype(np.float32) for c in (3, 1, 1)]
    if name == "normal":
        return tuple(g0)
    if name in ("down40", "up40"):
        return tuple(np.ldexp(a, -40 if name == "down40" else 40).astype(np.float32) for a in g0)
    if name == "same_sign":
        return tuple(np.full_like(a, np.nextafter(np.float32(2), np.float32(0))) for a in g0)
    if name == "sparse":
        out = [np.zeros_like(a) for a in g0]
        for n in range(N):
            if n == SPARSE_ZERO_VIEW:
                continue
            for py, px, what in SPARSE_PIXELS:
                for a, a0, key in zip(out, g0, "cdT"):
                    if key in what:
                        a[n, :, py, px] = a0[n, :, py, px]
        return tuple(out)
    if name == "two_scale":
        out = [a.copy() for a in g0]
        for a in out:
            a[..., TWO_SCALE_X:] = np.ldexp(a[..., TWO_SCALE_X:], -20)
        return tuple(out)
    n0, py, px = POISON
    if name == "inf_pixel":
        g0[0][n0, :, py, px] = np.inf
    elif name == "nan_pixel":
        g0[1][n0, 0, py, px] = np.nan
    else:
        raise KeyError(name)
    return tuple(g0)


def nonzero_pixels(name, N):
    """{view: [(py, px), ...]} of the pixels of `sparse` that carry a gradient / of the poisoned pixel."""
    if name == "sparse":
        return {n: [(py, px) for py, px, _ in SPARSE_PIXELS] for n in range(N) if n != SPARSE_ZERO_VIEW}
    return {POISON[0]: [POISON[1:]]}


@functools.lru_cache(maxsize=None)
def scene(tex, vpm=None, dtype="f32", shaded=False, field=None):
    """The volume-path inputs on texture `tex`: `_deep_cases.grad_case`'s dict (rgba holding the STORED values) plus ac, H, W, vpm, Ht, Wt and,
    shaded, the shading image (the colours moved to 1.3 rgb - 0.15 first, as `_deep_cases.twin_case` does).  vpm = 2: four views, two per MPI.
    No upstream gradients: `with_upstream` adds a family's.  Computed once and left unchanged.  field: a ray field of tests/_ray_field_cases.py
    by name in place of the pinhole camera's rays (None: the camera's own); the references below read the same tensor."""
    Ht, Wt = TEXTURES[tex]
    N = M * (vpm or 1)
    rgba = oracle.synth_rgba(41, (M, D, 4, Ht, Wt))
    if shaded:
        rgba[:, :, :3] = 1.3 * rgba[:, :, :3] - 0.15
    rgba[:, :, 3] = 0.05 + 0.55 * rgba[:, :, 3]
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype]
    rgba = torch.from_numpy(rgba).to(tdt).float().numpy()
    ray, eye, zd = _cam(N, H, W, seed=42, tilt=0.3)
    if field is not None:
        import _ray_field_cases
        ray = _ray_field_cases.apply(field, ray)
    v2m = np.asarray([n // (vpm or 1) for n in range(N)], dtype=np.int32)
    case = dict(rgba=rgba, dhw=_dhw(M, D, last=LAST_EXTENT.get(tex, 0.5)), ray=ray, eye=eye, zd=zd, v2m=v2m, dtype=tdt, D=D, N=N, M=M, ac=True, H=H, W=W, vpm=vpm, Ht=Ht, Wt=Wt)
    if shaded:
        from test_hip_shaded_render import make_shading
        case["shading"] = make_shading(5, torch.from_numpy(rgba)).numpy()
    return case


def with_upstream(case, family, seed=5):
    gc, gd, gT = upstream(family, case["N"], case["H"], case["W"], seed)
    return dict(case, gc=gc, gd=gd, gT=gT)


@functools.lru_cache(maxsize=None)
def volume_refs(tex, family, vpm=None, dtype="f32", shaded=False, field=None):
    """(float64, fp32) references of the volume gradient (shaded: each the pair (volume, shading)), computed once."""
    import _deep_cases
    case = with_upstream(scene(tex, vpm, dtype, shaded, field), family)
    return tuple(_deep_cases.volume_grad_ref(case, dt, align_corners=True, shading=case.get("shading")) for dt in (torch.float64, torch.float32))


@functools.lru_cache(maxsize=None)
def layout_parts(kind, tex):
    """The two image layouts on the scene of `tex`, with a background: (rgb, alpha planes | depth image, background) fp32 tensors and, for the
    depth-alpha layout, (plane_z, z_bounds)."""
    case = scene(tex)
    rgba = torch.from_numpy(case["rgba"])
    rgb, bg = rgba[:, 0, :3].contiguous(), rgba[:, -1, :3].contiguous()
    if kind == "shared":
        return (rgb, rgba[:, :, 3:].contiguous(), bg), None
    import test_hip_depth_alpha as DA
    Ht, Wt = TEXTURES[tex]
    depth, plane_z = DA._depth_image(M, max(Ht, Wt), D, 4)
    return (rgb, depth[:, :, :Ht, :Wt].contiguous(), bg), (plane_z, DA._bounds(4))


@functools.lru_cache(maxsize=None)
def layout_refs(kind, tex, family, vpm=None, field=None):
    """(float64, fp32) autograd gradients [rgb, alpha | depth, background] through `expand_shared_color` / `expand_depth_alpha`, computed once."""
    case = with_upstream(scene(tex, vpm, field=field), family)
    parts, extra = layout_parts(kind, tex)
    v2m = [int(m) for m in case["v2m"]]
    out = []
    for dt in (torch.float64, torch.float32):
        if kind == "shared":
            import test_hip_shared_color as SC
            out.append(SC._reference_grads(parts, case["dhw"], case["ray"], case["eye"], case["zd"], v2m, case["gc"], case["gd"], case["gT"], False, dt))
        else:
            import test_hip_depth_alpha as DA
            tup = (parts[0], parts[1], extra[0], parts[2], torch.as_tensor(case["dhw"]), case["ray"], case["eye"], case["zd"], extra[1])
            out.append(DA._reference_grads(tup, True, v2m, case["gc"], case["gd"], case["gT"], False, dt))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def geometry_refs(tex, family):
    """float64 gradients (dhw, ray, eye, z_dir) of tests/_geometry_ref.py for colour and depth upstream (the geometry reference has no T output)."""
    from _geometry_ref import geometry_grads
    case = with_upstream(scene(tex), family)
    return geometry_grads(case["rgba"], case["dhw"], case["ray"], case["eye"], case["zd"], case["v2m"], case["gc"], case["gd"], align_corners=True)


# ---- masks --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _coords(tex, vpm):
    case = scene(tex, vpm)
    return oracle.coords(case["dhw"], case["ray"], case["eye"], case["Ht"], case["Wt"], view_to_mpi=case["v2m"])


def _near(tex, vpm, pixels):
    """[M,D,Ht,Wt] bool: the texels within 2 (in x and in y) of a sample position, on that plane, of one of `pixels` = {view: (ys, xs) index arrays}
    -- the CPU oracle's coordinate chain."""
    case = scene(tex, vpm)
    Ht, Wt = case["Ht"], case["Wt"]
    ix, iy = _coords(tex, vpm)
    near = np.zeros((M, D, Ht, Wt), dtype=bool)
    for n, (ys, xs) in pixels.items():
        m = int(case["v2m"][n])
        for k in range(D):
            sx, sy = ix[n, k][ys, xs].astype(np.float64).ravel(), iy[n, k][ys, xs].astype(np.float64).ravel()
            ok = np.isfinite(sx) & np.isfinite(sy) & (np.abs(sx) < 1e6) & (np.abs(sy) < 1e6)
            sx, sy = sx[ok], sy[ok]
            x0, y0 = np.ceil(sx - 2).astype(np.int64), np.ceil(sy - 2).astype(np.int64)
            for dy in range(5):
                for dx in range(5):
                    xt, yt = x0 + dx, y0 + dy
                    on = (xt <= sx + 2) & (yt <= sy + 2) & (xt >= 0) & (xt < Wt) & (yt >= 0) & (yt < Ht)
                    near[m, k, yt[on], xt[on]] = True
    return near


@functools.lru_cache(maxsize=None)
def far_mask(tex, family, vpm=None):
    """[M,D,Ht,Wt] bool: texels more than 2 away from every sample position, on that plane, of the pixels of `family` that carry a (non-zero /
    poisoned) gradient.  For an image shared by the planes take `.all(1)`."""
    N = M * (vpm or 1)
    pix = {n: (np.array([p[0] for p in v]), np.array([p[1] for p in v])) for n, v in nonzero_pixels(family, N).items()}
    return ~_near(tex, vpm, pix)


@functools.lru_cache(maxsize=None)
def right_region(tex, vpm=None):
    """R [M,D,Ht,Wt] bool of `two_scale`: texels more than 2 away from every sample of a pixel with x < 64."""
    N = M * (vpm or 1)
    ys, xs = (a.ravel() for a in np.meshgrid(np.arange(H), np.arange(TWO_SCALE_X), indexing="ij"))
    return ~_near(tex, vpm, {n: (ys, xs) for n in range(N)})


def mask_for(mask, g):
    """`mask` [M,D,Ht,Wt] broadcast to gradient `g`: [M,D,C,Ht,Wt] per plane; [M,C,Ht,Wt] (an image shared by the planes) all planes at once."""
    if g.ndim == 5:
        return np.broadcast_to(mask[:, :, None], g.shape)
    return np.broadcast_to(mask.all(1)[:, None], g.shape)


def peak_texels(tex, vpm=None):
    """Per plane the texel (m, k, y, x) that carries the poisoned pixel's largest bilinear weight (>= 0.25), and whether all four taps lie inside."""
    case = scene(tex, vpm)
    ix, iy = _coords(tex, vpm)
    n0, py, px = POISON
    out = []
    for k in range(D):
        x, y = float(ix[n0, k, py, px]), float(iy[n0, k, py, px])
        inside = 0 <= np.floor(x) and np.floor(x) + 1 <= case["Wt"] - 1 and 0 <= np.floor(y) and np.floor(y) + 1 <= case["Ht"] - 1
        out.append((int(case["v2m"][n0]), k, int(np.floor(y + 0.5)), int(np.floor(x + 0.5)), bool(inside)))
    return out


# ---- which path the 64 x 8 tile backward takes --------------------------------------------------------------------------------------------------
def tile_paths(tex, view=0, tw=64, th=8, pitch=80, rows=19):
    """For every (tile, plane) of `view`: (fits, hbits, wide) by `item_box<1>` / `tile_box` (gmpi_device.hpp) and the headroom rule of
    render_backward_tile2_body `build_tables` (render_backward.hip), restated in float64: the box is the extent of the tile's four corner pixels
    grown by 1/64 texel and the 2 x 2 support; the density comes from the area of the corners' quadrilateral, bound = ceil(8 npix / area) + 8 taps,
    hbits = min(11, bits(bound - 1)); two words per cell when hbits >= 9 and the box rows fill at most half of the buffer."""
    case = scene(tex)
    dhw, ray, eye = (np.asarray(case[k], dtype=np.float64) for k in ("dhw", "ray", "eye"))
    Ht, Wt = case["Ht"], case["Wt"]
    cap = pitch * rows * 4
    out = []
    for y0 in range(0, H, th):
        for x0 in range(0, W, tw):
            y1, x1 = min(y0 + th - 1, H - 1), min(x0 + tw - 1, W - 1)
            npix = (x1 - x0 + 1) * (y1 - y0 + 1)
            r = ray[view][:, [y0, y0, y1, y1], [x0, x1, x0, x1]]            # corners (x0,y0) (x1,y0) (x0,y1) (x1,y1)
            for d, ph, pw in dhw[case["v2m"][view]]:
                s = (d - eye[view, 2]) / r[2]
                u, v = 2 * (eye[view, 0] + r[0] * s) / pw, 2 * (eye[view, 1] + r[1] * s) / ph
                cx, cy = (u + 1) * (Wt - 1) / 2, (v + 1) * (Ht - 1) / 2
                slack = 1.0 / 64
                nx = int(np.floor(cx.max() + slack)) + 1 - int(np.floor(cx.min() - slack)) + 1
                ny = int(np.floor(cy.max() + slack)) + 1 - int(np.floor(cy.min() - slack)) + 1
                fits = nx <= pitch and ny <= rows
                quad2 = abs((cx[0] * cy[1] - cx[1] * cy[0]) + (cx[1] * cy[3] - cx[3] * cy[1]) + (cx[3] * cy[2] - cx[2] * cy[3]) + (cx[2] * cy[0] - cx[0] * cy[2]))
                area = max(min(int(0.5 * quad2), (nx - 1) * (ny - 1)), 1)
                bound = (8 * npix + area - 1) // area + 8
                hbits = min(11, int(bound - 1).bit_length())
                wide = hbits >= 9 and ny * 4 * pitch <= cap // 2
                out.append(dict(fits=fits, hbits=hbits, wide=wide, nx=nx, ny=ny, area=area, margin=min(pitch - nx, rows - ny) if fits else max(nx - pitch, ny - rows)))
    return out


# ---- every reference a family is compared against -----------------------------------------------------------------------------------------------
def reference_sets(tex, family):
    """[(label, vpm, [float64 gradients], [fp32 gradients])] of the references tests/test_hip_upstream_gradients.py compares with on texture
    `tex`: the volume gradient (fp32 and bf16 storage; two views per MPI on the twins' texture), the shaded pair, the two layouts' triples."""
    out = []
    for label, vpm, dtype in (("volume", None, "f32"), ("volume bf16", None, "bf16")) + ((("volume vpm2", 2, "f32"),) if tex == "twin" else ()):
        r64, r32 = volume_refs(tex, family, vpm, dtype)
        out.append((label, vpm, [r64], [r32]))
    r64, r32 = volume_refs(tex, family, None, "f32", True)
    out.append(("shaded", None, list(r64), list(r32)))
    for kind in ("shared", "depth"):
        r64, r32 = layout_refs(kind, tex, family)
        out.append((kind, None, list(r64), list(r32)))
    return out
