"""Ray fields that are not a pinhole camera's, on the scenes of tests/_upstream_cases.py, and the host restatement of the rule the LDS-staged kernels
size a tile's texel box by: tests/test_ray_field_cases_cpu.py checks on the CPU, on the inputs and references alone, the conditions that make the
GPU comparisons mean something; tests/test_hip_ray_fields.py runs the staged kernels on exactly these inputs.  CPU only (numpy), never imported
by the product, and it imports nothing of the product: the kernels' tile shapes and buffer limits are read out of their sources (`constants`).

Every staged kernel takes a tile's texel box on a plane from the tile's four CORNER pixels (gmpi_device.hpp `tile_corners`, `corner_extent`,
`item_box`); a pixel whose 2 x 2 taps the box does not hold takes a per-lane path.  A pinhole camera never sends a pixel there.  The fields below
leave every corner pixel of every tiling the kernels use bit-identical (`fixed_mask`), so every box is the pinhole field's, and move the others:

    pinhole    the unchanged field: the control, no footprint leaves its box
    permuted   a seeded quarter of the free pixels exchange their rays among themselves across the whole image, the same exchange in every view
               (`permutation`): their footprints land far from their tile's box.  A render of the permuted field under permuted upstream
               gradients is the pinhole render's sum in another order
    bulge      ray_y += A gy(y) gx(x), ray_x += A / 2 gy(y) gx(x), gx and gy sin^2 bumps between consecutive fixed columns / rows and 0 on them,
               NOT renormalised (the references read the same tensor; a float32 renormalisation would move the corner bits): a continuum of
               footprints that straddle a box edge -- where an off-by-one of the in-box test lives

`classify` sorts every (pixel, plane) of a view with a non-zero weight into in_box / straddle / far / unstaged under one tiling."""
import functools
import os
import re

import numpy as np

import oracle
import _upstream_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ml-gmpi_amd", "csrc")
FIELDS = ("pinhole", "permuted", "bulge")
MOVED = FIELDS[1:]
BULGE_A = 0.04           # ray units: 0.04 / (plane extent 0.25 / 2) of half a texture in y, half of that in x (5.6 x 4.1 texels on `twin`)
PERMUTED_FRACTION = 4    # one free pixel in four takes part in the exchange
PERMUTED_SEED = 1234
IN_BOX, STRADDLE, FAR, UNSTAGED, NO_WEIGHT = 0, 1, 2, 3, 4
CLASSES = ("in_box", "straddle", "far", "unstaged", "no_weight")
BOX_SLACK = np.float32(1.0 / 64)   # kBoxSlack (gmpi_device.hpp)


# ---- the kernels' own constants ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def constants():
    """{name: int} of the tile shapes and staging limits, read out of the kernel sources."""
    def grab(fname, names):
        src = open(os.path.join(CSRC, fname)).read()
        out = {}
        for name in names:
            m = re.search(r"\b%s = (\d+)\b" % name, src)
            assert m, (fname, name)
            out[name] = int(m.group(1))
        return out
    c = {}
    c.update(grab("render_backward.hip", ("kBwdTW", "kBwdTH", "kBwdPitch", "kBwdRows", "kBwdDefaultGeo")))
    src = open(os.path.join(CSRC, "render_backward.hip")).read()
    for name in ("B2Tall", "B2Wide"):
        m = re.search(r"using %s = B2Geo<(\d+), (\d+), (\d+), (\d+)>;" % name, src)
        assert m, name
        c[name] = tuple(int(v) for v in m.groups())
    c.update(grab("render_shared.hip", ("kSAP", "kSAR")))
    c.update(grab("gmpi_backward.hpp", ("kTileW", "kTileH", "kCW", "kCH")))
    c.update(grab("gmpi_staged_forward.hpp", ("kSFW", "kSFH", "kSFPitch", "kSFRows", "kSFTPI")))
    c.update(grab("render_u8.hip", ("kUW", "kUH", "kUPitch", "kURows", "kUTPI")))
    return c


@functools.lru_cache(maxsize=None)
def tilings():
    """{name: (tile width, tile height, texels per box line, box rows, texels per loader item)} of every staged kernel the GPU tests run:
      backward   the volume tile backward's shipped geometry with its chunk and shaded instances (render_backward.hip kB2Pitch x kB2Rows of B2Wide)
      backward1  the first tile backward's (kBwdPitch x kBwdRows; B2Tall is the same): a one-column texture or 64-bit plane offsets reach it
      alpha      the shared-colour tile backward's alpha box (render_shared.hip kSAP x kSAR)
      window     the cross-plane window: the shared-colour tile backward's colour sums, the depth-alpha tile backward, the depth window forward
      forward    the staged shared-colour and shaded forwards' buffer (gmpi_staged_forward.hpp), loaded in items of 4 texels
      u8         the uint8 staged forward (render_u8.hip), loaded in items of 4 texels"""
    c = constants()
    wide = c["B2Wide"] if c["kBwdDefaultGeo"] == 2 else c["B2Tall"]
    assert c["B2Tall"] == (c["kBwdTW"], c["kBwdTH"], c["kBwdPitch"], c["kBwdRows"])
    return {
        "backward": wide + (1,),
        "backward1": (c["kBwdTW"], c["kBwdTH"], c["kBwdPitch"], c["kBwdRows"], 1),
        "alpha": (c["kTileW"], c["kTileH"], c["kSAP"], c["kSAR"], 1),
        "window": (c["kTileW"], c["kTileH"], c["kCW"], c["kCH"], 1),
        "forward": (c["kSFW"], c["kSFH"], c["kSFPitch"], c["kSFRows"], c["kSFTPI"]),
        "u8": (c["kUW"], c["kUH"], c["kUPitch"], c["kURows"], c["kUTPI"]),
    }


# ---- fixed pixels -----------------------------------------------------------------------------------------------------------------------------------
def _corner_lines(size, step):
    """First and last column (row) of every tile, clamped as `tile_corners` clamps."""
    out = set()
    for c0 in range(0, size, step):
        out.update((c0, min(c0 + step - 1, size - 1)))
    return out


@functools.lru_cache(maxsize=None)
def fixed_axes(H=U.H, W=U.W):
    """(X0, Y0): the sorted corner columns and rows of every tiling."""
    xs, ys = set(), set()
    for tw, th, *_ in tilings().values():
        xs |= _corner_lines(W, tw)
        ys |= _corner_lines(H, th)
    return tuple(sorted(xs)), tuple(sorted(ys))


@functools.lru_cache(maxsize=None)
def fixed_mask(H=U.H, W=U.W):
    """[H,W] bool: x in X0 or y in Y0 -- a superset of every tile's corner pixels."""
    X0, Y0 = fixed_axes(H, W)
    m = np.zeros((H, W), dtype=bool)
    m[:, list(X0)] = True
    m[list(Y0), :] = True
    m.setflags(write=False)
    return m


# ---- the fields ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def permutation(H=U.H, W=U.W):
    """pi [H W] int64: the pixel whose ray (and, for the comparison with the pinhole run, whose upstream gradient) pixel q takes; the identity on
    the fixed pixels and on three free pixels in four."""
    free = np.flatnonzero(~fixed_mask(H, W).ravel())
    g = np.random.default_rng(PERMUTED_SEED)
    chosen = np.sort(g.choice(free, size=len(free) // PERMUTED_FRACTION, replace=False))
    pi = np.arange(H * W, dtype=np.int64)
    pi[chosen] = chosen[g.permutation(len(chosen))]
    pi.setflags(write=False)
    return pi


def permute_pixels(a):
    """a [..., H, W] with the pixels exchanged as `permuted` exchanges the rays: out[..., q] = a[..., pi[q]]."""
    a = np.asarray(a)
    H, W = a.shape[-2:]
    return np.ascontiguousarray(a.reshape(*a.shape[:-2], H * W)[..., permutation(H, W)].reshape(a.shape))


def _bump(size, lines):
    """sin^2 between consecutive members of `lines`, exactly 0 on them."""
    g = np.zeros(size, dtype=np.float64)
    for a, b in zip(lines[:-1], lines[1:]):
        for i in range(a + 1, b):
            g[i] = np.sin(np.pi * (i - a) / (b - a)) ** 2
    return g


def apply(field, ray):
    """ray [N,3,H,W] float32 of a pinhole camera -> the field's rays (a new array; `pinhole`: a copy)."""
    ray = np.asarray(ray)
    assert ray.dtype == np.float32 and ray.ndim == 4 and ray.shape[1] == 3
    H, W = ray.shape[-2:]
    if field == "pinhole":
        return ray.copy()
    if field == "permuted":
        return permute_pixels(ray)
    if field == "bulge":
        X0, Y0 = fixed_axes(H, W)
        b = (BULGE_A * _bump(H, Y0)[:, None] * _bump(W, X0)[None, :])
        free = ~fixed_mask(H, W)
        assert not b[~free].any()
        out = ray.copy()
        out[:, 1] = np.where(free, ray[:, 1] + b.astype(np.float32), ray[:, 1])
        out[:, 0] = np.where(free, ray[:, 0] + (0.5 * b).astype(np.float32), ray[:, 0])
        return out
    raise KeyError(field)


def scene(tex, field, vpm=None, dtype="f32", shaded=False):
    """`_upstream_cases.scene` with the field's rays (computed once, left unchanged)."""
    return U.scene(tex, vpm, dtype, shaded, None if field == "pinhole" else field)


# ---- item_box<TPI> / tile_box and the in-box test, restated ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _coords(tex, field, vpm=None):
    case = scene(tex, field, vpm)
    return oracle.coords(case["dhw"], case["ray"], case["eye"], case["Ht"], case["Wt"], view_to_mpi=case["v2m"])   # the exact fp32 chain (plane_coord)


def boxes(tex, field, tiling, view=0, vpm=None):
    """[(y0, y1, x0, x1, [per plane (bx, by, width in texels, rows) or None: not staged])] for every tile of `view`: corner_extent + item_box<TPI>
    (gmpi_device.hpp) on the corner pixels' fp32 coordinates -- extent grown by 1 / 64 texel and the 2 x 2 support, the first column aligned down
    to a loader item; not staged when a corner image is not finite (>= 1e6) or the box exceeds the kernel's buffer."""
    tw, th, pitch, rows, tpi = tilings()[tiling]
    case = scene(tex, field, vpm)
    ix, iy = _coords(tex, field, vpm)
    out = []
    for y0 in range(0, case["H"], th):
        for x0 in range(0, case["W"], tw):
            y1, x1 = min(y0 + th - 1, case["H"] - 1), min(x0 + tw - 1, case["W"] - 1)
            per_plane = []
            for k in range(case["D"]):
                cx = ix[view, k][[y0, y0, y1, y1], [x0, x1, x0, x1]]
                cy = iy[view, k][[y0, y0, y1, y1], [x0, x1, x0, x1]]
                if not (np.all(np.abs(cx) < 1e6) and np.all(np.abs(cy) < 1e6)):
                    per_plane.append(None)
                    continue
                bx0, bx1 = int(np.floor(cx.min() - BOX_SLACK)), int(np.floor(cx.max() + BOX_SLACK)) + 1
                by0, by1 = int(np.floor(cy.min() - BOX_SLACK)), int(np.floor(cy.max() + BOX_SLACK)) + 1
                bx = bx0 & ~(tpi - 1)
                items, nrows = (bx1 - bx) // tpi + 1, by1 - by0 + 1
                per_plane.append((bx, by0, tpi * items, nrows) if items <= pitch // tpi and nrows <= rows else None)
            out.append((y0, y1, x0, x1, per_plane))
    return out


def footprints(tex, field, view=0, vpm=None):
    """(x0, y0, any_w) [D,H,W]: `footprint` + the tap gates of `make_taps` (gmpi_device.hpp, gmpi_shared.hpp) in fp32 -- the integer corner, -2 for
    coordinates out of range, and whether any of the four weights survives the zeroing of the taps outside the texture."""
    case = scene(tex, field, vpm)
    Ht, Wt = case["Ht"], case["Wt"]
    ix, iy = (a[view] for a in _coords(tex, field, vpm))
    one = np.float32(1)
    with np.errstate(invalid="ignore"):
        fx0, fy0 = np.floor(ix), np.floor(iy)
        wx1, wx0, wy1, wy0 = ix - fx0, (fx0 + one) - ix, iy - fy0, (fy0 + one) - iy
        x0 = np.where((fx0 >= -2) & (fx0 <= Wt), fx0, -2).astype(np.int64)
        y0 = np.where((fy0 >= -2) & (fy0 <= Ht), fy0, -2).astype(np.int64)
    x0in, x1in = (x0 >= 0) & (x0 <= Wt - 1), (x0 >= -1) & (x0 <= Wt - 2)
    y0in, y1in = (y0 >= 0) & (y0 <= Ht - 1), (y0 >= -1) & (y0 <= Ht - 2)
    any_w = ((x0in & y0in & (wx0 * wy0 != 0)) | (x1in & y0in & (wx1 * wy0 != 0)) | (x0in & y1in & (wx0 * wy1 != 0)) | (x1in & y1in & (wx1 * wy1 != 0)))
    return x0, y0, any_w


@functools.lru_cache(maxsize=None)
def classify(tex, field, tiling, view=0, vpm=None):
    """[D,H,W] int8 class of every (plane, pixel) of `view` under `tiling`: NO_WEIGHT (every weight zero: the kernels skip it or read a sentinel),
    UNSTAGED (the tile's box on that plane is not staged), IN_BOX (all four taps inside the box: lx >= 0, ly >= 0, lx + 1 < width, ly + 1 < rows),
    STRADDLE (not in the box, at least one tap inside), FAR (no tap inside)."""
    x0, y0, any_w = footprints(tex, field, view, vpm)
    cls = np.full(x0.shape, NO_WEIGHT, dtype=np.int8)
    for ty0, ty1, tx0, tx1, per_plane in boxes(tex, field, tiling, view, vpm):
        for k, bb in enumerate(per_plane):
            sl = (k, slice(ty0, ty1 + 1), slice(tx0, tx1 + 1))
            if bb is None:
                c = np.full(x0[sl].shape, UNSTAGED, dtype=np.int8)
            else:
                lx, ly = x0[sl] - bb[0], y0[sl] - bb[1]
                inx = [(lx + d >= 0) & (lx + d < bb[2]) for d in (0, 1)]
                iny = [(ly + d >= 0) & (ly + d < bb[3]) for d in (0, 1)]
                inb = inx[0] & inx[1] & iny[0] & iny[1]
                assert np.array_equal(inb, (lx >= 0) & (ly >= 0) & (lx + 1 < bb[2]) & (ly + 1 < bb[3]))   # the kernels' spelling
                some = (inx[0] | inx[1]) & (iny[0] | iny[1])
                c = np.where(inb, IN_BOX, np.where(some, STRADDLE, FAR)).astype(np.int8)
            cls[sl] = np.where(any_w[sl], c, NO_WEIGHT)
    cls.setflags(write=False)
    return cls


def counts(tex, field, tiling, view=0, vpm=None):
    """{class name: number of (pixel, plane) pairs}."""
    cls = classify(tex, field, tiling, view, vpm)
    return {name: int((cls == i).sum()) for i, name in enumerate(CLASSES)}


def mixed_tiles(tex, field, tiling, view=0):
    """Number of (tile, plane) pairs that hold in_box, straddle and far lanes together."""
    cls = classify(tex, field, tiling, view)
    n = 0
    for ty0, ty1, tx0, tx1, per_plane in boxes(tex, field, tiling, view):
        for k in range(len(per_plane)):
            c = cls[k, ty0:ty1 + 1, tx0:tx1 + 1]
            n += int((c == IN_BOX).any() and (c == STRADDLE).any() and (c == FAR).any())
    return n


# ---- images of one pixel row / column: the texel gather without a usable homography ----------------------------------------------------------------
LINES = ((1, 40), (40, 1))   # (H, W): `homography_kernel` (render_backward_gather.hip) asks for W >= 2 and H >= 2 and writes valid = 0 otherwise
LINE_TEX = "twin"


@functools.lru_cache(maxsize=None)
def line_scene(H, W):
    """The scene of `twin` seen by a pinhole camera of H x W pixels, with N(0,1) upstream gradients."""
    from test_hip_edge_cases import _cam
    base = U.scene(LINE_TEX)
    ray, eye, zd = _cam(base["N"], H, W, seed=42, tilt=0.3)
    gc, gd, gT = U.upstream("normal", base["N"], H, W, 5)
    return dict(base, ray=ray, eye=eye, zd=zd, H=H, W=W, gc=gc, gd=gd, gT=gT)


@functools.lru_cache(maxsize=None)
def line_refs(kind, H, W):
    """(float64, fp32) gradient lists of the volume ("volume") or of a layout's three images ("shared" / "depth") on `line_scene`."""
    import torch
    case = line_scene(H, W)
    out = []
    for dt in (torch.float64, torch.float32):
        if kind == "volume":
            import _deep_cases
            out.append([_deep_cases.volume_grad_ref(case, dt, align_corners=True)])
            continue
        parts, extra = U.layout_parts(kind, LINE_TEX)
        v2m = [int(m) for m in case["v2m"]]
        if kind == "shared":
            import test_hip_shared_color as SC
            out.append(list(SC._reference_grads(parts, case["dhw"], case["ray"], case["eye"], case["zd"], v2m, case["gc"], case["gd"], case["gT"], False, dt)))
        else:
            import test_hip_depth_alpha as DA
            tup = (parts[0], parts[1], extra[0], parts[2], torch.as_tensor(case["dhw"]), case["ray"], case["eye"], case["zd"], extra[1])
            out.append(list(DA._reference_grads(tup, True, v2m, case["gc"], case["gd"], case["gT"], False, dt)))
    return tuple(out)


# ---- references --------------------------------------------------------------------------------------------------------------------------------------
def volume_refs(tex, field, family, vpm=None, dtype="f32", shaded=False):
    return U.volume_refs(tex, family, vpm, dtype, shaded, None if field == "pinhole" else field)


def layout_refs(kind, tex, field, family):
    return U.layout_refs(kind, tex, family, None, None if field == "pinhole" else field)


def reference_sets(tex, field, family):
    """`_upstream_cases.reference_sets` through the field's rays."""
    out = []
    for label, vpm, dtype in (("volume", None, "f32"), ("volume bf16", None, "bf16")) + ((("volume vpm2", 2, "f32"),) if tex == "twin" else ()):
        r64, r32 = volume_refs(tex, field, family, vpm, dtype)
        out.append((label, vpm, [r64], [r32]))
    r64, r32 = volume_refs(tex, field, family, None, "f32", True)
    out.append(("shaded", None, list(r64), list(r32)))
    for kind in ("shared", "depth"):
        r64, r32 = layout_refs(kind, tex, field, family)
        out.append((kind, None, list(r64), list(r32)))
    return out
