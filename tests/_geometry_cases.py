"""The inputs of the geometry pass's output tests, in one place, and the host restatements they are sized by: tests/test_geometry_cases_cpu.py
checks on the CPU, on the inputs and the float64 references alone, the conditions that make the GPU comparisons mean something;
tests/test_hip_geometry_outputs.py runs render_backward_geometry.hip on exactly these inputs.  CPU only (numpy / torch); the kernel's tile shape and
the reducers' width are read out of its source (`constants`), so that a change of a constant moves the frames' tile counts with it.

The frames (H, W), all over 24 x 28 texels:
    TALL   1030 x 70   258 x 2 = 516 tiles of 64 x 4 pixels, ragged on both axes: four threads of the 256-wide slab reducers take three trips, the others
                       two; 516 is no multiple of the 8 the tile remap deals by
    WIDE   18 x 3300   5 x 52 = 260 tiles: four threads take two trips
    ROW    1 x 40      a row of a 40 x 40 camera's ray field: one wave of four holds pixels, 40 lanes of it
    COL    40 x 1      a column of the same field: one lane of 64 per wave
    SMALL  10 x 72     3 x 2 = 6 tiles, ragged on both axes
The sources: "volume" (RGBA), "shared" (shared colour with a background image), "depth" (depth alpha, n_z_bins = 4)."""
import functools
import os
import re

import numpy as np
import torch

import oracle
from _geometry_ref import geometry_grads
from test_hip_edge_cases import _cam, _dhw
from test_hip_geometry_grad import _grads_in, _smooth_rgba
from test_hip_geometry_layouts import _bounds, _images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "ml-gmpi_amd", "csrc", "render_backward_geometry.hip")
SOURCES = ("volume", "shared", "depth")
GEO = ("dhw", "ray", "eye", "zd")
FRAMES = dict(TALL=(1030, 70), WIDE=(18, 3300), ROW=(1, 40), COL=(40, 1), SMALL=(10, 72), DEEP=(40, 72))
HT, WT = 24, 28
N_Z_BINS = 4
LINE_CAMERA, LINE_ROW, LINE_COL = 40, 13, 27   # ROW / COL: row 13 resp. column 27 of a 40 x 40 camera's field


# ---- the kernel's own constants and what the host derives from them -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def constants():
    """{name: int} of kGTW, kGTH (the pixel tile), kGRed (threads of the slab reducers) and kGChunk (planes per LDS chunk), read out of the source."""
    src = open(KERNEL).read()
    out = {}
    for name in ("kGTW", "kGTH", "kGRed", "kGChunk"):
        m = re.search(r"\b%s = (\d+)\b" % name, src)
        assert m, name
        out[name] = int(m.group(1))
    return out


def tiles(H, W):
    """`tiles_of`: the 64 x 4 pixel tiles of an H x W frame."""
    c = constants()
    return ((W + c["kGTW"] - 1) // c["kGTW"]) * ((H + c["kGTH"] - 1) // c["kGTH"])


def workspace_floats(N, H, W, D, dhw, pz):
    """The slab layout of the kernel's comment in floats: 6 [+ 3 D with dhw] components of N * tiles floats, then [with pz] D more behind them, each
    of the two parts rounded up to 256 bytes."""
    up = lambda floats: (4 * floats + 255) // 256 * 64
    slots = N * tiles(H, W)
    return up((6 + (3 * D if dhw else 0)) * slots) + (up(D * slots) if pz else 0)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------
def camera(frame, N, seed=62):
    """(ray [N,3,H,W], eye, z_dir) of `_cam` at the frame's size; ROW and COL are slices of a 40 x 40 camera's field."""
    H, W = FRAMES[frame]
    if frame in ("ROW", "COL"):
        ray, eye, zd = _cam(N, LINE_CAMERA, LINE_CAMERA, seed=seed, tilt=0.3)
        ray = ray[:, :, LINE_ROW:LINE_ROW + 1, :] if frame == "ROW" else ray[:, :, :, LINE_COL:LINE_COL + 1]
        return np.ascontiguousarray(ray), eye, zd
    return _cam(N, H, W, seed=seed, tilt=0.3)


class Case(dict):
    """One problem: source, frame, H, W, N, M, D, images (volume: (rgba,); layouts: (rgb, mid, bg, pz) as `_images` gives them), zb, dhw, ray, eye,
    zd, v2m (int32 [N]), vpm (uniform views per MPI or None), gc, gd, gT (N(0,1) unless the case says otherwise), with_T (whether the case's own loss
    reaches T).  Built once per key and left unchanged."""
    __getattr__ = dict.__getitem__

    def __hash__(self):
        return hash(self["key"])

    def __eq__(self, other):
        return self is other


def _finish(key, source, frame, M, D, images, v2m, vpm, seed, upstream=None):
    H, W = FRAMES[frame]
    N = len(v2m)
    ray, eye, zd = camera(frame, N, seed + 1)
    gc, gd = _grads_in((N, H, W), seed + 2)
    gT = np.random.default_rng(seed + 3).standard_normal((N, 1, H, W)).astype(np.float32)
    if upstream is not None:   # (mean, relative sigma) of gc, gd, gT: upstream gradients of one sign each
        g = np.random.default_rng(seed + 4)
        gc, gd, gT = ((m * (1.0 + upstream[1] * g.standard_normal(a.shape))).astype(np.float32) for m, a in zip(upstream[0], (gc, gd, gT)))
    c = Case(key=key, source=source, frame=frame, H=H, W=W, N=N, M=M, D=D, images=images, zb=_bounds(N_Z_BINS) if source == "depth" else None,
             dhw=_dhw(M, D), ray=ray, eye=eye, zd=zd, v2m=np.asarray(v2m, np.int32), vpm=vpm, gc=gc, gd=gd, gT=gT, with_T=upstream is not None)
    return c


@functools.lru_cache(maxsize=None)
def case(source, frame, D, M=2, v2m=(0, 1), vpm=None, smooth=False, pz_rows=False, bf16=False, seed=61):
    """White noise (smooth: `_smooth_rgba`'s 6 x 6 grid upsampled) on HT x WT texels.  bf16: values a bf16 volume stores exactly (volume only)."""
    assert source in SOURCES and not (bf16 and source != "volume")
    if source == "volume":
        images = (_smooth_rgba(seed, (M, D, 4, HT, WT)) if smooth else oracle.synth_rgba(seed, (M, D, 4, HT, WT), bf16_round=bf16),)
    else:
        images = _images(source, seed, M, D, HT, WT, smooth=smooth, pz_rows=pz_rows)
    return _finish(("case", source, frame, D, M, v2m, vpm, smooth, pz_rows, bf16, seed), source, frame, M, D, images, v2m, vpm, seed)


def with_nan(c, mpis):
    """The images of `c` with every texel of the MPIs `mpis` NaN (new arrays; plane_z stays)."""
    out = []
    for i, a in enumerate(c.images):
        a = None if a is None else a.copy()
        if a is not None and not (c.source == "depth" and i == 3):
            a[list(mpis)] = np.nan
        out.append(a)
    return tuple(out)


# ---- deep stacks for the per-plane bars of the two layouts ---------------------------------------------------------------------------------------------
DEEP_D = (32, 97)
DEPTH_LO, DEPTH_HI = 0.22, 1.27   # the depth ramp's ends: the surface (where plane_z - depth enters the alpha ramp) passes every plane
DEPTH_NOISE = 0.02
DEEP_UPSTREAM = ((-1.0, 10.0, 20.0), 0.25)   # depth: gc = -(1 + N / 4), gd = 10 (1 + N / 4), gT = 20 (1 + N / 4); see layout_deep_case


@functools.lru_cache(maxsize=None)
def layout_deep_case(layout, D):
    """Two tilted views of two MPIs on the DEEP frame, inputs in which every plane carries weight.
    shared: the thin smooth alpha stack of `_deep_cases.geometry_case` over a smooth colour and background image.
    depth:  a depth image that ramps along the texture's diagonal over the whole range of plane_z (its central part, which the cameras see) plus small
            smooth noise, plane_z [M, D] = linspace(0, 1, D) per MPI, n_z_bins = 4: every plane is the visible surface somewhere.  plane_z.grad[m, k]
            is ONE sum over every pixel: under N(0,1) upstream gradients it is a random walk that leaves some plane below 1e-3 of the largest (measured
            on the float64 reference: 3e-5 .. 6e-4), and under a depth loss of one sign it changes sign where the stack behind a plane stops being
            opaque.  So this case's loss is L = sum gc C + gd Z + gT T with gc < 0 < gd < gT / z (DEEP_UPSTREAM, 25 % noise) over a background darker
            than the colour image: raising any plane's alpha then lowers every term (dT/da < 0; d Z/da_k = T_k (z_k P - sum_j w'_j (z_j - z_k)) with P
            the transmittance behind k, and gd z_k P < gT P; C moves towards rgb > what lies behind), every plane_z sum has one sign and no plane
            cancels."""
    from _visible import thin
    assert layout in ("shared", "depth")
    M = 2
    vol = _smooth_rgba(5, (M, D, 4, HT, WT))
    rgb, bg = vol[:, 0, :3].copy(), vol[:, -1, :3].copy()
    if layout == "shared":
        g = torch.Generator().manual_seed(5)
        coarse = 0.1 + 0.8 * (0.25 + 0.5 * torch.rand((M * D, 1, 6, 6), generator=g, dtype=torch.float64))
        fine = torch.nn.functional.interpolate(coarse, size=(HT, WT), mode="bilinear", align_corners=True).clamp(0, 1)
        full = np.concatenate((np.zeros((M, D, 3, HT, WT), np.float32), fine.reshape(M, D, 1, HT, WT).float().numpy()), 2)
        images = (rgb, thin(full)[:, :, 3:].copy(), bg, None)
    else:
        y = np.arange(HT, dtype=np.float64)[:, None] / (HT - 1)
        x = np.arange(WT, dtype=np.float64)[None, :] / (WT - 1)
        t = np.clip((0.5 * (x + y) - 0.2) / 0.6, 0.0, 1.0)
        noise = _smooth_rgba(6, (M, 1, 4, HT, WT))[:, 0, :1].astype(np.float64) - 0.5
        depth = (DEPTH_LO + (DEPTH_HI - DEPTH_LO) * t)[None, None] + DEPTH_NOISE * noise
        pz = np.stack([np.linspace(0.0, 1.0, D)] * M).astype(np.float32)
        images = (rgb, depth.astype(np.float32), 0.5 * bg, pz)
    return _finish(("deep", layout, D), layout, "DEEP", M, D, images, (0, 1), None, 64, upstream=DEEP_UPSTREAM if layout == "depth" else None)


# ---- the float64 references (computed once per key, left unchanged) --------------------------------------------------------------------------------------
def expanded(c, images=None):
    """The fp32 volume the case's images stand for (the volume itself for "volume"), as numpy."""
    from test_hip_geometry_layouts import _expanded
    images = c.images if images is None else images
    if c.source == "volume":
        return images[0]
    return _expanded(c.source, *(None if a is None else torch.from_numpy(a) for a in images), c.zb)


@functools.lru_cache(maxsize=None)
def reference(c, ac=True, with_T=None):
    """{dhw, ray, eye, zd[, pz]}: the float64 oracle's gradients of sum gc colour + gd depth [+ gT T] (tests/_geometry_ref.py; with T
    tests/_transmittance_ref.py; plane_z: tests/test_hip_plane_z_grad.py `_reference`) as numpy arrays."""
    import _transmittance_ref as tr
    if with_T is None:
        return reference(c, ac, c.with_T)
    vol = expanded(c)
    if with_T:
        g = tr.grads(vol, c.dhw, c.ray, c.eye, c.zd, c.v2m, c.gc, c.gd, c.gT, align_corners=ac)[1:]
    else:
        g = geometry_grads(vol, c.dhw, c.ray, c.eye, c.zd, c.v2m, c.gc, c.gd, align_corners=ac)
    out = dict(zip(GEO, g))
    if c.source == "depth":
        from test_hip_plane_z_grad import _reference
        stored = tuple(None if a is None else torch.from_numpy(a) for a in c.images)
        out["pz"] = _reference(stored, (c.dhw, c.ray, c.eye, c.zd), (c.gc, c.gd, c.gT if with_T else None), ac, c.zb, c.v2m)[0]
    for a in out.values():
        a.setflags(write=False)
    return out
