"""The inputs of the deep-plane tests, in one place: tests/test_visible_stacks_cpu.py checks on the CPU that every plane of them is visible
and that the fp32 reference chain is close enough to float64 for the per-slab gradient bar to mean something; tests/test_hip_deep_planes.py and
tests/test_hip_deep_gradients.py run the kernels on exactly these inputs; tests/test_hip_chunk_gradients.py and tests/test_hip_shaded_gradients.py
run the chunked and the shaded twins of the volume backward on the `twin_case` inputs at the end.  CPU only (numpy / torch), never imported by the product."""
import functools

import numpy as np
import torch

import oracle
import _transmittance_ref
from _visible import make_alpha
from test_hip_backward import _rot_cam
from test_hip_edge_cases import _cam, _dhw

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

# ---- forward ------------------------------------------------------------------------------------------------------------------------------------
DEPTHS = [1, 2, 31, 32, 33, 95, 96, 97, 193]     # around the strip kernel's 32-entry ring and the 96-plane chunks
SMALL_CASES = [dict(seed=20 + D, B=1, D=D, S=64) for D in DEPTHS]
TILTED_CASE = dict(seed=31, B=2, D=97, S=256, extreme=True)   # 2-sigma poses: chunk boundaries crossed on the half-tile path


def small_cases():
    """(cfg, alpha law) of the tile / strip kernel cases (one or two planes: the thin law only, which is the noise law there)."""
    return [(c, a) for c in SMALL_CASES + [TILTED_CASE] for a in ("thin", "surface") if c["D"] > 2 or a == "thin"]


# the six shapes of test_strip_kernel_plane_split_regimes (6-way, 3-way, unsplit, D not divisible by the split, fewer planes than parts) ...
SPLIT_CASES = [dict(seed=51, B=1, D=96, S=256), dict(seed=52, B=2, D=7, S=256), dict(seed=53, B=1, D=4, S=128),
               dict(seed=54, B=4, D=50, S=256), dict(seed=55, B=8, D=20, S=256), dict(seed=56, B=2, D=33, S=512, extreme=True)]
TWO_WAVES_CASE = dict(seed=71, B=6, D=96, S=256)   # ... and the 2-waves-per-SIMD instance (1025-2048 strips), 96 planes deep
# full-size shapes (test_full_size_window_against_oracle): rendered at full size on the GPU, compared on 64 x 64 oracle windows
FULL_SIZE = [dict(S=1024, D=96, B=1, dtype=torch.bfloat16), dict(S=1024, D=256, B=1, dtype=torch.float32, preset="MetFaces"),
             dict(S=1024, D=96, B=2, dtype=torch.bfloat16, extreme=True), dict(S=1024, D=96, B=1, dtype=torch.float32, extreme=True),
             dict(S=1024, D=96, B=1, dtype=torch.float16)]


SHARED_VIEWS = dict(S=512, D=96, B=8)               # 8 camera-path views of one MPI (test_full_size_windows_config2_and_config4_against_oracle)
AUTO_SHARES = dict(S=1024, D=256, B=3)               # test_config5_shape_auto_shares_the_views_between_band_and_tile_kernel
SHARED_COLOUR = [dict(seed=1, B=2, D=32, S=96), dict(seed=2, B=2, D=96, S=96)]
DEPTH_CASE = dict(B=2, D=96, S=64)                   # LightRenderer.compute_depth


def windows(S):
    return [(0, 0), (S - 64, S - 64), (S // 2 - 32, S // 2 + 7), (13, S - 64)]


# ---- backward -----------------------------------------------------------------------------------------------------------------------------------
H, W, HT, WT = 96, 160, 80, 96    # 3 x 5 tiles of 32 x 32 pixels (6 x 10 of 16 x 16), a texture that is not square
GRAD_CASES = {
    "d32-thin": dict(D=32, alpha="thin"), "d32-surface": dict(D=32, alpha="surface"),
    "d97-thin": dict(D=97, alpha="thin"), "d97-surface": dict(D=97, alpha="surface"),
    "d129-thin": dict(D=129, alpha="thin"), "d129-surface": dict(D=129, alpha="surface"),
    "d97-surface-rotated": dict(D=97, alpha="surface", cam="rot"),
    "d97-thin-bf16": dict(D=97, alpha="thin", dtype="bf16"),
    "d32-surface-f16": dict(D=32, alpha="surface", dtype="f16"),
    "d97-thin-ragged": dict(D=97, alpha="thin", N=3, v2m=[0, 1, 1]),
}


def grad_case(name):
    """-> dict(rgba [M,D,4,HT,WT] float32 holding the STORED values, dhw, ray, eye, zd, v2m, gc, gd, gT, dtype)."""
    cfg = GRAD_CASES[name]
    D, N, M = cfg["D"], cfg.get("N", 2), 2
    dtype = DTYPES[cfg.get("dtype", "f32")]
    rgba = make_alpha(oracle.synth_rgba(41, (M, D, 4, HT, WT)), cfg["alpha"], dtype=None if dtype is torch.float32 else dtype)
    if cfg.get("cam") == "rot":
        ray, eye, zd = _rot_cam(N, H, W, 0.25, -0.1, 0.5)
        dhw = _dhw(M, D, ext=0.30, last=0.6)
    else:
        ray, eye, zd = _cam(N, H, W, seed=42, tilt=0.3)
        dhw = _dhw(M, D)
    g = np.random.default_rng(5)
    gc = g.standard_normal((N, 3, H, W)).astype(np.float32)
    gd = g.standard_normal((N, 1, H, W)).astype(np.float32)
    gT = g.standard_normal((N, 1, H, W)).astype(np.float32)
    v2m = np.asarray(cfg.get("v2m", np.arange(N) % M), dtype=np.int32)
    return dict(rgba=rgba, dhw=dhw, ray=ray, eye=eye, zd=zd, v2m=v2m, gc=gc, gd=gd, gT=gT, dtype=dtype, D=D, N=N, M=M)


def volume_grad_ref(case, dtype, align_corners=True, shading=None, out_pm1=False):
    """d(sum gC colour + sum gZ depth + sum gT T) / d rgba of tests/_transmittance_ref.render in `dtype` (float64: the reference; float32: the same
    chain at the kernels' precision, for e_ref) -> float64 numpy array.  With a shading ([M,1,Ht,Wt], or ONE image [1,1,Ht,Wt] expanded over the
    MPIs) the render is that of `shaded_volume(rgba, shading)` in `dtype` (tests/test_hip_shaded_render.py) and the result is the pair (gradient
    w.r.t. rgba, gradient w.r.t. the shading as it was passed: for one expanded image the sum over the MPIs).  out_pm1: the colour is 2 C - 1."""
    c = lambda a: torch.as_tensor(a).to(dtype)
    vol = c(case["rgba"]).clone().requires_grad_(True)
    s = None
    if shading is not None:
        from test_hip_shaded_render import shaded_volume
        s = c(shading).clone().requires_grad_(True)
        rendered = shaded_volume(vol, s.expand(vol.shape[0], -1, -1, -1), dtype)
    else:
        rendered = vol
    color, depth, T = _transmittance_ref.render(rendered, c(case["dhw"]), c(case["ray"]), c(case["eye"]), c(case["zd"]), case["v2m"],
                                                align_corners=align_corners)
    if out_pm1:
        color = 2 * color - 1
    ((color * c(case["gc"])).sum() + (depth * c(case["gd"])).sum() + (T * c(case["gT"])).sum()).backward()
    if s is None:
        return vol.grad.double().numpy()
    return vol.grad.double().numpy(), s.grad.double().numpy()


# ---- the twins of the volume backward: one chunk of a plane-chunked stack (CHUNK = true) and the shaded render (Shade = ShadeK) ---------------------
# 20 x 150 pixels: three columns of 64-pixel tiles, the last 22 wide, and three rows of 8, the last 4 high (five columns of 32 and two rows of 16 for
# the kernel a one-column texture takes); texture 36 x 52 unless the case says otherwise.  chunk / shaded: which of the two twins runs the case.
TWIN_H, TWIN_W, TWIN_HT, TWIN_WT = 20, 150, 36, 52
TWIN_CASES = {
    "t97-thin": dict(D=97, alpha="thin", ac=True, chunk=True, shaded=True),
    "t129-surface-ac0": dict(D=129, alpha="surface", ac=False, chunk=True, shaded=True),
    "t200-thin": dict(D=200, alpha="thin", ac=True, chunk=True, shaded=False),
    "t97-thin-bf16": dict(D=97, alpha="thin", ac=True, dtype="bf16", chunk=True, shaded=True),
    "t97-surface-f16-ac0": dict(D=97, alpha="surface", ac=False, dtype="f16", chunk=False, shaded=True),
    "t12-ragged": dict(D=12, alpha="thin", ac=True, tex=(36, 50), chunk=False, shaded=True),          # Wt % 4 != 0
    "t12-ragged-ac0": dict(D=12, alpha="thin", ac=False, tex=(36, 50), chunk=False, shaded=True),
    "t12-column": dict(D=12, alpha="thin", ac=True, tex=(36, 1), chunk=True, shaded=True),            # Wt < 2
    "t12-column-ac0": dict(D=12, alpha="thin", ac=False, tex=(36, 1), chunk=True, shaded=True),
    "t6-minified": dict(D=6, alpha="thin", ac=True, tex=(250, 190), img=(24, 40), chunk=False, shaded=True),   # no tile box fits
    "t12-views-v2m": dict(D=12, alpha="thin", ac=False, N=3, v2m=[0, 1, 1], chunk=True, shaded=True),
    "t12-views-vpm": dict(D=12, alpha="thin", ac=False, N=4, v2m=[0, 0, 1, 1], vpm=2, chunk=True, shaded=True),
}


def twin_keys(which):
    """(name, shaded) of every case the `which` twin runs ("chunk": unshaded inputs; "shaded": the colours moved and a shading image)."""
    return [(n, which == "shaded") for n, cfg in TWIN_CASES.items() if cfg[which]]


@functools.lru_cache(maxsize=None)
def twin_case(name, shaded=False):
    """`grad_case`'s dict on the small frame, plus ac, H, W, vpm (uniform views per MPI, or None) and, for a shaded case, shading [M,1,Ht,Wt] fp32:
    the colours are moved to 1.3 rgb - 0.15 before the storage rounding, so that with a shading in [0.4, 1.6] both branches of the clip are taken
    (products above 1 and below 0); the kernels are then run with range_check="off".  Computed once and left unchanged."""
    cfg = TWIN_CASES[name]
    D, N, M = cfg["D"], cfg.get("N", 2), 2
    (Ht, Wt), (Hh, Ww) = cfg.get("tex", (TWIN_HT, TWIN_WT)), cfg.get("img", (TWIN_H, TWIN_W))
    dtype = DTYPES[cfg.get("dtype", "f32")]
    rgba = oracle.synth_rgba(41, (M, D, 4, Ht, Wt))
    if shaded:
        rgba[:, :, :3] = 1.3 * rgba[:, :, :3] - 0.15
    rgba = make_alpha(rgba, cfg["alpha"], dtype=None if dtype is torch.float32 else dtype)
    ray, eye, zd = _cam(N, Hh, Ww, seed=42, tilt=0.3)
    g = np.random.default_rng(5)
    gc = g.standard_normal((N, 3, Hh, Ww)).astype(np.float32)
    gd = g.standard_normal((N, 1, Hh, Ww)).astype(np.float32)
    gT = g.standard_normal((N, 1, Hh, Ww)).astype(np.float32)
    v2m = np.asarray(cfg.get("v2m", np.arange(N) % M), dtype=np.int32)
    case = dict(rgba=rgba, dhw=_dhw(M, D), ray=ray, eye=eye, zd=zd, v2m=v2m, gc=gc, gd=gd, gT=gT, dtype=dtype, D=D, N=N, M=M, ac=cfg["ac"],
                H=Hh, W=Ww, vpm=cfg.get("vpm"))
    if shaded:
        from test_hip_shaded_render import make_shading
        case["shading"] = make_shading(5, torch.from_numpy(rgba)).numpy()
    return case


@functools.lru_cache(maxsize=None)
def twin_refs(name, shaded=False, out_pm1=False, one_shading=False):
    """(float64, fp32) references of a twin case, computed once: each the volume gradient, or -- shaded -- the pair (volume, shading).
    one_shading: MPI 0's shading image expanded over all MPIs (its gradient is the sum over them)."""
    case = twin_case(name, shaded)
    s = case.get("shading")
    if one_shading:
        s = s[:1]
    return tuple(volume_grad_ref(case, dt, align_corners=case["ac"], shading=s, out_pm1=out_pm1) for dt in (torch.float64, torch.float32))


# ---- shared-colour backward: alpha gradient per plane, D = 32 and one plane more than the tile backward's tables hold ------------------------------
SHARED_GRAD = [dict(D=32, S=96), dict(D=129, S=48)]


def shared_grad_case(cfg, with_bg, dtype=torch.float32):
    """The `_bwd_case` of tests/test_hip_shared_color.py on a thin stack: 4 views of 2 MPIs, loss over colour, depth and T."""
    from test_hip_parity import _random_case
    rgba, dhw, ray, eye, zd = _random_case(seed=5, B=4, D=cfg["D"], S=cfg["S"], alpha="thin")
    q = lambda t: t.contiguous().to(dtype)
    parts = (q(rgba[:2, 0, :3]), q(rgba[:2, :, 3:]), q(rgba[:2, -1, :3]) if with_bg else None)
    g = np.random.default_rng(7)
    S = cfg["S"]
    gc, gd, gT = (g.standard_normal((4, c, S, S)).astype(np.float32) for c in (3, 1, 1))
    return parts, dhw[:2], ray, eye, zd, [0, 0, 1, 1], gc, gd, gT


# ---- geometry pass: dhw.grad per (MPI, plane) row -------------------------------------------------------------------------------------------------
GEOMETRY = [dict(D=32), dict(D=97)]


def geometry_case(cfg):
    """A smooth volume (6 x 6 noise grid per plane and channel, upsampled: no O(1) jumps of the position gradient at texel edges) with thinned
    alpha, two tilted views of two MPIs."""
    import torch.nn.functional as F
    from _visible import thin
    M, D, Ht, Wt, N, Hh, Ww = 2, cfg["D"], 40, 48, 2, 40, 72
    g = torch.Generator().manual_seed(5)
    coarse = 0.25 + 0.5 * torch.rand((M * D, 4, 6, 6), generator=g, dtype=torch.float64)
    coarse[:, 3] = 0.1 + 0.8 * coarse[:, 3]
    fine = F.interpolate(coarse, size=(Ht, Wt), mode="bilinear", align_corners=True).clamp(0, 1)
    rgba = thin(fine.reshape(M, D, 4, Ht, Wt).float().numpy())
    ray, eye, zd = _cam(N, Hh, Ww, seed=64, tilt=0.3)
    g = np.random.default_rng(65)
    gc = g.standard_normal((N, 3, Hh, Ww)).astype(np.float32)
    gd = g.standard_normal((N, 1, Hh, Ww)).astype(np.float32)
    return rgba, _dhw(M, D), ray, eye, zd, np.arange(N), gc, gd
