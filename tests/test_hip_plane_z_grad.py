"""Gradient of the depth-alpha render w.r.t. plane_z (MPI(geometry_grad="all"): gmpi_mpi_render_depth_geometry_backward_pz_launch, the PZ instances of
render_backward_geometry.hip).  The reference is float64 torch autograd with plane_z as a leaf: the expanded volume built in float64 from the tensors
as stored, the clamp decisions (`inside`) taken from the fp32 difference as the kernel takes them, rendered with tests/_geometry_ref.py
(tests/_transmittance_ref.py where the loss reaches T).  The bar is `_check`'s for dhw of tests/test_hip_geometry_grad.py, unchanged:
|got - ref| <= 1e-4 |ref| over all (m, k) in strict-order mode on white noise, x 10 in the default mode on smooth inputs.  Also: the translation
invariance against depth.grad, determinism, every other gradient undisturbed, plane_ds.grad end to end against central differences of the HIP forward,
and the behaviour without "all"."""
import numpy as np
import pytest
import torch

import _transmittance_ref as tr
from _geometry_ref import geometry_render
from test_hip_edge_cases import _cam, _dhw
from test_hip_geometry_grad import _grads_in, _smooth_rgba, _t  # noqa: F401  (_smooth_rgba: through _images(smooth=True))
from test_hip_geometry_layouts import BASE, DTYPES, _bounds, _case_id, _images, _render, _smooth_grid

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GEO = ("dhw", "ray", "eye", "zd")
IMAGES = ("rgb", "depth", "bg")


# ---- the two sides ---------------------------------------------------------------------------------------------------------------------------------
def _stored(images, dtype, view=False):
    """(rgb, depth, bg) on the device in the storage dtype (depth optionally as the channel view of an RGB-D tensor) and plane_z (fp32)."""
    rgb, depth, bg, pz = (None if a is None else _t(a) for a in images)
    rgb, depth, bg = (None if a is None else a.to(dtype) for a in (rgb, depth, bg))
    if view:
        depth = torch.cat((rgb, depth), 1)[:, 3:]
        assert not depth.is_contiguous()
    return rgb, depth, bg, pz


def _hip(stored, geo, up, ac, strict, zb, *, needs=("pz",), geometry_grad="all", depth_backward="pixel", v2m=None, views_per_mpi=None, out_pm1=False):
    """One render and backward on the device.  `needs`: the names among pz, rgb, depth, bg, dhw, ray, eye, zd that require grad.  Returns
    {name: gradient as numpy, or None}, the outputs as numpy."""
    from ml_gmpi_amd import MPI
    rgb, depth, bg, pz = stored
    t = dict(rgb=rgb, depth=depth, bg=bg, pz=pz, **{k: _t(a) for k, a in zip(GEO, geo)})
    t = {k: None if a is None else a.detach().requires_grad_(k in needs) for k, a in t.items()}   # (fresh leaves over the same storage: views stay views)
    gc, gd, gT = up
    mpi = MPI(align_corners=ac, strict_order=strict, on_out_of_plane="raise", geometry_grad=geometry_grad)
    kw = dict(views_per_mpi=views_per_mpi) if views_per_mpi is not None else dict(view_to_mpi=_t(np.asarray(v2m, np.int32)))
    out = _render(mpi, "depth", t["rgb"], t["depth"], t["bg"], t["pz"], zb, [t[k] for k in GEO], out_pm1=out_pm1, want_transmittance=gT is not None,
                  depth_backward=depth_backward, **kw)
    loss = (out["color"] * _t(gc)).sum()
    if gd is not None:
        loss = loss + (out["depth"] * _t(gd)).sum()
    if gT is not None:
        loss = loss + (out["T"] * _t(gT)).sum()
    if loss.requires_grad:
        loss.backward()
    torch.cuda.synchronize()
    grads = {k: None if a is None or a.grad is None else a.grad.float().cpu().numpy() for k, a in t.items()}
    return grads, {k: out[k].detach().cpu().numpy() for k in ("color", "depth")}


def _reference(stored, geo, up, ac, zb, v2m, out_pm1=False, strict_lower_bound=False):
    """float64 autograd with plane_z (and the depth image) as leaves -> (plane_z.grad in plane_z's shape, depth.grad [M,1,Ht,Wt]) as numpy.  The volume
    is `expand_depth_alpha`'s in float64 of the tensors as stored; where the clamp passes the gradient is decided by the fp32 difference, bounds
    included, as depth_ramp decides it (strict_lower_bound: a tap exactly on the lower bound passes none -- what a skip of such planes would give)."""
    from ml_gmpi_amd.depth_alpha import ramp_constants
    rgb, depth, bg, pz = (None if a is None else a.detach().float().cpu() for a in stored)
    lo, hi, den = ramp_constants(*zb)
    M, D = depth.shape[0], pz.shape[-1]
    pz_leaf = pz.double().requires_grad_(True)
    d_leaf = depth.double().requires_grad_(True)
    pz_md = (pz_leaf if pz.ndim == 2 else pz_leaf[None].expand(M, D)).reshape(M, D, 1, 1)
    t32 = (pz if pz.ndim == 2 else pz[None].expand(M, D)).reshape(M, D, 1, 1) - depth.reshape(M, 1, *depth.shape[2:])   # fp32, as the kernel forms it
    below, above = t32 < np.float32(lo), t32 > np.float32(hi)
    if strict_lower_bound:
        below = t32 <= np.float32(lo)
    t64 = pz_md - d_leaf.reshape(M, 1, *depth.shape[2:])
    t64 = torch.where(below, torch.full_like(t64, lo), torch.where(above, torch.full_like(t64, hi), t64))
    alpha = (t64 - lo) / den                                               # [M,D,Ht,Wt]
    col = rgb.double()[:, None].expand(M, D, 3, *rgb.shape[2:])
    if bg is not None:
        col = torch.cat((col[:, :-1], bg.double()[:, None]), 1)
    vol = torch.cat((col, alpha[:, :, None]), 2)
    g = [torch.as_tensor(a).double() for a in geo]
    gc, gd, gT = up
    if gT is None:
        color, dep = geometry_render(vol, *g, v2m, align_corners=ac)
        T = None
    else:
        color, dep, T = tr.render(vol, *g, v2m, align_corners=ac)
    if out_pm1:
        color = 2 * color - 1
    loss = (color * torch.as_tensor(gc).double()).sum()
    if gd is not None:
        loss = loss + (dep * torch.as_tensor(gd).double()).sum()
    if gT is not None:
        loss = loss + (T * torch.as_tensor(gT).double()).sum()
    loss.backward()
    return pz_leaf.grad.numpy(), d_leaf.grad.numpy()


def _bar(got, ref, scale=1.0):
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    n = float(np.linalg.norm(ref))
    assert n > 0
    e = float(np.linalg.norm(got.astype(np.float64) - ref))
    print(f"plane_z: |got - ref| = {e:.3e}, |ref| = {n:.3e}, ratio {e / n:.3e}")
    assert e <= scale * 1e-4 * n, ("plane_z", e, n)


def _problem(cfg, seed=3, smooth=False):
    """(images as numpy, geo, (gc, gd, gT), v2m, views_per_mpi) of one case, as tests/test_hip_geometry_layouts.py builds them."""
    N, M, D, H, W, Ht, Wt = (cfg[k] for k in ("N", "M", "D", "H", "W", "Ht", "Wt"))
    rgb, depth, bg, pz = _images("depth", seed, M, D, Ht, Wt, smooth=smooth, pz_rows=cfg.get("pz_rows", False))
    if not cfg.get("bg", True):
        bg = None
    ray, eye, zd = _cam(N, H, W, seed=seed + 1, tilt=0.3)
    if cfg.get("miss"):
        eye[0, 0] += 0.2
    vpm = cfg.get("vpm")
    v2m = np.asarray(cfg.get("v2m", [n // vpm for n in range(N)] if vpm else np.arange(N) % M))
    gc, gd = _grads_in((N, H, W), seed + 2)
    gd = None if cfg.get("no_depth") else gd
    gT = np.random.default_rng(seed + 3).standard_normal((N, 1, H, W)).astype(np.float32) if cfg.get("gT") else None
    return (rgb, depth, bg, pz), (_dhw(M, D), ray, eye, zd), (gc, gd, gT), v2m, vpm


# ---- strict-order mode on white noise against float64 autograd ------------------------------------------------------------------------------------
EVERYTHING = ("pz",) + IMAGES + GEO
STRICT_CASES = [
    dict(BASE, ac=True, bg=True), dict(BASE, ac=True, bg=False), dict(BASE, ac=False, bg=True), dict(BASE, ac=False, bg=False),   # plane_z [D], M = 2: the sum over MPIs
    dict(BASE, ac=True, nz=256), dict(BASE, ac=False, nz=256),                      # step-like ramp: most taps are off the ramp
    dict(BASE, ac=False, pz_rows=True),                                             # plane_z [M, D]
    dict(N=3, M=1, D=5, Ht=16, Wt=16, H=33, W=17, ac=False, vpm=3),                 # three views of one MPI
    dict(N=4, M=2, D=4, Ht=20, Wt=20, H=18, W=30, ac=False, v2m=[1, 0, 1, 1], pz_rows=True),   # ragged view_to_mpi
    dict(N=4, M=2, D=4, Ht=20, Wt=20, H=18, W=30, ac=True, v2m=[1, 0, 1, 1]),
    dict(N=2, M=1, D=98, Ht=48, Wt=48, H=40, W=72, ac=True, vpm=2),                 # past the 96-plane chunk, ragged tiles
    dict(BASE, ac=True, dtype="bf16"), dict(BASE, ac=False, dtype="f16"),
    dict(BASE, ac=True, view=True), dict(BASE, ac=True, dtype="bf16", view=True, pz_rows=True),   # depth = channel view of an RGB-D tensor
    dict(BASE, ac=True, gT=True), dict(BASE, ac=False, gT=True, no_depth=True),     # the loss reaches T
    dict(BASE, ac=True, out_pm1=True),
    dict(N=2, M=2, D=5, Ht=24, Wt=24, H=24, W=24, ac=False, miss=True),             # view 0 partly misses every plane
    dict(BASE, ac=True, needs=EVERYTHING), dict(BASE, ac=False, pz_rows=True, needs=EVERYTHING, gT=True),   # every input requires grad at once
]


@pytest.mark.parametrize("cfg", STRICT_CASES, ids=_case_id)
def test_strict_matches_float64_autograd(cfg):
    """plane_z alone requires grad (no image, no camera) unless the case says otherwise."""
    images, geo, up, v2m, vpm = _problem(cfg)
    zb = _bounds(cfg.get("nz", 4))
    stored = _stored(images, DTYPES[cfg.get("dtype", "f32")], cfg.get("view", False))
    needs = cfg.get("needs", ("pz",))
    got, _ = _hip(stored, geo, up, cfg["ac"], True, zb, needs=needs, v2m=v2m, views_per_mpi=vpm, out_pm1=cfg.get("out_pm1", False))
    ref, _ = _reference(stored, geo, up, cfg["ac"], zb, v2m, out_pm1=cfg.get("out_pm1", False))
    assert got["pz"].shape == images[3].shape
    for k in EVERYTHING:
        assert (got[k] is not None) == (k in needs and not (k == "bg" and images[2] is None)), k
    if cfg.get("nz", 4) == 4:
        assert np.all(ref != 0)   # a wide ramp: every plane has texels on it
    _bar(got["pz"], ref)


def test_default_mode_on_smooth_inputs():
    cfg = dict(N=3, M=2, D=7, Ht=28, Wt=20, H=30, W=26, v2m=[0, 1, 1], pz_rows=True)
    for ac in (True, False):
        images, geo, up, v2m, _ = _problem(cfg, seed=5, smooth=True)
        stored = _stored(images, torch.float32)
        got, _ = _hip(stored, geo, up, ac, False, _bounds(4), v2m=v2m)
        ref, _ = _reference(stored, geo, up, ac, _bounds(4), v2m)
        _bar(got["pz"], ref, scale=10.0)


def test_a_tap_exactly_on_the_lower_bound_carries_the_gradient():
    """A block of depth texels at f32(plane_z[k] - lo): f32(plane_z[k] - d) == lo there, the ramp is exactly 0 and the clamp passes the gradient.  The
    footprints inside the block have four zero ramp taps on plane k -- the planes the instances without plane_z skip."""
    from ml_gmpi_amd.depth_alpha import ramp_constants
    cfg = dict(BASE, ac=True)
    images, geo, up, v2m, vpm = _problem(cfg, seed=2)
    rgb, depth, bg, pz = images
    zb = _bounds(4)
    lo = np.float32(ramp_constants(*zb)[0])
    k = 3
    d = np.float32(pz[k] - lo)
    for _ in range(8):   # (the rounded difference need not hit lo at once: walk d by ulps)
        if np.float32(pz[k] - d) == lo:
            break
        d = np.nextafter(d, np.float32(np.inf) if np.float32(pz[k] - d) > lo else np.float32(-np.inf))
    assert np.float32(pz[k] - d) == lo
    depth[:, :, 4:20, 5:23] = d
    stored = _stored((rgb, depth, bg, pz), torch.float32)
    got, _ = _hip(stored, geo, up, True, True, zb, v2m=v2m)
    ref, _ = _reference(stored, geo, up, True, zb, v2m)
    without, _ = _reference(stored, geo, up, True, zb, v2m, strict_lower_bound=True)
    assert abs(ref[k] - without[k]) > 1e-2 * np.linalg.norm(ref)   # (the block's term is far above the bar: skipping it would fail)
    _bar(got["pz"], ref)


# ---- translation invariance, determinism, nothing else moves ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ac", [True, False])
def test_translation_invariance_against_the_depth_gradient(ac):
    """Shifting plane_z[m, :] and depth[m] by the same amount changes no alpha: sum_k g_pz[m,k] = -sum_{y,x} depth.grad[m]."""
    images, geo, up, v2m, vpm = _problem(dict(BASE, pz_rows=True), seed=4)
    got, _ = _hip(_stored(images, torch.float32), geo, up, ac, True, _bounds(4), needs=("pz", "depth"), v2m=v2m, depth_backward="pixel")
    for m in range(BASE["M"]):
        lhs = abs(float(got["pz"][m].astype(np.float64).sum() + got["depth"][m].astype(np.float64).sum()))
        rhs = 1e-4 * float(np.abs(got["pz"][m]).astype(np.float64).sum())
        print(f"MPI {m}: |sum g_pz + sum g_depth| = {lhs:.3e}, bound {rhs:.3e}")
        assert rhs > 0 and lhs <= rhs, (m, lhs, rhs)


def test_two_runs_give_the_same_bits():
    images, geo, up, v2m, vpm = _problem(dict(BASE), seed=1)
    stored = _stored(images, torch.float32)
    a, _ = _hip(stored, geo, up, True, False, _bounds(4), needs=("pz", "dhw"), v2m=v2m)
    b, _ = _hip(stored, geo, up, True, False, _bounds(4), needs=("pz", "dhw"), v2m=v2m)
    assert np.abs(a["pz"]).max() > 0
    assert np.array_equal(a["pz"], b["pz"]) and np.array_equal(a["dhw"], b["dhw"])


@pytest.mark.parametrize("depth_backward", ["gather", "pixel", "tile"])
@pytest.mark.parametrize("strict", [False, True])
def test_nothing_else_moves(depth_backward, strict):
    """With and without plane_z.requires_grad: the gradients of dhw, ray, eye and z_dir are bit-identical; the image gradients are bit-identical under
    "gather" (no atomics) and agree to 2e-5 max|g| + 1e-6 under "pixel" and "tile" (fp32 atomics: the bar of
    tests/test_hip_geometry_layouts.py::test_image_gradients_are_undisturbed)."""
    images, geo, up, v2m, vpm = _problem(dict(BASE), seed=0)
    stored = _stored(images, torch.float32)
    run = lambda needs: _hip(stored, geo, up, True, strict, _bounds(4), needs=needs, views_per_mpi=1, depth_backward=depth_backward)[0]
    with_pz, without = run(EVERYTHING), run(IMAGES + GEO)
    assert with_pz["pz"] is not None and without["pz"] is None
    for k in GEO:
        assert np.abs(without[k]).max() > 0 and np.array_equal(with_pz[k], without[k]), k
    for k in IMAGES:
        assert np.abs(without[k]).max() > 0
        if depth_backward == "gather":
            assert np.array_equal(with_pz[k], without[k]), k
        else:
            assert float(np.abs(with_pz[k] - without[k]).max()) <= 2e-5 * float(np.abs(without[k]).max()) + 1e-6, k


# ---- the behaviour without "all" ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry_grad", [False, True])
def test_without_all_plane_z_is_detached_as_ever(geometry_grad):
    images, geo, up, v2m, vpm = _problem(dict(BASE), seed=1)
    stored = _stored(images, torch.float32)
    got, out = _hip(stored, geo, up, True, False, _bounds(4), needs=("pz", "rgb"), geometry_grad=geometry_grad, v2m=v2m)
    plain, out0 = _hip(stored, geo, up, True, False, _bounds(4), needs=("rgb",), geometry_grad=geometry_grad, v2m=v2m)
    assert got["pz"] is None and got["rgb"] is not None
    assert np.array_equal(out["color"], out0["color"]) and np.array_equal(out["depth"], out0["depth"])
    got, _ = _hip(stored, geo, up, True, False, _bounds(4), needs=("pz",), geometry_grad=geometry_grad, v2m=v2m)   # nothing is recorded
    assert got["pz"] is None


def test_normalized_plane_z_gives_the_renderers_own_bits():
    from ml_gmpi_amd import make_renderer
    for D in (5, 32):
        r = make_renderer("FFHQ", n_planes=D, device=DEV)
        assert torch.equal(r.normalized_plane_z(r.dynamic_mpi_plane_dhws[:, 0]).to(DEV), r.get_xyz_single_res(64, 64, only_z=True)[1].reshape(-1))


# ---- end to end: one learnable plane_ds through dhw[..., 0] and normalized_plane_z against central differences of the HIP forward ------------------
E2E = dict(S=64, D=5, seed=13, grid=4, n_z_bins=2, h=2e-4)


def _e2e_inputs():
    S, D = E2E["S"], E2E["D"]
    win = (np.sin(np.pi * (np.arange(S) + 0.5) / S) ** 2).astype(np.float32)
    win2 = win[:, None] * win[None, :]
    vol = _smooth_grid(E2E["seed"], (1, D, 4, S, S), E2E["grid"]) * win2
    depth = _smooth_grid(E2E["seed"] + 1, (1, 1, 4, S, S), E2E["grid"])[:, 0, :1] + 2.0 * (1.0 - win2)
    g = np.random.default_rng(91)
    wc, wd = g.standard_normal((1, 3, S, S)).astype(np.float32), g.standard_normal((1, 1, S, S)).astype(np.float32)
    return vol[:, 0, :3].copy(), depth.astype(np.float32), vol[:, -1, :3].copy(), wc, wd


def test_plane_distance_gradient_end_to_end_matches_finite_differences():
    """The procedure and the bars of tests/test_hip_geometry_layouts.py::test_pose_gradient_end_to_end_matches_finite_differences on the D plane
    distances: its smooth 64^2 inputs (4 x 4 noise grid, faded towards the border), D = 5, yaw = pitch = 0.1, central differences of the HIP forward
    with h = 2e-4, cos >= 0.999 and |a - f| <= 1e-2 |f|.

    THE INPUTS WERE CHOSEN FOR THE PROCEDURE, as there: a central difference averages across the kinks of the bilinear interpolant and of the ramp's
    clamps, the gradient does not.  The float64 restatement (tests/_geometry_ref.py on the expanded volume with plane_ds feeding dhw[..., 0] and,
    normalised, plane_z; its own central difference against its own autograd, same loss, pose and h) gives |a - f| / |f| over seeds 9 / 11 / 13 / 15 / 17:
    n_z_bins = 1: 3.0e-2, 3.9e-3, 2.2e-2, 9.3e-3, 1.1e-2;  2: 1.3e-2, 6.5e-3, 1.4e-3, 2.2e-2, 1.8e-2;  4: 1.2e-1, 1.7e-1, 2.1e-1, 1.1e-2, 4.0e-1.
    Used here: the seed and ramp width at which the restatement's own error is smallest, 1.4e-3 (seed 13, n_z_bins = 2; |a| = 4.3e3)."""
    from ml_gmpi_amd import make_renderer
    S, D, h = E2E["S"], E2E["D"], E2E["h"]
    r = make_renderer("FFHQ", n_planes=D, device=DEV, geometry_grad="all")
    rgb, depth, bg, wc, wd = (_t(a) for a in _e2e_inputs())
    static = r.static_mpi_plane_dhws.to(DEV)
    ds0 = static[:, 0].clone()

    def loss_of(plane_ds):
        r.dynamic_mpi_plane_dhws = torch.cat((plane_ds[:, None], static[:, 1:]), 1)
        out_rgb, out_depth = r.render_depth(rgb, depth, S, S, z_range=1, n_z_bins=E2E["n_z_bins"], plane_z=r.normalized_plane_z(plane_ds), background_rgb=bg,
                                            assert_not_out_of_last_plane=False, given_yaws=torch.tensor([[0.1]]), given_pitches=torch.tensor([[0.1]]))[:2]
        return (out_rgb * wc).sum() + 10.0 * (out_depth * wd).sum()

    try:
        ds = ds0.clone().requires_grad_(True)
        loss_of(ds).backward()
        a = ds.grad.double().cpu().numpy()
        f = np.zeros(D)
        with torch.no_grad():
            for k in range(D):
                e = torch.zeros_like(ds0)
                e[k] = h
                f[k] = float(loss_of(ds0 + e).double() - loss_of(ds0 - e).double()) / (2 * h)
    finally:
        r.dynamic_mpi_plane_dhws = r.static_mpi_plane_dhws
    cos = float(a @ f / (np.linalg.norm(a) * np.linalg.norm(f)))
    print(f"plane_ds: analytic {a}, central differences {f}, cos {cos:.6f}, |a - f| / |f| = {np.linalg.norm(a - f) / np.linalg.norm(f):.3e}")
    assert cos >= 0.999, (cos, a, f)
    assert np.linalg.norm(a - f) <= 1e-2 * np.linalg.norm(f), (a, f)
