"""Gradient through the transmittance output T = prod_k (1 - a_k + 1e-10) of the render and of compute_depth: every backward path against the
float64 oracle of tests/_transmittance_ref.py, the geometry pass (geometry_grad=True), a c2w gradient end to end against finite differences of
the HIP forward, determinism, and that nothing changes without a gradient on T (the old entries, `_ex` with NULL and `_ex` with gT = 0 agree bit
for bit)."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import _transmittance_ref as tr
from test_hip_edge_cases import _cam, _dhw
from test_hip_geometry_grad import _check, _rot, _smooth_rgba

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ULP = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}   # (the volume gradient comes back in the volume's dtype)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _mpi(path, ac, strict, geometry=False):
    from ml_gmpi_amd import MPI
    return MPI(align_corners=ac, strict_order=strict, on_out_of_plane="raise", geometry_grad=geometry,
               variant="gather" if path == "gather" else "auto", backward="gather" if path == "pair" else "atomic")


def _upstream(N, H, W, seed, color=True, depth=True):
    g = np.random.default_rng(seed)
    gc = g.standard_normal((N, 3, H, W)).astype(np.float32) if color else None
    gd = g.standard_normal((N, 1, H, W)).astype(np.float32) if depth else None
    return gc, gd, g.standard_normal((N, 1, H, W)).astype(np.float32)


def _render_grad(mpi, rgba, dhw, ray, eye, zd, gc, gd, gT, dtype=torch.float32, geometry=False, **kw):
    """HIP: the gradient of sum gC C + gZ Z + gT T w.r.t. the volume [and the geometry], and the stored volume (for the oracle)."""
    vol = _t(rgba).to(dtype).requires_grad_(True)
    geo = [_t(a).requires_grad_(geometry) for a in (dhw, ray, eye, zd)]
    out = mpi.render_views(vol, *geo, check_last_plane=False, want_transmittance=True, **kw)
    assert out["T"].requires_grad
    loss = (out["T"] * _t(gT)).sum()
    if gc is not None:
        loss = loss + (out["color"] * _t(gc)).sum()
    if gd is not None:
        loss = loss + (out["depth"] * _t(gd)).sum()
    loss.backward()
    g = [vol.grad.float().cpu().numpy()] + ([a.grad.cpu().numpy() for a in geo] if geometry else [])
    return g, vol.detach().float().cpu().numpy()


def _assert_volume_grad(got, ref, name, ulp=0.0):
    scale = np.abs(ref).max()
    assert scale > 0
    err = np.abs(got - ref)
    assert np.all(np.isfinite(got)), name
    assert np.all(err <= 2e-5 * scale + 1e-6 + ulp * np.abs(ref)), (name, float(err.max()), float(scale))


# ---- 1. T.sum().backward(): every path, every storage dtype, both align_corners modes, strict and default order ------------------------------
CASES = [(path, dt, ac, strict) for path in ("tile2", "gather", "tile1", "pair") for dt in DTYPES for ac in (True, False) for strict in (False, True)
         if not (path == "pair" and not ac)]


@pytest.mark.parametrize("path,dt,ac,strict", CASES)
def test_transmittance_only_loss_matches_float64(path, dt, ac, strict):
    N, M, D, H, W = 2, 2, 6, 24, 40
    Ht, Wt = (20, 1) if path == "tile1" else (24, 28)   # (a texture one texel wide: the round-1 tile kernel)
    rgba = oracle.synth_rgba(101, (M, D, 4, Ht, Wt), bf16_round=dt == "bf16")
    ray, eye, zd = _cam(N, H, W, seed=102, tilt=0.3)
    dhw = _dhw(M, D)
    gT = np.ones((N, 1, H, W), np.float32)
    (got,), stored = _render_grad(_mpi(path, ac, strict), rgba, dhw, ray, eye, zd, None, None, gT, dtype=DTYPES[dt], views_per_mpi=1)
    ref = tr.grads(stored, dhw, ray, eye, zd, np.arange(N), g_T=gT, align_corners=ac)[0]
    assert np.abs(ref[:, :, :3]).max() == 0 and np.abs(got[:, :, :3]).max() == 0   # dT/drgb = 0
    _assert_volume_grad(got, ref, (path, dt, ac, strict), ULP[dt])


# ---- 2. mixed loss on ragged views; opaque, nearly opaque and underflowing stacks; the paths agree -------------------------------------------
def _hard_stack(M, D, Ht, Wt, seed):
    rgba = oracle.synth_rgba(seed, (M, D, 4, Ht, Wt))
    rgba[0, 2, 3, : Ht // 2] = 1.0               # exactly opaque in the middle
    rgba[0, 3, 3, Ht // 2:] = 1.0 - 1e-6         # nearly opaque
    rgba[1, 1:6, 3, :, : Wt // 2] = 1.0          # five exactly opaque planes in a row: T_out underflows, the kernels rebuild it
    return rgba


def test_mixed_loss_on_ragged_views_and_hard_stacks():
    # (default order: there the forward's bilinear sample and the backward's are the same fma chain.  In strict order the forward rounds the
    #  sample once per op and the backward does not: behind a 1 - 1e-6 plane one ulp of alpha is 6 % of om, for every output alike)
    strict = False
    N, M, D, H, W, Ht, Wt = 5, 2, 8, 20, 30, 24, 24
    rgba = _hard_stack(M, D, Ht, Wt, 111)
    ray, eye, zd = _cam(N, H, W, seed=112, tilt=0.3)
    dhw = _dhw(M, D)
    gc, gd, gT = _upstream(N, H, W, 113)
    results = {}
    for name, kw in (("v2m", dict(view_to_mpi=_t(np.array([1, 0, 1, 1, 0], np.int32)))), ("counts", dict(views_per_mpi=[2, 3]))):
        v2m = np.array([1, 0, 1, 1, 0]) if name == "v2m" else np.array([0, 0, 1, 1, 1])
        ref = tr.grads(rgba, dhw, ray, eye, zd, v2m, gc, gd, gT)[0]
        assert np.all(np.isfinite(ref))
        for path in ("tile2", "gather"):
            (got,), _ = _render_grad(_mpi(path, True, strict), rgba, dhw, ray, eye, zd, gc, gd, gT, **kw)
            _assert_volume_grad(got, ref, (name, path))
            results[(name, path)] = got
    for name in ("v2m", "counts"):
        a, b = results[(name, "tile2")], results[(name, "gather")]
        assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max()
    # uniform views: the atomics-free pair against the tile kernel and the float64 oracle
    N2 = 4
    ray2, eye2, zd2 = _cam(N2, H, W, seed=114, tilt=0.3)
    gc2, gd2, gT2 = _upstream(N2, H, W, 115)
    ref = tr.grads(rgba, dhw, ray2, eye2, zd2, np.array([0, 0, 1, 1]), gc2, gd2, gT2)[0]
    outs = [_render_grad(_mpi(path, True, strict), rgba, dhw, ray2, eye2, zd2, gc2, gd2, gT2, views_per_mpi=2)[0][0]
            for path in ("pair", "tile2")]
    for got in outs:
        _assert_volume_grad(got, ref, "uniform")
    assert np.abs(outs[0] - outs[1]).max() <= 1e-5 * np.abs(outs[1]).max()


# ---- 3. geometry_grad=True: the position gradients pick the T term up through the alpha sample gradient ---------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
def test_geometry_grad_strict_on_white_noise(mixed):
    N, M, D, H, W = 3, 2, 6, 20, 22
    rgba = oracle.synth_rgba(121, (M, D, 4, 24, 28))
    rgba[0, 2:6, 3, :8] = 1.0                     # four exactly opaque planes: underflowing T
    ray, eye, zd = _cam(N, H, W, seed=122, tilt=0.3)
    dhw, v2m = _dhw(M, D), np.array([0, 1, 1])
    gc, gd, gT = _upstream(N, H, W, 123, color=mixed, depth=mixed)
    got, stored = _render_grad(_mpi("tile2", True, True, geometry=True), rgba, dhw, ray, eye, zd, gc, gd, gT, geometry=True,
                               view_to_mpi=_t(v2m.astype(np.int32)))
    ref = tr.grads(stored, dhw, ray, eye, zd, v2m, gc, gd, gT)
    assert np.abs(ref[2]).max() > 0 and np.linalg.norm(ref[1]) > 0
    _assert_volume_grad(got[0], ref[0], "rgba")
    _check(got[1:], ref[1:])


@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("mixed", [False, True])
def test_geometry_grad_default_mode_on_smooth_volumes(ac, mixed):
    N, M, D, H, W = 3, 2, 7, 30, 26
    rgba = _smooth_rgba(131, (M, D, 4, 28, 20))
    ray, eye, zd = _cam(N, H, W, seed=132, tilt=0.3)
    dhw, v2m = _dhw(M, D), np.array([0, 1, 1])
    gc, gd, gT = _upstream(N, H, W, 133, color=mixed, depth=mixed)
    got, stored = _render_grad(_mpi("tile2", ac, False, geometry=True), rgba, dhw, ray, eye, zd, gc, gd, gT, geometry=True,
                               view_to_mpi=_t(v2m.astype(np.int32)))
    ref = tr.grads(stored, dhw, ray, eye, zd, v2m, gc, gd, gT, align_corners=ac)
    _check(got[1:], ref[1:], scale=10.0)


# ---- 4. end to end: render(want_transmittance=True), rays_from_c2w, a T-only loss -> c2w.grad against finite differences ----------------------
def test_pose_gradient_of_a_transmittance_loss_matches_finite_differences():
    from ml_gmpi_amd import make_renderer, rays_from_c2w
    S, D = 64, 8
    r = make_renderer("FFHQ", n_planes=D, device=DEV, geometry_grad=True)
    win = np.sin(np.pi * (np.arange(S) + 0.5) / S) ** 2
    vol = _t(_smooth_rgba(9, (1, D, 4, S, S), mode="bicubic") * (win[:, None] * win[None, :]).astype(np.float32))
    with torch.no_grad():
        c2w0 = r.render(vol, S, S, given_yaws=torch.tensor([[0.1]]), given_pitches=torch.tensor([[0.1]]),
                        assert_not_out_of_last_plane=False)[2].double()
    wT = _t(np.random.default_rng(141).standard_normal((1, 1, S, S)).astype(np.float32))

    def loss_of(c2w):
        ray, eye, zd = rays_from_c2w(r, c2w)
        info = dict(batch_yaws=torch.zeros(1, 1), batch_pitches=torch.zeros(1, 1), batch_tf_c2w=c2w.detach(),
                    batch_ray_dir=[ray], batch_eye_pos=[eye], batch_z_dir=[zd])
        T = r.render(vol, S, S, given_cam_infos=info, assert_not_out_of_last_plane=False, want_transmittance=True)[4]
        return 10.0 * (T * wT).sum()

    c2w = c2w0.clone().requires_grad_(True)
    loss_of(c2w).backward()
    G = c2w.grad.cpu()
    R0 = c2w0[0, :3, :3].cpu()
    analytic, fd = [], []
    for i in range(6):
        if i < 3:
            analytic.append(float(G[0, i, 3]))

            def step(h, ax=i):
                c = c2w0.clone()
                c[0, ax, 3] += h
                return c
        else:
            K = (_rot(i - 3, 1e-6) - _rot(i - 3, -1e-6)) / 2e-6
            analytic.append(float((G[0, :3, :3] * (K @ R0)).sum()))

            def step(h, ax=i - 3):
                c = c2w0.clone()
                c[0, :3, :3] = (_rot(ax, h).to(c) @ R0.to(c)).to(c)
                return c
        h = 2e-4
        with torch.no_grad():
            fd.append(float(loss_of(step(h)) - loss_of(step(-h))) / (2 * h))
    a, f = np.array(analytic), np.array(fd)
    cos = float(a @ f / (np.linalg.norm(a) * np.linalg.norm(f)))
    assert cos >= 0.999, (cos, a, f)
    assert np.linalg.norm(a - f) <= 1e-2 * np.linalg.norm(f), (a, f)


# ---- 5. determinism with gT: the pair and the geometry pass -----------------------------------------------------------------------------------
def test_pair_and_geometry_pass_are_bit_reproducible_with_gT():
    N, M, D, S = 4, 2, 8, 48
    rgba = _hard_stack(M, D, S, S, 151)
    ray, eye, zd = _cam(N, S, S, seed=152, tilt=0.3)
    dhw = _dhw(M, D)
    gc, gd, gT = _upstream(N, S, S, 153)
    for geometry in (False, True):
        runs = [_render_grad(_mpi("pair", True, False, geometry=geometry), rgba, dhw, ray, eye, zd, gc, gd, gT, geometry=geometry,
                             views_per_mpi=2)[0] for _ in range(2)]
        for x, y in zip(*runs):
            assert np.array_equal(x, y)


# ---- 6. nothing changes without gT ------------------------------------------------------------------------------------------------------------
def test_a_loss_without_T_is_bitwise_unchanged():
    N, M, D, S = 2, 2, 6, 32
    rgba, dhw = oracle.synth_rgba(161, (M, D, 4, S, S)), _dhw(M, D)
    ray, eye, zd = _cam(N, S, S, seed=162, tilt=0.3)
    gc, gd, _ = _upstream(N, S, S, 163)
    mpi = _mpi("pair", True, False, geometry=True)   # (bit-reproducible paths: the pair and the geometry pass)
    grads = []
    for want_T in (True, False):
        vol = _t(rgba).requires_grad_(True)
        geo = [_t(a).requires_grad_(True) for a in (dhw, ray, eye, zd)]
        out = mpi.render_views(vol, *geo, views_per_mpi=1, check_last_plane=False, want_transmittance=want_T)
        assert (out["T"] is not None) == want_T
        ((out["color"] * _t(gc)).sum() + (out["depth"] * _t(gd)).sum()).backward()
        grads.append([vol.grad.cpu()] + [g.grad.cpu() for g in geo])
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    # T's values do not depend on whether T requires grad
    with torch.no_grad():
        T0 = mpi.render_views(_t(rgba), _t(dhw), _t(ray), _t(eye), _t(zd), views_per_mpi=1, want_transmittance=True)["T"]
    T1 = mpi.render_views(_t(rgba).requires_grad_(True), _t(dhw), _t(ray), _t(eye), _t(zd), views_per_mpi=1, want_transmittance=True)["T"]
    assert T1.requires_grad and not T0.requires_grad
    assert torch.equal(T0, T1.detach())


@pytest.mark.parametrize("path", ["tile2", "gather", "tile1", "pair", "geometry"])
def test_abi_old_entry_ex_with_null_and_ex_with_zero_gT_agree_bitwise(path):
    from ml_gmpi_amd import _lib
    lib = _lib.load_library()
    # small launches whose results do not depend on the order of atomics: one tile, or footprints that never share a texel
    N, M, D = 1, 1, 5
    H, W, Ht, Wt = (8, 8, 16, 1) if path == "tile1" else (8, 8, 96, 96)
    rgba, dhw = oracle.synth_rgba(171, (M, D, 4, Ht, Wt)), _dhw(M, D)
    ray, eye, zd = _cam(N, H, W, seed=172, tilt=0.2)
    gc, gd, _ = _upstream(N, H, W, 173)
    mpi = _mpi(path, True, False)
    res = mpi.render_views(_t(rgba), _t(dhw), _t(ray), _t(eye), _t(zd), views_per_mpi=1, check_last_plane=False, want_transmittance=True,
                           _in_autograd_fn=True)
    p, keep = res.pop("_bwd")
    p.rgb_out = p.depth_out = p.status = None
    gc, gd, zero = _t(gc), _t(gd), torch.zeros((N, 1, H, W), dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    ws = None
    if path in ("pair", "geometry"):
        need = int(lib.gmpi_render_backward_workspace_bytes(ctypes.byref(p))) if path == "pair" else \
            int(lib.gmpi_render_geometry_backward_workspace_bytes(ctypes.byref(p), 1))
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    outs = []
    for mode in ("old", "null", "zero"):
        if path == "geometry":
            o = [torch.full(s, 7.0, device=DEV) for s in ((N, 3, H, W), (N, 3), (N, 3), (M, D, 3))]
            ptr = [x.data_ptr() for x in o]
            if mode == "old":
                rc = lib.gmpi_mpi_render_geometry_backward_launch(ctypes.byref(p), gc.data_ptr(), gd.data_ptr(), *ptr, stream)
            else:
                rc = lib.gmpi_mpi_render_geometry_backward_ex_launch(ctypes.byref(p), gc.data_ptr(), gd.data_ptr(),
                                                                     zero.data_ptr() if mode == "zero" else None, *ptr, stream)
        else:
            o = [torch.zeros((M, D, 4, Ht, Wt), dtype=torch.float32, device=DEV)]
            gs = (ctypes.c_int64 * 5)(*o[0].stride())
            if mode == "old":
                rc = lib.gmpi_mpi_render_backward_launch(ctypes.byref(p), gc.data_ptr(), gd.data_ptr(), o[0].data_ptr(), gs, stream)
            else:
                rc = lib.gmpi_mpi_render_backward_ex_launch(ctypes.byref(p), gc.data_ptr(), gd.data_ptr(),
                                                            zero.data_ptr() if mode == "zero" else None, o[0].data_ptr(), gs, stream)
        _lib.check(rc, path)
        torch.cuda.synchronize()
        outs.append([x.cpu() for x in o])
    assert float(outs[0][0].abs().max()) > 0
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b), path


# ---- 7. compute_depth --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
def test_compute_depth_gradient_through_depth_and_transmittance(dt):
    from ml_gmpi_amd import compute_depth
    B, D, H, W = 2, 7, 12, 40
    rgba = oracle.synth_rgba(181, (B, D, 4, H, W), bf16_round=dt == "bf16")
    rgba[0, 1:6, 3, :4] = 1.0        # five exactly opaque planes: T underflows, the backward rebuilds it
    rgba[1, 3, 3, :, :8] = 1.0 - 1e-6
    ds = np.linspace(1.2, 0.9, D).astype(np.float32)
    g = np.random.default_rng(182)
    gz, gT = g.standard_normal((B, 1, H, W)).astype(np.float32), g.standard_normal((B, 1, H, W)).astype(np.float32)
    vol = _t(rgba).to(DTYPES[dt]).requires_grad_(True)
    depth, T = compute_depth(vol[:, :, 3:], _t(ds), want_transmittance=True)
    assert depth.requires_grad and T.requires_grad
    ((depth * _t(gz)).sum() + (T * _t(gT)).sum()).backward()
    got = vol.grad.float().cpu().numpy()
    a = torch.from_numpy(vol.detach().float().cpu().numpy()[:, :, 3:]).double().requires_grad_(True)
    rd, rT = tr.alpha_depth(a, ds.astype(np.float64))
    ((rd * torch.from_numpy(gz).double()).sum() + (rT * torch.from_numpy(gT).double()).sum()).backward()
    assert np.abs(depth.detach().cpu().numpy() - rd.detach().numpy()).max() <= 1e-5
    assert np.all(got[:, :, :3] == 0)
    _assert_volume_grad(got[:, :, 3:], a.grad.numpy(), dt, ULP[dt])
    # T only, depth only
    for which in ("T", "depth"):
        vol.grad = None
        depth, T = compute_depth(vol[:, :, 3:], _t(ds), want_transmittance=True)
        ((T * _t(gT)).sum() if which == "T" else (depth * _t(gz)).sum()).backward()
        a.grad = None
        rd, rT = tr.alpha_depth(a, ds.astype(np.float64))
        ((rT * torch.from_numpy(gT).double()).sum() if which == "T" else (rd * torch.from_numpy(gz).double()).sum()).backward()
        _assert_volume_grad(vol.grad.float().cpu().numpy()[:, :, 3:], a.grad.numpy(), (dt, which), ULP[dt])
    with pytest.raises(NotImplementedError):
        compute_depth(vol[:, :, 3:], _t(ds).requires_grad_(True))
    with torch.no_grad():   # no autograd: the values are the same
        d0, T0 = compute_depth(vol[:, :, 3:], _t(ds), want_transmittance=True)
    d1, T1 = compute_depth(vol[:, :, 3:], _t(ds), want_transmittance=True)
    assert torch.equal(d0, d1.detach()) and torch.equal(T0, T1.detach())
