"""Gradient of the render w.r.t. the sample positions (MPI(geometry_grad=True): dhw, ray_dir, eye_pos, z_dir; render_backward_geometry.hip)
against the float64 oracle of tests/_geometry_ref.py, its determinism, that nothing changes with the flag off, and c2w.grad end to end through
ml_gmpi_amd.rays_from_c2w against finite differences of the HIP forward."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from _geometry_ref import geometry_grads
from test_hip_edge_cases import _cam, _dhw

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _smooth_rgba(seed, shape, mode="bilinear"):
    """A 6 x 6 noise grid per channel, upsampled to Ht x Wt: a volume whose position gradient has no O(1) jumps at texel edges."""
    M, D, C, Ht, Wt = shape
    g = torch.Generator().manual_seed(seed)
    coarse = 0.25 + 0.5 * torch.rand((M * D, C, 6, 6), generator=g, dtype=torch.float64)
    coarse[:, 3] = 0.1 + 0.5 * coarse[:, 3]
    fine = F.interpolate(coarse, size=(Ht, Wt), mode=mode, align_corners=True).clamp(0, 1)
    return fine.reshape(M, D, C, Ht, Wt).float().numpy()


def _run(rgba, dhw, ray, eye, zd, v2m, gc, gd, ac, strict, dtype=torch.float32, views_per_mpi=None, backward="atomic", rgba_grad=False):
    """HIP gradients (dhw, ray, eye, zd[, rgba]) and the stored volume the kernel read (for the oracle)."""
    vol = _t(rgba).to(dtype)
    if rgba_grad:
        vol.requires_grad_(True)
    geo = [_t(a).requires_grad_(True) for a in (dhw, ray, eye, zd)]
    mpi = MPI(align_corners=ac, strict_order=strict, on_out_of_plane="raise", geometry_grad=True, backward=backward)
    kw = dict(views_per_mpi=views_per_mpi) if views_per_mpi is not None else dict(view_to_mpi=_t(np.asarray(v2m, np.int32)))
    out = mpi.render_views(vol, *geo, check_last_plane=False, **kw)
    loss = (out["color"] * _t(gc)).sum()
    if gd is not None:
        loss = loss + (out["depth"] * _t(gd)).sum()
    loss.backward()
    grads = [g.grad.cpu().numpy() for g in geo]
    if rgba_grad:
        grads.append(vol.grad.cpu())
    return grads, vol.detach().float().cpu().numpy()


def _check(got, ref, scale=1.0):
    g_dhw, g_ray, g_eye, g_z = got
    r_dhw, r_ray, r_eye, r_z = ref
    err = np.abs(g_ray - r_ray).max()
    assert err <= scale * 1e-4 * np.abs(r_ray).max(), ("ray_dir", err, np.abs(r_ray).max())
    for name, a, b in (("eye_pos", g_eye, r_eye), ("z_dir", g_z, r_z)):
        for n in range(a.shape[0]):
            e = np.linalg.norm(a[n] - b[n])
            assert e <= scale * 1e-4 * np.linalg.norm(b[n]), (name, n, e, np.linalg.norm(b[n]))
    e = np.linalg.norm(g_dhw - r_dhw)
    assert e <= scale * 1e-4 * np.linalg.norm(r_dhw), ("dhw", e, np.linalg.norm(r_dhw))


def _grads_in(shape, seed):
    g = np.random.default_rng(seed)
    N, H, W = shape
    return g.standard_normal((N, 3, H, W)).astype(np.float32), g.standard_normal((N, 1, H, W)).astype(np.float32)


from ml_gmpi_amd import MPI  # noqa: E402


@pytest.mark.parametrize("cfg", [
    dict(N=2, M=2, D=6, Ht=24, Wt=28, H=20, W=22, ac=True),
    dict(N=3, M=1, D=5, Ht=16, Wt=16, H=33, W=17, ac=False, vpm=3),                  # three views of one MPI sum into one dhw gradient
    dict(N=2, M=1, D=98, Ht=48, Wt=48, H=40, W=72, ac=True, vpm=2),                  # more planes than a chunk, ragged tiles
    dict(N=4, M=2, D=4, Ht=20, Wt=20, H=18, W=30, ac=False, v2m=[1, 0, 1, 1]),      # ragged view_to_mpi
    dict(N=2, M=2, D=6, Ht=24, Wt=28, H=20, W=22, ac=True, dtype="bf16"),
    dict(N=2, M=2, D=6, Ht=24, Wt=28, H=20, W=22, ac=False, dtype="f16"),
    dict(N=2, M=2, D=6, Ht=24, Wt=28, H=20, W=22, ac=True, no_depth=True),
    dict(N=1, M=1, D=8, Ht=32, Wt=32, H=32, W=32, ac=True, opaque=True),
    dict(N=2, M=2, D=5, Ht=24, Wt=24, H=24, W=24, ac=False, miss=True),             # view 0 partly misses every plane
])
def test_geometry_grad_strict_matches_oracle(cfg):
    N, M, D, H, W = cfg["N"], cfg["M"], cfg["D"], cfg["H"], cfg["W"]
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16}.get(cfg.get("dtype"), torch.float32)
    rgba = oracle.synth_rgba(61, (M, D, 4, cfg["Ht"], cfg["Wt"]), last_alpha_one=cfg.get("opaque", False),
                             bf16_round=cfg.get("dtype") == "bf16")
    if cfg.get("opaque"):
        rgba[:, 2:6, 3, : cfg["Ht"] // 3, :] = 1.0   # four exactly opaque planes in a row: the forward's T underflows, the pass re-walks
    ray, eye, zd = _cam(N, H, W, seed=62, tilt=0.3)
    if cfg.get("miss"):
        eye[0, 0] += 0.2
    dhw = _dhw(M, D)
    vpm = cfg.get("vpm")
    v2m = np.asarray(cfg.get("v2m", [n // vpm for n in range(N)] if vpm else np.arange(N) % M))
    gc, gd = _grads_in((N, H, W), 63)
    if cfg.get("no_depth"):
        gd = None
    got, stored = _run(rgba, dhw, ray, eye, zd, v2m, gc, gd, cfg["ac"], True, dtype=dtype, views_per_mpi=vpm)
    ref = geometry_grads(stored, dhw, ray, eye, zd, v2m, gc, gd, align_corners=cfg["ac"])
    assert np.abs(ref[1]).max() > 0 and np.linalg.norm(ref[0]) > 0
    if cfg.get("miss"):
        assert (np.abs(got[1][0]).sum(0) == 0).mean() > 0.05   # the rays that miss every plane carry no gradient
    _check(got, ref)


@pytest.mark.parametrize("ac", [True, False])
def test_geometry_grad_default_mode_on_smooth_volumes(ac):
    N, M, D, H, W = 3, 2, 7, 30, 26
    rgba = _smooth_rgba(5, (M, D, 4, 28, 20))
    ray, eye, zd = _cam(N, H, W, seed=64, tilt=0.3)
    dhw = _dhw(M, D)
    v2m = np.array([0, 1, 1])
    gc, gd = _grads_in((N, H, W), 65)
    got, stored = _run(rgba, dhw, ray, eye, zd, v2m, gc, gd, ac, False)
    ref = geometry_grads(stored, dhw, ray, eye, zd, v2m, gc, gd, align_corners=ac)
    _check(got, ref, scale=10.0)


def test_geometry_grad_is_deterministic_and_leaves_the_volume_gradient_alone():
    N, M, D, S = 4, 2, 8, 48
    rgba = oracle.synth_rgba(71, (M, D, 4, S, S))
    ray, eye, zd = _cam(N, S, S, seed=72, tilt=0.3)
    dhw = _dhw(M, D)
    gc, gd = _grads_in((N, S, S), 73)
    for backward in ("gather", "atomic"):
        a, _ = _run(rgba, dhw, ray, eye, zd, None, gc, gd, True, False, views_per_mpi=2, backward=backward, rgba_grad=True)
        b, _ = _run(rgba, dhw, ray, eye, zd, None, gc, gd, True, False, views_per_mpi=2, backward=backward, rgba_grad=True)
        for x, y in zip(a[:4], b[:4]):
            assert np.array_equal(x, y)   # no atomics: the same bits every run
        # the volume gradient with the flag off
        vol = _t(rgba).requires_grad_(True)
        mpi = MPI(on_out_of_plane="raise", backward=backward)
        out = mpi.render_views(vol, _t(dhw), _t(ray), _t(eye), _t(zd), views_per_mpi=2, check_last_plane=False)
        ((out["color"] * _t(gc)).sum() + (out["depth"] * _t(gd)).sum()).backward()
        want = vol.grad.cpu()
        if backward == "gather":
            assert torch.equal(a[4], want)
        else:
            assert float((a[4] - want).abs().max()) <= 2e-5 * float(want.abs().max()) + 1e-6


def test_flag_off_changes_nothing():
    N, M, D, S = 2, 2, 6, 32
    rgba, dhw = oracle.synth_rgba(81, (M, D, 4, S, S)), _dhw(M, D)
    ray, eye, zd = _cam(N, S, S, seed=82, tilt=0.3)
    with torch.no_grad():
        a = MPI(on_out_of_plane="raise", geometry_grad=True).render_views(_t(rgba), _t(dhw), _t(ray), _t(eye), _t(zd), views_per_mpi=1)
        b = MPI(on_out_of_plane="raise").render_views(_t(rgba), _t(dhw), _t(ray), _t(eye), _t(zd), views_per_mpi=1)
    assert torch.equal(a["color"], b["color"]) and torch.equal(a["depth"], b["depth"])
    mpi = MPI(on_out_of_plane="raise")
    vol, r = _t(rgba).requires_grad_(True), _t(ray).requires_grad_(True)
    out = mpi.render_views(vol, _t(dhw), r, _t(eye), _t(zd), views_per_mpi=1)
    out["color"].sum().backward()
    assert r.grad is None and vol.grad is not None
    with pytest.raises(NotImplementedError):
        mpi.render_views(_t(rgba), _t(dhw).requires_grad_(True), _t(ray), _t(eye), _t(zd))


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return torch.from_numpy(R)


def test_pose_gradient_end_to_end_matches_finite_differences():
    from ml_gmpi_amd import make_renderer, rays_from_c2w
    S, D = 64, 8
    r = make_renderer("FFHQ", n_planes=D, device=DEV, geometry_grad=True)
    # (bicubic: C1 across the coarse cells, and faded to 0 towards the texture's border -- the zero padding beyond it would put a kink of O(1)
    #  slope into every pixel that sees the border: finite differences average across kinks, the gradient does not)
    win = np.sin(np.pi * (np.arange(S) + 0.5) / S) ** 2
    vol = _t(_smooth_rgba(9, (1, D, 4, S, S), mode="bicubic") * (win[:, None] * win[None, :]).astype(np.float32))
    with torch.no_grad():
        c2w0 = r.render(vol, S, S, given_yaws=torch.tensor([[0.1]]), given_pitches=torch.tensor([[0.1]]),
                        assert_not_out_of_last_plane=False)[2].double()
    g = np.random.default_rng(91)
    wc, wd = _t(g.standard_normal((1, 3, S, S)).astype(np.float32)), _t(g.standard_normal((1, 1, S, S)).astype(np.float32))

    def loss_of(c2w):
        ray, eye, zd = rays_from_c2w(r, c2w)
        info = dict(batch_yaws=torch.zeros(1, 1), batch_pitches=torch.zeros(1, 1), batch_tf_c2w=c2w.detach(),
                    batch_ray_dir=[ray], batch_eye_pos=[eye], batch_z_dir=[zd])
        rgb, depth = r.render(vol, S, S, given_cam_infos=info, assert_not_out_of_last_plane=False)[:2]
        return (rgb * wc).sum() + 10.0 * (depth * wd).sum()

    c2w = c2w0.clone().requires_grad_(True)
    loss_of(c2w).backward()
    G = c2w.grad.cpu()
    R0 = c2w0[0, :3, :3].cpu()
    analytic, fd = [], []
    for i in range(6):
        if i < 3:   # translation along world axis i
            analytic.append(float(G[0, i, 3]))
            def step(h, ax=i):
                c = c2w0.clone()
                c[0, ax, 3] += h
                return c
            h = 2e-4
        else:       # small rotation about world axis i - 3, applied to the camera's rotation: d R = K R
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
