"""GPU tests of compute_depth_ramp (gmpi_ramp_depth_launch / gmpi_ramp_depth_backward_launch: LightRenderer.compute_depth of a depth-alpha MPI
without the alpha planes) and of LightRenderer.render_depth.  The forward's definition is `compute_depth` on `depth_alpha_planes(...)`: bit for
bit against oracle.alpha_depth on planes made on the CPU.  The backward goes against float64 autograd of tests/_ramp_cases.ramp_chain (pinned to
that oracle without a GPU by tests/test_light_depth_alpha_cpu.py).  Run on the MI355X box:  python -m pytest tests -m gpu"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _ramp_cases as rc
from _torch_ref import torch_light_render, torch_render
from _util import load_npz
from test_hip_depth_alpha import E_REF_CAP, _bounds, _depth_image
from test_hip_shared_color import DTYPES, _compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BINS = [4, 32, 256]


@functools.lru_cache(maxsize=None)
def _reference(n_z_bins, dtype=torch.float32, reach=None):
    """(depth image, oracle depth, oracle T) of the base case.  Cached: shared by the tests, never written to."""
    depth = rc.depth_image(n_z_bins, dtype, reach)
    pz, ds = rc.plane_tables()
    return (depth,) + tuple(rc.oracle_reference(depth, pz, *_bounds(n_z_bins), ds))


def _run(depth_dev, plane_z, n_z_bins, plane_ds):
    from ml_gmpi_amd import compute_depth_ramp
    lo, hi = _bounds(n_z_bins)
    with torch.no_grad():
        z, t = compute_depth_ramp(depth_dev, plane_z.to(DEV), lo, hi, plane_ds, want_transmittance=True)
        z_only = compute_depth_ramp(depth_dev, plane_z.to(DEV), lo, hi, plane_ds)
    assert z.dtype == t.dtype == torch.float32 and z.shape == t.shape == (depth_dev.shape[0], 1, *depth_dev.shape[-2:])
    assert torch.equal(z, z_only) or bool(torch.isnan(z).any())
    return z.cpu().numpy(), t.cpu().numpy()


# ---- forward: bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_z_bins", [4, 256])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_forward_has_the_bits_of_the_oracle_on_the_planes(dtype, n_z_bins):
    import ml_gmpi_amd
    depth, z_ref, t_ref = _reference(n_z_bins, dtype)
    pz, ds = rc.plane_tables()
    if dtype is torch.float32:   # both starts of the backward's sweep are exercised by this case
        opaque = float((t_ref < 1e-30).mean())
        assert opaque >= 0.25 and 1 - opaque >= 0.25, opaque
    z, t = _run(depth.to(DEV), pz, n_z_bins, ds)
    assert np.array_equal(z, z_ref) and np.array_equal(t, t_ref)
    planes = ml_gmpi_amd.depth_alpha_planes(depth, pz, *_bounds(n_z_bins)).to(DEV)   # made on the CPU, copied
    with torch.no_grad():
        z2, t2 = ml_gmpi_amd.compute_depth(planes, ds, want_transmittance=True)
    assert np.array_equal(z, z2.cpu().numpy()) and np.array_equal(t, t2.cpu().numpy())
    # (a surface, not a constant: the image spans half of plane_z's range, its expected depth about half of plane_ds' 0.17)
    assert float(z_ref.max() - z_ref.min()) > 0.05


@pytest.mark.parametrize("variant", ["plane_z_per_mpi", "channel_view", "padded_rows", "expanded_batch", "one_plane", "w256", "w257"])
def test_forward_variants(variant):
    n_z_bins = 4
    lo, hi = _bounds(n_z_bins)
    pz, ds = rc.plane_tables()
    depth = rc.depth_image(n_z_bins)
    B, _, H, W = depth.shape
    if variant == "plane_z_per_mpi":
        pz = torch.stack([pz, pz * 0.9 + 0.03])
        dev_depth = depth.to(DEV)
    elif variant == "channel_view":
        rgbd = torch.rand((B, 4, H, W), generator=torch.Generator().manual_seed(1))
        rgbd[:, 3:] = depth
        dev_depth = rgbd.to(DEV)[:, 3:]
        assert not dev_depth.is_contiguous()
    elif variant == "padded_rows":
        buf = torch.full((B, 1, H, W + 3), float("nan"), device=DEV)
        buf[..., :W] = depth.to(DEV)
        dev_depth = buf[..., :W]
        assert dev_depth.stride(2) == W + 3
    elif variant == "expanded_batch":
        depth = depth[:1].expand(3, 1, H, W)
        dev_depth = depth[:1].to(DEV).expand(3, 1, H, W)
        assert dev_depth.stride(0) == 0
    elif variant == "one_plane":
        pz, ds = pz[5:6], ds[5:6]
        dev_depth = depth.to(DEV)
    else:
        depth = depth[..., :int(variant[1:])].contiguous()
        dev_depth = depth.to(DEV)
    z_ref, t_ref = rc.oracle_reference(depth, pz, lo, hi, ds)
    z, t = _run(dev_depth, pz, n_z_bins, ds)
    assert np.array_equal(z, z_ref) and np.array_equal(t, t_ref)
    assert 0 < float((t_ref < 0.5).mean()) and float(np.abs(z_ref).max()) > 0.5


def test_forward_nan_and_inf_texels_stay_in_their_texels():
    n_z_bins = 4
    lo, hi = _bounds(n_z_bins)
    pz, ds = rc.plane_tables()
    depth, z_clean, t_clean = _reference(n_z_bins)
    bad = depth.clone()
    bad[0, 0, 2, 17], bad[1, 0, 4, 299] = float("nan"), float("inf")
    z_ref, t_ref = rc.oracle_reference(bad, pz, lo, hi, ds)
    z, t = _run(bad.to(DEV), pz, n_z_bins, ds)
    assert np.array_equal(z, z_ref, equal_nan=True) and np.array_equal(t, t_ref, equal_nan=True)
    assert np.isnan(z[0, 0, 2, 17]) and z[1, 0, 4, 299] == 0 and t[1, 0, 4, 299] == 1   # (+inf: in front of no plane)
    keep = np.ones(z.shape, bool)
    keep[0, 0, 2, 17] = keep[1, 0, 4, 299] = False
    assert np.array_equal(z[keep], z_clean[keep]) and np.array_equal(t[keep], t_clean[keep])


# ---- backward ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _upstreams():
    g = np.random.default_rng(7)
    return tuple(torch.from_numpy(g.standard_normal((rc.B, 1, rc.H, rc.W)).astype(np.float32)) for _ in range(2))


def _chain_grad(depth, n_z_bins, gz, gt, dtype):
    pz, ds = rc.plane_tables()
    d = depth.to(dtype).clone().requires_grad_(True)
    z, t = rc.ramp_chain(d, pz, *_bounds(n_z_bins), ds, dtype)
    loss = torch.zeros((), dtype=dtype)
    for out, g in ((z, gz), (t, gt)):
        if g is not None:
            loss = loss + (out * g.to(dtype)).sum()
    loss.backward()
    return d.grad.double().numpy()


def _hip_grad(depth, n_z_bins, gz, gt):
    from ml_gmpi_amd import compute_depth_ramp
    pz, ds = rc.plane_tables()
    d = depth.to(DEV).clone().requires_grad_(True)
    z, t = compute_depth_ramp(d, pz.to(DEV), *_bounds(n_z_bins), ds, want_transmittance=True)
    loss = 0
    for out, g in ((z, gz), (t, gt)):
        if g is not None:
            loss = loss + (out * g.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert d.grad.dtype == depth.dtype and d.grad.shape == depth.shape
    return d.grad


def _check_backward(n_z_bins, dtype, reach, use_z, use_t):
    depth = rc.depth_image(n_z_bins, dtype, reach)
    gz, gt = (g if on else None for g, on in zip(_upstreams(), (use_z, use_t)))
    ref64, ref32 = _chain_grad(depth, n_z_bins, gz, gt, torch.float64), _chain_grad(depth, n_z_bins, gz, gt, torch.float32)
    scale = float(np.abs(ref64).max())
    e_ref = float(np.abs(ref32 - ref64).max()) / scale
    label = f"ramp backward n_z_bins {n_z_bins} {dtype} reach {reach} {'Z' * use_z}{'T' * use_t}"
    print(label, f"max|g_ref| {scale:.3e} e_ref {e_ref:.2e}")
    assert scale >= 1e-3, scale            # a gradient that vanishes would pass for free
    assert e_ref <= E_REF_CAP, e_ref
    got = _hip_grad(depth, n_z_bins, gz, gt).float().cpu().double().numpy()
    _compare((got,), (ref64,), (ref32,), dtype, label + " (depth image)", False, False)


# (gT alone on the base case with 32 or 256 bins: every texel ends opaque, max|g_ref| is 1e-16 -- nothing to compare; it runs on the holes case)
@pytest.mark.parametrize("combo", [(True, False), (True, True)], ids=["Z", "ZT"])
@pytest.mark.parametrize("n_z_bins", BINS)
def test_backward_matches_float64_autograd_of_the_chain(n_z_bins, combo):
    _check_backward(n_z_bins, torch.float32, None, *combo)


def test_backward_through_the_transmittance_alone():
    _check_backward(4, torch.float32, None, False, True)


@pytest.mark.parametrize("combo", [(True, False), (False, True), (True, True)], ids=["Z", "T", "ZT"])
@pytest.mark.parametrize("n_z_bins", [4, 256])
def test_backward_with_holes_behind_the_last_plane(n_z_bins, combo):
    _check_backward(n_z_bins, torch.float32, 1.35, *combo)


@pytest.mark.parametrize("n_z_bins", BINS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_backward_16_bit_storage_returns_the_gradient_in_the_inputs_dtype(dtype, n_z_bins):
    _check_backward(n_z_bins, dtype, None, True, True)


def test_backward_unused_outputs_are_passed_as_null_and_count_as_zero():
    from ml_gmpi_amd import compute_depth_ramp
    n_z_bins = 4
    depth = rc.depth_image(n_z_bins)
    gz, gt = _upstreams()
    zero = torch.zeros_like(gz)
    only_z, only_t = _hip_grad(depth, n_z_bins, gz, None), _hip_grad(depth, n_z_bins, None, gt)
    assert torch.equal(only_z, _hip_grad(depth, n_z_bins, gz, zero)) and torch.equal(only_t, _hip_grad(depth, n_z_bins, zero, gt))
    assert float(only_z.abs().max()) > 1e-3 and float(only_t.abs().max()) > 1e-3
    # the depth alone, T never asked for
    pz, ds = rc.plane_tables()
    d = depth.to(DEV).clone().requires_grad_(True)
    (compute_depth_ramp(d, pz.to(DEV), *_bounds(n_z_bins), ds) * gz.to(DEV)).sum().backward()
    assert torch.equal(d.grad, only_z)


def test_backward_entry_adds_into_a_padded_gradient_view():
    from ml_gmpi_amd import _lib, compute_depth_ramp
    from ml_gmpi_amd.depth_alpha import ramp_constants
    n_z_bins = 4
    depth = rc.depth_image(n_z_bins)
    B, _, H, W = depth.shape
    gz, gt = _upstreams()
    want = _hip_grad(depth, n_z_bins, gz, gt)
    lib = _lib.load_library()
    pz, ds = (t.to(DEV) for t in rc.plane_tables())
    d, gz_d, gt_d = depth.to(DEV), gz.to(DEV), gt.to(DEV)
    ramp = _lib.GmpiDepthAlpha()
    ramp.struct_size = ctypes.sizeof(_lib.GmpiDepthAlpha)
    ramp.plane_z, ramp.plane_z_stride = pz.data_ptr(), 0
    ramp.z_lo, ramp.z_hi, ramp.z_den = ramp_constants(*_bounds(n_z_bins))
    buf = torch.zeros((B, 1, H, W + 3), device=DEV)
    with torch.no_grad():
        _, T = compute_depth_ramp(d, pz, *_bounds(n_z_bins), ds, want_transmittance=True)   # (what the autograd node hands its backward)
    stream = torch.cuda.current_stream().cuda_stream
    launch = lambda: lib.gmpi_ramp_depth_backward_launch(d.data_ptr(), _lib.DTYPE_F32, d.stride(0), d.stride(2), ctypes.byref(ramp), ds.data_ptr(),
                                                         T.data_ptr(), gz_d.data_ptr(), gt_d.data_ptr(), buf.data_ptr(), buf.stride(0), buf.stride(2), B,
                                                         rc.D, H, W, stream)
    assert launch() == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[..., :W], want) and float(buf[..., W:].abs().max()) == 0
    assert launch() == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[..., :W], 2 * want) and float(buf[..., W:].abs().max()) == 0   # added into, not overwritten


def test_backward_nan_texel_changes_its_own_gradient_only():
    n_z_bins = 4
    depth = rc.depth_image(n_z_bins)
    gz, gt = _upstreams()
    clean = _hip_grad(depth, n_z_bins, gz, gt).cpu().numpy()
    bad = depth.clone()
    bad[1, 0, 3, 260] = float("nan")
    got = _hip_grad(bad, n_z_bins, gz, gt).cpu().numpy()
    keep = np.ones(got.shape, bool)
    keep[1, 0, 3, 260] = False
    assert np.array_equal(got[keep], clean[keep])
    assert got[1, 0, 3, 260] == 0   # torch.clamp passes no gradient where the difference is NaN


# ---- LightRenderer.render_depth ----------------------------------------------------------------------------------------------------------------
def _light_inputs(n_z_bins):
    fx = load_npz("light_render.npz")
    base = torch.from_numpy(fx["rgba"])
    depth, plane_z = _depth_image(base.shape[0], base.shape[-1], base.shape[1], n_z_bins)
    return base[:, 0, :3].contiguous(), depth, base[:, -1, :3].contiguous(), plane_z, torch.from_numpy(fx["dhw"]), torch.from_numpy(fx["xyz"])


def _new_light():
    import ml_gmpi_amd
    L = ml_gmpi_amd.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, ka_max=1.3, kd_max=0.9, n_grow_iters=1)
    L.step = 4
    return L


def _light_direction(L, seed, B):
    from ml_gmpi_amd import poses
    torch.manual_seed(seed)
    c2w, _, _ = poses.gen_sphere_path(n_cams=B, sphere_center=L.sphere_center, sphere_r=1.0, yaw_mean=L.l_h_mean, yaw_std=L.l_h_std,
                                      pitch_mean=L.l_v_mean, pitch_std=L.l_v_std, n_truncated_stds=2, flag_rnd=True,
                                      sample_method="truncated_gaussian")
    return poses._unit(L.sphere_center.reshape(1, 3) - torch.FloatTensor(c2w[:, :3, 3]))


def _bar(got, r64, r32, of_one=False):
    """max(1e-5, 4 e_ref) of the reference's maximum (the forward: of 1), e_ref = the fp32 torch chain on the CPU against float64.  Returns
    (max error, bound, e_ref, max|ref|)."""
    scale = 1.0 if of_one else float(r64.abs().max())
    e_ref = float((r32.double() - r64).abs().max()) / scale
    return float((got.double().cpu() - r64).abs().max()), max(1e-5, 4 * e_ref) * scale, e_ref, scale


@pytest.mark.parametrize("n_z_bins", [4, 256])
@pytest.mark.parametrize("with_bg", [False, True])
def test_light_renderer_render_depth(with_bg, n_z_bins):
    from ml_gmpi_amd import depth_alpha_planes, expand_depth_alpha
    dev = torch.device(DEV)
    rgb0, depth0, bg0, plane_z, dhw, xyz = _light_inputs(n_z_bins)
    lo, hi = _bounds(n_z_bins)
    g = np.random.default_rng(3)
    g_rgb, g_bg = (torch.from_numpy(g.standard_normal(rgb0.shape).astype(np.float32)) for _ in range(2))
    L, L2, L3 = _new_light(), _new_light(), _new_light()
    ins = [t.to(dev).requires_grad_(True) for t in (rgb0, depth0, bg0)]
    torch.manual_seed(11)
    o_rgb, o_depth, o_bg = L.render_depth(ins[0], ins[1], dhw, xyz.to(dev), plane_z=plane_z, z_range=1, n_z_bins=n_z_bins,
                                          background=ins[2] if with_bg else None)
    state = torch.get_rng_state()
    # (a) the schedule and the RNG advance as in `render` on the expanded volume
    torch.manual_seed(11)
    with torch.no_grad():
        L2.render(expand_depth_alpha(rgb0, depth0, plane_z, lo, hi, bg0 if with_bg else None).to(dev), dhw, xyz.to(dev))
    assert torch.equal(state, torch.get_rng_state())
    assert (L.step, L.cur_ka, L.cur_kd) == (L2.step, L2.cur_ka, L2.cur_kd) == (5, 1.3, 0.9)
    assert (o_bg is None) == (not with_bg) and o_depth is ins[1]
    assert o_rgb.dtype == torch.float32 and o_rgb.shape == rgb0.shape
    # (b) the colours of render_shared on the planes, made on the CPU
    torch.manual_seed(11)
    with torch.no_grad():
        s_rgb, _, s_bg = L3.render_shared(rgb0.to(dev), depth_alpha_planes(depth0, plane_z, lo, hi).to(dev), dhw, xyz.to(dev),
                                          background=bg0.to(dev) if with_bg else None)
    assert torch.equal(o_rgb.detach(), s_rgb) and (not with_bg or torch.equal(o_bg.detach(), s_bg))
    # (c) forward and gradients against float64 torch_light_render on expand_depth_alpha
    loss = (o_rgb * g_rgb.to(dev)).sum() + ((o_bg * g_bg.to(dev)).sum() if with_bg else 0)
    loss.backward()
    ld = _light_direction(L, 11, rgb0.shape[0])
    refs = {}
    for dt in (torch.float64, torch.float32):
        rin = [t.to(dt).requires_grad_(True) for t in (rgb0, depth0, bg0)]
        ref = torch_light_render(expand_depth_alpha(rin[0], rin[1], plane_z, lo, hi, rin[2] if with_bg else None), dhw[:, 0].to(dt), xyz[-1].to(dt),
                                 ld.to(dt), L.cur_ka, L.cur_kd, L._k1d.to(dt))
        r_rgb, r_bg = ref[:, 0, :3], ref[:, -1, :3]
        ((r_rgb * g_rgb.to(dt)).sum() + ((r_bg * g_bg.to(dt)).sum() if with_bg else 0)).backward()
        refs[dt] = dict(rgb=r_rgb.detach(), bg=r_bg.detach(), g_rgb=rin[0].grad, g_depth=rin[1].grad, g_bg=rin[2].grad)
    got = dict(rgb=o_rgb.detach(), bg=o_bg.detach() if with_bg else None, g_rgb=ins[0].grad, g_depth=ins[1].grad, g_bg=ins[2].grad)
    for name in ("rgb", "bg", "g_rgb", "g_depth", "g_bg"):
        if not with_bg and name in ("bg", "g_bg"):
            assert got[name] is None
            continue
        err, bound, e_ref, scale = _bar(got[name], refs[torch.float64][name], refs[torch.float32][name], of_one=name in ("rgb", "bg"))
        print(f"light render_depth bg {with_bg} n_z_bins {n_z_bins} {name}: max|ref| {scale:.3e} e_ref {e_ref:.2e} err {err:.3e} bound {bound:.3e}")
        assert scale >= 1e-3 and e_ref <= E_REF_CAP, (name, scale, e_ref)
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("n_z_bins", [4, 256])
def test_g_step_chain_light_render_depth_into_render_depth(n_z_bins):
    """generator -> LightRenderer.render_depth -> MPIRenderer.render_depth with nothing larger than an image, against the same chain through
    expand_depth_alpha, LightRenderer.render and render.  The bar is test_light_renderer_render_depth's, max(1e-5, 4 e_ref) of the reference's
    maximum; e_ref: the two steps as a torch chain on the CPU (torch_light_render, torch_render), fp32 against float64, same loss."""
    from ml_gmpi_amd import expand_depth_alpha, make_renderer
    dev = torch.device(DEV)
    rgb0, depth0, bg0, plane_z, dhw, xyz = _light_inputs(n_z_bins)
    lo, hi = _bounds(n_z_bins)
    B, S, D = rgb0.shape[0], rgb0.shape[-1], plane_z.numel()
    r = make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise")
    torch.manual_seed(5)
    with torch.no_grad():
        r.set_cam(r.cam_fov, S, S)
        cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    infos = dict(zip(["batch_yaws", "batch_pitches", "batch_tf_c2w", "batch_ray_dir", "batch_eye_pos", "batch_z_dir"], cam))
    g = np.random.default_rng(9)
    g_c = torch.from_numpy(g.standard_normal((B, 3, S, S)).astype(np.float32))
    g_d = torch.from_numpy(g.standard_normal((B, 1, S, S)).astype(np.float32))
    kw = dict(given_cam_infos=infos, assert_not_out_of_last_plane=False)
    grads = {}
    for layout in ("depth", "volume"):
        L = _new_light()
        ins = [t.to(dev).requires_grad_(True) for t in (rgb0, depth0, bg0)]
        torch.manual_seed(11)
        if layout == "depth":
            rgb2, depth2, bg2 = L.render_depth(ins[0], ins[1], r.static_mpi_plane_dhws, xyz.to(dev), plane_z=plane_z, z_range=1, n_z_bins=n_z_bins, background=ins[2])
            out = r.render_depth(rgb2, depth2, S, S, z_range=1, n_z_bins=n_z_bins, plane_z=plane_z.to(dev), background_rgb=bg2, **kw)
        else:
            vol = L.render(expand_depth_alpha(ins[0], ins[1], plane_z, lo, hi, ins[2]), r.static_mpi_plane_dhws, xyz.to(dev))
            out = r.render(vol, S, S, **kw)
        ((out[0] * g_c.to(dev)).sum() + (out[1] * g_d.to(dev)).sum()).backward()
        torch.cuda.synchronize()
        grads[layout] = [i.grad.cpu() for i in ins]
        ld, ka, kd, k1d = _light_direction(L, 11, B), L.cur_ka, L.cur_kd, L._k1d
    for gr in grads["depth"]:
        assert bool(torch.isfinite(gr).all())
    # e_ref of the chain on the CPU
    ray, eye, zd = (torch.cat(cam[i]).cpu() for i in (3, 4, 5))
    dhw_r = r.static_mpi_plane_dhws.reshape(1, -1, 3).expand(B, -1, -1)
    cpu = {}
    for dt in (torch.float64, torch.float32):
        rin = [t.to(dt).requires_grad_(True) for t in (rgb0, depth0, bg0)]
        vol = torch_light_render(expand_depth_alpha(rin[0], rin[1], plane_z, lo, hi, rin[2]), r.static_mpi_plane_dhws[:, 0].to(dt), xyz[-1].to(dt), ld.to(dt),
                                 ka, kd, k1d.to(dt))
        color, dep = torch_render(vol, dhw_r.to(dt), ray.to(dt), eye.to(dt), zd.to(dt), list(range(B)))
        (((2 * color - 1) * g_c.to(dt)).sum() + (dep * g_d.to(dt)).sum()).backward()
        cpu[dt] = [i.grad for i in rin]
    for name, got, want, r64, r32 in zip(("rgb", "depth", "background"), grads["depth"], grads["volume"], cpu[torch.float64], cpu[torch.float32]):
        scale = float(want.abs().max())
        e_ref = float((r32.double() - r64).abs().max()) / float(r64.abs().max())
        err, bound = float((got - want).abs().max()), max(1e-5, 4 * e_ref) * scale
        print(f"G-step chain n_z_bins {n_z_bins} {name}: max|g| {scale:.3e} e_ref {e_ref:.2e} |depth path - volume path| {err:.3e} bound {bound:.3e}"
              f" |volume path - float64| {float((want.double() - r64).abs().max()):.3e}")
        assert scale >= 1e-3 and e_ref <= E_REF_CAP, (name, scale, e_ref)
        assert err <= bound, (name, err, bound)
