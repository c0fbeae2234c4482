"""GPU tests of the shading augmentation (csrc/light_kernels.hip, ml_gmpi_amd.light) over the shape / dtype / layout matrix of
tests/_light_cases.py: non-square and ragged shapes, W % 4 != 0 (the scalar instances of the two apply kernels), a second x-block of the scalar
and of the vector instances, fp32 / bf16 / fp16 volumes, padded rows, an expanded batch, a misaligned base, a channel slice.

The whole pipeline is compared with float64 `torch_light_render` on the stored values and with `oracle.light_shade`, forward and backward, and
every kernel on its own so that a failure names it.  Bars (tests/test_light_shapes_cpu.py shows, without a GPU, that they mean something):
  pipeline / shading kernel vs float64   max(1e-5, 4 n0), n0 = the fp32 CPU chain against float64 on the same inputs (_light_cases.N0)
  pipeline vs oracle.light_shade         1e-5 where n0 <= 2.5e-6, max(1e-5, 4 n0) otherwise
  backward                               max(2e-4, 4 e_ref) max|g_ref| (+ the exact half ulp of a 16-bit result), e_ref = the fp32 CPU chain
  apply forward, g_rgba, alpha, masks    bit-exact;  g_shading: 3D 2^-24 sum|terms| per texel (fp32 summation of 3D products)
Run on the MI355X box:  python -m pytest tests -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import _light_cases as lc
from _util import load_npz
from test_hip_shared_color import _half_ulp
from test_light_render import _scipy_blur

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = list(lc.CASES)


def _renderer():
    import ml_gmpi_amd
    return ml_gmpi_amd.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, blur_ksize=lc.BLUR_KSIZE)


def _device_args(inp):
    dev = torch.device(DEV)
    return (torch.from_numpy(inp["plane_ds"]).reshape(-1, 1).to(dev), torch.from_numpy(inp["xyz"]).to(dev), torch.from_numpy(inp["light_dir"]).to(dev),
            inp["ka"], inp["kd"])


def _dtype_code(dtype):
    from ml_gmpi_amd import _lib
    return {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}[dtype]


# ---- the whole pipeline ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_pipeline_forward_matches_float64_and_oracle(name):
    inp = lc.inputs(name)
    vol = lc.lay_out(inp["stored"].to(DEV), inp["layout"])
    assert lc.takes_vector_instance(vol) == (inp["W"] % 4 == 0 and inp["layout"] in ("contiguous", "rowpad4", "expand", "chanslice"))
    out, depth, T, shading = _renderer()._forward_kernels(vol, *_device_args(inp))
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == tuple(vol.shape)
    got = out.cpu().numpy()
    values = inp["values"].float().numpy()
    want64 = lc.reference(inp)
    want32, _ = oracle.light_shade(values, inp["plane_ds"], inp["xyz"], inp["light_dir"], inp["ka"], inp["kd"])
    n0, bar = lc.N0[name], lc.bar(name)
    bar32 = 1e-5 if n0 <= 2.5e-6 else bar
    e64, e32 = float(np.abs(got - want64).max()), float(np.abs(got - want32).max())
    print(f"{name}: forward vs float64 {e64:.3e} (bar {bar:.1e}) vs oracle {e32:.3e} (bar {bar32:.1e})")
    assert np.array_equal(got[:, :, 3], values[:, :, 3])            # alpha passes through untouched
    assert e64 <= bar and e32 <= bar32, (e64, bar, e32, bar32)


@pytest.mark.parametrize("name", NAMES)
def test_pipeline_backward_matches_float64_autograd(name):
    from ml_gmpi_amd.light import _LightFunction
    inp = lc.inputs(name)
    dtype, expand = inp["dtype"], inp["layout"] == "expand"
    leaf = (inp["stored"][:1] if expand else inp["stored"]).to(DEV).requires_grad_(True)
    vol = leaf.expand(inp["stored"].shape) if expand else lc.lay_out(leaf, inp["layout"])
    out = _LightFunction.apply(vol, _renderer(), *_device_args(inp))
    assert out.requires_grad
    (out * torch.from_numpy(inp["g"]).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert leaf.grad.dtype == dtype and tuple(leaf.grad.shape) == tuple(leaf.shape)   # (the expanded batch: summed over the copies)
    got = leaf.grad.double().cpu().numpy()
    _, g64 = lc.reference(inp, grad=True)
    _, g32 = lc.reference(inp, dtype=torch.float32, grad=True)
    scale = float(np.abs(g64).max())
    e_ref = float(np.abs(g32 - g64).max()) / scale
    flat = max(2e-4, 4 * e_ref) * scale
    bound = flat + _half_ulp(np.maximum(np.abs(got), np.abs(g64)), dtype)             # (the rounding acted on the kernel's value)
    if expand and dtype is not torch.float32:   # each copy's gradient was rounded to the storage dtype before autograd added them up
        _, per_copy = lc.reference(dict(inp, layout="contiguous"), grad=True)
        bound = bound + sum(_half_ulp(np.abs(per_copy[b:b + 1]) + flat, dtype) for b in range(lc.B))
    err = np.abs(got - g64)
    print(f"{name}: backward max|g_ref| {scale:.3e} e_ref {e_ref:.2e} max err {err.max():.3e} ({err.max() / scale:.2e} rel, flat bar "
          f"{flat / scale:.1e}) alpha part {err[:, :, 3].max():.3e} margin {(err - bound).max():.2e}")
    assert np.abs(g64[:, :, :3]).max() > 0 and np.abs(g64[:, :, 3]).max() > 0
    assert (err <= bound).all(), (float(err.max()), scale, e_ref)
    assert float(np.abs(out.detach().cpu().numpy() - lc.reference(inp)).max()) <= lc.bar(name)


@pytest.mark.parametrize("shape", [(21, 37), (40, 256)])
@pytest.mark.parametrize("dt", list(lc.DTYPES))
def test_clip_mask_is_closed_at_both_bounds(shape, dt):
    """ka = 1, kd = 0: the shading is exactly 1, rgb * s sits ON the bounds for texels that are exactly 0 or exactly 1, and torch.clip passes the
    gradient there (min <= x <= max).  Every quantity is exact: out == the volume, the gradient == the upstream gradient (rounded to the dtype)."""
    from ml_gmpi_amd.light import _LightFunction
    H, W = shape
    dtype = lc.DTYPES[dt]
    stored = lc.stored_volume(7, H, W, dtype)
    assert (stored[:, :, :3] == 0).any() and (stored[:, :, :3] == 1).any()
    g = torch.from_numpy(np.random.default_rng(8).standard_normal(stored.shape).astype(np.float32))
    leaf = stored.to(DEV).requires_grad_(True)
    dev = torch.device(DEV)
    out = _LightFunction.apply(leaf, _renderer(), torch.from_numpy(lc.PLANE_DS).reshape(-1, 1).to(dev), torch.from_numpy(lc.texel_grid(H, W)).to(dev),
                               torch.from_numpy(lc.LIGHT_DIRS).to(dev), 1.0, 0.0)
    (out * g.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(out.detach().cpu(), stored.float())
    assert torch.equal(leaf.grad.cpu(), g.to(dtype))
    # the same through float64 autograd of the reference: it is the upstream gradient there too
    inp = dict(values=stored.double(), plane_ds=lc.PLANE_DS, xyz=lc.texel_grid(H, W), light_dir=lc.LIGHT_DIRS, ka=1.0, kd=0.0, g=g.numpy(), layout="contiguous")
    _, g64 = lc.reference(inp, grad=True)
    assert np.array_equal(g64, g.double().numpy())


@pytest.mark.parametrize("name", ["21x37", "50x18"])
def test_render_matches_the_reference_at_nonsquare_shapes(name):
    """`LightRenderer.render` itself (schedule, RNG, light) against the reference's own output at H != W.  Bar as for the oracle: today's 1e-5 where
    the reference's fp32 chain is within 2.5e-6 of float64, max(1e-5, 4 n0) otherwise, n0 measured here on the reference's side."""
    import ml_gmpi_amd
    fx = load_npz("light_render_nonsquare.npz")
    dev = torch.device(DEV)
    rgba, ref = fx[f"rgba_{name}"], fx[f"ref_{name}"]
    xyz = torch.from_numpy(fx[f"xyz_last_{name}"])[None].to(dev)          # render reads mpi_tex_pix_xyz[-1]
    L = ml_gmpi_amd.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, ka_max=0.6, kd_max=0.9, n_grow_iters=2)
    torch.manual_seed(321)
    for _ in range(3):
        out = L.render(torch.from_numpy(rgba).to(dev), torch.from_numpy(fx["dhw"]), xyz)
    assert np.allclose([L.cur_ka, L.cur_kd], fx[f"ka_kd_{name}"], rtol=0, atol=1e-12)
    inp = dict(values=torch.from_numpy(rgba).double(), plane_ds=fx["dhw"][:, 0], xyz=fx[f"xyz_last_{name}"], light_dir=fx[f"light_dir_{name}"],
               ka=L.cur_ka, kd=L.cur_kd, layout="contiguous")
    n0 = float(np.abs(ref - lc.reference(inp)).max())
    bar = 1e-5 if n0 <= 2.5e-6 else max(1e-5, 4 * n0)
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print(f"{name}: render vs the reference {err:.3e} (n0 {n0:.2e}, bar {bar:.1e})")
    assert err <= bar


def test_render_takes_a_volume_expanded_over_the_planes():
    """stride(1) == 0 (one plane shown D times) is a legal torch view; the apply entries refuse a plane stride of 0, so `render` has to hand
    them a copy -- forward and backward."""
    import ml_gmpi_amd
    dev = torch.device(DEV)
    H, W = 21, 37
    base = lc.stored_volume(3, H, W, torch.float32, planes=3)[:, 1:2].contiguous().to(dev)   # (a middle plane: smooth alpha below 1, a block of rgb == 0)
    dhw = torch.from_numpy(np.stack([lc.PLANE_DS, np.ones(lc.D, np.float32), np.ones(lc.D, np.float32)], 1))
    xyz = torch.from_numpy(lc.texel_grid(H, W))[None].to(dev)
    g = torch.from_numpy(np.random.default_rng(4).standard_normal((lc.B, lc.D, 4, H, W)).astype(np.float32)).to(dev)
    res = []
    for expanded in (True, False):
        leaf = base.clone().requires_grad_(True)
        vol = leaf.expand(lc.B, lc.D, 4, H, W)
        assert vol.stride(1) == 0
        L = ml_gmpi_amd.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, ka_max=0.6, kd_max=0.9, n_grow_iters=1)
        L.step = 3
        torch.manual_seed(9)
        out = L.render(vol if expanded else vol.contiguous(), dhw, xyz)
        (out * g).sum().backward()
        res.append((out.detach(), leaf.grad))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0])
    # the gradients are the same chain twice; torch's backward of the replicate padding (the border normals) adds with atomics, so the last bits
    # may differ from run to run: the backward's own fp32 bar, which each run keeps against float64
    scale = float(res[1][1].abs().max())
    diff = float((res[0][1] - res[1][1]).abs().max())
    print(f"plane-expanded volume: max|g| {scale:.3e}, expanded vs contiguous {diff:.3e}")
    assert scale > 0 and diff <= 2e-4 * scale
    alpha = base.expand(lc.B, lc.D, 4, H, W)[:, :, 3:]
    ds = torch.from_numpy(lc.PLANE_DS).to(dev)
    assert alpha.stride(1) == 0 and torch.equal(ml_gmpi_amd.light.compute_depth(alpha, ds), ml_gmpi_amd.light.compute_depth(alpha.contiguous(), ds))


# ---- kernel by kernel ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 300), (8, 1032), (5, 7), (50, 18), (24, 260)])
def test_blur_kernel_matches_scipy_on_wide_and_ragged_images(shape):
    H, W = shape
    depth = np.random.default_rng(6).uniform(0.9, 1.2, size=(3, 1, H, W)).astype(np.float32)
    got = _renderer().blurrer_func(torch.from_numpy(depth).to(DEV)).cpu().numpy()
    err = float(np.abs(got - _scipy_blur(depth)).max())
    print(f"blur {H}x{W}: {err:.3e} (bar 1.5e-6)")
    assert got.shape == depth.shape and err <= 1.5e-6


@pytest.mark.parametrize("shape", lc.SHAPES)
def test_shading_kernel_matches_float64_from_the_same_blurred_depth(shape):
    H, W = shape
    inp = lc.inputs(f"{H}x{W}-f32-contiguous")
    depth, _ = oracle.alpha_depth(inp["values"][:, :, 3:].float().numpy(), inp["plane_ds"])
    blurred = _scipy_blur(depth).astype(np.float32)                                    # one fp32 image for both sides
    args = (inp["light_dir"], inp["ka"], inp["kd"])
    got = _renderer().shading(torch.from_numpy(blurred).to(DEV), torch.from_numpy(inp["xyz"]).to(DEV), torch.from_numpy(inp["light_dir"]).to(DEV),
                              inp["ka"], inp["kd"]).cpu().numpy()
    s64 = lc.shading_numpy(blurred[:, 0], inp["xyz"], *args, np.float64)
    n0_s = float(np.abs(lc.shading_numpy(blurred[:, 0], inp["xyz"], *args, np.float32) - s64).max())   # the same formula in fp32 on the CPU
    bar = max(1e-5, 4 * n0_s)
    err = float(np.abs(got - s64).max())
    print(f"shading {H}x{W}: {err:.3e} (fp32 numpy floor {n0_s:.2e}, bar {bar:.1e}) range {s64.min():.3f} .. {s64.max():.3f}")
    assert got.shape == (lc.B, H, W) and got.dtype == np.float32
    assert err <= bar


def _apply_operands(name):
    """The case's volume view on the device, with a few colours outside [0, 1] (the entry clips whatever it is given), and a random shading image."""
    inp = lc.inputs(name)
    stored = inp["stored"].clone()
    stored[:, 0, :3, 0, :2] = -0.5
    stored[:, 3, :3, -1, -2:] = 1.5
    vol = lc.lay_out(stored.to(DEV), inp["layout"])
    rng = np.random.default_rng(21)
    H, W = inp["H"], inp["W"]
    s = rng.uniform(0.25, 1.75, size=(lc.B, H, W)).astype(np.float32)
    g = rng.standard_normal((lc.B, lc.D, 4, H, W)).astype(np.float32)
    return inp, vol, vol.float().cpu().numpy(), s, g


@pytest.mark.parametrize("name", NAMES)
def test_apply_entry_is_bit_exact(name):
    from ml_gmpi_amd import _lib
    lib = _lib.load_library()
    inp, vol, v, s, _ = _apply_operands(name)
    H, W = inp["H"], inp["W"]
    s_d = torch.from_numpy(s).to(DEV)
    out = torch.full((lc.B, lc.D, 4, H, W), float("nan"), dtype=torch.float32, device=DEV)
    rc = lib.gmpi_light_apply_launch(vol.data_ptr(), _dtype_code(inp["dtype"]), (ctypes.c_int64 * 5)(*vol.stride()), s_d.data_ptr(), out.data_ptr(),
                                     lc.B, lc.D, H, W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    got = out.cpu().numpy()
    want = v.copy()
    want[:, :, :3] = np.clip(v[:, :, :3] * s[:, None, None], np.float32(0), np.float32(1))   # one fp32 product and a clamp: nothing to tolerate
    assert np.array_equal(got, want), (np.isnan(got).sum(), float(np.nanmax(np.abs(got - want))))
    assert (want[:, :, :3] == 0).any() and (want[:, :, :3] == 1).any()


@pytest.mark.parametrize("name", NAMES)
def test_apply_backward_entry_masks_exactly_and_sums_within_the_fp32_bound(name):
    from ml_gmpi_amd import _lib
    lib = _lib.load_library()
    inp, vol, v, s, g = _apply_operands(name)
    H, W = inp["H"], inp["W"]
    s_d, g_d = torch.from_numpy(s).to(DEV), torch.from_numpy(g).to(DEV)
    g_rgba = torch.full((lc.B, lc.D, 4, H, W), float("nan"), dtype=torch.float32, device=DEV)
    g_s = torch.full((lc.B, H, W), float("nan"), dtype=torch.float32, device=DEV)
    rc = lib.gmpi_light_apply_backward_launch(vol.data_ptr(), _dtype_code(inp["dtype"]), (ctypes.c_int64 * 5)(*vol.stride()), s_d.data_ptr(),
                                              g_d.data_ptr(), g_rgba.data_ptr(), g_s.data_ptr(), lc.B, lc.D, H, W,
                                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    t = v[:, :, :3] * s[:, None, None]                                  # fp32, as the kernel forms it
    passes = (t >= 0) & (t <= 1)                                        # the closed mask of torch.clip
    want = g.copy()
    want[:, :, :3] = np.where(passes, g[:, :, :3] * s[:, None, None], np.float32(0))
    got = g_rgba.cpu().numpy()
    assert np.array_equal(got, want), (np.isnan(got).sum(), float(np.nanmax(np.abs(got - want))))
    terms = np.where(passes, g[:, :, :3].astype(np.float64) * v[:, :, :3].astype(np.float64), 0.0)
    want_s, mag = terms.sum((1, 2)), np.abs(terms).sum((1, 2))
    bound = 3 * lc.D * 2.0 ** -24 * mag                                 # 3D products, each rounded once, added in fp32 one after the other
    err = np.abs(g_s.cpu().numpy() - want_s)
    print(f"{name}: g_shading max err {err.max():.3e}, worst err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    assert passes.any() and not passes.all()


# ---- C ABI argument errors -------------------------------------------------------------------------------------------------------------------------
def test_argument_error_codes_of_the_light_entries():
    """Every refusal below returns before a launch; the valid call next to it shows that the other arguments were right."""
    from ml_gmpi_amd import _lib
    lib = _lib.load_library()
    dev = torch.device(DEV)
    Bn, Dn, H, W = 2, 3, 12, 20
    NULL, E_NULL, E_SHAPE, E_DTYPE, E_STRIDE = None, -1, -2, -3, -4
    SENT = 7.0
    vol = torch.rand((Bn, Dn, 4, H, W), device=dev)
    img = lambda: torch.full((Bn, 1, H, W), SENT, device=dev)
    depth, blurred, shading, g_shading = torch.rand((Bn, 1, H, W), device=dev) + 0.5, img(), img(), img()
    out, g_rgba, g_out = torch.full_like(vol, SENT), torch.full_like(vol, SENT), torch.rand_like(vol)
    k1 = lc.k1d().to(dev)
    xyz, ld = torch.from_numpy(lc.texel_grid(H, W)).to(dev), torch.from_numpy(lc.LIGHT_DIRS).to(dev)
    ds = torch.from_numpy(lc.PLANE_DS[:Dn].copy()).to(dev)
    T = torch.rand((Bn, 1, H, W), device=dev)
    st = lambda *s: (ctypes.c_int64 * 5)(*s)
    good = vol.stride()
    p = lambda t: t.data_ptr()

    def untouched(*tensors):
        torch.cuda.synchronize()
        return all(bool((t == SENT).all()) for t in tensors)

    # gmpi_light_blur_launch(depth, blurred, B, H, W, kernel1d, ksize, stream)
    blur = lambda d=p(depth), o=p(blurred), b=Bn, h=H, w=W, k=p(k1), ks=9: lib.gmpi_light_blur_launch(d, o, b, h, w, k, ks, None)
    assert blur(d=NULL) == E_NULL and blur(o=NULL) == E_NULL and blur(k=NULL) == E_NULL
    assert blur(ks=8) == E_SHAPE and blur(ks=0) == E_SHAPE and blur(h=4) == E_SHAPE and blur(w=4) == E_SHAPE and blur(b=-1) == E_SHAPE
    assert blur(ks=2 * H + 1) == E_SHAPE                                 # ksize / 2 >= H: reflect padding needs pad < size
    assert blur(b=0) == 0 and blur(b=0, d=NULL, o=NULL, k=NULL) == 0 and untouched(blurred)
    assert blur() == 0 and not untouched(blurred)

    # gmpi_light_shading_launch(depth_blurred, xyz_last, light_dir, ka, kd, B, H, W, shading, stream)
    shade = lambda d=p(blurred), x=p(xyz), l=p(ld), b=Bn, h=H, w=W, o=p(shading): lib.gmpi_light_shading_launch(d, x, l, 0.6, 0.9, b, h, w, o, None)
    assert shade(d=NULL) == E_NULL and shade(x=NULL) == E_NULL and shade(l=NULL) == E_NULL and shade(o=NULL) == E_NULL
    assert shade(h=2) == E_SHAPE and shade(w=2) == E_SHAPE and shade(b=-1) == E_SHAPE
    assert shade(b=0) == 0 and shade(b=0, d=NULL, x=NULL, l=NULL, o=NULL) == 0 and untouched(shading)
    assert shade() == 0 and not untouched(shading)

    # gmpi_light_apply_launch(rgba, dtype, stride[5], shading, out, B, D, H, W, stream)
    apply = lambda v=p(vol), dt=0, s=st(*good), sh=p(shading), o=p(out), b=Bn, d=Dn, h=H, w=W: lib.gmpi_light_apply_launch(v, dt, s, sh, o, b, d, h, w, None)
    assert apply(v=NULL) == E_NULL and apply(s=NULL) == E_NULL and apply(sh=NULL) == E_NULL and apply(o=NULL) == E_NULL
    assert apply(d=0) == E_SHAPE and apply(h=0) == E_SHAPE and apply(w=-3) == E_SHAPE and apply(b=-1) == E_SHAPE
    assert apply(b=256, d=256) == E_SHAPE                                # B * D == 65536: one plane per grid z
    assert apply(dt=7) == E_DTYPE and apply(dt=-1) == E_DTYPE
    assert apply(s=st(good[0], good[1], good[2], good[3], 2)) == E_STRIDE            # innermost stride != 1
    assert apply(s=st(good[0], good[1], good[2], W - 1, 1)) == E_STRIDE              # row stride < W
    assert apply(s=st(-good[0], good[1], good[2], good[3], 1)) == E_STRIDE           # negative batch stride
    assert apply(s=st(good[0], 0, good[2], good[3], 1)) == E_STRIDE and apply(s=st(good[0], good[1], 0, good[3], 1)) == E_STRIDE
    assert apply(b=0) == 0 and apply(b=0, v=NULL, s=NULL, sh=NULL, o=NULL) == 0 and untouched(out)
    assert apply(s=st(0, good[1], good[2], good[3], 1)) == 0 and not untouched(out)   # a batch stride of 0 is legal

    # gmpi_light_apply_backward_launch(rgba, dtype, stride[5], shading, grad_out, grad_rgba, grad_shading, B, D, H, W, stream)
    def bwd(v=p(vol), dt=0, s=st(*good), sh=p(shading), go=p(g_out), gr=p(g_rgba), gs=p(g_shading), b=Bn, d=Dn, h=H, w=W):
        return lib.gmpi_light_apply_backward_launch(v, dt, s, sh, go, gr, gs, b, d, h, w, None)
    for k in ("v", "s", "sh", "go", "gr", "gs"):
        assert bwd(**{k: NULL}) == E_NULL, k
    assert bwd(d=0) == E_SHAPE and bwd(h=0) == E_SHAPE and bwd(w=0) == E_SHAPE and bwd(b=-1) == E_SHAPE
    assert bwd(dt=3) == E_DTYPE
    assert bwd(s=st(good[0], good[1], good[2], good[3], 2)) == E_STRIDE and bwd(s=st(good[0], good[1], good[2], W - 1, 1)) == E_STRIDE
    assert bwd(s=st(-1, good[1], good[2], good[3], 1)) == E_STRIDE and bwd(s=st(good[0], 0, good[2], good[3], 1)) == E_STRIDE
    assert bwd(b=0) == 0 and untouched(g_rgba, g_shading)
    assert bwd() == 0 and not untouched(g_rgba) and not untouched(g_shading)

    # gmpi_alpha_depth_backward_ex_launch(alpha, dtype, sb, sd, srow, plane_ds, T, g_depth, g_T, grad_alpha, gb, gd, grow, B, D, H, W, stream)
    alpha = vol[:, :, 3:]
    ga = torch.full((Bn, Dn, 1, H, W), SENT, device=dev)
    gdep = torch.rand((Bn, 1, H, W), device=dev)

    def adb(ex=True, a=p(alpha), dt=0, sb=alpha.stride(0), sd=alpha.stride(1), sr=alpha.stride(3), pd=p(ds), t=p(T), gd_=p(gdep), gT=NULL, o=p(ga),
            gb=ga.stride(0), gdd=ga.stride(1), gr=ga.stride(3), b=Bn, d=Dn, h=H, w=W):
        if ex:
            return lib.gmpi_alpha_depth_backward_ex_launch(a, dt, sb, sd, sr, pd, t, gd_, gT, o, gb, gdd, gr, b, d, h, w, None)
        return lib.gmpi_alpha_depth_backward_launch(a, dt, sb, sd, sr, pd, t, gd_, o, gb, gdd, gr, b, d, h, w, None)
    for ex in (True, False):
        assert adb(ex, a=NULL) == E_NULL and adb(ex, pd=NULL) == E_NULL and adb(ex, o=NULL) == E_NULL
        assert adb(ex, d=0) == E_SHAPE and adb(ex, h=0) == E_SHAPE and adb(ex, w=0) == E_SHAPE and adb(ex, b=-1) == E_SHAPE
        assert adb(ex, dt=5) == E_DTYPE
        assert adb(ex, sb=-1) == E_STRIDE and adb(ex, sd=0) == E_STRIDE and adb(ex, sr=W - 1) == E_STRIDE
        assert adb(ex, gb=0) == E_STRIDE and adb(ex, gdd=0) == E_STRIDE and adb(ex, gr=W - 1) == E_STRIDE
        assert adb(ex, b=0) == 0
    assert adb(False, gd_=NULL) == E_NULL                                # the plain entry needs the depth gradient
    assert adb(True, gd_=NULL, gT=NULL) == 0 and untouched(ga)           # nothing to add
    ga.zero_()
    assert adb(True, t=NULL) == 0                                        # the transmittance is optional: rebuilt front to back
    torch.cuda.synchronize()
    assert float(ga.abs().max()) > 0 and bool(torch.isfinite(ga).all())
