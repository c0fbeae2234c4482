"""GPU tests of LightRenderer(middle="hip"): the adjoint kernels of the shading augmentation's image-sized middle (csrc/light_kernels.hip:
light_shading_backward_kernel, gaussian_blur_backward_kernel), the shade-images pair of the shared-colour and depth-alpha layouts, and the autograd
nodes of ml_gmpi_amd.light built on them.  Bars:
  shading backward, pipeline, shading_image   max(2e-4, 4 e_ref) max|g_ref| (+ the exact half ulp of a 16-bit result), e_ref = the fp32 CPU torch chain
                                              against float64 on the same inputs (tests/test_hip_light_shapes.py's rule for the backward)
  blur adjoint                                n 2^-24 sum|terms| per texel, n = the number of terms the texel sums, against the transposed dense
                                              float64 operator; the kernel sums rows first, n_x + n_y <= n roundings
  render_shared / render_depth                tests/test_hip_light_depth_alpha.py's max(1e-5, 4 e_ref) of the reference's maximum
  shade images                                bit-exact (one fp32 product and a clamp); g_shading: 6 2^-24 sum|terms| (six products, added in fp32)
The index math of the references is pinned without a GPU by tests/test_light_middle_cpu.py.  Run on the MI355X box:  python -m pytest tests -m gpu"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _light_cases as lc
import _light_middle_ref as mr
from _torch_ref import torch_light_render
from test_hip_depth_alpha import E_REF_CAP, _bounds
from test_hip_light_depth_alpha import _bar, _light_direction, _light_inputs
from test_hip_shared_color import _half_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _renderer(middle="hip"):
    import ml_gmpi_amd
    return ml_gmpi_amd.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, blur_ksize=lc.BLUR_KSIZE, middle=middle)


def _lib_and_stream():
    from ml_gmpi_amd import _lib
    return _lib.load_library(), torch.cuda.current_stream().cuda_stream


def test_query_46_reports_the_entries():
    lib, _ = _lib_and_stream()
    assert lib.gmpi_query(46) == 1 and lib.gmpi_query(45) == -1


# ---- the shading-backward entry alone ------------------------------------------------------------------------------------------------------------
def _shading_backward(blurred, xyz, light, kd, g_s):
    """gmpi_light_shading_backward_launch on numpy operands -> grad_blurred [B,H,W] (numpy fp32); the output starts as NaN."""
    lib, stream = _lib_and_stream()
    d = torch.from_numpy(np.ascontiguousarray(blurred, np.float32)).to(DEV)
    Bn, _, H, W = d.shape
    x, l = torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(DEV), torch.from_numpy(np.ascontiguousarray(light, np.float32)).to(DEV)
    g = torch.from_numpy(np.ascontiguousarray(g_s, np.float32)).to(DEV)
    out = torch.full((Bn, H, W), float("nan"), device=DEV)
    rc = lib.gmpi_light_shading_backward_launch(d.data_ptr(), x.data_ptr(), l.data_ptr(), float(kd), g.data_ptr(), Bn, H, W, out.data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _shading_case(H, W):
    """(blurred fp32, xyz, upstream gradient fp32) of a shape.  Cached: shared by the tests, never written to."""
    g_s = np.random.default_rng(300 + H * W).standard_normal((mr.B, H, W)).astype(np.float32)
    return mr.surface(200 + H * W, H, W), lc.texel_grid(H, W), g_s


def _check_shading_backward(H, W, g_s, label):
    blurred, xyz, _ = _shading_case(H, W)
    _, g64 = mr.middle_autograd(blurred, xyz, lc.LIGHT_DIRS, lc.KA, lc.KD, [1.0], g_s)
    _, g32 = mr.middle_autograd(blurred, xyz, lc.LIGHT_DIRS, lc.KA, lc.KD, [1.0], g_s, dtype=torch.float32)
    got = _shading_backward(blurred, xyz, lc.LIGHT_DIRS, lc.KD, g_s)
    scale = float(np.abs(g64).max())
    e_ref = float(np.abs(g32.astype(np.float64) - g64).max()) / scale
    bar = max(2e-4, 4 * e_ref) * scale
    err = float(np.abs(got - g64[:, 0]).max())
    print(f"shading backward {H}x{W} {label}: max|g_ref| {scale:.3e} e_ref {e_ref:.2e} err {err:.3e} ({err / scale:.2e} rel, bar {bar / scale:.1e})")
    assert scale > 0 and np.isfinite(got).all()
    assert err <= bar, (err, bar)


# (3, 3) / (3, 8): a cell takes a whole image / column; (24, 260), (8, 1032): a second x-block and beyond
@pytest.mark.parametrize("shape", [(3, 3), (3, 8), (5, 7), (21, 37), (24, 260), (8, 1032)])
def test_shading_backward_matches_float64_autograd_from_the_same_blurred_depth(shape):
    H, W = shape
    _check_shading_backward(H, W, _shading_case(H, W)[2], "dense")


@pytest.mark.parametrize("where", ["ring", "corners"])
@pytest.mark.parametrize("shape", [(3, 8), (21, 37), (24, 260)])
def test_shading_backward_sums_the_replicas_of_a_border_gradient(shape, where):
    """An upstream gradient on the border ring (or the four corners) alone reaches the depth only through the replica sums."""
    H, W = shape
    full = _shading_case(H, W)[2]
    g_s = np.zeros_like(full)
    if where == "ring":
        g_s[:, 0], g_s[:, -1], g_s[:, :, 0], g_s[:, :, -1] = full[:, 0], full[:, -1], full[:, :, 0], full[:, :, -1]
    else:
        for y, x in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
            g_s[:, y, x] = full[:, y, x]
    _check_shading_backward(H, W, g_s, where)


@pytest.mark.parametrize("shape", [(5, 7), (24, 260)])
def test_shading_backward_is_exactly_zero_where_nothing_passes(shape):
    H, W = shape
    _, xyz, g_s = _shading_case(H, W)
    smooth = mr.surface(5, H, W, noise=0.0, bump=0.002)
    # a light pointing away from every normal: the diffuse term is 0 everywhere (the forward kernel says so), the clamp passes nothing
    away = -lc.LIGHT_DIRS
    s = _renderer().shading(torch.from_numpy(smooth).to(DEV), torch.from_numpy(xyz).to(DEV), torch.from_numpy(away).to(DEV), lc.KA, lc.KD).cpu().numpy()
    assert (s == np.float32(lc.KA)).all()
    assert (_shading_backward(smooth, xyz, away, lc.KD, g_s) == 0).all()
    # the same light the right way round: a gradient; with kd = 0 none
    assert np.abs(_shading_backward(smooth, xyz, lc.LIGHT_DIRS, lc.KD, g_s)).max() > 0
    assert (_shading_backward(smooth, xyz, lc.LIGHT_DIRS, 0.0, g_s) == 0).all()
    # a zero depth image: every normal is exactly 0; the output is finite, all zeros (torch autograd of the same formula: NaN)
    got = _shading_backward(np.zeros_like(smooth), xyz, lc.LIGHT_DIRS, lc.KD, g_s)
    assert np.isfinite(got).all() and (got == 0).all()


# ---- the blur adjoint alone ------------------------------------------------------------------------------------------------------------------------
def _blur_pair(x, y):
    """(blur(x), blur^T(y)) by the two kernels, numpy fp32 [B,H,W] each."""
    lib, stream = _lib_and_stream()
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    Bn, H, W = x.shape
    k = lc.k1d().to(DEV)
    fwd, adj = torch.full_like(xd, float("nan")), torch.full_like(yd, float("nan"))
    assert lib.gmpi_light_blur_launch(xd.data_ptr(), fwd.data_ptr(), Bn, H, W, k.data_ptr(), lc.BLUR_KSIZE, stream) == 0
    assert lib.gmpi_light_blur_backward_launch(yd.data_ptr(), adj.data_ptr(), Bn, H, W, k.data_ptr(), lc.BLUR_KSIZE, stream) == 0
    torch.cuda.synchronize()
    return fwd.cpu().numpy(), adj.cpu().numpy()


# (5, 7): H = r + 1, both reflected preimages of a row are live at once; (32, 33): W % 4 = 1; (24, 260), (8, 1032): further x-blocks
@pytest.mark.parametrize("shape", [(5, 7), (9, 6), (32, 33), (24, 260), (8, 1032)])
def test_blur_adjoint_matches_the_transposed_dense_operator(shape):
    H, W = shape
    rng = np.random.default_rng(500 + H * W)
    x, y = (rng.standard_normal((3, H, W)).astype(np.float32) for _ in range(2))
    k = lc.k1d().double().numpy()
    my, mx = mr.blur_matrix(H, k), mr.blur_matrix(W, k)
    cy, cx = mr.blur_matrix(H, np.ones_like(k)), mr.blur_matrix(W, np.ones_like(k))          # how many taps of output j read input i
    fwd, adj = _blur_pair(x, y)
    t = lambda m_y, g, m_x: np.einsum("jy,bjx->byx", m_y, np.einsum("bjk,kx->bjx", g, m_x))   # My^T g Mx
    want, mag = t(my, y.astype(np.float64), mx), t(my, np.abs(y).astype(np.float64), mx)     # (the weights are positive: sum|terms| = |M|^T |g| |M|)
    n = np.outer(cy.sum(0), cx.sum(0))[None]                                                 # terms per texel
    err, bound = np.abs(adj - want), n * U * mag
    print(f"blur adjoint {H}x{W}: max err {err.max():.3e}, worst err / bound {np.max(err / bound):.3f}, terms per texel {int(n.min())} .. {int(n.max())}")
    assert n.min() >= (lc.BLUR_KSIZE // 2 + 1) ** 2 and (n.sum() == lc.BLUR_KSIZE ** 2 * H * W)
    assert (err <= bound).all()
    # <blur(x), y> = <x, blur^T(y)>: each side within the summation bound of its kernel (the forward: 81 terms of two roundings each)
    lhs, rhs = (fwd.astype(np.float64) * y).sum(), (x * adj.astype(np.float64)).sum()
    fwd_mag = np.einsum("yj,bjx->byx", my, np.einsum("bjk,xk->bjx", np.abs(x).astype(np.float64), mx))   # My |x| Mx^T
    slack = ((lc.BLUR_KSIZE ** 2 + 1) * U * fwd_mag * np.abs(y)).sum() + (bound * np.abs(x)).sum()
    print(f"blur adjoint {H}x{W}: <blur x, y> - <x, blur^T y> = {lhs - rhs:.3e} (bound {slack:.3e})")
    assert abs(lhs - rhs) <= slack


# ---- the whole pipeline ----------------------------------------------------------------------------------------------------------------------------
def _device_args(inp):
    dev = torch.device(DEV)
    return (torch.from_numpy(inp["plane_ds"]).reshape(-1, 1).to(dev), torch.from_numpy(inp["xyz"]).to(dev), torch.from_numpy(inp["light_dir"]).to(dev),
            inp["ka"], inp["kd"])


@pytest.mark.parametrize("name", list(lc.CASES))
def test_pipeline_backward_with_the_hip_middle_matches_float64_autograd(name):
    """tests/test_hip_light_shapes.py::test_pipeline_backward_matches_float64_autograd with middle="hip": the same inputs, the same bound."""
    from ml_gmpi_amd.light import _LightFunction
    inp = lc.inputs(name)
    dtype, expand = inp["dtype"], inp["layout"] == "expand"
    leaf = (inp["stored"][:1] if expand else inp["stored"]).to(DEV).requires_grad_(True)
    vol = leaf.expand(inp["stored"].shape) if expand else lc.lay_out(leaf, inp["layout"])
    out = _LightFunction.apply(vol, _renderer("hip"), *_device_args(inp))
    assert out.requires_grad
    (out * torch.from_numpy(inp["g"]).to(DEV)).sum().backward()
    with torch.no_grad():
        out_torch = _LightFunction.apply(vol.detach(), _renderer("torch"), *_device_args(inp))
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), out_torch)                                       # the forward does not depend on the mode
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
    print(f"{name}: hip middle, backward max|g_ref| {scale:.3e} e_ref {e_ref:.2e} max err {err.max():.3e} ({err.max() / scale:.2e} rel, flat bar "
          f"{flat / scale:.1e}) alpha part {err[:, :, 3].max():.3e} margin {(err - bound).max():.2e}")
    assert np.abs(g64[:, :, :3]).max() > 0 and np.abs(g64[:, :, 3]).max() > 0
    assert (err <= bound).all(), (float(err.max()), scale, e_ref)
    assert float(np.abs(out.detach().cpu().numpy() - lc.reference(inp)).max()) <= lc.bar(name)


def _shading_image_grad(name, seed=9):
    """d sum(shading_image * g) / d volume through LightRenderer(middle="hip").shading_image -> (gradient on the device, light direction, ka, kd, g)."""
    import ml_gmpi_amd
    inp = lc.inputs(name)
    dev = torch.device(DEV)
    L = ml_gmpi_amd.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, ka_max=lc.KA, kd_max=lc.KD, n_grow_iters=1, blur_ksize=lc.BLUR_KSIZE, middle="hip")
    L.step = 3
    dhw = torch.from_numpy(np.stack([lc.PLANE_DS, np.ones(lc.D, np.float32), np.ones(lc.D, np.float32)], 1))
    g = torch.from_numpy(np.random.default_rng(seed).standard_normal((lc.B, 1, inp["H"], inp["W"])).astype(np.float32))
    leaf = inp["stored"].to(dev).requires_grad_(True)
    torch.manual_seed(seed)
    s = L.shading_image(leaf, dhw, torch.from_numpy(inp["xyz"])[None].to(dev))
    assert s.requires_grad and s.dtype == torch.float32 and tuple(s.shape) == (lc.B, 1, inp["H"], inp["W"])
    (s * g.to(dev)).sum().backward()
    torch.cuda.synchronize()
    return inp, leaf.grad, s.detach(), _light_direction(L, seed, lc.B), L.cur_ka, L.cur_kd, g


@pytest.mark.parametrize("name", ["21x37-f32-contiguous", "5x7-f32-contiguous", "24x260-bf16-contiguous", "8x1032-f16-contiguous"])
def test_shading_image_under_autograd_with_the_hip_middle(name):
    inp, grad, s, ld, ka, kd, g = _shading_image_grad(name)
    assert (ka, kd) == (lc.KA, lc.KD) and grad.dtype == inp["dtype"]
    refs = {}
    for dt in (torch.float64, torch.float32):
        v = inp["values"].to(dt)
        alpha = v[:, :, 3:].clone().requires_grad_(True)
        vol = torch.cat((torch.full_like(v[:, :, :3], 1.0 / 16), alpha), 2)                # a colour that never clips: out * 16 is the shading
        out = torch_light_render(vol, torch.from_numpy(lc.PLANE_DS).to(dt), torch.from_numpy(inp["xyz"]).to(dt), ld.to(dt), ka, kd, lc.k1d().to(dt))
        (out[:, 0, :1] * 16 * g.to(dt)).sum().backward()
        refs[dt] = alpha.grad.double().numpy()
    g64 = refs[torch.float64]
    got = grad.double().cpu().numpy()
    assert float(np.abs(got[:, :, :3]).max()) == 0                                          # the colours do not enter the shading
    scale = float(np.abs(g64).max())
    e_ref = float(np.abs(refs[torch.float32] - g64).max()) / scale
    bound = max(2e-4, 4 * e_ref) * scale + _half_ulp(np.maximum(np.abs(got[:, :, 3:]), np.abs(g64)), inp["dtype"])
    err = np.abs(got[:, :, 3:] - g64)
    print(f"{name}: shading_image, hip middle: max|g_ref| {scale:.3e} e_ref {e_ref:.2e} max err {err.max():.3e} margin {(err - bound).max():.2e}")
    assert scale > 0 and (err <= bound).all()


def test_two_backward_runs_give_the_same_bits():
    """The middle's kernels are gathers without atomics (the volume-sized ends already were): shading_image's and the pipeline's gradients repeat
    bit for bit."""
    from ml_gmpi_amd.light import _LightFunction
    a, b = _shading_image_grad("24x260-f32-contiguous"), _shading_image_grad("24x260-f32-contiguous")
    assert torch.equal(a[1], b[1]) and float(a[1].abs().max()) > 0
    inp = lc.inputs("24x260-f32-contiguous")
    grads = []
    for _ in range(2):
        leaf = inp["stored"].to(DEV).requires_grad_(True)
        (_LightFunction.apply(leaf, _renderer("hip"), *_device_args(inp)) * torch.from_numpy(inp["g"]).to(DEV)).sum().backward()
        grads.append(leaf.grad)
    torch.cuda.synchronize()
    assert torch.equal(grads[0], grads[1])


# ---- the shade-images pair ---------------------------------------------------------------------------------------------------------------------------
def _image_args(t):
    from ml_gmpi_amd import _lib
    code = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}[t.dtype]
    return t.data_ptr(), code, (ctypes.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))


@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("shape", [(5, 7), (24, 260)])
def test_shade_images_entries_are_exact_on_strided_images_of_two_dtypes(shape, with_bg):
    """A bf16 colour image with padded rows, an fp16 background that is a channel slice; colours outside [0, 1], on the bounds, and one NaN."""
    lib, stream = _lib_and_stream()
    H, W = shape
    Bn = 2
    rng = np.random.default_rng(31 + W)
    c_host = torch.from_numpy(rng.uniform(-0.25, 1.25, (Bn, 3, H, W)).astype(np.float32)).to(torch.bfloat16)
    b_host = torch.from_numpy(rng.uniform(-0.25, 1.25, (Bn, 3, H, W)).astype(np.float32)).to(torch.float16)
    c_host[:, :, 0, :2], c_host[:, :, 1, :2] = 0.0, 1.0
    c_host[0, 1, 2, 3] = float("nan")
    buf = torch.zeros((Bn, 3, H, W + 3), dtype=torch.bfloat16, device=DEV)
    buf[..., :W] = c_host.to(DEV)
    wide = torch.zeros((Bn, 5, H, W), dtype=torch.float16, device=DEV)
    wide[:, 1:4] = b_host.to(DEV)
    c, bg = buf[..., :W], (wide[:, 1:4] if with_bg else None)
    assert not c.is_contiguous() and (bg is None or not bg.is_contiguous())
    s = rng.uniform(0.25, 1.75, (Bn, H, W)).astype(np.float32)
    s[:, 0, :2] = 1.0                                                  # c * s sits ON the bounds there
    g_c, g_b = (rng.standard_normal((Bn, 3, H, W)).astype(np.float32) for _ in range(2))
    s_d, gc_d, gb_d = (torch.from_numpy(a).to(DEV) for a in (s, g_c, g_b))
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    o_c, o_b, gr_c, gr_b, gr_s = nan(Bn, 3, H, W), nan(Bn, 3, H, W), nan(Bn, 3, H, W), nan(Bn, 3, H, W), nan(Bn, H, W)
    none = (None, 0, None)
    p = lambda t: t.data_ptr() if with_bg else None
    assert lib.gmpi_light_shade_images_launch(*_image_args(c), *(_image_args(bg) if with_bg else none), s_d.data_ptr(), o_c.data_ptr(), p(o_b),
                                              Bn, H, W, stream) == 0
    assert lib.gmpi_light_shade_images_backward_launch(*_image_args(c), *(_image_args(bg) if with_bg else none), s_d.data_ptr(), gc_d.data_ptr(), p(gb_d),
                                                       gr_c.data_ptr(), p(gr_b), gr_s.data_ptr(), Bn, H, W, stream) == 0
    torch.cuda.synchronize()
    want_s = np.zeros((Bn, H, W))
    mag = np.zeros((Bn, H, W))
    for img, g, out, grad in ((c_host, g_c, o_c, gr_c),) + (((b_host, g_b, o_b, gr_b),) if with_bg else ()):
        v = img.float().numpy()
        t = v * s[:, None]                                              # fp32, as the kernel forms it
        with np.errstate(invalid="ignore"):
            passes = (t >= 0) & (t <= 1)                                # the closed mask of torch.clip; a NaN passes nothing
            want = np.where(np.isnan(t), np.float32(0), np.clip(t, np.float32(0), np.float32(1)))   # (a NaN colour shades to 0)
        assert np.array_equal(out.cpu().numpy(), want)
        assert np.array_equal(grad.cpu().numpy(), np.where(passes, g * s[:, None], np.float32(0)))
        terms = np.where(passes, g.astype(np.float64) * np.nan_to_num(v).astype(np.float64), 0.0)
        want_s, mag = want_s + terms.sum(1), mag + np.abs(terms).sum(1)
        assert passes.any() and not passes.all() and (want == 0).any() and (want == 1).any()
    err = np.abs(gr_s.cpu().numpy() - want_s)
    assert (err <= 6 * U * mag).all(), float(err.max())
    if not with_bg:
        assert bool(torch.isnan(o_b).all()) and bool(torch.isnan(gr_b).all())             # nothing written without a background
    # an upstream gradient that is NULL counts as zero; an output that is NULL is skipped
    only_s = nan(Bn, H, W)
    assert lib.gmpi_light_shade_images_backward_launch(*_image_args(c), *none, s_d.data_ptr(), None, None, None, None, only_s.data_ptr(), Bn, H, W,
                                                       stream) == 0
    torch.cuda.synchronize()
    assert float(only_s.abs().max()) == 0


# ---- render_shared / render_depth with the node of kernels -------------------------------------------------------------------------------------------
def _new_light(middle):
    import ml_gmpi_amd
    L = ml_gmpi_amd.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, ka_max=1.3, kd_max=0.9, n_grow_iters=1, middle=middle)
    L.step = 4
    return L


def _layout_run(layout, middle, n_z_bins, with_bg, leaves=(True, True, True), dtypes=(torch.float32,) * 3):
    """One step of render_depth / render_shared on the fixture of tests/test_hip_light_depth_alpha.py (render_shared: on its alpha planes, made on
    the CPU) -> (outputs, input gradients or None, the shading image of the same step by shading_image(), reference gradients by dtype)."""
    from ml_gmpi_amd import depth_alpha_planes, expand_depth_alpha, expand_shared_color
    dev = torch.device(DEV)
    rgb0, depth0, bg0, plane_z, dhw, xyz = _light_inputs(n_z_bins)
    lo, hi = _bounds(n_z_bins)
    geo0 = depth0 if layout == "depth" else depth_alpha_planes(depth0, plane_z, lo, hi)
    host = [t.to(dt) for t, dt in zip((rgb0, geo0, bg0), dtypes)]
    rng = np.random.default_rng(3)
    g_rgb, g_bg = (torch.from_numpy(rng.standard_normal(rgb0.shape).astype(np.float32)) for _ in range(2))
    L = _new_light(middle)
    ins = [t.to(dev).requires_grad_(req) for t, req in zip(host, leaves)]
    bg = ins[2] if with_bg else None
    torch.manual_seed(11)
    if layout == "depth":
        o_rgb, o_geo, o_bg = L.render_depth(ins[0], ins[1], dhw, xyz.to(dev), plane_z=plane_z, z_range=1, n_z_bins=n_z_bins, background=bg)
    else:
        o_rgb, o_geo, o_bg = L.render_shared(ins[0], ins[1], dhw, xyz.to(dev), background=bg)
    assert o_geo is ins[1] and (o_bg is None) == (not with_bg) and o_rgb.dtype == torch.float32
    ((o_rgb * g_rgb.to(dev)).sum() + ((o_bg * g_bg.to(dev)).sum() if with_bg else 0)).backward()
    torch.cuda.synchronize()
    # the shading of the same step, from shading_image() on the expanded volume
    L2 = _new_light("torch")
    expand = (lambda c, d, b: expand_depth_alpha(c, d, plane_z, lo, hi, b)) if layout == "depth" else expand_shared_color
    torch.manual_seed(11)
    with torch.no_grad():
        shading = L2.shading_image(expand(host[0].float(), host[1].float(), host[2].float() if with_bg else None).to(dev), dhw, xyz.to(dev))
    ld = _light_direction(L, 11, rgb0.shape[0])
    refs = {}
    for dt in (torch.float64, torch.float32):
        rin = [t.to(dt).requires_grad_(True) for t in host]
        ref = torch_light_render(expand(rin[0], rin[1], rin[2] if with_bg else None), dhw[:, 0].to(dt), xyz[-1].to(dt), ld.to(dt), L.cur_ka, L.cur_kd,
                                 L._k1d.to(dt))
        r_rgb, r_bg = ref[:, 0, :3], ref[:, -1, :3]
        ((r_rgb * g_rgb.to(dt)).sum() + ((r_bg * g_bg.to(dt)).sum() if with_bg else 0)).backward()
        refs[dt] = dict(rgb=r_rgb.detach(), bg=r_bg.detach(), g_rgb=rin[0].grad, g_geo=rin[1].grad, g_bg=rin[2].grad)
    got = dict(rgb=o_rgb.detach(), bg=o_bg.detach() if with_bg else None, g_rgb=ins[0].grad, g_geo=ins[1].grad, g_bg=ins[2].grad)
    return got, ins, shading, refs


@pytest.mark.parametrize("n_z_bins", [4, 256])
@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("layout", ["depth", "shared"])
def test_layout_renders_with_the_hip_middle(layout, with_bg, n_z_bins):
    got, ins, shading, refs = _layout_run(layout, "hip", n_z_bins, with_bg)
    torch_mode, _, _, _ = _layout_run(layout, "torch", n_z_bins, with_bg)
    label = f"light render_{layout} hip bg {with_bg} n_z_bins {n_z_bins}"
    for name, image in (("rgb", ins[0]),) + ((("bg", ins[2]),) if with_bg else ()):
        # the node's shading has the bits of shading_image(), and the colour is ONE fp32 product of it and a clamp -- the torch mode's own
        # expression, so the result is that expression's, bit for bit
        assert torch.equal(got[name], torch.clip(image.detach().float() * shading, 0.0, 1.0)), name
        # against the torch mode's colours: its shading is a restatement with another blur (two GEMMs), so the two differ by the forward's noise
        err, bound, e_ref, _ = _bar(got[name], refs[torch.float64][name], refs[torch.float32][name], of_one=True)
        diff = float((got[name] - torch_mode[name]).abs().max())
        print(f"{label} {name}: vs float64 {err:.3e} (bound {bound:.3e}, e_ref {e_ref:.2e}); |hip mode - torch mode| {diff:.3e}")
        assert err <= bound and diff <= 2 * bound, (name, err, diff, bound)
    for name in ("g_rgb", "g_geo", "g_bg"):
        if not with_bg and name == "g_bg":
            assert got[name] is None
            continue
        err, bound, e_ref, scale = _bar(got[name], refs[torch.float64][name], refs[torch.float32][name])
        print(f"{label} {name}: max|ref| {scale:.3e} e_ref {e_ref:.2e} err {err:.3e} bound {bound:.3e}")
        assert scale >= 1e-3 and e_ref <= E_REF_CAP, (name, scale, e_ref)
        assert err <= bound, (name, err, bound)
        assert got[name].dtype == torch.float32


@pytest.mark.parametrize("layout", ["depth", "shared"])
def test_layout_renders_with_only_the_geometry_requiring_grad_and_16_bit_colours(layout):
    """Only the depth image / the alpha planes require grad: the colour gradients get no buffer, and the depth's is the full run's, bit for bit.
    Then bf16 colours and an fp16 background: each gradient comes back in its tensor's dtype, within the bar plus that dtype's half ulp."""
    full, _, _, _ = _layout_run(layout, "hip", 4, True)
    only, _, _, _ = _layout_run(layout, "hip", 4, True, leaves=(False, True, False))
    assert only["g_rgb"] is None and only["g_bg"] is None and torch.equal(only["g_geo"], full["g_geo"])
    assert torch.equal(only["rgb"], full["rgb"]) and torch.equal(only["bg"], full["bg"])
    dtypes = (torch.bfloat16, torch.float32, torch.float16)
    got, _, _, refs = _layout_run(layout, "hip", 4, True, dtypes=dtypes)
    for name, dt in zip(("g_rgb", "g_geo", "g_bg"), dtypes):
        assert got[name].dtype == dt
        r64 = refs[torch.float64][name]
        _, bound, e_ref, scale = _bar(got[name], r64, refs[torch.float32][name])
        err = (got[name].double().cpu() - r64).abs().numpy()
        slack = bound + _half_ulp(np.maximum(np.abs(got[name].double().cpu().numpy()), np.abs(r64.numpy())), dt)
        print(f"light render_{layout} hip mixed dtypes {name}: max|ref| {scale:.3e} e_ref {e_ref:.2e} err {err.max():.3e} bound {bound:.3e}")
        assert scale >= 1e-3 and e_ref <= E_REF_CAP and (err <= slack).all(), (name, float(err.max()), bound)


# ---- C ABI argument errors ---------------------------------------------------------------------------------------------------------------------------
def test_argument_error_codes_of_the_middle_entries():
    """Every refusal below returns before a launch; the valid call next to it shows that the other arguments were right."""
    lib, _ = _lib_and_stream()
    dev = torch.device(DEV)
    Bn, H, W = 2, 12, 20
    NULL, E_NULL, E_SHAPE, E_DTYPE, E_STRIDE = None, -1, -2, -3, -4
    SENT = 7.0
    img = lambda: torch.full((Bn, 1, H, W), SENT, device=dev)
    col = lambda: torch.full((Bn, 3, H, W), SENT, device=dev)
    blurred, g_s, g_blurred, g_depth = torch.rand((Bn, 1, H, W), device=dev) + 0.5, torch.rand((Bn, 1, H, W), device=dev), img(), img()
    k1 = lc.k1d().to(dev)
    xyz, ld = torch.from_numpy(lc.texel_grid(H, W)).to(dev), torch.from_numpy(lc.LIGHT_DIRS).to(dev)
    rgb, bg, shading = torch.rand((Bn, 3, H, W), device=dev), torch.rand((Bn, 3, H, W), device=dev), torch.rand((Bn, 1, H, W), device=dev) + 0.5
    o_rgb, o_bg, gr_rgb, gr_bg, gr_s = col(), col(), col(), col(), img()
    go_rgb, go_bg = torch.rand_like(rgb), torch.rand_like(bg)
    st = lambda *s: (ctypes.c_int64 * 3)(*s)
    good = (rgb.stride(0), rgb.stride(1), rgb.stride(2))
    p = lambda t: t.data_ptr()

    def untouched(*tensors):
        torch.cuda.synchronize()
        return all(bool((t == SENT).all()) for t in tensors)

    # gmpi_light_shading_backward_launch(depth_blurred, xyz_last, light_dir, kd, grad_shading, B, H, W, grad_blurred, stream)
    sb = lambda d=p(blurred), x=p(xyz), l=p(ld), g=p(g_s), b=Bn, h=H, w=W, o=p(g_blurred): lib.gmpi_light_shading_backward_launch(d, x, l, 0.9, g, b, h, w, o, None)
    for k in ("d", "x", "l", "g", "o"):
        assert sb(**{k: NULL}) == E_NULL, k
    assert sb(h=2) == E_SHAPE and sb(w=2) == E_SHAPE and sb(b=-1) == E_SHAPE and sb(b=65536) == E_SHAPE and sb(h=65536) == E_SHAPE
    assert sb(b=0) == 0 and sb(b=0, d=NULL, x=NULL, l=NULL, g=NULL, o=NULL) == 0 and untouched(g_blurred)
    assert sb() == 0 and not untouched(g_blurred)

    # gmpi_light_blur_backward_launch(grad_blurred, grad_depth, B, H, W, kernel1d, ksize, stream)
    bb = lambda g=p(g_s), o=p(g_depth), b=Bn, h=H, w=W, k=p(k1), ks=9: lib.gmpi_light_blur_backward_launch(g, o, b, h, w, k, ks, None)
    assert bb(g=NULL) == E_NULL and bb(o=NULL) == E_NULL and bb(k=NULL) == E_NULL
    assert bb(ks=8) == E_SHAPE and bb(ks=0) == E_SHAPE and bb(h=4) == E_SHAPE and bb(w=4) == E_SHAPE and bb(b=-1) == E_SHAPE
    assert bb(ks=2 * H + 1) == E_SHAPE and bb(b=65536) == E_SHAPE
    assert bb(b=0) == 0 and bb(b=0, g=NULL, o=NULL, k=NULL) == 0 and untouched(g_depth)
    assert bb() == 0 and not untouched(g_depth)

    # gmpi_light_shade_images_launch(rgb, dtype, stride[3], background, dtype, stride[3], shading, rgb_out, background_out, B, H, W, stream)
    def si(c=p(rgb), cdt=0, cs=st(*good), g=p(bg), gdt=0, gs=st(*good), s=p(shading), oc=p(o_rgb), og=p(o_bg), b=Bn, h=H, w=W):
        return lib.gmpi_light_shade_images_launch(c, cdt, cs, g, gdt, gs, s, oc, og, b, h, w, None)
    assert si(c=NULL) == E_NULL and si(cs=NULL) == E_NULL and si(gs=NULL) == E_NULL and si(s=NULL) == E_NULL and si(oc=NULL) == E_NULL and si(og=NULL) == E_NULL
    assert si(h=0) == E_SHAPE and si(w=-3) == E_SHAPE and si(b=-1) == E_SHAPE and si(b=65536) == E_SHAPE
    assert si(cdt=7) == E_DTYPE and si(cdt=-1) == E_DTYPE and si(gdt=3) == E_DTYPE
    assert si(cs=st(-1, good[1], good[2])) == E_STRIDE and si(cs=st(good[0], 0, good[2])) == E_STRIDE and si(cs=st(good[0], good[1], W - 1)) == E_STRIDE
    assert si(gs=st(good[0], good[1], W - 1)) == E_STRIDE
    assert si(b=0) == 0 and si(b=0, c=NULL, cs=NULL, s=NULL, oc=NULL) == 0 and untouched(o_rgb, o_bg)
    assert si(g=NULL, gdt=9, gs=NULL, og=NULL) == 0 and not untouched(o_rgb) and untouched(o_bg)   # no background: its dtype and strides are not read
    assert si(cs=st(0, good[1], good[2])) == 0 and not untouched(o_bg)                              # a batch stride of 0 is legal

    # gmpi_light_shade_images_backward_launch(rgb, dtype, stride, background, dtype, stride, shading, g_rgb_out, g_bg_out, g_rgb, g_bg, g_shading, B, H, W, stream)
    def sib(c=p(rgb), cdt=0, cs=st(*good), g=p(bg), gdt=0, gs=st(*good), s=p(shading), goc=p(go_rgb), gog=p(go_bg), gc=p(gr_rgb), gg=p(gr_bg), gsh=p(gr_s),
            b=Bn, h=H, w=W):
        return lib.gmpi_light_shade_images_backward_launch(c, cdt, cs, g, gdt, gs, s, goc, gog, gc, gg, gsh, b, h, w, None)
    assert sib(c=NULL) == E_NULL and sib(cs=NULL) == E_NULL and sib(gs=NULL) == E_NULL and sib(s=NULL) == E_NULL
    assert sib(gc=NULL, gg=NULL, gsh=NULL) == E_NULL                        # nothing to write
    assert sib(g=NULL) == E_NULL and sib(g=NULL, gog=NULL) == E_NULL       # a background gradient, in or out, without a background
    assert sib(h=0) == E_SHAPE and sib(w=0) == E_SHAPE and sib(b=-1) == E_SHAPE and sib(h=65536) == E_SHAPE
    assert sib(cdt=3) == E_DTYPE and sib(gdt=-1) == E_DTYPE
    assert sib(cs=st(good[0], good[1], W - 1)) == E_STRIDE and sib(gs=st(good[0], -good[1], good[2])) == E_STRIDE
    assert sib(b=0) == 0 and untouched(gr_rgb, gr_bg, gr_s)
    assert sib(g=NULL, gog=NULL, gg=NULL) == 0 and not untouched(gr_rgb) and not untouched(gr_s) and untouched(gr_bg)
    assert sib(goc=NULL, gog=NULL, gc=NULL, gsh=NULL) == 0 and not untouched(gr_bg)
