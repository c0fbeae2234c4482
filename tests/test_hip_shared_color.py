"""GPU tests of the shared-colour layout (one colour image per MPI, D alpha planes, optional background for the last plane).  The definition is
the render of `expand_shared_color(rgb, alpha, background)`: the forward is checked against `oracle.render` on that volume, the backward against
float64 autograd of the torch reference through `expand_shared_color` on the CPU.  Run on the MI355X box:  python -m pytest tests -m gpu"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import oracle
from _torch_ref import torch_light_render, torch_render
import _transmittance_ref
from _util import load_npz
from test_hip_parity import TOL, _random_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _parts(rgba, dtype=torch.float32):
    """(rgb, alpha, background) taken out of a white-noise volume, rounded to the storage dtype (the reference gets the rounded values)."""
    q = lambda t: t.contiguous().to(dtype)
    return q(rgba[:, 0, :3]), q(rgba[:, :, 3:]), q(rgba[:, -1, :3])


def _expand(rgb, alpha, bg):
    from ml_gmpi_amd import expand_shared_color
    return expand_shared_color(rgb.float(), alpha.float(), None if bg is None else bg.float())


def shared_render(rgb, alpha, bg, dhw, ray, eye, zd, *, ac=True, variant="auto", strict=False, views_per_mpi=1, view_to_mpi=None,
                  check_last=False, range_check="touched", out_pm1=False, alpha_as_view=False):
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    t = lambda a: None if a is None else a.to(dev)
    alpha_d = t(alpha)
    if alpha_as_view:   # the alpha planes as the strided view rgba[:, :, 3:] of an ordinary volume
        vol = torch.full((alpha.shape[0], alpha.shape[1], 4, *alpha.shape[-2:]), 0.5, dtype=alpha.dtype, device=dev)
        vol[:, :, 3:] = alpha_d
        alpha_d = vol[:, :, 3:]
        assert not alpha_d.is_contiguous()
    mpi = MPI(align_corners=ac, variant=variant, strict_order=strict, range_check=range_check, on_out_of_plane="raise")
    v2m = None if view_to_mpi is None else torch.as_tensor(np.asarray(view_to_mpi, dtype=np.int32)).to(dev)
    with torch.no_grad():
        out = mpi.render_views_shared(t(rgb), alpha_d, t(dhw), t(ray), t(eye), t(zd), background=t(bg), views_per_mpi=views_per_mpi,
                                      view_to_mpi=v2m, check_last_plane=check_last, want_transmittance=True, out_pm1=out_pm1)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _check_forward(rgb, alpha, bg, dhw, ray, eye, zd, ac, v2m=None, **kw):
    orc = oracle.render(_expand(rgb, alpha, bg).numpy(), dhw, ray, eye, zd, view_to_mpi=v2m, align_corners=ac, threads=True)
    for variant in ("auto", "gather"):
        strict = shared_render(rgb, alpha, bg, dhw, ray, eye, zd, ac=ac, variant=variant, strict=True, **kw)
        for k in ("color", "depth", "T"):
            assert np.array_equal(strict[k], orc[k]), (variant, k, np.abs(strict[k] - orc[k]).max())
        fast = shared_render(rgb, alpha, bg, dhw, ray, eye, zd, ac=ac, variant=variant, **kw)
        errs = {k: float(np.abs(fast[k] - orc[k]).max()) for k in ("color", "depth", "T")}
        print("default mode", variant, errs)
        assert errs["color"] <= 0.5 * TOL and errs["depth"] <= TOL and errs["T"] <= TOL, (variant, errs)   # [0,1] colour: half the [-1,1] bar
        assert int(fast["status"][0]) == 0


FWD_CASES = [
    dict(seed=1, B=2, D=8, S=96),
    dict(seed=4, B=3, D=7, S=100, T=77),                   # H, W no multiple of any tile, Ht, Wt != H, W
    dict(seed=2, B=2, D=12, S=112, T=128, extreme=True),   # tilted poses: rays leave the planes
    dict(seed=6, B=1, D=1, S=40),                          # one plane (with a background: the plane IS the background)
]


@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", FWD_CASES)
def test_forward_matches_the_oracle_on_the_expanded_volume(cfg, dtype, ac, with_bg):
    rgba, dhw, ray, eye, zd = _random_case(**cfg)
    rgb, alpha, bg = _parts(rgba, dtype)
    _check_forward(rgb, alpha, bg if with_bg else None, dhw, ray, eye, zd, ac)


@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("grouping", ["uniform", "ragged", "view_to_mpi"])
def test_forward_view_groupings_and_alpha_view(grouping, with_bg):
    rgba, dhw, ray, eye, zd = _random_case(seed=9, B=4, D=6, S=72, T=64)
    rgb, alpha, bg = _parts(rgba[:2])
    dhw = dhw[:2]
    kw, v2m = {"uniform": (dict(views_per_mpi=2), [0, 0, 1, 1]), "ragged": (dict(views_per_mpi=[1, 3]), [0, 1, 1, 1]),
               "view_to_mpi": (dict(view_to_mpi=[1, 0, 0, 1]), [1, 0, 0, 1])}[grouping]
    _check_forward(rgb, alpha, bg if with_bg else None, dhw, ray, eye, zd, True, v2m=v2m, alpha_as_view=True, **kw)


def test_forward_full_size_g_step_shape_on_oracle_windows():
    """1024^2 x 32 planes x 4 MPIs (the G-step shape), checked on 64 x 64 windows of the image the way tests/test_hip_properties.py does it."""
    from ml_gmpi_amd import make_renderer, expand_shared_color
    dev = torch.device(DEV)
    S, D, B = 1024, 32, 4
    r = make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise")
    r.set_cam(r.cam_fov, S, S)
    g = torch.Generator(device=dev).manual_seed(6)
    rgb = torch.rand((B, 3, S, S), device=dev, generator=g)
    alpha = torch.rand((B, D, 1, S, S), device=dev, generator=g)
    bg = torch.rand((B, 3, S, S), device=dev, generator=g)
    torch.manual_seed(6)
    cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    ray, eye, zd = torch.cat(cam[3]), torch.cat(cam[4]), torch.cat(cam[5])
    dhw = r._dhw_on_device().expand(B, -1, -1).contiguous()
    vol = expand_shared_color(rgb, alpha, bg).cpu().numpy()
    wins = [(0, 0), (S - 64, S - 64), (S // 2 - 32, S // 2 + 7), (13, S - 64)]
    outs = {}
    for strict in (True, False):
        r.mpi.strict_order = strict
        with torch.no_grad():
            outs[strict] = r.mpi.render_views_shared(rgb, alpha, dhw, ray, eye, zd, background=bg, want_transmittance=True, check_last_plane=True)
    for (y0, x0) in wins:
        win = ray[:, :, y0:y0 + 64, x0:x0 + 64].contiguous().cpu()
        orc = oracle.render(vol, dhw.cpu(), win, eye.cpu(), zd.cpu(), threads=True)
        for key, bar in (("color", 0.5 * TOL), ("depth", TOL), ("T", TOL)):
            got = outs[True][key][:, :, y0:y0 + 64, x0:x0 + 64].cpu().numpy()
            assert np.array_equal(got, orc[key]), (key, y0, x0, np.abs(got - orc[key]).max())
            dflt = outs[False][key][:, :, y0:y0 + 64, x0:x0 + 64].cpu().numpy()
            assert np.abs(dflt - orc[key]).max() <= bar, ("default mode", key, y0, x0, np.abs(dflt - orc[key]).max())


@pytest.mark.parametrize("where", ["rgb", "background", "alpha"])
def test_out_of_range_value_sets_the_range_bit(where):
    from ml_gmpi_amd import MPI
    rgba, dhw, ray, eye, zd = _random_case(seed=3, B=1, D=5, S=64)
    rgb, alpha, bg = _parts(rgba)
    clean = shared_render(rgb, alpha, bg, dhw, ray, eye, zd, range_check="touched")
    assert int(clean["status"][0]) == 0
    {"rgb": rgb, "background": bg, "alpha": alpha}[where].view(-1, 64, 64)[0, 32, 32] = 1.5   # the image centre: every frontal view samples it
    dev = torch.device(DEV)
    for variant in ("auto", "gather"):
        mpi = MPI(variant=variant, on_out_of_plane="raise")
        with torch.no_grad():
            out = mpi.render_views_shared(rgb.to(dev), alpha.to(dev), dhw.to(dev), ray.to(dev), eye.to(dev), zd.to(dev), background=bg.to(dev),
                                          defer_status=True)
        assert int(out["status"][0].item()) & 2, (where, variant)
        with pytest.raises(AssertionError):
            mpi.render_views_shared(rgb.to(dev), alpha.to(dev), dhw.to(dev), ray.to(dev), eye.to(dev), zd.to(dev), background=bg.to(dev))
        full = MPI(variant=variant, range_check="full", on_out_of_plane="raise")
        with pytest.raises(AssertionError):
            full.render_views_shared(rgb.to(dev), alpha.to(dev), dhw.to(dev), ray.to(dev), eye.to(dev), zd.to(dev), background=bg.to(dev))
    # without a background the background tensor is not there to be tested; the value in rgb / alpha still is
    if where != "background":
        out = None
        with pytest.raises(AssertionError):
            out = shared_render(rgb, alpha, None, dhw, ray, eye, zd)
        assert out is None


def test_check_last_plane_sets_bit_one_on_the_pose_that_sets_it_today():
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    rgba, dhw, ray, eye, zd = _random_case(seed=2, B=2, D=6, S=64, extreme=True)
    dhw = dhw.clone()
    dhw[:, -1, 1:] *= 0.5   # a last plane the tilted rays leave
    rgb, alpha, bg = _parts(rgba)
    t = lambda a: a.to(dev)
    mpi = MPI(on_out_of_plane="raise")
    with torch.no_grad():
        today = mpi.render_views(t(_expand(rgb, alpha, bg)), t(dhw), t(ray), t(eye), t(zd), check_last_plane=True, defer_status=True)
        shared = mpi.render_views_shared(t(rgb), t(alpha), t(dhw), t(ray), t(eye), t(zd), background=t(bg), check_last_plane=True, defer_status=True)
        off = mpi.render_views_shared(t(rgb), t(alpha), t(dhw), t(ray), t(eye), t(zd), background=t(bg), check_last_plane=False, defer_status=True)
    assert int(today["status"][0].item()) & 1
    assert int(shared["status"][0].item()) == int(today["status"][0].item())
    assert int(off["status"][0].item()) == 0
    with pytest.raises(RuntimeError):
        mpi.render_views_shared(t(rgb), t(alpha), t(dhw), t(ray), t(eye), t(zd), background=t(bg), check_last_plane=True)


# ---- backward ---------------------------------------------------------------------------------------------------------------------------------
def _reference_grads(parts, dhw, ray, eye, zd, v2m, gc, gd, gT, out_pm1, dtype):
    """d(sum gC colour + sum gZ depth + sum gT T) / d(rgb, alpha, background) of the torch reference through expand_shared_color, in `dtype`.
    Colour and depth: tests/_torch_ref.torch_render (grid_sample).  It has no transmittance output; when gT is given the chain is
    tests/_transmittance_ref.render, this project's float64 reference of the transmittance gradient (same composite, explicit bilinear taps)."""
    from ml_gmpi_amd import expand_shared_color
    ins = [None if p is None else p.to(dtype).clone().requires_grad_(True) for p in parts]
    vol = expand_shared_color(*ins)
    c = lambda a: torch.as_tensor(a).to(dtype)
    if gT is None:
        color, depth = torch_render(vol, c(dhw), c(ray), c(eye), c(zd), v2m)
        T = None
    else:
        color, depth, T = _transmittance_ref.render(vol, c(dhw), c(ray), c(eye), c(zd), v2m)
    if out_pm1:
        color = 2 * color - 1
    loss = torch.zeros((), dtype=dtype)
    for out, g in ((color, gc), (depth, gd), (T, gT)):
        if g is not None:
            loss = loss + (out * c(g)).sum()
    loss.backward()
    return [None if i is None else (i.grad if i.grad is not None else torch.zeros_like(i)).double().numpy() for i in ins]


def _hip_grads(parts, dhw, ray, eye, zd, vpm, gc, gd, gT, out_pm1, variant, needs=(True, True, True)):
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    ins = [None if p is None else p.to(dev).clone().requires_grad_(n) for p, n in zip(parts, needs)]
    mpi = MPI(variant=variant, on_out_of_plane="raise")
    t = lambda a: torch.as_tensor(a).to(dev)
    out = mpi.render_views_shared(ins[0], ins[1], t(dhw), t(ray), t(eye), t(zd), background=ins[2], views_per_mpi=vpm, check_last_plane=False,
                                  out_pm1=out_pm1, want_transmittance=True)
    loss = 0
    for key, g in (("color", gc), ("depth", gd), ("T", gT)):
        if g is not None:
            loss = loss + (out[key] * t(g)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return ins, out


def _bwd_case(D, S, with_bg, dtype, seed=5):
    rgba, dhw, ray, eye, zd = _random_case(seed=seed, B=4, D=D, S=S)
    rgb, alpha, bg = _parts(rgba[:2], dtype)
    if with_bg:
        # white-noise alphas hide the last plane behind D - 1 others (max |g background| ~ 1e-5 at D = 32, where the absolute term of the
        # bound would hide any error): thin the planes out
        alpha = (alpha.float() * 0.1).to(dtype)
    g = np.random.default_rng(7)
    N = 4
    gc = g.standard_normal((N, 3, S, S)).astype(np.float32)
    gd = g.standard_normal((N, 1, S, S)).astype(np.float32)
    gT = g.standard_normal((N, 1, S, S)).astype(np.float32)
    return (rgb, alpha, bg if with_bg else None), dhw[:2], ray, eye, zd, [0, 0, 1, 1], gc, gd, gT


_SIG_BITS = {torch.bfloat16: 8, torch.float16: 11}   # significant bits of the 16-bit storage formats


def _half_ulp(x, dtype):
    """Half a unit in the last place of every element of x in `dtype` (0 for fp32: the gradient is not rounded again).  For |x| in [2^e, 2^(e+1))
    the spacing of a format with p significant bits is 2^(e+1-p), half of it 2^(e-p): between 2^-(p+1) |x| and 2^-p |x|, i.e. for bf16 (p = 8)
    between 2^-9 |x| (top of a binade) and 2^-8 |x| (bottom), for fp16 (p = 11) between 2^-12 |x| and 2^-11 |x|."""
    if dtype not in _SIG_BITS:
        return np.zeros_like(x)
    _, e = np.frexp(np.abs(x))          # |x| = m 2^e, m in [0.5, 1)  ->  |x| in [2^(e-1), 2^e)
    return np.where(x == 0, 0.0, np.ldexp(1.0, e - 1 - _SIG_BITS[dtype]))
_NAMES = ("rgb", "alpha", "background")


def _compare(got, ref64, ref32, dtype, label, colour_reaches, with_bg):
    """The kernel may deviate by max(5e-5, 4 e_ref) max|g_ref| + 1e-6 per gradient tensor, e_ref = the largest deviation of the SAME op chain in
    fp32 on the CPU from float64, relative to max|g_ref| (the factor 4: another summation order; the shared image sums D times as many terms as the
    cells the project's 5e-5 bar was set for).  16-bit inputs: the gradient comes back in the input's dtype, one more rounding per element: half an
    ulp of the element on top -- the exact half ulp of the format (`_half_ulp`), which reaches 2^-8 |x| for bf16 and 2^-11 |x| for fp16 at the bottom
    of a binade: a flat relative 2^-9 / 2^-12 is half an ulp only at the top of one, and a correctly rounded result misses it."""
    failures = []
    if with_bg and colour_reaches:   # the comparison of the background gradient must mean something
        ratio = np.abs(ref64[2]).max() / np.abs(ref64[0]).max()
        print(label, "max|g_ref background| / max|g_ref rgb| =", ratio)
        assert ratio >= 1e-2, ratio
    for name, g, r64, r32 in zip(_NAMES, got, ref64, ref32):
        if r64 is None:
            continue
        scale = float(np.abs(r64).max())
        e_ref = float(np.abs(r32 - r64).max()) / scale if scale > 0 else 0.0
        bound = max(5e-5, 4 * e_ref) * scale + 1e-6 + _half_ulp(np.maximum(np.abs(g), np.abs(r64)), dtype)   # (the rounding acted on the kernel's value)
        err = np.abs(g - r64)
        worst = float((err - bound).max())
        print(f"{label} {name}: max|g_ref| {scale:.3e} e_ref {e_ref:.2e} max err {float(err.max()):.3e} ({float(err.max()) / max(scale, 1e-30):.2e} rel) margin {worst:.2e}")
        if worst > 0:
            failures.append((name, float(err.max()), scale, e_ref))
    assert not failures, (label, failures)


COMBOS = [c for c in itertools.product([True, False], repeat=3) if any(c)]   # (g_color, g_depth, g_T): every combination that reaches an output


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "".join(n for n, on in zip("CZT", c) if on))
@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_matches_float64_autograd_through_expand(dtype, with_bg, combo):
    parts, dhw, ray, eye, zd, v2m, gc, gd, gT = _bwd_case(8, 64, with_bg, dtype)
    gc, gd, gT = (g if on else None for g, on in zip((gc, gd, gT), combo))
    for out_pm1 in ((False, True) if combo[0] else (False,)):
        ref64 = _reference_grads(parts, dhw, ray, eye, zd, v2m, gc, gd, gT, out_pm1, torch.float64)
        ref32 = _reference_grads(parts, dhw, ray, eye, zd, v2m, gc, gd, gT, out_pm1, torch.float32)
        for variant in ("auto", "gather"):
            ins, _ = _hip_grads(parts, dhw, ray, eye, zd, 2, gc, gd, gT, out_pm1, variant)
            for i in ins:
                assert i is None or (i.grad is not None and i.grad.dtype == dtype and i.grad.shape == i.shape)
            got = [None if i is None else i.grad.double().cpu().numpy() for i in ins]
            _compare(got, ref64, ref32, dtype, f"{variant} pm1={out_pm1}", combo[0], with_bg)


@pytest.mark.parametrize("with_bg", [False, True])
def test_backward_32_planes_96_pixels(with_bg):
    """D = 32 (the training depth), 96 x 96: three tile rows and columns, the colour window collects 32 planes."""
    parts, dhw, ray, eye, zd, v2m, gc, gd, gT = _bwd_case(32, 96, with_bg, torch.float32)
    ref64 = _reference_grads(parts, dhw, ray, eye, zd, v2m, gc, gd, gT, True, torch.float64)
    ref32 = _reference_grads(parts, dhw, ray, eye, zd, v2m, gc, gd, gT, True, torch.float32)
    for variant in ("auto", "gather"):
        ins, _ = _hip_grads(parts, dhw, ray, eye, zd, 2, gc, gd, gT, True, variant)
        got = [None if i is None else i.grad.double().cpu().numpy() for i in ins]
        _compare(got, ref64, ref32, torch.float32, f"D=32 {variant}", True, with_bg)


def test_backward_tilted_poses_move_the_colour_window():
    """The 2-sigma corner of the pose range at 256^2: the tile's texel boxes drift over the planes (the colour window is re-anchored) and leave
    the texture; the tile kernel against the one-pixel-per-lane kernel and against float64."""
    rgba, dhw, ray, eye, zd = _random_case(seed=8, B=2, D=16, S=256, extreme=True)
    parts = _parts(rgba)
    parts = (parts[0], (parts[1] * 0.2), parts[2])
    g = np.random.default_rng(1)
    gc = g.standard_normal((2, 3, 256, 256)).astype(np.float32)
    gd = g.standard_normal((2, 1, 256, 256)).astype(np.float32)
    ref64 = _reference_grads(parts, dhw, ray, eye, zd, [0, 1], gc, gd, None, False, torch.float64)
    ref32 = _reference_grads(parts, dhw, ray, eye, zd, [0, 1], gc, gd, None, False, torch.float32)
    for variant in ("auto", "gather"):
        ins, _ = _hip_grads(parts, dhw, ray, eye, zd, 1, gc, gd, None, False, variant)
        got = [i.grad.double().cpu().numpy() for i in ins]
        _compare(got, ref64, ref32, torch.float32, f"tilted {variant}", True, True)


def _staged_tile_planes(dhw, ray, eye, T):
    """(staged, all) (tile, plane) pairs of render_shared_tile_kernel for these views, replayed on the CPU: tools/shared_window_replay.py's boxes() with its
    default box limit, the kernel's 56 x 27."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("shared_window_replay", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                                                                       "shared_window_replay.py"))
    replay = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(replay)
    assert (replay.AP, replay.AR) == (56, 27)
    bb = replay.boxes(dhw[0].numpy(), ray.numpy(), eye.numpy(), T)
    return int((bb[..., 2] > 0).sum()), int(bb[..., 2].size)


def test_backward_minification_every_tile_scatters_straight_to_global_memory():
    """64 x 64 pixels over 256 x 256 texels: a 32 x 16 pixel tile covers 63 .. 128 x 37 .. 65 texels on every plane, more than the 56 x 27 box the
    tile kernel stages, so the whole launch takes the direct scatter of both gradients.  Replayed on the CPU (tools/shared_window_replay.py, boxes(),
    --box 56x27): 0 of the 96 (tile, plane) pairs -- 2 views x 8 tiles x 6 planes -- are staged; asserted below."""
    S, T, D = 64, 256, 6
    rgba, dhw, ray, eye, zd = _random_case(seed=11, B=2, D=D, S=S, T=T)
    assert _staged_tile_planes(dhw, ray, eye, T) == (0, 96)
    parts = _parts(rgba)
    parts = (parts[0], (parts[1] * 0.2), parts[2])
    g = np.random.default_rng(3)
    gc = g.standard_normal((2, 3, S, S)).astype(np.float32)
    gd = g.standard_normal((2, 1, S, S)).astype(np.float32)
    ref64 = _reference_grads(parts, dhw, ray, eye, zd, [0, 1], gc, gd, None, False, torch.float64)
    ref32 = _reference_grads(parts, dhw, ray, eye, zd, [0, 1], gc, gd, None, False, torch.float32)
    for variant in ("auto", "gather"):
        ins, _ = _hip_grads(parts, dhw, ray, eye, zd, 1, gc, gd, None, False, variant)
        got = [i.grad.double().cpu().numpy() for i in ins]
        _compare(got, ref64, ref32, torch.float32, f"minification {variant}", True, True)


def test_backward_ragged_sizes_100_pixels_over_77_texels():
    """100 x 100 pixels (4 x 7 tiles, the last column 4 pixels wide, the last row 4 pixels high) over 77 x 77 texels, 7 planes, three MPIs with a
    background: lanes outside the image, tiles clamped at both image borders, a texture that is no multiple of anything."""
    S, T, D, B = 100, 77, 7, 3
    rgba, dhw, ray, eye, zd = _random_case(seed=4, B=B, D=D, S=S, T=T)
    parts = _parts(rgba)
    g = np.random.default_rng(4)
    gc = g.standard_normal((B, 3, S, S)).astype(np.float32)
    gd = g.standard_normal((B, 1, S, S)).astype(np.float32)
    gT = g.standard_normal((B, 1, S, S)).astype(np.float32)
    ref64 = _reference_grads(parts, dhw, ray, eye, zd, [0, 1, 2], gc, gd, gT, True, torch.float64)
    ref32 = _reference_grads(parts, dhw, ray, eye, zd, [0, 1, 2], gc, gd, gT, True, torch.float32)
    for variant in ("auto", "gather"):
        ins, _ = _hip_grads(parts, dhw, ray, eye, zd, 1, gc, gd, gT, True, variant)
        got = [i.grad.double().cpu().numpy() for i in ins]
        _compare(got, ref64, ref32, torch.float32, f"ragged {variant}", True, True)


def test_backward_rgb_grad_excludes_the_background_plane_and_partial_needs():
    from ml_gmpi_amd import MPI
    parts, dhw, ray, eye, zd, v2m, gc, gd, gT = _bwd_case(8, 64, True, torch.float32)
    dev = torch.device(DEV)
    t = lambda a: torch.as_tensor(a).to(dev)
    # the volume backward of the parent commit on the expanded volume: rgb.grad is the sum over planes 0 .. D-2 only
    vol = _expand(*parts).to(dev).requires_grad_(True)
    mpi = MPI(on_out_of_plane="raise")
    out = mpi.render_views(vol, t(dhw), t(ray), t(eye), t(zd), views_per_mpi=2, check_last_plane=False)
    ((out["color"] * t(gc)).sum() + (out["depth"] * t(gd)).sum()).backward()
    gv = vol.grad.double().cpu().numpy()
    full, _ = _hip_grads(parts, dhw, ray, eye, zd, 2, gc, gd, None, False, "auto")
    D = parts[1].shape[1]
    scale = np.abs(gv).max()
    assert np.abs(full[0].grad.double().cpu().numpy() - gv[:, :D - 1, :3].sum(1)).max() <= 5e-5 * np.abs(gv[:, :D - 1, :3].sum(1)).max() + 1e-6
    assert np.abs(full[2].grad.double().cpu().numpy() - gv[:, D - 1, :3]).max() <= 5e-5 * scale + 1e-6
    assert np.abs(full[1].grad.double().cpu().numpy() - gv[:, :, 3:]).max() <= 5e-5 * scale + 1e-6
    assert np.abs(full[0].grad.double().cpu().numpy() - gv[:, :, :3].sum(1)).max() > 1e-3 * scale   # (the last plane's share is not small here)
    # only some of the inputs require grad: the others get none, the wanted ones the same values (up to the order of the atomic adds)
    for needs in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        for variant in ("auto", "gather"):
            ins, _ = _hip_grads(parts, dhw, ray, eye, zd, 2, gc, gd, None, False, variant, needs=needs)
            for i, f, n in zip(ins, full, needs):
                if not n:
                    assert i.grad is None
                else:
                    ref = f.grad.double().cpu().numpy()
                    assert np.abs(i.grad.double().cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-7, (needs, variant)


def test_unused_transmittance_stays_on_the_path_without_g_T(monkeypatch):
    """A T output nobody uses arrives as None in the backward: the launch gets NULL for grad_transmittance (seen at the C entry itself), the result
    is the one of g_T = None -- and a T that is used with a zero gradient gives the same values through the other path, which does get a pointer."""
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    real = lib.gmpi_mpi_render_shared_backward_launch
    seen = []

    def spy(*args):
        seen.append(args[4])   # grad_transmittance
        return real(*args)
    monkeypatch.setattr(lib, "gmpi_mpi_render_shared_backward_launch", spy)
    parts, dhw, ray, eye, zd, v2m, gc, gd, gT = _bwd_case(8, 64, False, torch.float32)
    a, out = _hip_grads(parts, dhw, ray, eye, zd, 2, gc, gd, None, False, "gather")
    assert out["T"] is not None
    assert seen == [None], seen
    b, _ = _hip_grads(parts, dhw, ray, eye, zd, 2, gc, gd, np.zeros_like(gT), False, "gather")
    assert len(seen) == 2 and seen[1] is not None and int(seen[1]) != 0, seen
    for x, y in zip(a[:2], b[:2]):
        gx, gy = x.grad.double().cpu().numpy(), y.grad.double().cpu().numpy()
        assert np.abs(gx - gy).max() <= 1e-5 * np.abs(gx).max() + 1e-7


def test_backward_129_planes_takes_the_one_pixel_per_lane_kernel_through_auto():
    """D = 129 is one plane more than the tile backward's tables hold: variant "auto" then runs the one-pixel-per-lane kernel.  Same bound as the
    other backward cases, and the two variants agree up to the order of the atomic adds."""
    rgba, dhw, ray, eye, zd = _random_case(seed=13, B=2, D=129, S=48)
    parts = _parts(rgba)
    parts[1][:, :-1] *= 0.01   # (128 thin planes in front of an ordinary last one: the background still receives a gradient worth comparing)
    g = np.random.default_rng(2)
    gc = g.standard_normal((2, 3, 48, 48)).astype(np.float32)
    gd = g.standard_normal((2, 1, 48, 48)).astype(np.float32)
    gT = g.standard_normal((2, 1, 48, 48)).astype(np.float32)
    ref64 = _reference_grads(parts, dhw, ray, eye, zd, [0, 1], gc, gd, gT, False, torch.float64)
    ref32 = _reference_grads(parts, dhw, ray, eye, zd, [0, 1], gc, gd, gT, False, torch.float32)
    got = {}
    for variant in ("auto", "gather"):
        ins, _ = _hip_grads(parts, dhw, ray, eye, zd, 1, gc, gd, gT, False, variant)
        got[variant] = [i.grad.double().cpu().numpy() for i in ins]
        _compare(got[variant], ref64, ref32, torch.float32, f"D=129 {variant}", True, True)
    for x, y in zip(got["auto"], got["gather"]):
        assert np.abs(x - y).max() <= 1e-5 * np.abs(y).max() + 1e-7


def test_mixed_storage_dtypes_are_refused():
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    rgba, dhw, ray, eye, zd = _random_case(seed=3, B=1, D=3, S=32)
    rgb, alpha, bg = (t.to(dev) for t in _parts(rgba))
    t = lambda a: a.to(dev)
    mpi = MPI(on_out_of_plane="raise")
    with pytest.raises(TypeError):
        mpi.render_views_shared(rgb, alpha.to(torch.bfloat16), t(dhw), t(ray), t(eye), t(zd))
    with pytest.raises(TypeError):
        mpi.render_views_shared(rgb, alpha, t(dhw), t(ray), t(eye), t(zd), background=bg.to(torch.float16))


def test_geometry_grad_raises_for_the_shared_layout():
    from ml_gmpi_amd import make_renderer, rays_from_c2w
    dev = torch.device(DEV)
    S, D = 64, 4
    r = make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise", geometry_grad=True)
    r.set_cam(r.cam_fov, S, S)
    torch.manual_seed(0)
    cam = r.sample_cam_poses(1, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    c2w = cam[2].to(dev).clone().requires_grad_(True)
    ray, eye, zd = rays_from_c2w(r, c2w)
    rgb, alpha = torch.rand((1, 3, S, S), device=dev), torch.rand((1, D, 1, S, S), device=dev)
    with pytest.raises(NotImplementedError):
        r.mpi.render_views_shared(rgb, alpha, r._dhw_for(1), ray, eye, zd)
    from ml_gmpi_amd import MPI
    out = MPI(backward="gather").render_views_shared(rgb.requires_grad_(True), alpha, r._dhw_for(1), ray.detach(), eye.detach(), zd.detach())
    out["color"].sum().backward()   # backward="gather" takes the atomic shared path
    assert rgb.grad is not None and float(rgb.grad.abs().max()) > 0


# ---- C ABI argument errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_error_codes():
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    dev = torch.device(DEV)
    rgba, dhw, ray, eye, zd = _random_case(seed=3, B=1, D=3, S=32)
    rgb, alpha, bg = (t.to(dev) for t in _parts(rgba))
    dhw, ray, eye, zd = (t.to(dev).float().contiguous() for t in (dhw, ray, eye, zd))
    color, depth = torch.empty((1, 3, 32, 32), device=dev), torch.empty((1, 1, 32, 32), device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)

    def params():
        p = L.GmpiRenderParams()
        p.struct_size = ctypes.sizeof(L.GmpiRenderParams)
        p.flags, p.variant, p.rgba_dtype = L.FLAG_ALIGN_CORNERS, L.VARIANT_AUTO, L.DTYPE_F32
        p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = 1, 1, 3, 32, 32, 32, 32, 1
        p.rgba = alpha.data_ptr()
        for i, s in enumerate(alpha.stride()):
            p.rgba_stride[i] = s
        p.rgba_stride[2] = 0   # ignored
        p.dhw, p.ray_dir, p.eye_pos, p.z_dir = dhw.data_ptr(), ray.data_ptr(), eye.data_ptr(), zd.data_ptr()
        p.rgb_out, p.depth_out, p.status = color.data_ptr(), depth.data_ptr(), status.data_ptr()
        return p

    def shared(with_bg=True):
        s = L.GmpiSharedColor()
        s.struct_size = ctypes.sizeof(L.GmpiSharedColor)
        s.rgb = rgb.data_ptr()
        for i in range(3):
            s.rgb_stride[i] = rgb.stride(i)
            s.background_stride[i] = bg.stride(i)
        s.background = bg.data_ptr() if with_bg else None
        return s

    fwd = lambda p, s: lib.gmpi_mpi_render_shared_launch(ctypes.byref(p) if p is not None else None, ctypes.byref(s) if s is not None else None, None)
    assert fwd(params(), shared()) == 0
    assert fwd(None, shared()) == -1 and fwd(params(), None) == -1                       # GMPI_E_NULL
    s = shared(); s.rgb = None
    assert fwd(params(), s) == -1
    p = params(); p.rgb_out = None
    assert fwd(p, shared()) == -1
    p = params(); p.D = 0
    assert fwd(p, shared()) == -2                                                        # GMPI_E_SHAPE
    p = params(); p.rgba_dtype = 7
    assert fwd(p, shared()) == -3                                                        # GMPI_E_DTYPE
    p = params(); p.rgba_stride[4] = 2
    assert fwd(p, shared()) == -4                                                        # GMPI_E_STRIDE
    s = shared(); s.rgb_stride[2] = 8
    assert fwd(params(), s) == -4
    s = shared(); s.background_stride[1] = -1
    assert fwd(params(), s) == -4
    p = params(); p.struct_size -= 8
    assert fwd(p, shared()) == -5                                                        # GMPI_E_ABI
    s = shared(); s.struct_size += 8
    assert fwd(params(), s) == -5
    p = params(); p.flags |= 1 << 30
    assert fwd(p, shared()) == -7                                                        # GMPI_E_FLAGS
    p = params(); p.variant = L.VARIANT_BAND
    assert fwd(p, shared()) == -6                                                        # GMPI_E_VARIANT
    # D == 1 with a background is legal
    p = params(); p.D = 1
    assert fwd(p, shared()) == 0
    # backward
    g_out = torch.zeros((1, 3, 32, 32), device=dev)
    g_rgb, g_alpha, g_bg = torch.zeros_like(rgb), torch.zeros_like(alpha), torch.zeros_like(bg)
    s3 = lambda t, dims: (ctypes.c_int64 * 3)(*[t.stride(d) for d in dims])

    def bwd(p, s, go=g_out.data_ptr(), gr=g_rgb.data_ptr(), ga=g_alpha.data_ptr(), gb=g_bg.data_ptr(), grs=None):
        return lib.gmpi_mpi_render_shared_backward_launch(ctypes.byref(p), ctypes.byref(s), go, None, None, gr, grs or s3(g_rgb, (0, 1, 2)), ga,
                                                          s3(g_alpha, (0, 1, 3)), gb, s3(g_bg, (0, 1, 2)), None)
    p = params(); p.rgb_out = p.depth_out = None
    assert bwd(p, shared()) == 0
    assert bwd(p, shared(), gr=None, gb=None) == 0 and bwd(p, shared(), ga=None) == 0    # any of the three may be NULL
    assert bwd(p, shared(), go=None) == -1
    assert bwd(p, shared(), gr=None, ga=None, gb=None) == -1
    assert bwd(p, shared(with_bg=False)) == -1                                           # a background gradient without a background
    assert bwd(p, shared(with_bg=False), gb=None) == 0
    assert bwd(p, shared(), grs=(ctypes.c_int64 * 3)(3 * 32 * 32, 32 * 32, 8)) == -4
    torch.cuda.synchronize()
    assert int(status[0].item()) == 0


# ---- host layer ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bg", [False, True])
def test_renderer_render_shared_matches_render_and_consumes_the_same_rng(with_bg):
    from ml_gmpi_amd import make_renderer
    dev = torch.device(DEV)
    S, D, B = 128, 8, 2
    rgba, _, _, _, _ = _random_case(seed=12, B=B, D=D, S=S)
    rgb, alpha, bg = (t.to(dev) for t in _parts(rgba))
    bg = bg if with_bg else None
    vol = _expand(rgb, alpha, bg)
    res, states = [], []
    for shared in (False, True):
        r = make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise", range_check="full")
        torch.manual_seed(21)
        with torch.no_grad():
            for _ in range(3):   # (a repeated request: the look-ahead pose queue is in use)
                out = r.render_shared(rgb, alpha, S, S, background_rgb=bg, want_transmittance=True) if shared else r.render(vol, S, S, want_transmittance=True)
        torch.cuda.synchronize()
        res.append(out)
        states.append(torch.get_rng_state())
    assert torch.equal(states[0], states[1])
    a, b = res
    assert len(a) == len(b) == 5
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])           # c2w, angles
    assert float((a[0] - b[0]).abs().max()) <= TOL and float((a[1] - b[1]).abs().max()) <= TOL and float((a[4] - b[4]).abs().max()) <= TOL


def test_light_renderer_render_shared_matches_the_reference_on_the_expanded_volume():
    import ml_gmpi_amd
    from ml_gmpi_amd import expand_shared_color, poses
    fx = load_npz("light_render.npz")
    dev = torch.device(DEV)
    base = torch.from_numpy(fx["rgba"])
    rgb0, alpha0, bg0 = base[:, 0, :3].contiguous(), base[:, :, 3:].contiguous(), base[:, -1, :3].contiguous()
    dhw, xyz = torch.from_numpy(fx["dhw"]), torch.from_numpy(fx["xyz"])
    g = np.random.default_rng(3)
    g_rgb, g_bg = (torch.from_numpy(g.standard_normal(rgb0.shape).astype(np.float32)) for _ in range(2))
    g_alpha = torch.from_numpy(g.standard_normal(alpha0.shape).astype(np.float32))
    for with_bg in (False, True):
        L = ml_gmpi_amd.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, ka_max=1.3, kd_max=0.9, n_grow_iters=1)
        L2 = ml_gmpi_amd.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, ka_max=1.3, kd_max=0.9, n_grow_iters=1)
        L.step = L2.step = 4
        ins = [t.to(dev).requires_grad_(True) for t in (rgb0, alpha0, bg0)]
        torch.manual_seed(11)
        o_rgb, o_alpha, o_bg = L.render_shared(ins[0], ins[1], dhw, xyz.to(dev), background=ins[2] if with_bg else None)
        state = torch.get_rng_state()
        torch.manual_seed(11)
        with torch.no_grad():
            L2.render(expand_shared_color(rgb0, alpha0, bg0 if with_bg else None).to(dev), dhw, xyz.to(dev))
        assert torch.equal(state, torch.get_rng_state())
        assert (L.step, L.cur_ka, L.cur_kd) == (L2.step, L2.cur_ka, L2.cur_kd) == (5, 1.3, 0.9)
        assert (o_bg is None) == (not with_bg) and o_alpha is ins[1]
        loss = (o_rgb * g_rgb.to(dev)).sum() + (o_alpha * g_alpha.to(dev)).sum() + ((o_bg * g_bg.to(dev)).sum() if with_bg else 0)
        loss.backward()
        # reference: same light (same RNG draw), float64, on the expanded volume
        torch.manual_seed(11)
        c2w, _, _ = poses.gen_sphere_path(n_cams=2, sphere_center=L.sphere_center, sphere_r=1.0, yaw_mean=L.l_h_mean, yaw_std=L.l_h_std,
                                          pitch_mean=L.l_v_mean, pitch_std=L.l_v_std, n_truncated_stds=2, flag_rnd=True,
                                          sample_method="truncated_gaussian")
        ld = poses._unit(L.sphere_center.reshape(1, 3) - torch.FloatTensor(c2w[:, :3, 3])).double()
        rin = [t.double().requires_grad_(True) for t in (rgb0, alpha0, bg0)]
        ref = torch_light_render(expand_shared_color(rin[0], rin[1], rin[2] if with_bg else None), dhw[:, 0].double(), xyz[-1].double(), ld,
                                 L.cur_ka, L.cur_kd, L._k1d.double())
        r_rgb, r_alpha, r_bg = ref[:, 0, :3], ref[:, :, 3:], ref[:, -1, :3]
        rloss = (r_rgb * g_rgb.double()).sum() + (r_alpha * g_alpha.double()).sum() + ((r_bg * g_bg.double()).sum() if with_bg else 0)
        rloss.backward()
        errs = dict(rgb=float((o_rgb.detach().cpu().double() - r_rgb.detach()).abs().max()))
        if with_bg:
            errs["bg"] = float((o_bg.detach().cpu().double() - r_bg.detach()).abs().max())
        gerr = {n: (float((i.grad.cpu().double() - r.grad).abs().max()), float(r.grad.abs().max()))
                for n, i, r in zip(_NAMES, ins, rin) if r.grad is not None and i.grad is not None}
        print("light render_shared: forward errors", errs, "gradient (max err, max|ref|)", gerr)
        assert all(e <= 1e-5 for e in errs.values()), errs
        for n, (e, s) in gerr.items():
            assert e <= 1e-5 * max(s, 1.0), (n, e, s)
