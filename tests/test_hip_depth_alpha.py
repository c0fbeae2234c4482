"""GPU tests of the depth-alpha layout (one colour image and one depth image per MPI, optional background for the last plane; the alpha of a
plane is a ramp of plane_z - depth).  The definition is the render of `expand_depth_alpha(rgb.float(), depth.float(), ...)`: the forward is checked
against `oracle.render` on that volume (strict order: bit for bit), the backward against float64 autograd of the torch reference through
`expand_depth_alpha` on the CPU.  Run on the MI355X box:  python -m pytest tests -m gpu"""
import functools

import numpy as np
import pytest
import torch

import oracle
from _torch_ref import torch_render
import _transmittance_ref
from test_hip_parity import TOL, _random_case
from test_hip_shared_color import COMBOS, DTYPES, _compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_REF_CAP = 2e-4   # the fp32 torch chain against float64, relative to max|g_ref|: a case beyond it gets other inputs, not another cap


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def _bounds(n_z_bins):
    from ml_gmpi_amd import depth_alpha_bounds
    return depth_alpha_bounds(1, n_z_bins)


def _knife_edges(depth, plane_z, lo, hi, margin):
    """Texels with some plane_z[k] - depth within `margin` of either bound of the ramp (in the fp32 arithmetic of the definition)."""
    from ml_gmpi_amd.depth_alpha import ramp_constants
    lo32, hi32, _ = ramp_constants(lo, hi)
    t = plane_z.reshape(1, -1, 1, 1) - depth.float()
    return (((t - lo32).abs() < margin) | ((t - hi32).abs() < margin)).any(1, keepdim=True)


def _depth_image(B, T, D, n_z_bins, dtype=torch.float32, reach=None, seed=11):
    """5 x 5 uniform noise, bilinearly upsampled (align_corners=True), scaled to 0.15 + 0.7 c, plus 0.02 (U - 0.5) per texel; `reach`: scaled so
    that its maximum is `reach` (holes: beyond the last plane's ramp).  Every texel within 1e-4 of a bound of some plane's ramp gets + 3.3e-4 until
    none is left: no gradient sits on the clamp's knife edge."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand((B, 1, 5, 5), generator=g)
    depth = 0.15 + 0.7 * torch.nn.functional.interpolate(c, size=(T, T), mode="bilinear", align_corners=True)
    depth = depth + 0.02 * (torch.rand((B, 1, T, T), generator=g) - 0.5)
    if reach is not None:
        depth = depth * (reach / float(depth.max()))
    plane_z = torch.linspace(0, 1, D)
    lo, hi = _bounds(n_z_bins)
    for _ in range(8):
        edge = _knife_edges(depth, plane_z, lo, hi, 1e-4)
        if not bool(edge.any()):
            break
        depth = depth + 3.3e-4 * edge
    assert not bool(_knife_edges(depth, plane_z, lo, hi, 1e-4).any())
    if dtype is not torch.float32:
        # 16-bit storage moves a texel by up to 2^-9 of its value and puts some on dyadic values that meet a bound exactly (0.25 below the plane at 0.5);
        # + 3.3e-4 is below its resolution.  What must hold for the stored values: no difference within a few fp32 ulps of a bound (the float64
        # reference and the fp32 kernel then agree on which side it lies).  Such texels move up by 2^-7 of their value (one to two bf16 steps).
        depth = depth.to(dtype)
        for _ in range(8):
            edge = _knife_edges(depth, plane_z, lo, hi, 1e-6)
            if not bool(edge.any()):
                break
            depth = torch.where(edge, (depth.float() * (1 + 2.0 ** -7)).to(dtype), depth)
        assert not bool(_knife_edges(depth, plane_z, lo, hi, 1e-6).any())
    return depth, plane_z


@functools.lru_cache(maxsize=None)
def _case(seed, B, D, S, n_z_bins, T=None, extreme=False, dtype=torch.float32, reach=None, M=None, depth_seed=11):
    """(rgb, depth, plane_z, background, dhw, ray, eye, zd, (z_lo, z_hi)): poses and colours of test_hip_parity._random_case (rgb = plane 0's colour,
    background = plane D-1's), the first M MPIs.  Cached: shared by the tests, never written to."""
    rgba, dhw, ray, eye, zd = _random_case(seed=seed, B=B, D=D, S=S, T=T, extreme=extreme)
    M = M or B
    q = lambda t: t[:M].contiguous().to(dtype)
    depth, plane_z = _depth_image(M, T or S, D, n_z_bins, dtype, reach, depth_seed)
    return q(rgba[:, 0, :3]), depth, plane_z, q(rgba[:, -1, :3]), dhw[:M].contiguous(), ray, eye, zd, _bounds(n_z_bins)


def _expand(rgb, depth, plane_z, bg, zb, dtype=torch.float32):
    from ml_gmpi_amd import expand_depth_alpha
    return expand_depth_alpha(rgb.to(dtype), depth.to(dtype), plane_z, zb[0], zb[1], None if bg is None else bg.to(dtype))


def depth_render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, *, ac=True, variant="auto", strict=False, views_per_mpi=1, view_to_mpi=None,
                 check_last=False, range_check="touched", out_pm1=False, depth_as_view=False, defer_status=False):
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    t = lambda a: None if a is None else a.to(dev)
    depth_d = t(depth)
    if depth_as_view:   # the depth image as the strided view rgbd[:, 3:] of an RGB-D tensor
        rgbd = torch.cat((t(rgb), depth_d), 1)
        depth_d = rgbd[:, 3:]
        assert not depth_d.is_contiguous()
    mpi = MPI(align_corners=ac, variant=variant, strict_order=strict, range_check=range_check, on_out_of_plane="raise")
    v2m = None if view_to_mpi is None else torch.as_tensor(np.asarray(view_to_mpi, dtype=np.int32)).to(dev)
    with torch.no_grad():
        out = mpi.render_views_depth(t(rgb), depth_d, t(plane_z), zb, t(dhw), t(ray), t(eye), t(zd), background=t(bg), views_per_mpi=views_per_mpi,
                                     view_to_mpi=v2m, check_last_plane=check_last, want_transmittance=True, out_pm1=out_pm1, defer_status=defer_status)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _check_forward(case, bg_on, ac, v2m=None, variants=("auto",), **kw):
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = case
    bg = bg if bg_on else None
    orc = oracle.render(_expand(rgb, depth, plane_z, bg, zb).numpy(), dhw, ray, eye, zd, view_to_mpi=v2m, align_corners=ac, threads=True)
    for variant in variants:
        strict = depth_render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, ac=ac, variant=variant, strict=True, **kw)
        for k in ("color", "depth", "T"):
            assert np.array_equal(strict[k], orc[k]), (variant, k, np.abs(strict[k] - orc[k]).max())
        fast = depth_render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, ac=ac, variant=variant, **kw)
        errs = {k: float(np.abs(fast[k] - orc[k]).max()) for k in ("color", "depth", "T")}
        print("default mode", variant, errs)
        assert errs["color"] <= 0.5 * TOL and errs["depth"] <= TOL and errs["T"] <= TOL, (variant, errs)   # [0,1] colour: half the [-1,1] bar
        assert int(strict["status"][0]) == 0 and int(fast["status"][0]) == 0
    return orc


# ---- forward -----------------------------------------------------------------------------------------------------------------------------------
FWD_CASES = [
    dict(seed=1, B=2, D=8, S=96, n_z_bins=4),                             # wide ramp: three to four planes on it
    dict(seed=4, B=3, D=7, S=100, T=77, n_z_bins=32),                     # H, W no multiple of any tile, Ht, Wt != H, W
    dict(seed=2, B=2, D=12, S=112, T=128, n_z_bins=4, extreme=True),      # tilted poses: rays leave the planes
    dict(seed=6, B=1, D=1, S=40, n_z_bins=4),                             # one plane (with a background: the plane IS the background)
    dict(seed=1, B=2, D=32, S=96, n_z_bins=256),                          # step-like ramp: narrower than the plane spacing
]


@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", FWD_CASES)
def test_forward_matches_the_oracle_on_the_expanded_volume(cfg, dtype, ac, with_bg):
    _check_forward(_case(dtype=dtype, **cfg), with_bg, ac)


def test_forward_gather_variant_is_the_same_kernel():
    case = _case(seed=1, B=2, D=8, S=96, n_z_bins=4)
    _check_forward(case, True, True, variants=("gather", "lds", "band"))   # (every name reaches the one kernel: GATHER as such, the others as AUTO)


def test_forward_holes_show_the_background_of_the_scene():
    """depth reaches 1.35: beyond plane_z = 1 by more than the ramp, every plane's alpha is 0 there and the pixel stays transparent.  (Depth seed 13:
    its high values lie where these two views look -- 13 % of the pixels on the CPU oracle; seed 11 puts them at the rim, 2 %.)"""
    case = _case(seed=1, B=2, D=8, S=96, n_z_bins=4, reach=1.35, depth_seed=13)
    for with_bg in (False, True):
        orc = _check_forward(case, with_bg, True)
        frac = float((orc["T"] > 0.5).mean())
        print("pixels with T_out > 0.5:", frac)
        assert frac >= 0.10, frac


@pytest.mark.parametrize("grouping", ["uniform", "ragged", "view_to_mpi"])
def test_forward_view_groupings_and_a_strided_depth_view(grouping):
    case = _case(seed=9, B=4, D=6, S=72, n_z_bins=4, T=64, M=2)
    kw, v2m = {"uniform": (dict(views_per_mpi=2), [0, 0, 1, 1]), "ragged": (dict(views_per_mpi=[1, 3]), [0, 1, 1, 1]),
               "view_to_mpi": (dict(view_to_mpi=[1, 0, 0, 1]), [1, 0, 0, 1])}[grouping]
    _check_forward(case, grouping != "ragged", True, v2m=v2m, depth_as_view=True, **kw)


def test_plane_table_per_mpi():
    """plane_z [M, D]: every MPI compares its depth with its own table."""
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = _case(seed=1, B=2, D=8, S=96, n_z_bins=4)
    table = torch.stack([plane_z, plane_z * 0.9 + 0.03])
    from ml_gmpi_amd import expand_depth_alpha
    orc = oracle.render(expand_depth_alpha(rgb, depth, table, *zb, bg).numpy(), dhw, ray, eye, zd, threads=True)
    got = depth_render(rgb, depth, table, bg, dhw, ray, eye, zd, zb, strict=True)
    for k in ("color", "depth", "T"):
        assert np.array_equal(got[k], orc[k]), k
    one = depth_render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, strict=True)
    assert np.array_equal(one["color"][0], got["color"][0]) and not np.array_equal(one["color"][1], got["color"][1])


@pytest.mark.parametrize("where", ["depth_nan", "rgb", "background"])
def test_range_bit(where):
    from ml_gmpi_amd import MPI
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = (t.clone() if isinstance(t, torch.Tensor) else t for t in _case(seed=3, B=1, D=5, S=64, n_z_bins=4))
    clean = depth_render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, defer_status=True)
    assert int(clean["status"][0]) == 0
    # the image centre: every frontal view samples it (the colours on the planes whose alpha there is not 0: the last plane's is)
    {"depth_nan": depth, "rgb": rgb, "background": bg}[where].view(-1, 64, 64)[0, 32, 32] = float("nan") if where == "depth_nan" else 1.5
    out = depth_render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, defer_status=True)
    assert int(out["status"][0]) & 2, where
    with pytest.raises(AssertionError):
        depth_render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb)
    off = depth_render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, range_check="off", defer_status=True)
    assert int(off["status"][0]) == 0
    if where != "depth_nan":   # range_check="full" passes over the colour images
        dev = torch.device(DEV)
        t = lambda a: a.to(dev)
        with pytest.raises(AssertionError):
            MPI(range_check="full", on_out_of_plane="raise").render_views_depth(t(rgb), t(depth), t(plane_z), zb, t(dhw), t(ray), t(eye), t(zd), background=t(bg))


def test_check_last_plane_sets_bit_one_on_the_pose_that_sets_it_on_the_volume_path():
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = _case(seed=2, B=2, D=6, S=64, n_z_bins=4, extreme=True)
    dhw = dhw.clone()
    dhw[:, -1, 1:] *= 0.5   # a last plane the tilted rays leave
    t = lambda a: a.to(dev)
    mpi = MPI(on_out_of_plane="raise")
    args = (t(rgb), t(depth), t(plane_z), zb, t(dhw), t(ray), t(eye), t(zd))
    with torch.no_grad():
        today = mpi.render_views(t(_expand(rgb, depth, plane_z, bg, zb)), t(dhw), t(ray), t(eye), t(zd), check_last_plane=True, defer_status=True)
        on = mpi.render_views_depth(*args, background=t(bg), check_last_plane=True, defer_status=True)
        off = mpi.render_views_depth(*args, background=t(bg), check_last_plane=False, defer_status=True)
    assert int(today["status"][0].item()) & 1
    assert int(on["status"][0].item()) == int(today["status"][0].item())
    assert int(off["status"][0].item()) == 0
    with pytest.raises(RuntimeError):
        mpi.render_views_depth(*args, background=t(bg), check_last_plane=True)


# ---- backward ----------------------------------------------------------------------------------------------------------------------------------
def _reference_grads(case, bg_on, v2m, gc, gd, gT, out_pm1, dtype):
    """d(sum gC colour + sum gZ depth + sum gT T) / d(rgb, depth, background) of the torch reference through expand_depth_alpha, in `dtype`
    (colour and depth: tests/_torch_ref.torch_render; with a gT: tests/_transmittance_ref.render, as tests/test_hip_shared_color.py)."""
    from ml_gmpi_amd import expand_depth_alpha
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = case
    ins = [None if p is None else p.to(dtype).clone().requires_grad_(True) for p in (rgb, depth, bg if bg_on else None)]
    vol = expand_depth_alpha(ins[0], ins[1], plane_z, zb[0], zb[1], ins[2])
    c = lambda a: torch.as_tensor(a).to(dtype)
    if gT is None:
        color, dep = torch_render(vol, c(dhw), c(ray), c(eye), c(zd), v2m)
        T = None
    else:
        color, dep, T = _transmittance_ref.render(vol, c(dhw), c(ray), c(eye), c(zd), v2m)
    if out_pm1:
        color = 2 * color - 1
    loss = torch.zeros((), dtype=dtype)
    for out, g in ((color, gc), (dep, gd), (T, gT)):
        if g is not None:
            loss = loss + (out * c(g)).sum()
    loss.backward()
    return [None if i is None else (i.grad if i.grad is not None else torch.zeros_like(i)).double().numpy() for i in ins]


def _hip_grads(case, bg_on, vpm, gc, gd, gT, out_pm1, needs=(True, True, True), variant="auto"):
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = case
    ins = [None if p is None else p.to(dev).clone().requires_grad_(n) for p, n in zip((rgb, depth, bg if bg_on else None), needs)]
    mpi = MPI(variant=variant, on_out_of_plane="raise")
    t = lambda a: torch.as_tensor(a).to(dev)
    out = mpi.render_views_depth(ins[0], ins[1], t(plane_z), zb, t(dhw), t(ray), t(eye), t(zd), background=ins[2], views_per_mpi=vpm,
                                 check_last_plane=False, out_pm1=out_pm1, want_transmittance=True)
    loss = 0
    for key, g in (("color", gc), ("depth", gd), ("T", gT)):
        if g is not None:
            loss = loss + (out[key] * t(g)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return ins, out


def _upstream(N, S, seed=7):
    g = np.random.default_rng(seed)
    return tuple(g.standard_normal((N, c, S, S)).astype(np.float32) for c in (3, 1, 1))


def _compare_capped(got, ref64, ref32, dtype, label, colour_reaches, with_bg):
    """tests/test_hip_shared_color._compare's rule -- max(5e-5, 4 e_ref) max|g_ref| + 1e-6 + half an ulp of the storage dtype -- under the condition
    e_ref <= 2e-4 per tensor, and with its check that the background gradient means something when the colour gradient reaches it (max|g_ref
    background| >= 1e-2 max|g_ref rgb|: the surface hides the last plane, but the rays that miss the nearer, smaller planes see it -- max|g_ref
    background| is 1.0 to 6.6 in these cases on the CPU)."""
    for name, r64, r32 in zip(("rgb", "depth", "background"), ref64, ref32):
        if r64 is not None and float(np.abs(r64).max()) > 0:
            e_ref = float(np.abs(r32 - r64).max()) / float(np.abs(r64).max())
            print(f"{label} {name}: e_ref {e_ref:.2e}")
            assert e_ref <= E_REF_CAP, (label, name, e_ref)
    _compare(got, ref64, ref32, dtype, label, colour_reaches, with_bg)


BWD_CASES = {
    "wide": (dict(seed=5, B=4, D=8, S=64, n_z_bins=4, M=2), 2),
    "narrow": (dict(seed=5, B=4, D=8, S=64, n_z_bins=32, M=2), 2),
    "steps": (dict(seed=5, B=2, D=32, S=96, n_z_bins=256, M=1), 2),
}


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "".join(n for n, on in zip("CZT", c) if on))
@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("name", list(BWD_CASES))
def test_backward_matches_float64_autograd_through_expand(name, with_bg, combo):
    """The T-only combination takes the case's depth scaled to reach 1.35 (holes).  Behind an opaque surface T_out is ~1e-10 per opaque plane, so a
    gradient that comes from T alone is a rounding residue there -- max|g_ref| 4e-6 / 2e-4 at n_z_bins = 32 / 256 and the fp32 torch chain itself off by
    0.34 / 0.02 of it on the CPU (1 - a cancels for a tap a few ulps below 1), far beyond the e_ref cap; at the holes' rims T_out is of order 1, max|g_ref|
    10 to 600, and e_ref 2e-6 to 6e-6.  The inputs were changed, not the cap."""
    cfg, vpm = BWD_CASES[name]
    if combo == (False, False, True):
        cfg = dict(cfg, reach=1.35)
    case = _case(**cfg)
    N, S = cfg["B"], cfg["S"]
    v2m = [n // vpm for n in range(N)]
    gc, gd, gT = (g if on else None for g, on in zip(_upstream(N, S), combo))
    for out_pm1 in ((False, True) if combo[0] else (False,)):
        ref64 = _reference_grads(case, with_bg, v2m, gc, gd, gT, out_pm1, torch.float64)
        ref32 = _reference_grads(case, with_bg, v2m, gc, gd, gT, out_pm1, torch.float32)
        ins, _ = _hip_grads(case, with_bg, vpm, gc, gd, gT, out_pm1)
        for i in ins:
            assert i is None or (i.grad is not None and i.grad.dtype == torch.float32 and i.grad.shape == i.shape)
        got = [None if i is None else i.grad.double().cpu().numpy() for i in ins]
        assert float(np.abs(got[1]).max()) > 0
        _compare_capped(got, ref64, ref32, torch.float32, f"{name} pm1={out_pm1}", combo[0], with_bg)


def test_backward_opaque_stack_starts_from_the_re_walked_transmittance():
    """D = 16, n_z_bins = 4: behind the surface several planes are exactly opaque, the forward's T_out underflows for most pixels and the sweep starts
    from the transmittance the kernel re-walks over the ramp samples."""
    cfg = dict(seed=5, B=2, D=16, S=48, n_z_bins=4, M=1)
    case = _case(**cfg)
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = case
    orc = oracle.render(_expand(rgb, depth, plane_z, bg, zb).numpy(), dhw, ray, eye, zd, view_to_mpi=[0, 0], threads=True)
    frac = float((orc["T"] < 1e-30).mean())
    print("pixels with T_out < 1e-30:", frac)
    assert frac >= 0.5, frac
    gc, gd, gT = _upstream(2, 48)
    ref64 = _reference_grads(case, True, [0, 0], gc, gd, gT, False, torch.float64)
    ref32 = _reference_grads(case, True, [0, 0], gc, gd, gT, False, torch.float32)
    for variant in ("auto", "gather"):
        ins, _ = _hip_grads(case, True, 2, gc, gd, gT, False, variant=variant)
        _compare_capped([i.grad.double().cpu().numpy() for i in ins], ref64, ref32, torch.float32, f"opaque stack {variant}", True, True)


def test_backward_holes_reach_the_background_and_the_transmittance():
    """depth reaches 1.35: the last plane and T_out are visible through the holes' rims; every upstream gradient at once."""
    cfg = dict(seed=1, B=2, D=8, S=64, n_z_bins=4, reach=1.35, depth_seed=13)
    case = _case(**cfg)
    gc, gd, gT = _upstream(2, 64)
    ref64 = _reference_grads(case, True, [0, 1], gc, gd, gT, True, torch.float64)
    ref32 = _reference_grads(case, True, [0, 1], gc, gd, gT, True, torch.float32)
    assert np.abs(ref64[2]).max() >= 1e-2 * np.abs(ref64[0]).max()   # (the background gradient means something here)
    ins, _ = _hip_grads(case, True, 1, gc, gd, gT, True)
    _compare_capped([i.grad.double().cpu().numpy() for i in ins], ref64, ref32, torch.float32, "holes", True, True)


def test_backward_partial_requires_grad():
    cfg, vpm = BWD_CASES["wide"]
    case = _case(**cfg)
    gc, gd, _ = _upstream(cfg["B"], cfg["S"])
    full, _ = _hip_grads(case, True, vpm, gc, gd, None, False)
    for needs in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)):
        ins, _ = _hip_grads(case, True, vpm, gc, gd, None, False, needs=needs)
        for i, f, n in zip(ins, full, needs):
            if not n:
                assert i.grad is None
            else:   # the same values, up to the order of the atomic adds
                ref = f.grad.double().cpu().numpy()
                assert np.abs(i.grad.double().cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-7, needs


@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_backward_16_bit_storage_returns_gradients_in_the_inputs_dtype(dtype, with_bg):
    cfg, vpm = BWD_CASES["wide"]
    case = _case(dtype=dtype, **cfg)
    N, S = cfg["B"], cfg["S"]
    v2m = [n // vpm for n in range(N)]
    gc, gd, gT = _upstream(N, S)
    ins, _ = _hip_grads(case, with_bg, vpm, gc, gd, gT, False)
    for i in ins:
        assert i is None or (i.grad is not None and i.grad.dtype == dtype and i.grad.shape == i.shape)
    ref64 = _reference_grads(case, with_bg, v2m, gc, gd, gT, False, torch.float64)   # (of the stored values)
    ref32 = _reference_grads(case, with_bg, v2m, gc, gd, gT, False, torch.float32)
    _compare_capped([None if i is None else i.grad.double().cpu().numpy() for i in ins], ref64, ref32, dtype, f"{dtype}", True, with_bg)


@pytest.mark.parametrize("poison", ["inf_upstream", "nan_depth", "nan_colour"])
def test_backward_with_a_non_finite_value_writes_inside_the_gradient_images_only(poison):
    """A tap outside the texture has weight 0 and an unclamped address (rows -2 .. Ht, columns -2 .. Wt): the weight alone may keep it from being
    written, whatever the gradient is -- inf * 0 and NaN * 0 are NaN, not 0.  The three gradient images are the interiors of larger zero-filled
    buffers (4 guard rows and columns all round: every address a tap can name lies inside the buffer); tilted poses whose rays leave the planes,
    align_corners (border footprints start on the last row / column), and one non-finite value: an infinite upstream gradient on the image border
    and centre, a NaN depth texel, or a NaN colour texel with the range check off.  The guards must stay exactly zero."""
    import ctypes
    from ml_gmpi_amd import MPI, _lib
    from ml_gmpi_amd.hip_mpi import _depth_alpha, _shared_color
    dev = torch.device(DEV)
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = (t.clone().to(dev) if isinstance(t, torch.Tensor) else t
                                                      for t in _case(seed=2, B=2, D=6, S=64, n_z_bins=4, extreme=True))
    N, S, G = 2, 64, 4
    gc, gd, gT = (torch.as_tensor(g).to(dev) for g in _upstream(N, S))
    if poison == "inf_upstream":
        gc[:, :, 0, :] = gc[:, :, -1, :] = gc[:, :, :, 0] = gc[:, :, :, -1] = float("inf")
        gc[:, :, 32, 32] = float("-inf")
        gd[:, :, -1, -1] = float("inf")
    elif poison == "nan_depth":
        depth[:, 0, 32, 32] = depth[:, 0, 0, 0] = depth[:, 0, -1, -1] = float("nan")
    else:
        rgb[:, 1, 32, 32] = rgb[:, 0, -1, -1] = bg[:, 2, 0, 0] = float("nan")
    mpi = MPI(range_check="off", on_out_of_plane="raise")
    with torch.no_grad():
        res = mpi.render_views_depth(rgb, depth, plane_z, zb, dhw, ray, eye, zd, background=bg, want_transmittance=True, defer_status=True,
                                     _in_autograd_fn=True)
    p = _lib.GmpiRenderParams.from_buffer_copy(res.pop("_bwd")[0])
    p.rgb_out = p.depth_out = p.status = None
    bufs = [torch.zeros((2, c, S + 2 * G, S + 2 * G), device=dev) for c in (3, 1, 3)]
    views = [b[:, :, G:-G, G:-G] for b in bufs]
    args = []
    for v in views:
        args += [v.data_ptr(), (ctypes.c_int64 * 3)(*v.stride()[:3])]
    rc = _lib.load_library().gmpi_mpi_render_depth_backward_launch(
        ctypes.byref(p), ctypes.byref(_shared_color(rgb, bg)), ctypes.byref(_depth_alpha(plane_z.to(dev), *zb)), gc.data_ptr(), gd.data_ptr(), gT.data_ptr(),
        *args, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for name, b, v in zip(("rgb", "depth", "background"), bufs, views):
        assert int(torch.count_nonzero(v)) > 0, name             # (the launch did write the image; NaN counts as non-zero)
        guard = b.clone()
        guard[:, :, G:-G, G:-G] = 0
        assert int(torch.count_nonzero(guard)) == 0, (poison, name, int(torch.count_nonzero(guard)))


# ---- host layer --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bg", [False, True])
def test_renderer_render_depth_matches_render_and_consumes_the_same_rng(with_bg):
    from ml_gmpi_amd import depth_alpha_bounds, expand_depth_alpha, make_renderer
    dev = torch.device(DEV)
    S, D, B = 64, 8, 2
    rgb, depth, _, bg, *_ = _case(seed=12, B=B, D=D, S=S, n_z_bins=4)
    rgb, depth, bg = rgb.to(dev), depth.to(dev), (bg.to(dev) if with_bg else None)
    res, states = [], []
    for layout in ("volume", "depth"):
        r = make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise", range_check="full")
        plane_z = r.get_xyz_single_res(S, S, only_z=True)[1].reshape(-1)
        vol = expand_depth_alpha(rgb, depth, plane_z, *depth_alpha_bounds(2, 4), bg)
        torch.manual_seed(21)
        with torch.no_grad():
            for _ in range(3):   # (a repeated request: the look-ahead pose queue is in use)
                out = (r.render_depth(rgb, depth, S, S, z_range=2, n_z_bins=4, background_rgb=bg, want_transmittance=True) if layout == "depth"
                       else r.render(vol, S, S, want_transmittance=True))
        torch.cuda.synchronize()
        res.append(out)
        states.append(torch.get_rng_state())
    assert torch.equal(states[0], states[1])
    a, b = res
    assert len(a) == len(b) == 5
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])           # c2w, angles
    assert float((a[0] - b[0]).abs().max()) <= TOL and float((a[1] - b[1]).abs().max()) <= TOL and float((a[4] - b[4]).abs().max()) <= TOL
    assert float(b[0].std()) > 0.05   # (a scene, not a constant image)


def test_refusals():
    from ml_gmpi_amd import MPI, make_renderer, rays_from_c2w
    dev = torch.device(DEV)
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = (t.to(dev) if isinstance(t, torch.Tensor) else t for t in _case(seed=3, B=1, D=5, S=64, n_z_bins=4))
    mpi = MPI(on_out_of_plane="raise")
    with pytest.raises(TypeError):
        mpi.render_views_depth(rgb, depth.to(torch.bfloat16), plane_z, zb, dhw, ray, eye, zd)
    with pytest.raises(TypeError):
        mpi.render_views_depth(rgb, depth, plane_z, zb, dhw, ray, eye, zd, background=bg.to(torch.float16))
    u8 = lambda t: (t * 255).to(torch.uint8)
    with pytest.raises(TypeError):
        mpi.render_views_depth(u8(rgb), u8(depth), plane_z, zb, dhw, ray, eye, zd, background=u8(bg))
    for name in ("lds", "wave", "band"):   # kernels this layout does not have are refused by name, not replaced
        with pytest.raises(ValueError):
            mpi.render_views_depth(rgb, depth, plane_z, zb, dhw, ray, eye, zd, variant=name)
    r = make_renderer("FFHQ", n_planes=5, device=dev, on_out_of_plane="raise", geometry_grad=True)
    r.set_cam(r.cam_fov, 64, 64)
    torch.manual_seed(0)
    cam = r.sample_cam_poses(1, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    ray_g, eye_g, zd_g = rays_from_c2w(r, cam[2].to(dev).clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        r.mpi.render_views_depth(rgb, depth, plane_z, zb, r._dhw_for(1), ray_g, eye_g, zd_g)
    with pytest.raises(NotImplementedError):
        r.mpi.render_views_depth(rgb, depth, plane_z, zb, r._dhw_for(1).clone().requires_grad_(True), ray, eye, zd)
    out = r.mpi.render_views_depth(rgb, depth.clone().requires_grad_(True), plane_z, zb, r._dhw_for(1), ray_g.detach(), eye_g.detach(), zd_g.detach())
    out["color"].sum().backward()   # detached camera tensors: the layout renders and back-propagates under geometry_grad=True
