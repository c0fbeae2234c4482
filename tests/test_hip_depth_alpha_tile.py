"""GPU tests of the tile backward of the depth-alpha layout (`render_views_depth(..., depth_backward="tile")`,
gmpi_mpi_render_depth_backward_tile_launch): against float64 autograd of the torch reference through `expand_depth_alpha` under the rule of
tests/test_hip_depth_alpha.py (`_compare_capped`: e_ref <= 2e-4), and against the one-pixel-per-lane backward ("pixel") within the order of the
atomic adds, 1e-5 max|ref| + 1e-7.  Every test that means to run the tile kernel watches the C entry: a silent fall-back to the one-pixel path does
not pass.  Run on the MI355X box:  python -m pytest tests -m gpu"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from _torch_ref import torch_render
import _transmittance_ref
from test_hip_depth_alpha import BWD_CASES, E_REF_CAP, _case, _compare_capped, _reference_grads, _upstream
from test_hip_shared_color import COMBOS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE_ENTRY = "gmpi_mpi_render_depth_backward_tile_launch"
PIXEL_ENTRY = "gmpi_mpi_render_depth_backward_launch"
assert E_REF_CAP == 2e-4


@pytest.fixture
def spy(monkeypatch):
    """Both backward entries of the loaded library, wrapped: spy[name] lists (D, variant) of every call."""
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    seen = {TILE_ENTRY: [], PIXEL_ENTRY: []}
    for name in seen:
        def wrapped(*args, _real=getattr(lib, name), _log=seen[name]):
            p = args[0]._obj
            _log.append((int(p.D), int(p.variant)))
            return _real(*args)
        monkeypatch.setattr(lib, name, wrapped)
    return seen


def _ran_tile(spy, calls=1, D=None):
    """The tile entry was called `calls` times since the last look (AUTO, and with D planes), the one-pixel entry not at all."""
    t, q = list(spy[TILE_ENTRY]), list(spy[PIXEL_ENTRY])
    del spy[TILE_ENTRY][:], spy[PIXEL_ENTRY][:]
    assert len(t) == calls and not q, (t, q)
    assert all(v == 0 for _, v in t), t                  # GMPI_VARIANT_AUTO: the entry launches the tile kernel (D <= 128)
    assert D is None or all(d == D for d, _ in t), t


def _hip_grads(case, bg_on, gc, gd, gT, out_pm1, *, depth_backward, align_corners=True, views_per_mpi=1, view_to_mpi=None, plane_z=None,
               needs=(True, True, True), variant="auto", range_check="touched", depth_as_view=False):
    """The gradients of (rgb, depth, background) as float64 arrays (None: no gradient asked or returned) and their dtypes."""
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    rgb, depth, pz, bg, dhw, ray, eye, zd, zb = case
    pz = pz if plane_z is None else plane_z
    t = lambda a: torch.as_tensor(a).to(dev)
    ins = [None if p is None else p.to(dev).clone() for p in (rgb, depth, bg if bg_on else None)]
    depth_in = ins[1]
    if depth_as_view:   # the depth image as the strided view rgbd[:, 3:] of an RGB-D tensor
        rgbd = torch.cat((ins[0], ins[1]), 1)
        ins[1] = rgbd[:, 3:]
        assert not ins[1].is_contiguous()
        leaf = rgbd.requires_grad_(needs[1])
        depth_in = leaf[:, 3:]
    for i, n in zip((0, 2), (needs[0], needs[2])):
        if ins[i] is not None:
            ins[i].requires_grad_(n)
    if not depth_as_view:
        depth_in.requires_grad_(needs[1])
    mpi = MPI(align_corners=align_corners, variant=variant, range_check=range_check, on_out_of_plane="raise")
    v2m = None if view_to_mpi is None else torch.as_tensor(np.asarray(view_to_mpi, dtype=np.int32)).to(dev)
    out = mpi.render_views_depth(ins[0], depth_in, t(pz), zb, t(dhw), t(ray), t(eye), t(zd), background=ins[2], views_per_mpi=views_per_mpi,
                                 view_to_mpi=v2m, check_last_plane=False, out_pm1=out_pm1, want_transmittance=True, depth_backward=depth_backward)
    loss = 0
    for key, g in (("color", gc), ("depth", gd), ("T", gT)):
        if g is not None:
            loss = loss + (out[key] * t(g)).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = [None if ins[0] is None else ins[0].grad, (leaf.grad[:, 3:] if leaf.grad is not None else None) if depth_as_view else depth_in.grad,
             None if ins[2] is None else ins[2].grad]
    return [None if g is None else g.double().cpu().numpy() for g in grads], [None if g is None else g.dtype for g in grads]


def _reference_grads_ac(case, bg_on, v2m, gc, gd, gT, out_pm1, dtype, ac):
    """test_hip_depth_alpha._reference_grads with the reference's align_corners argument."""
    from ml_gmpi_amd import expand_depth_alpha
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = case
    ins = [None if p is None else p.to(dtype).clone().requires_grad_(True) for p in (rgb, depth, bg if bg_on else None)]
    vol = expand_depth_alpha(ins[0], ins[1], plane_z, zb[0], zb[1], ins[2])
    c = lambda a: torch.as_tensor(a).to(dtype)
    color, dep, *rest = (torch_render if gT is None else _transmittance_ref.render)(vol, c(dhw), c(ray), c(eye), c(zd), v2m, align_corners=ac)
    T = rest[0] if rest else None
    if out_pm1:
        color = 2 * color - 1
    loss = torch.zeros((), dtype=dtype)
    for out, g in ((color, gc), (dep, gd), (T, gT)):
        if g is not None:
            loss = loss + (out * c(g)).sum()
    loss.backward()
    return [None if i is None else (i.grad if i.grad is not None else torch.zeros_like(i)).double().numpy() for i in ins]


@functools.lru_cache(maxsize=None)
def _refs(cfg_items, bg_on, v2m, combo, out_pm1, ac=True):
    """(float64, fp32) reference gradients of a case, computed once and shared; never written to."""
    cfg = dict(cfg_items)
    case = _case(**cfg)
    gc, gd, gT = (g if on else None for g, on in zip(_upstream(len(v2m), cfg["S"]), combo))
    if ac:
        return tuple(_reference_grads(case, bg_on, list(v2m), gc, gd, gT, out_pm1, dt) for dt in (torch.float64, torch.float32))
    return tuple(_reference_grads_ac(case, bg_on, list(v2m), gc, gd, gT, out_pm1, dt, False) for dt in (torch.float64, torch.float32))


def _key(cfg):
    return tuple(sorted(cfg.items(), key=lambda kv: kv[0]))


def _close(a, b, label):
    """Two variants of one computation: up to the order of the atomic adds."""
    for name, x, y in zip(("rgb", "depth", "background"), a, b):
        assert (x is None) == (y is None), (label, name)
        if x is not None:
            err, scale = float(np.abs(x - y).max()), float(np.abs(y).max())
            print(f"{label} {name}: tile vs pixel {err:.3e} of max {scale:.3e}")
            assert err <= 1e-5 * scale + 1e-7, (label, name, err, scale)


def _check(cfg, bg_on, v2m, combo, out_pm1, spy, label, *, vpm=1, ac=True, against_pixel=False, **kw):
    case = _case(**cfg)
    gc, gd, gT = (g if on else None for g, on in zip(_upstream(len(v2m), cfg["S"]), combo))
    ref64, ref32 = _refs(_key(cfg), bg_on, tuple(v2m), combo, out_pm1, ac)
    got, dtypes = _hip_grads(case, bg_on, gc, gd, gT, out_pm1, depth_backward="tile", align_corners=ac, views_per_mpi=vpm, **kw)
    _ran_tile(spy, D=cfg["D"])
    assert all(d is None or d == torch.float32 for d in dtypes)
    assert float(np.abs(got[1]).max()) > 0
    _compare_capped(got, ref64, ref32, torch.float32, label, combo[0], bg_on)
    if against_pixel:
        pix, _ = _hip_grads(case, bg_on, gc, gd, gT, out_pm1, depth_backward="pixel", align_corners=ac, views_per_mpi=vpm, **kw)
        assert not spy[TILE_ENTRY] and len(spy[PIXEL_ENTRY]) == 1
        del spy[PIXEL_ENTRY][:]
        _close(got, pix, label)
    return got


ALL = (True, True, True)


# ---- 1: the cases of the one-pixel kernel's test, every combination of upstream gradients -----------------------------------------------------
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "".join(n for n, on in zip("CZT", c) if on))
@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("name", list(BWD_CASES))
def test_tile_backward_matches_float64_autograd_through_expand(name, with_bg, combo, spy):
    """As test_hip_depth_alpha's: the T-only combination takes the case's depth scaled to reach 1.35 (holes)."""
    cfg, vpm = BWD_CASES[name]
    if combo == (False, False, True):
        cfg = dict(cfg, reach=1.35)
    v2m = [n // vpm for n in range(cfg["B"])]
    for out_pm1 in ((False, True) if combo[0] else (False,)):
        _check(cfg, with_bg, v2m, combo, out_pm1, spy, f"{name} pm1={out_pm1}", vpm=vpm)


@pytest.mark.parametrize("with_bg", [False, True])
def test_tile_backward_without_align_corners(with_bg, spy):
    cfg, vpm = BWD_CASES["wide"]
    v2m = [n // vpm for n in range(cfg["B"])]
    _check(cfg, with_bg, v2m, ALL, True, spy, "wide ac=False", vpm=vpm, ac=False, against_pixel=True)


# ---- 2, 3: the re-walked transmittance, holes --------------------------------------------------------------------------------------------------
def test_tile_backward_opaque_stack_starts_from_the_re_walked_transmittance(spy):
    """D = 16, n_z_bins = 4, two views of one MPI: the forward's T_out underflows for most pixels (test_hip_depth_alpha asserts >= half of them)."""
    cfg = dict(seed=5, B=2, D=16, S=48, n_z_bins=4, M=1)
    _check(cfg, True, [0, 0], ALL, False, spy, "opaque stack", vpm=2, against_pixel=True)


def test_tile_backward_holes_reach_the_background_and_the_transmittance(spy):
    cfg = dict(seed=1, B=2, D=8, S=64, n_z_bins=4, reach=1.35, depth_seed=13)
    ref64, _ = _refs(_key(cfg), True, (0, 1), ALL, True)
    assert np.abs(ref64[2]).max() >= 1e-2 * np.abs(ref64[0]).max()
    _check(cfg, True, [0, 1], ALL, True, spy, "holes")


# ---- 4 - 8: the window moves, ragged shapes, no box fits, the plane limit, the case the kernel is for ------------------------------------------
def _bg_share(cfg, v2m):
    ref64, _ = _refs(_key(cfg), True, tuple(v2m), ALL, True)
    return float(np.abs(ref64[2]).max() / np.abs(ref64[0]).max())


@pytest.mark.parametrize("n_z_bins", [4, 256])
def test_tile_backward_tilted_poses_move_the_window(n_z_bins, spy):
    """256 x 256, 16 planes, tilted poses: the tile's boxes drift out of the 64 x 32 window several times per tile (a replay of the box and
    re-anchor logic on the CPU: 6.1 flushes per tile on average, at most 12, every tile more than one)."""
    cfg = dict(seed=8, B=2, D=16, S=256, extreme=True, n_z_bins=n_z_bins)
    assert _bg_share(cfg, [0, 1]) >= 0.4
    _check(cfg, True, [0, 1], ALL, True, spy, f"tilted {n_z_bins}", against_pixel=True)


def test_tile_backward_ragged_image_and_texture(spy):
    """100 x 100 pixels over 77 x 77 texels, 7 planes, 3 MPIs: the image is no multiple of the tile, Ht, Wt != H, W."""
    cfg = dict(seed=4, B=3, D=7, S=100, T=77, n_z_bins=32)
    assert _bg_share(cfg, [0, 1, 2]) >= 0.4
    _check(cfg, True, [0, 1, 2], ALL, True, spy, "ragged", against_pixel=True)


def test_tile_backward_minification_scatters_directly(spy):
    """64 x 64 pixels over 256 x 256 texels: every tile's box exceeds the window on every plane (replay: 96 of 96 unstaged): the whole launch takes
    the direct scatter."""
    cfg = dict(seed=3, B=2, D=6, S=64, T=256, n_z_bins=4)
    assert _bg_share(cfg, [0, 1]) >= 0.4
    _check(cfg, True, [0, 1], ALL, True, spy, "minify", against_pixel=True)


@pytest.mark.parametrize("D", [128, 129])
def test_tile_backward_deep_stacks(D, spy):
    """D = 128 is the most the tile kernel takes.  D = 129 goes through the SAME entry, which then launches the one-pixel-per-lane kernel (documented
    at the entry; what the test can see is that the entry was called with 129 planes and returned the right gradients)."""
    cfg = dict(seed=13, B=2, S=48, n_z_bins=4, D=D)
    assert _bg_share(cfg, [0, 1]) >= 0.4
    _check(cfg, True, [0, 1], ALL, True, spy, f"deep {D}", against_pixel=(D == 129))


def test_tile_backward_32_planes_wide_ramp(spy):
    """32 planes, a ramp eight planes wide, two views of one MPI: most planes of most pixels add to the depth image."""
    cfg = dict(seed=5, B=2, D=32, S=96, n_z_bins=4, M=1)
    assert _bg_share(cfg, [0, 0]) >= 0.4
    _check(cfg, True, [0, 0], ALL, True, spy, "wide 32", vpm=2, against_pixel=True)


# ---- 9: outside the bound's assumption ---------------------------------------------------------------------------------------------------------
def test_tile_backward_colours_far_outside_the_unit_range_do_not_wrap(spy):
    """rgb and background x 64 (range check off): the depth bound assumes colours in [0, 1], so its terms exceed the tile scale; the lanes whose
    scaled terms reach 2^42 must go to global memory and the staged sums must not wrap."""
    cfg, vpm = BWD_CASES["wide"]
    rgb, depth, pz, bg, dhw, ray, eye, zd, zb = _case(**cfg)
    case = (rgb * 64, depth, pz, bg * 64, dhw, ray, eye, zd, zb)
    v2m = [n // vpm for n in range(cfg["B"])]
    gc, gd, gT = _upstream(cfg["B"], cfg["S"])
    ref64 = _reference_grads(case, True, v2m, gc, gd, gT, True, torch.float64)
    ref32 = _reference_grads(case, True, v2m, gc, gd, gT, True, torch.float32)
    assert np.abs(ref64[2]).max() >= 0.4 * np.abs(ref64[0]).max()
    got, _ = _hip_grads(case, True, gc, gd, gT, True, depth_backward="tile", views_per_mpi=vpm, range_check="off")
    _ran_tile(spy, D=cfg["D"])
    _compare_capped(got, ref64, ref32, torch.float32, "wide colours x 64", True, True)


# ---- 10: groupings -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouping", ["uniform", "ragged", "view_to_mpi", "plane_table"])
def test_tile_backward_view_groupings_a_strided_depth_view_and_a_plane_table_per_mpi(grouping, spy):
    cfg = dict(seed=9, B=4, D=6, S=72, T=64, n_z_bins=4, M=2)
    case = _case(**cfg)
    gc, gd, gT = _upstream(4, 72)
    kw = {"uniform": dict(views_per_mpi=2), "ragged": dict(views_per_mpi=[1, 3]), "view_to_mpi": dict(view_to_mpi=[1, 0, 0, 1]),
          "plane_table": dict(views_per_mpi=2, plane_z=torch.stack([case[2], case[2] * 0.9 + 0.03]))}[grouping]
    kw["depth_as_view"] = grouping != "plane_table"
    bg_on = grouping != "ragged"
    got, _ = _hip_grads(case, bg_on, gc, gd, gT, True, depth_backward="tile", **kw)
    _ran_tile(spy, D=6)
    pix, _ = _hip_grads(case, bg_on, gc, gd, gT, True, depth_backward="pixel", **kw)
    assert not spy[TILE_ENTRY] and len(spy[PIXEL_ENTRY]) == 1
    assert all(float(np.abs(g).max()) > 0 for g in got if g is not None)
    _close(got, pix, grouping)
    if grouping == "plane_table":   # (the table is read: one table for both MPIs gives another gradient for the second)
        one, _ = _hip_grads(case, bg_on, gc, gd, gT, True, depth_backward="tile", views_per_mpi=2)
        assert np.abs(one[1][0] - got[1][0]).max() <= 1e-5 * np.abs(got[1][0]).max() + 1e-7 and np.abs(one[1][1] - got[1][1]).max() > 1e-3 * np.abs(got[1][1]).max()


# ---- 11: partial requires_grad, 16-bit storage -------------------------------------------------------------------------------------------------
def test_tile_backward_partial_requires_grad(spy):
    cfg, vpm = BWD_CASES["wide"]
    case = _case(**cfg)
    gc, gd, _ = _upstream(cfg["B"], cfg["S"])
    full, _ = _hip_grads(case, True, gc, gd, None, False, depth_backward="tile", views_per_mpi=vpm)
    _ran_tile(spy)
    for needs in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)):
        got, _ = _hip_grads(case, True, gc, gd, None, False, depth_backward="tile", views_per_mpi=vpm, needs=needs)
        _ran_tile(spy)
        for g, f, n in zip(got, full, needs):
            if not n:
                assert g is None
            else:   # the same values, up to the order of the atomic adds
                assert np.abs(g - f).max() <= 1e-5 * np.abs(f).max() + 1e-7, needs


@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_tile_backward_16_bit_storage_returns_gradients_in_the_inputs_dtype(dtype, with_bg, spy):
    cfg, vpm = BWD_CASES["wide"]
    cfg = dict(cfg, dtype=dtype)
    case = _case(**cfg)
    v2m = [n // vpm for n in range(cfg["B"])]
    gc, gd, gT = _upstream(cfg["B"], cfg["S"])
    got, dtypes = _hip_grads(case, with_bg, gc, gd, gT, False, depth_backward="tile", views_per_mpi=vpm)
    _ran_tile(spy)
    assert all(d is None or d == dtype for d in dtypes) and dtypes[0] == dtype and dtypes[1] == dtype
    ref64, ref32 = _refs(_key(cfg), with_bg, tuple(v2m), ALL, False)   # (of the stored values)
    _compare_capped(got, ref64, ref32, dtype, f"{dtype}", True, with_bg)


# ---- 12: guards --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", ["inf_upstream", "nan_depth", "nan_colour"])
def test_tile_backward_with_a_non_finite_value_writes_inside_the_gradient_images_only(poison):
    """test_hip_depth_alpha's guard test through the new C entry: 4 guard rows and columns around each gradient image, tilted poses whose rays leave
    the planes, one non-finite value.  Checks the weight gating of the LDS adds, the flush's in-texture test and the non-finite fall-back to the
    direct scatter: the guards stay exactly zero, each image is written."""
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
    assert p.variant == _lib.VARIANT_AUTO and p.D == 6
    bufs = [torch.zeros((2, c, S + 2 * G, S + 2 * G), device=dev) for c in (3, 1, 3)]
    views = [b[:, :, G:-G, G:-G] for b in bufs]
    args = []
    for v in views:
        args += [v.data_ptr(), (ctypes.c_int64 * 3)(*v.stride()[:3])]
    rc = _lib.load_library().gmpi_mpi_render_depth_backward_tile_launch(
        ctypes.byref(p), ctypes.byref(_shared_color(rgb, bg)), ctypes.byref(_depth_alpha(plane_z.to(dev), *zb)), gc.data_ptr(), gd.data_ptr(), gT.data_ptr(),
        *args, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for name, b, v in zip(("rgb", "depth", "background"), bufs, views):
        assert int(torch.count_nonzero(v)) > 0, name             # (the launch did write the image; NaN counts as non-zero)
        guard = b.clone()
        guard[:, :, G:-G, G:-G] = 0
        assert int(torch.count_nonzero(guard)) == 0, (poison, name, int(torch.count_nonzero(guard)))


# ---- 13: host layer ----------------------------------------------------------------------------------------------------------------------------
def test_renderer_render_depth_with_the_tile_backward(spy):
    from ml_gmpi_amd import make_renderer
    dev = torch.device(DEV)
    S, D, B = 64, 8, 2
    rgb0, depth0, _, bg0, *_ = _case(seed=12, B=B, D=D, S=S, n_z_bins=4)
    grads, states = [], []
    for how in ("pixel", "tile"):
        r = make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise")
        rgb, depth, bg = (t.to(dev).clone().requires_grad_(True) for t in (rgb0, depth0, bg0))
        torch.manual_seed(21)
        out = r.render_depth(rgb, depth, S, S, z_range=2, n_z_bins=4, background_rgb=bg, want_transmittance=True, depth_backward=how)
        g = torch.Generator().manual_seed(3)
        w = [torch.randn(o.shape, generator=g).to(dev) for o in (out[0], out[1], out[4])]
        sum((o * x).sum() for o, x in zip((out[0], out[1], out[4]), w)).backward()
        torch.cuda.synchronize()
        states.append(torch.get_rng_state())
        grads.append([t.grad.double().cpu().numpy() for t in (rgb, depth, bg)])
        if how == "tile":
            _ran_tile(spy, D=D)
        else:
            assert len(spy[PIXEL_ENTRY]) == 1 and not spy[TILE_ENTRY]
            del spy[PIXEL_ENTRY][:]
    assert torch.equal(states[0], states[1])
    assert all(float(np.abs(g).max()) > 0 for g in grads[1])
    _close(grads[1], grads[0], "renderer")
    with pytest.raises(ValueError):
        r.render_depth(rgb, depth, S, S, z_range=2, n_z_bins=4, background_rgb=bg, depth_backward="window")
