"""GPU tests of the staged shared-colour forward (`variant="lds"` of `MPI.render_views_shared`, render_shared_forward.hip): per 32 x 16 pixel tile
and plane the texel box of the alpha plane and of the colour image goes through LDS.  The yardstick is `oracle.render` on
`expand_shared_color(rgb, alpha, background)`, as in tests/test_hip_shared_color.py.  Run on the MI355X box:  python -m pytest tests -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from test_hip_parity import TOL, _random_case
from test_hip_shared_color import _expand, _hip_grads, _parts, shared_render

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TILE_H_THREADS = 512   # a tile is gmpi_query(12) pixels wide and 512 / width high


# ---- the corner-box rule, restated in float64 ---------------------------------------------------------------------------------------------------
def _caps():
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    tw, cap_w, cap_h = lib.gmpi_query(12), lib.gmpi_query(13), lib.gmpi_query(14)
    assert tw > 0 and cap_w > 0 and cap_h > 0, (tw, cap_w, cap_h)
    return tw, TILE_H_THREADS // tw, cap_w, cap_h


def _boxes(dhw, ray, eye, Ht, Wt, ac, v2m=None):
    """(width, height) in texels of the box every (view, tile, plane) spans: from the tile's four corner pixels, 1/64 texel of slack, the tap to
    the right of / below the last corner included.  float64 restatement of plane_coord (gmpi_device.hpp)."""
    tw, th, _, _ = _caps()
    dhw, ray, eye = (np.asarray(a, dtype=np.float64) for a in (dhw, ray, eye))
    N, _, H, W = ray.shape
    out = []
    for n in range(N):
        m = n if v2m is None else v2m[n]
        for y0 in range(0, H, th):
            for x0 in range(0, W, tw):
                ys, xs = [y0, min(y0 + th - 1, H - 1)], [x0, min(x0 + tw - 1, W - 1)]
                r = ray[n][:, ys][:, :, xs].reshape(3, 4)                  # the four corner rays
                for d, ph, pw in dhw[m]:
                    s = (d - eye[n, 2]) / r[2]
                    u, v = 2 * (eye[n, 0] + r[0] * s) / pw, 2 * (eye[n, 1] + r[1] * s) / ph
                    if ac:
                        ix, iy = (u + 1) * (Wt - 1) / 2, (v + 1) * (Ht - 1) / 2
                    else:
                        u = np.where((u >= -1) & (u <= 1), u * 0.95, u)
                        v = np.where((v >= -1) & (v <= 1), v * 0.95, v)
                        ix, iy = ((u + 1) * Wt - 1) / 2, ((v + 1) * Ht - 1) / 2
                    w = (np.floor(ix.max() + 1 / 64) + 1) - np.floor(ix.min() - 1 / 64) + 1
                    h = (np.floor(iy.max() + 1 / 64) + 1) - np.floor(iy.min() - 1 / 64) + 1
                    out.append((w, h))
    return np.array(out)


def _fit_counts(boxes):
    """(boxes that fit with 2 texels to spare whatever the alignment of their first column, boxes that cannot fit, all)."""
    _, _, cap_w, cap_h = _caps()
    spare = (boxes[:, 0] + 3 + 2 <= cap_w) & (boxes[:, 1] + 2 <= cap_h)    # 3 texels: the first column is rounded down to a multiple of 4
    never = (boxes[:, 0] > cap_w) | (boxes[:, 1] > cap_h)
    return int(spare.sum()), int(never.sum()), len(boxes)


# ---- spies on the C ABI: which variant reached the launch, what the support query said -------------------------------------------------------
@pytest.fixture
def abi(monkeypatch):
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    real_launch, real_supports = lib.gmpi_mpi_render_shared_launch, lib.gmpi_render_shared_supports
    seen = dict(launched=[], supports=[])

    def launch(p, sc, stream):
        seen["launched"].append(int(p._obj.variant))
        return real_launch(p, sc, stream)

    def supports(p, sc):
        rc = real_supports(p, sc)
        seen["supports"].append(rc)
        if rc == 0:   # what the query refuses, the explicit launch refuses too
            assert real_launch(p, sc, None) == -6
        return rc
    monkeypatch.setattr(lib, "gmpi_mpi_render_shared_launch", launch)
    monkeypatch.setattr(lib, "gmpi_render_shared_supports", supports)
    return seen


_ORACLE = {}


def _oracle(key, rgb, alpha, bg, dhw, ray, eye, zd, ac, v2m):
    if key not in _ORACLE:
        _ORACLE[key] = oracle.render(_expand(rgb, alpha, bg).numpy(), dhw, ray, eye, zd, view_to_mpi=v2m, align_corners=ac, threads=True)
    return _ORACLE[key]


def _check(abi, key, rgb, alpha, bg, dhw, ray, eye, zd, ac, v2m=None, must_support=True, **kw):
    orc = _oracle(key, rgb, alpha, bg, dhw, ray, eye, zd, ac, v2m)
    gather = shared_render(rgb, alpha, bg, dhw, ray, eye, zd, ac=ac, variant="gather", strict=True, **kw)
    abi["launched"].clear(), abi["supports"].clear()
    strict = shared_render(rgb, alpha, bg, dhw, ray, eye, zd, ac=ac, variant="lds", strict=True, **kw)
    fast = shared_render(rgb, alpha, bg, dhw, ray, eye, zd, ac=ac, variant="lds", **kw)
    from ml_gmpi_amd import _lib as L
    assert len(abi["supports"]) == 2 and len(abi["launched"]) == 2, abi
    if must_support:
        assert abi["supports"] == [1, 1] and abi["launched"] == [L.VARIANT_LDS] * 2, abi   # no silent fall-back to AUTO
    else:
        assert all(s in (0, 1) for s in abi["supports"]), abi
        assert abi["launched"] == [L.VARIANT_LDS if s == 1 else L.VARIANT_AUTO for s in abi["supports"]], abi
    for k in ("color", "depth", "T"):
        assert np.array_equal(strict[k], orc[k]), (k, np.abs(strict[k] - orc[k]).max())
        assert np.array_equal(strict[k], gather[k]), (k, np.abs(strict[k] - gather[k]).max())
    errs = {k: float(np.abs(fast[k] - orc[k]).max()) for k in ("color", "depth", "T")}
    print("default mode", errs)
    assert errs["color"] <= 0.5 * TOL and errs["depth"] <= TOL and errs["T"] <= TOL, errs   # [0,1] colour: half the [-1,1] bar
    assert int(strict["status"][0]) == 0 and int(fast["status"][0]) == 0


# ---- forward cases -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_box_fits_three_dtypes_both_align_corners(abi, dtype, ac, with_bg):
    cfg = dict(seed=1, B=2, D=8, S=96)
    rgba, dhw, ray, eye, zd = _random_case(**cfg)
    spare, never, n = _fit_counts(_boxes(dhw, ray, eye, 96, 96, ac))
    assert n == 288 and spare == n, (spare, never, n)
    rgb, alpha, bg = _parts(rgba, dtype)
    _check(abi, ("fits", dtype, ac, with_bg), rgb, alpha, bg if with_bg else None, dhw, ray, eye, zd, ac)


@pytest.mark.parametrize("T,must", [(80, True), (77, False)])
def test_ragged_image_and_texture_widths(abi, T, must):
    """100 x 100 pixels: the last tile row and column are ragged.  Wt = 80: must be staged; Wt = 77: rows are not 16-byte aligned, the query may say no."""
    rgba, dhw, ray, eye, zd = _random_case(seed=4, B=3, D=7, S=100, T=T)
    spare, never, n = _fit_counts(_boxes(dhw, ray, eye, T, T, True))
    assert spare == n and (T != 77 or n == 588), (spare, never, n)
    rgb, alpha, bg = _parts(rgba)
    for with_bg in (False, True):
        _check(abi, ("ragged", T, with_bg), rgb, alpha, bg if with_bg else None, dhw, ray, eye, zd, True, must_support=must)


def test_padded_rows_of_an_odd_width_are_staged(abi):
    """Wt = 77 inside rows of 80 texels: every base pointer and outer stride is a multiple of 16 bytes, so the query must say yes; the texels of a
    loader item past the end of a row are the neighbour's padding (here: 7.0, far out of range) and must read as zeros padding, unseen by the range check."""
    rgba, dhw, ray, eye, zd = _random_case(seed=4, B=3, D=7, S=100, T=77)
    rgb, alpha, bg = _parts(rgba)
    orc = _oracle(("ragged", 77, True), rgb, alpha, bg, dhw, ray, eye, zd, True, None)
    dev = torch.device(DEV)

    def padded(t):
        buf = torch.full((*t.shape[:-1], 80), 7.0, device=dev)
        buf[..., :77] = t.to(dev)
        return buf[..., :77]
    from ml_gmpi_amd import MPI, _lib as L
    mpi = MPI(variant="lds", strict_order=True, on_out_of_plane="raise")
    with torch.no_grad():
        out = mpi.render_views_shared(padded(rgb), padded(alpha), dhw.to(dev), ray.to(dev), eye.to(dev), zd.to(dev), background=padded(bg),
                                      want_transmittance=True)
    assert abi["supports"] == [1] and abi["launched"] == [L.VARIANT_LDS], abi
    for k in ("color", "depth", "T"):
        assert np.array_equal(out[k].cpu().numpy(), orc[k]), k
    assert int(out["status"][0].item()) == 0


def test_fall_back_is_counted_and_an_unpadded_last_row_is_not_staged(abi):
    """Two launches that ask for "lds" by name and run AUTO's kernel: contiguous Wt = 77 (the query says 0), and Wt = 77 in rows of 80 texels whose
    storage ends with the last texel of the last row (the query sees aligned strides and says 1, but the loader's last item of that row would read
    3 texels behind the allocation).  Both are counted on the module, warned about once, and match the oracle."""
    import ml_gmpi_amd.hip_mpi as hm
    from ml_gmpi_amd import MPI, _lib as L
    rgba, dhw, ray, eye, zd = _random_case(seed=4, B=3, D=7, S=100, T=77)
    rgb, alpha, bg = _parts(rgba)
    orc = _oracle(("ragged", 77, True), rgb, alpha, bg, dhw, ray, eye, zd, True, None)
    dev = torch.device(DEV)

    def tight(t):   # rows of 80 texels, nothing behind the last row's 77th
        n = t.numel() // 77
        flat = torch.full((n * 80 - 3,), 7.0, device=dev)
        strides = [80 * int(np.prod(t.shape[i + 1:-1])) for i in range(t.dim() - 1)] + [1]
        v = flat.as_strided(tuple(t.shape), strides)
        v.copy_(t.to(dev))
        return v
    geo = tuple(t.to(dev) for t in (dhw, ray, eye, zd))
    mpi = MPI(variant="lds", strict_order=True, on_out_of_plane="raise")
    hm._LDS_FALLBACK_WARNED = False
    with torch.no_grad():
        with pytest.warns(RuntimeWarning, match="lds"):
            a = mpi.render_views_shared(rgb.to(dev), alpha.to(dev), *geo, background=bg.to(dev), want_transmittance=True)
        b = mpi.render_views_shared(tight(rgb), tight(alpha), *geo, background=tight(bg), want_transmittance=True)
    assert abi["supports"] == [0, 1] and abi["launched"] == [L.VARIANT_AUTO] * 2, abi
    assert mpi.shared_lds_fallbacks == 2
    for out in (a, b):
        for k in ("color", "depth", "T"):
            assert np.array_equal(out[k].cpu().numpy(), orc[k]), k


def test_staged_and_gathered_planes_in_one_launch(abi):
    cfg = dict(seed=2, B=2, D=12, S=112, T=128, extreme=True)
    rgba, dhw, ray, eye, zd = _random_case(**cfg)
    _, _, cap_w, cap_h = _caps()
    boxes = _boxes(dhw, ray, eye, 128, 128, True)
    fits = (boxes[:, 0] + 3 <= cap_w) & (boxes[:, 1] <= cap_h)
    spare, never, n = _fit_counts(boxes)
    print("mixed case: boxes that fit", fits.mean(), "with spare", spare, "never", never, "of", n)
    assert spare > 0 and never > 0, (spare, never, n)
    rgb, alpha, bg = _parts(rgba)
    for with_bg in (False, True):
        _check(abi, ("mixed", with_bg), rgb, alpha, bg if with_bg else None, dhw, ray, eye, zd, True)


def test_large_boxes_of_tilted_views_fit(abi):
    rgba, dhw, ray, eye, zd = _random_case(seed=31, B=2, D=6, S=128, extreme=True)
    boxes = _boxes(dhw, ray, eye, 128, 128, True)
    _, _, cap_w, cap_h = _caps()
    assert ((boxes[:, 0] + 3 <= cap_w) & (boxes[:, 1] <= cap_h)).all(), (boxes[:, 0].max(), boxes[:, 1].max())
    print("largest box", boxes[:, 0].max(), "x", boxes[:, 1].max())
    rgb, alpha, bg = _parts(rgba)
    _check(abi, ("tilted",), rgb, alpha, bg, dhw, ray, eye, zd, True)


@pytest.mark.parametrize("cfg", [dict(seed=32, B=2, D=5, S=32, T=256), dict(seed=33, B=2, D=7, S=64, T=256)], ids=["S32", "S64"])
def test_no_box_fits_the_whole_launch_gathers_in_the_kernel(abi, cfg):
    rgba, dhw, ray, eye, zd = _random_case(**cfg)
    spare, never, n = _fit_counts(_boxes(dhw, ray, eye, 256, 256, True))
    assert never == n, (spare, never, n)
    rgb, alpha, bg = _parts(rgba)
    _check(abi, ("none", cfg["S"]), rgb, alpha, bg, dhw, ray, eye, zd, True)


def test_one_plane_that_is_the_background(abi):
    rgba, dhw, ray, eye, zd = _random_case(seed=6, B=1, D=1, S=40)
    spare, never, n = _fit_counts(_boxes(dhw, ray, eye, 40, 40, True))
    assert spare == n, (spare, never, n)
    rgb, alpha, bg = _parts(rgba)
    bg = (1.0 - bg).contiguous()   # (rgba[:, -1] IS rgba[:, 0] with one plane: a background that differs from rgb)
    _check(abi, ("one plane",), rgb, alpha, bg, dhw, ray, eye, zd, True)


@pytest.mark.parametrize("grouping", ["uniform", "ragged", "view_to_mpi"])
def test_view_groupings_alpha_view_and_expanded_rgb(abi, grouping):
    rgba, dhw, ray, eye, zd = _random_case(seed=9, B=4, D=6, S=72, T=64)
    rgb, alpha, bg = _parts(rgba[:2])
    dhw = dhw[:2]
    kw, v2m = {"uniform": (dict(views_per_mpi=2), [0, 0, 1, 1]), "ragged": (dict(views_per_mpi=[1, 3]), [0, 1, 1, 1]),
               "view_to_mpi": (dict(view_to_mpi=[1, 0, 0, 1]), [1, 0, 0, 1])}[grouping]
    spare, never, n = _fit_counts(_boxes(dhw, ray, eye, 64, 64, True, v2m=v2m))
    assert n == 360 and spare == n, (spare, never, n)
    rgb = rgb[:1].expand(2, -1, -1, -1)   # stride 0 on the MPI axis
    assert rgb.stride(0) == 0
    _check(abi, ("groupings", grouping), rgb, alpha, bg, dhw, ray, eye, zd, True, v2m=v2m, alpha_as_view=True, **kw)


@pytest.mark.parametrize("D", [97, 193])
def test_more_planes_than_one_table_chunk(abi, D):
    rgba, dhw, ray, eye, zd = _random_case(seed=14, B=1, D=D, S=64, alpha="thin")   # (thin planes: the deep ones still count)
    rgb, alpha, bg = _parts(rgba)
    _check(abi, ("deep", D), rgb, alpha, bg, dhw, ray, eye, zd, True)


# ---- status bits ---------------------------------------------------------------------------------------------------------------------------------
def _lds_status(rgb, alpha, bg, dhw, ray, eye, zd, **kw):
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    t = lambda a: None if a is None else torch.as_tensor(a).to(dev)
    mpi = MPI(variant="lds", on_out_of_plane="raise")
    with torch.no_grad():
        out = mpi.render_views_shared(t(rgb), t(alpha), t(dhw), t(ray), t(eye), t(zd), background=t(bg), defer_status=True, **kw)
    word = int(out["status"][0].item())
    out["status"].zero_()
    return word, out


@pytest.mark.parametrize("where", ["rgb", "background", "alpha"])
def test_out_of_range_value_sets_the_range_bit(abi, where):
    rgba, dhw, ray, eye, zd = _random_case(seed=3, B=1, D=5, S=64)
    rgb, alpha, bg = _parts(rgba)
    assert _lds_status(rgb, alpha, bg, dhw, ray, eye, zd)[0] == 0
    {"rgb": rgb, "background": bg, "alpha": alpha}[where].view(-1, 64, 64)[0, 32, 32] = 1.5   # the image centre: every frontal view samples it
    assert _lds_status(rgb, alpha, bg, dhw, ray, eye, zd)[0] == 2, where
    from ml_gmpi_amd import _lib as L
    assert set(abi["launched"]) == {L.VARIANT_LDS}


@pytest.mark.parametrize("where", ["rgb", "background", "alpha"])
def test_out_of_range_value_sets_the_range_bit_on_the_in_kernel_gather(abi, where):
    """No box fits (test_no_box_fits_...): every tap comes from the direct gather inside the staged kernel, which tests the taps it reads.  Pixels are
    8 texels apart here, so a block of 17 x 17 texels around the centre is poked: some footprint lies in it."""
    rgba, dhw, ray, eye, zd = _random_case(seed=32, B=2, D=5, S=32, T=256)
    spare, never, n = _fit_counts(_boxes(dhw, ray, eye, 256, 256, True))
    assert never == n, (spare, never, n)
    rgb, alpha, bg = _parts(rgba)
    assert _lds_status(rgb, alpha, bg, dhw, ray, eye, zd)[0] == 0
    {"rgb": rgb, "background": bg, "alpha": alpha}[where].view(-1, 256, 256)[0, 120:137, 120:137] = 1.5
    assert _lds_status(rgb, alpha, bg, dhw, ray, eye, zd)[0] == 2, where
    from ml_gmpi_amd import _lib as L
    assert abi["launched"] == [L.VARIANT_LDS] * 2 and abi["supports"] == [1, 1], abi


def test_negative_zero_is_in_range(abi):
    rgba, dhw, ray, eye, zd = _random_case(seed=3, B=1, D=5, S=64)
    rgb, alpha, bg = _parts(rgba)
    for t in (rgb, alpha, bg):
        t.view(-1, 64, 64)[:, 30:34, 30:34] = -0.0
    assert torch.signbit(alpha.view(-1, 64, 64)[0, 32, 32])
    assert _lds_status(rgb, alpha, bg, dhw, ray, eye, zd)[0] == 0
    from ml_gmpi_amd import _lib as L
    assert abi["launched"] == [L.VARIANT_LDS], abi


def test_last_plane_bit_on_the_pose_that_sets_it_today(abi):
    rgba, dhw, ray, eye, zd = _random_case(seed=2, B=2, D=6, S=64, extreme=True)
    dhw = dhw.clone()
    dhw[:, -1, 1:] *= 0.5   # a last plane the tilted rays leave
    rgb, alpha, bg = _parts(rgba)
    assert _lds_status(rgb, alpha, bg, dhw, ray, eye, zd, check_last_plane=True)[0] == 1
    assert _lds_status(rgb, alpha, bg, dhw, ray, eye, zd, check_last_plane=False)[0] == 0
    from ml_gmpi_amd import _lib as L
    assert abi["launched"] == [L.VARIANT_LDS] * 2, abi


def test_bad_view_index_is_clamped_and_reported(abi):
    rgba, dhw, ray, eye, zd = _random_case(seed=9, B=2, D=4, S=64)
    rgb, alpha, bg = _parts(rgba)
    v2m = torch.tensor([0, 5], dtype=torch.int32)
    word, out = _lds_status(rgb, alpha, bg, dhw, ray, eye, zd, view_to_mpi=v2m)
    assert word == 8
    ref = shared_render(rgb, alpha, bg, dhw, ray, eye, zd, variant="lds", view_to_mpi=[0, 1])   # (clamped to the last MPI)
    assert np.array_equal(out["color"].cpu().numpy(), ref["color"])


# ---- other checks --------------------------------------------------------------------------------------------------------------------------------
def test_nan_ray_component_gives_the_gather_kernels_pixels(abi):
    rgba, dhw, ray, eye, zd = _random_case(seed=1, B=2, D=8, S=96)
    rgb, alpha, bg = _parts(rgba)
    ray = ray.clone()
    ray[0, 0, 50, 41] = float("nan")      # inside a tile: that pixel alone
    ray[1, 2, 0, 0] = float("nan")        # a tile corner: the tile's boxes do not fit
    for strict in (True, False):
        a = shared_render(rgb, alpha, bg, dhw, ray, eye, zd, variant="lds", strict=strict)
        b = shared_render(rgb, alpha, bg, dhw, ray, eye, zd, variant="gather", strict=strict)
        for k in ("color", "depth", "T"):
            assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k
            assert np.array_equal(a[k], b[k], equal_nan=True), (k, strict)
        assert np.isnan(a["depth"][0, 0, 50, 41]) and int(np.isnan(a["depth"]).sum()) == 2
        assert int(a["status"][0]) == 0


def test_raw_abi_accepts_lds_and_still_refuses_wave_and_band():
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    dev = torch.device(DEV)
    rgba, dhw, ray, eye, zd = _random_case(seed=3, B=1, D=3, S=32)
    rgb, alpha, bg = (t.to(dev) for t in _parts(rgba))
    dhw, ray, eye, zd = (t.to(dev).float().contiguous() for t in (dhw, ray, eye, zd))
    color, depth = torch.empty((1, 3, 32, 32), device=dev), torch.empty((1, 1, 32, 32), device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    p = L.GmpiRenderParams()
    p.struct_size = ctypes.sizeof(L.GmpiRenderParams)
    p.flags, p.rgba_dtype = L.FLAG_ALIGN_CORNERS | L.FLAG_STRICT_ORDER, L.DTYPE_F32
    p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = 1, 1, 3, 32, 32, 32, 32, 1
    p.rgba = alpha.data_ptr()
    for i, s in enumerate(alpha.stride()):
        p.rgba_stride[i] = s
    p.dhw, p.ray_dir, p.eye_pos, p.z_dir = dhw.data_ptr(), ray.data_ptr(), eye.data_ptr(), zd.data_ptr()
    p.rgb_out, p.depth_out, p.status = color.data_ptr(), depth.data_ptr(), status.data_ptr()
    s = L.GmpiSharedColor()
    s.struct_size = ctypes.sizeof(L.GmpiSharedColor)
    s.rgb, s.background = rgb.data_ptr(), bg.data_ptr()
    for i in range(3):
        s.rgb_stride[i], s.background_stride[i] = rgb.stride(i), bg.stride(i)
    results = {}
    for name in ("gather", "lds", "auto"):
        p.variant = L.VARIANTS[name]
        assert lib.gmpi_render_shared_supports(ctypes.byref(p), ctypes.byref(s)) == 1, name
        assert lib.gmpi_mpi_render_shared_launch(ctypes.byref(p), ctypes.byref(s), None) == 0, name   # (the parent commit: -6 for "lds")
        torch.cuda.synchronize()
        results[name] = (color.clone(), depth.clone())
    assert torch.equal(results["lds"][0], results["gather"][0]) and torch.equal(results["lds"][1], results["gather"][1])
    for name in ("wave", "band"):
        p.variant = L.VARIANTS[name]
        assert lib.gmpi_mpi_render_shared_launch(ctypes.byref(p), ctypes.byref(s), None) == -6, name
        assert lib.gmpi_render_shared_supports(ctypes.byref(p), ctypes.byref(s)) == -6, name
    # an unaligned base pointer: the query says 0 for LDS and the launch refuses; AUTO still takes it
    p.variant = L.VARIANT_LDS
    p.rgba = alpha.data_ptr() + 4
    assert lib.gmpi_render_shared_supports(ctypes.byref(p), ctypes.byref(s)) == 0
    assert lib.gmpi_mpi_render_shared_launch(ctypes.byref(p), ctypes.byref(s), None) == -6
    p.D = 0
    assert lib.gmpi_render_shared_supports(ctypes.byref(p), ctypes.byref(s)) == -2
    assert lib.gmpi_render_shared_supports(None, ctypes.byref(s)) == -1
    # the backward entry knows AUTO and GATHER only, as before: LDS is refused before anything else is looked at
    p.rgba, p.D, p.variant = alpha.data_ptr(), 3, L.VARIANT_LDS
    nul = [None] * 9
    assert lib.gmpi_mpi_render_shared_backward_launch(ctypes.byref(p), ctypes.byref(s), *nul, None) == -6
    p.variant = L.VARIANT_AUTO
    assert lib.gmpi_mpi_render_shared_backward_launch(ctypes.byref(p), ctypes.byref(s), *nul, None) == -1   # (no gradients given)
    assert lib.gmpi_query(0) == 2 and lib.gmpi_query(12) == 32 and lib.gmpi_query(13) >= 36 and lib.gmpi_query(14) >= 19
    assert int(status[0].item()) == 0


def test_transmittance_out_pm1_and_caller_outputs_behave_as_with_gather(abi):
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    rgba, dhw, ray, eye, zd = _random_case(seed=1, B=2, D=8, S=96)
    rgb, alpha, bg = (t.to(dev) for t in _parts(rgba))
    geo = tuple(t.to(dev) for t in (dhw, ray, eye, zd))
    res = {}
    for variant in ("lds", "gather"):
        mpi = MPI(variant=variant, strict_order=True, on_out_of_plane="raise")
        out = dict(color=torch.full((2, 3, 96, 96), -7.0, device=dev), depth=torch.full((2, 1, 96, 96), -7.0, device=dev),
                   T=torch.full((2, 1, 96, 96), -7.0, device=dev))
        with torch.no_grad():
            plain = mpi.render_views_shared(rgb, alpha, *geo, background=bg)
            full = mpi.render_views_shared(rgb, alpha, *geo, background=bg, want_transmittance=True, out_pm1=True, out=out)
        assert plain["T"] is None
        assert full["color"] is out["color"] and full["depth"] is out["depth"] and full["T"] is out["T"]
        assert torch.equal(full["color"], 2.0 * plain["color"] - 1.0) and torch.equal(full["depth"], plain["depth"])
        res[variant] = (plain, full)
    for a, b in zip(res["lds"], res["gather"]):
        for k in ("color", "depth", "T"):
            assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k
    # the per-call variant overrides the module's own
    mpi = MPI(variant="gather", strict_order=True, on_out_of_plane="raise")
    abi["launched"].clear()
    with torch.no_grad():
        o = mpi.render_views_shared(rgb, alpha, *geo, background=bg, variant="lds")
        mpi.render_views_shared(rgb, alpha, *geo, background=bg, variant=None)
    from ml_gmpi_amd import _lib as L
    assert abi["launched"] == [L.VARIANT_LDS, L.VARIANT_GATHER]
    assert torch.equal(o["color"], res["lds"][0]["color"])


def test_autograd_through_the_staged_forward_gives_autos_gradients(abi):
    rgba, dhw, ray, eye, zd = _random_case(seed=1, B=2, D=8, S=96)
    parts = _parts(rgba)
    g = np.random.default_rng(5)
    gc, gd, gT = (g.standard_normal((2, c, 96, 96)).astype(np.float32) for c in (3, 1, 1))
    got = {}
    for variant in ("lds", "auto"):
        ins, out = _hip_grads(parts, dhw, ray, eye, zd, 1, gc, gd, gT, True, variant)
        got[variant] = ([i.grad.double().cpu().numpy() for i in ins], out)
    from ml_gmpi_amd import _lib as L
    assert abi["launched"] == [L.VARIANT_LDS, L.VARIANT_AUTO], abi
    for x, y in zip(got["lds"][0], got["auto"][0]):
        assert float(np.abs(y).max()) > 0
        assert np.abs(x - y).max() <= 1e-5 * np.abs(y).max() + 1e-7
    for k in ("color", "depth", "T"):
        assert float((got["lds"][1][k] - got["auto"][1][k]).abs().max()) <= TOL
