"""GPU tests of the window forward of the depth-alpha layout (`depth_forward="window"` of `MPI.render_views_depth`, render_depth_window.hip): per
32 x 16 pixel tile one window of rgb and depth texels in LDS that moves with the tile's texel boxes.  The yardsticks are `oracle.render` on
`expand_depth_alpha(...)` and the one-pixel kernel (`depth_forward="pixel"`), whose bits the window kernel must give in both modes.
Run on the MI355X box:  python -m pytest tests -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from test_hip_depth_alpha import _case, _check_forward, _expand, _hip_grads, depth_render  # noqa: F401
from test_hip_parity import TOL, _random_case  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TW, TH = 32, 16   # the pixel tile (kTileW, kTileH)
KEYS = ("color", "depth", "T")


def _window():
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    assert lib.gmpi_query(25) == 1
    return lib.gmpi_query(26), lib.gmpi_query(27), lib.gmpi_query(28)


# ---- the box rule and the window's moves, restated in float64 ------------------------------------------------------------------------------------
def _boxes(dhw, ray, eye, Ht, Wt, ac=True, v2m=None):
    """[view, tile, plane] -> (x, y, nx, ny) of the texel box the tile's four corner pixels span: 1/64 texel of slack, the tap to the right of /
    below the last corner included; nx = 0 where it is not staged -- corners that are not finite, or a box that, widened to whole items of 4
    texels, exceeds the window.  float64 restatement of plane_coord and tile_box."""
    cw, ch, _ = _window()
    dhw, ray, eye = (np.asarray(a, dtype=np.float64) for a in (dhw, ray, eye))
    N, _, H, W = ray.shape
    out = []
    for n in range(N):
        m = n if v2m is None else v2m[n]
        tiles = []
        for y0 in range(0, H, TH):
            for x0 in range(0, W, TW):
                ys, xs = [y0, min(y0 + TH - 1, H - 1)], [x0, min(x0 + TW - 1, W - 1)]
                r = ray[n][:, ys][:, :, xs].reshape(3, 4)                  # the four corner rays
                planes = []
                for d, ph, pw in dhw[m]:
                    with np.errstate(all="ignore"):
                        s = (d - eye[n, 2]) / r[2]
                        u, v = 2 * (eye[n, 0] + r[0] * s) / pw, 2 * (eye[n, 1] + r[1] * s) / ph
                        if ac:
                            ix, iy = (u + 1) * (Wt - 1) / 2, (v + 1) * (Ht - 1) / 2
                        else:
                            u = np.where((u >= -1) & (u <= 1), u * 0.95, u)
                            v = np.where((v >= -1) & (v <= 1), v * 0.95, v)
                            ix, iy = ((u + 1) * Wt - 1) / 2, ((v + 1) * Ht - 1) / 2
                    if not (np.all(np.abs(ix) < 1e6) and np.all(np.abs(iy) < 1e6)):
                        planes.append((0, 0, 0, 0))
                        continue
                    x, y = int(np.floor(ix.min() - 1 / 64)), int(np.floor(iy.min() - 1 / 64))
                    nx, ny = int(np.floor(ix.max() + 1 / 64)) + 2 - x, int(np.floor(iy.max() + 1 / 64)) + 2 - y
                    fits = ny <= ch and -(-(x + nx) // 4) * 4 - (x // 4) * 4 <= cw
                    planes.append((x, y, nx if fits else 0, ny))
                tiles.append(planes)
        out.append(tiles)
    return np.array(out)


def _loads(bb, background):
    """bb [D, 4] of one tile -> the number of whole-window loads of the kernel's front-to-back sweep (the reload of the colour channels before a
    background plane is not one)."""
    cw, ch, chunk = _window()
    D = len(bb)
    wx0 = wy0 = dx = dy = 0
    is_open, count = False, 0
    for k in range(D):
        x, y, nx, ny = (int(v) for v in bb[k])
        if nx == 0:
            continue
        if not (is_open and x >= wx0 and y >= wy0 and x + nx <= wx0 + cw and y + ny <= wy0 + ch):
            ahead = [b for b in bb[k + 1:min(k - k % chunk + chunk, D)] if b[2] > 0]   # the drift: towards the next staged box of the table chunk
            if ahead:
                ddx, ddy = 2 * int(ahead[0][0]) + int(ahead[0][2]) - (2 * x + nx), 2 * int(ahead[0][1]) + int(ahead[0][3]) - (2 * y + ny)
                dx, dy = ddx or dx, ddy or dy
            wx0 = -(-(x + nx) // 4) * 4 - cw if dx < 0 else (x // 4) * 4
            wy0 = y + ny - ch if dy < 0 else y
            is_open = True
            count += 1
    return count


def _replay(dhw, ray, eye, Ht, Wt, ac=True, v2m=None, background=True):
    """(boxes, staged boxes, window loads per tile [views x tiles], tiles with staged AND unstaged planes)."""
    bb = _boxes(dhw, ray, eye, Ht, Wt, ac, v2m)
    tiles = bb.reshape(-1, bb.shape[2], 4)
    loads = np.array([_loads(t, background) for t in tiles])
    staged = tiles[:, :, 2] > 0
    mixed = int((staged.any(1) & ~staged.all(1)).sum())
    return staged.size, int(staged.sum()), loads, mixed


# ---- spies on the C ABI: which entry ran, what the support query said ----------------------------------------------------------------------------
@pytest.fixture
def abi(monkeypatch):
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    real = {n: getattr(lib, n) for n in ("gmpi_mpi_render_depth_window_launch", "gmpi_render_depth_window_supports", "gmpi_mpi_render_depth_launch")}
    seen = dict(launched=[], supports=[])

    def window(p, sc, da, stream):
        seen["launched"].append("window")
        return real["gmpi_mpi_render_depth_window_launch"](p, sc, da, stream)

    def pixel(p, sc, da, stream):
        seen["launched"].append("pixel")
        return real["gmpi_mpi_render_depth_launch"](p, sc, da, stream)

    def supports(p, sc, da):
        rc = real["gmpi_render_depth_window_supports"](p, sc, da)
        seen["supports"].append(rc)
        if rc == 0:   # what the query refuses, the explicit launch refuses too
            assert real["gmpi_mpi_render_depth_window_launch"](p, sc, da, None) == -6
        return rc
    monkeypatch.setattr(lib, "gmpi_mpi_render_depth_window_launch", window)
    monkeypatch.setattr(lib, "gmpi_mpi_render_depth_launch", pixel)
    monkeypatch.setattr(lib, "gmpi_render_depth_window_supports", supports)
    return seen


def render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, *, how="window", ac=True, strict=False, views_per_mpi=1, view_to_mpi=None,
           check_last=False, range_check="touched", out_pm1=False, defer_status=False, on_device=False, mpi=None):
    """test_hip_depth_alpha.depth_render with `depth_forward`; on_device: the three images are device tensors already (views, padded rows)."""
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    t = lambda a: None if a is None else torch.as_tensor(a).to(dev)
    img = (lambda a: a) if on_device else t
    mpi = mpi or MPI(align_corners=ac, strict_order=strict, range_check=range_check, on_out_of_plane="raise")
    v2m = None if view_to_mpi is None else torch.as_tensor(np.asarray(view_to_mpi, dtype=np.int32)).to(dev)
    with torch.no_grad():
        out = mpi.render_views_depth(img(rgb), img(depth), t(plane_z), zb, t(dhw), t(ray), t(eye), t(zd), background=img(bg), views_per_mpi=views_per_mpi,
                                     view_to_mpi=v2m, check_last_plane=check_last, want_transmittance=True, out_pm1=out_pm1, defer_status=defer_status,
                                     depth_forward=how)
    torch.cuda.synchronize()
    res = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    if defer_status:
        out["status"].zero_()
    return res


_ORACLE = {}


def _oracle(key, case, bg_on, ac, v2m=None):
    if key not in _ORACLE:
        rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = case
        _ORACLE[key] = oracle.render(_expand(rgb, depth, plane_z, bg if bg_on else None, zb).numpy(), dhw, ray, eye, zd, view_to_mpi=v2m, align_corners=ac,
                                     threads=True)
    return _ORACLE[key]


def _check(abi, key, case, bg_on=True, ac=True, v2m=None, must_support=True, **kw):
    """Strict mode: the oracle's bits and the one-pixel kernel's; default mode: the one-pixel kernel's bits, within the bars of the oracle."""
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = case
    bg = bg if bg_on else None
    orc = _oracle(key, case, bg_on, ac, v2m)
    got = {}
    for strict in (True, False):
        pixel = render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, how="pixel", ac=ac, strict=strict, **kw)
        abi["launched"].clear(), abi["supports"].clear()
        window = render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, how="window", ac=ac, strict=strict, **kw)
        assert len(abi["supports"]) == 1 and len(abi["launched"]) == 1, abi
        if must_support:
            assert abi["supports"] == [1] and abi["launched"] == ["window"], abi   # no silent fall-back
        else:
            assert abi["launched"] == ["window" if abi["supports"] == [1] else "pixel"], abi
        for k in KEYS:
            assert np.array_equal(window[k], pixel[k]), (k, strict, np.abs(window[k] - pixel[k]).max())
        assert int(window["status"][0]) == 0 and int(pixel["status"][0]) == 0
        got[strict] = window
    for k in KEYS:
        assert np.array_equal(got[True][k], orc[k]), (k, np.abs(got[True][k] - orc[k]).max())
    errs = {k: float(np.abs(got[False][k] - orc[k]).max()) for k in KEYS}
    print("default mode", errs)
    assert errs["color"] <= 0.5 * TOL and errs["depth"] <= TOL and errs["T"] <= TOL, errs   # [0,1] colour: half the [-1,1] bar
    return got


# ---- forward cases -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_box_is_staged_three_dtypes_both_align_corners(abi, dtype, ac, with_bg):
    cfg = dict(seed=1, B=2, D=8, S=96, n_z_bins=4)
    case = _case(dtype=dtype, **cfg)
    n, staged, loads, _ = _replay(case[4], case[5], case[6], 96, 96, ac)
    print("window loads per tile: min", loads.min(), "mean", loads.mean(), "max", loads.max())
    assert n == 288 and staged == n and loads.min() >= 1 and loads.max() > 1, (n, staged, loads)   # every box staged; tiles that re-anchor
    _check(abi, ("fits", dtype, ac, with_bg), case, with_bg, ac)


def test_ragged_tiles_and_an_odd_texture_width(abi):
    """100 x 100 pixels: the last tile row and column are ragged.  Wt = 77, contiguous: rows are not 16-byte aligned, the query may say no -- the spy
    and the counter must agree."""
    from ml_gmpi_amd import MPI
    case = _case(seed=4, B=3, D=7, S=100, T=77, n_z_bins=32)
    n, staged, loads, _ = _replay(case[4], case[5], case[6], 77, 77)
    assert n == 588 and staged == n and loads.min() >= 1, (n, staged, loads)
    _check(abi, ("ragged", 77), case, must_support=False)
    mpi = MPI(strict_order=True, on_out_of_plane="raise")
    abi["launched"].clear(), abi["supports"].clear()
    render(*case, mpi=mpi)
    assert mpi.depth_window_fallbacks == abi["launched"].count("pixel") == abi["supports"].count(0)


def test_padded_rows_of_an_odd_width_must_be_staged(abi):
    """Wt = 77 inside rows of 80 texels: every base pointer and outer stride is a multiple of 16 bytes, so the query must say yes; the texels of a
    loader item past the end of a row are the row's padding (here: 7.0 resp. NaN, far out of range) and must read as zeros padding."""
    case = _case(seed=4, B=3, D=7, S=100, T=77, n_z_bins=32)
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = case
    orc = _oracle(("ragged", 77), case, True, True)
    dev = torch.device(DEV)

    def padded(t, fill):
        buf = torch.full((*t.shape[:-1], 80), fill, device=dev)
        buf[..., :77] = t.to(dev)
        return buf[..., :77]
    out = render(padded(rgb, 7.0), padded(depth, float("nan")), plane_z, padded(bg, 7.0), dhw, ray, eye, zd, zb, strict=True, on_device=True)
    assert abi["supports"] == [1] and abi["launched"] == ["window"], abi
    for k in KEYS:
        assert np.array_equal(out[k], orc[k]), k
    assert int(out["status"][0]) == 0


@pytest.mark.parametrize("n_z_bins", [4, 256])
def test_every_tile_re_anchors_under_tilted_views(abi, n_z_bins):
    case = _case(seed=8, B=2, D=16, S=256, n_z_bins=n_z_bins, extreme=True)
    n, staged, loads, _ = _replay(case[4], case[5], case[6], 256, 256)
    print("window loads per tile: min", loads.min(), "mean", loads.mean(), "max", loads.max(), "staged", staged, "of", n)
    assert loads.size == 256 and loads.min() >= 4 and loads.mean() >= 6 and loads.max() <= 16, loads   # every tile re-anchors, at least three times
    _check(abi, ("tilted", n_z_bins), case)


def test_staged_and_unstaged_planes_in_every_tile(abi):
    case = _case(seed=2, B=2, D=6, S=64, T=120, n_z_bins=4, extreme=True)
    n, staged, loads, mixed = _replay(case[4], case[5], case[6], 120, 120)
    print("staged", staged, "of", n, "tiles with both", mixed, "of", loads.size)
    assert n == 96 and 0 < staged < n and mixed == loads.size == 16, (n, staged, mixed)
    _check(abi, ("mixed",), case)


def test_nothing_fits_the_whole_launch_gathers_in_the_kernel(abi):
    case = _case(seed=3, B=2, D=6, S=64, T=256, n_z_bins=4)
    n, staged, loads, _ = _replay(case[4], case[5], case[6], 256, 256)
    assert n == 96 and staged == 0 and loads.max() == 0, (n, staged)
    _check(abi, ("none",), case)


def test_one_plane_that_is_the_background(abi):
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = _case(seed=6, B=1, D=1, S=40, n_z_bins=4)
    n, staged, loads, _ = _replay(dhw, ray, eye, 40, 40)
    assert staged == n and loads.min() == loads.max() == 1, (n, staged, loads)
    bg = (1.0 - bg).contiguous()   # (with one plane the case's background IS its rgb: a background that differs)
    plane_z = torch.ones(1)        # (the case's one plane lies at 0, in front of the surface: behind it, so that the plane is seen)
    got = _check(abi, ("one plane",), (rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb))
    other = render(rgb, depth, plane_z, None, dhw, ray, eye, zd, zb, strict=True)
    assert float(got[True]["color"].max()) > 0.5 and not np.array_equal(other["color"], got[True]["color"])   # (the background's colour was rendered)


@pytest.mark.parametrize("chunks", [1, 2])
def test_more_planes_than_one_table_chunk(abi, chunks):
    D = chunks * _window()[2] + 1
    case = _case(seed=13, B=2, D=D, S=48, n_z_bins=4)
    n, staged, loads, _ = _replay(case[4], case[5], case[6], 48, 48)
    assert staged == n, (n, staged)
    _check(abi, ("deep", D), case)


# ---- the tile-level plane skip ---------------------------------------------------------------------------------------------------------------------
def _step_case():
    return _case(seed=1, B=2, D=32, S=96, n_z_bins=256)   # step-like ramp: most planes lie in front of the surface


def test_plane_skip_step_like_ramp(abi):
    case = _step_case()
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = case
    from ml_gmpi_amd.depth_alpha import ramp_constants
    lo = ramp_constants(*zb)[0]
    in_front = float((plane_z.reshape(-1, 1) - float(depth.min()) <= lo).float().mean())
    print("planes in front of every texel:", in_front)
    assert in_front >= 0.1   # some planes are skipped for every tile, many more per tile
    for with_bg in (True, False):
        _check(abi, ("steps", with_bg), case, with_bg)


def test_plane_skip_keeps_the_last_plane_check(abi):
    """The pose and the shrunken last plane of test_check_last_plane_sets_bit_one...: bit 1, the same word as the one-pixel kernel, although the
    sampling of that plane is skipped where the window lies in front of its ramp."""
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = _case(seed=2, B=2, D=6, S=64, n_z_bins=256, extreme=True)
    dhw = dhw.clone()
    dhw[:, -1, 1:] *= 0.5   # a last plane the tilted rays leave
    depth = depth + 2.0     # the surface lies behind every plane: every staged plane is skipped
    res = {}
    for how in ("pixel", "window"):
        on = render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, how=how, check_last=True, defer_status=True)
        off = render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, how=how, check_last=False, defer_status=True)
        assert int(off["status"][0]) == 0
        res[how] = on
    assert int(res["window"]["status"][0]) == int(res["pixel"]["status"][0]) == 1
    for k in KEYS:
        assert np.array_equal(res["window"][k], res["pixel"][k]), k
    assert "window" in abi["launched"]
    step = _step_case()
    a, b = (render(*step, how=how, check_last=True, defer_status=True) for how in ("pixel", "window"))
    assert int(a["status"][0]) == int(b["status"][0]) and all(np.array_equal(a[k], b[k]) for k in KEYS)


def test_a_nan_depth_texel_disables_the_skip_and_sets_the_range_bit(abi):
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = _step_case()
    depth = depth.clone()
    depth.view(-1, 96, 96)[:, 48, 48] = float("nan")   # the image centre
    for strict in (True, False):
        a = render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, how="pixel", strict=strict, defer_status=True)
        b = render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, how="window", strict=strict, defer_status=True)
        for k in KEYS:
            assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k
            assert np.array_equal(a[k], b[k], equal_nan=True), (k, strict)
        assert np.isnan(a["color"]).any()
        assert int(a["status"][0]) == int(b["status"][0]) == 2
    assert abi["launched"].count("window") == 2


# ---- status bits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["rgb", "background"])
@pytest.mark.parametrize("fits", [True, False], ids=["staged", "nothing_fits"])
def test_out_of_range_colour_sets_the_range_bit(abi, where, fits):
    cfg = dict(seed=3, B=1, D=5, S=64, n_z_bins=4) if fits else dict(seed=3, B=2, D=6, S=64, T=256, n_z_bins=4)
    T = 64 if fits else 256
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = (t.clone() if isinstance(t, torch.Tensor) else t for t in _case(**cfg))
    n, staged, _, _ = _replay(dhw, ray, eye, T, T)
    assert staged == (n if fits else 0)
    assert int(render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, defer_status=True)["status"][0]) == 0
    if where == "background":
        depth = depth * 0.0 + 2.0   # the surface behind every plane but the last one's ramp end: only the background plane is blended
        plane_z = plane_z.clone()
        plane_z[-1] = 3.0
    lo_, hi_ = (T // 2, T // 2 + 1) if fits else (T // 2 - 8, T // 2 + 9)   # (pixels are 4 texels apart when nothing fits: a block of texels)
    {"rgb": rgb, "background": bg}[where].view(-1, T, T)[0, lo_:hi_, lo_:hi_] = 1.5
    a = render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, how="pixel", defer_status=True)
    b = render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, how="window", defer_status=True)
    assert int(a["status"][0]) == int(b["status"][0]) == 2, where
    assert abi["launched"][-1] == "window" and all(np.array_equal(a[k], b[k]) for k in KEYS)


def test_negative_zero_is_in_range(abi):
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = (t.clone() if isinstance(t, torch.Tensor) else t for t in _case(seed=3, B=1, D=5, S=64, n_z_bins=4))
    for t in (rgb, bg):
        t.view(-1, 64, 64)[:, 30:34, 30:34] = -0.0
    assert torch.signbit(rgb.view(-1, 64, 64)[0, 32, 32])
    assert int(render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, defer_status=True)["status"][0]) == 0
    assert abi["launched"] == ["window"], abi


def test_bad_view_index_is_clamped_and_reported(abi):
    case = _case(seed=9, B=2, D=4, S=64, n_z_bins=4)
    out = render(*case, view_to_mpi=[0, 5], defer_status=True)
    assert int(out["status"][0]) == 8
    ref = render(*case, view_to_mpi=[0, 1])   # (clamped to the last MPI)
    assert np.array_equal(out["color"], ref["color"]) and abi["launched"] == ["window"] * 2


# ---- other checks --------------------------------------------------------------------------------------------------------------------------------
def test_nan_ray_component_gives_the_one_pixel_kernels_pixels(abi):
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = _case(seed=1, B=2, D=8, S=96, n_z_bins=4)
    ray = ray.clone()
    ray[0, 0, 50, 41] = float("nan")      # inside a tile: that pixel alone
    ray[1, 2, 0, 0] = float("nan")        # a tile corner: the tile's boxes are not staged
    for strict in (True, False):
        a = render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, how="window", strict=strict)
        b = render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, how="pixel", strict=strict)
        for k in KEYS:
            assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k
            assert np.array_equal(a[k], b[k], equal_nan=True), (k, strict)
        assert int(a["status"][0]) == 0
    assert abi["launched"].count("window") == 2


def test_a_ray_field_that_is_no_pinholes_gives_the_one_pixel_kernels_pixels(abi):
    """Rows of rays swapped inside tiles: those pixels' footprints leave the window and their rays leave the corner rays' range, so they take the
    taps from global memory and every plane, skipped for the tile or not."""
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = _step_case()
    ray = ray.clone()
    ray[:, :, 20] = ray[:, :, 90].clone()
    ray[:, :, 70, 10:50] = ray[:, :, 3, 40:80].clone()
    for strict in (True, False):
        a = render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, how="window", strict=strict)
        b = render(rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb, how="pixel", strict=strict)
        assert all(np.array_equal(a[k], b[k]) for k in KEYS), strict
    assert abi["launched"].count("window") == 2


@pytest.mark.parametrize("grouping", ["uniform", "ragged", "view_to_mpi"])
def test_view_groupings_a_strided_depth_view_expanded_rgb_and_a_plane_table_per_mpi(abi, grouping):
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = _case(seed=9, B=4, D=6, S=72, n_z_bins=4, T=64, M=2)
    kw, v2m = {"uniform": (dict(views_per_mpi=2), [0, 0, 1, 1]), "ragged": (dict(views_per_mpi=[1, 3]), [0, 1, 1, 1]),
               "view_to_mpi": (dict(view_to_mpi=[1, 0, 0, 1]), [1, 0, 0, 1])}[grouping]
    n, staged, _, _ = _replay(dhw, ray, eye, 64, 64, v2m=v2m)
    assert n == 360 and staged == n, (n, staged)
    dev = torch.device(DEV)
    table = torch.stack([plane_z, plane_z * 0.9 + 0.03])
    rgb1 = rgb[:1].expand(2, -1, -1, -1)   # stride 0 on the MPI axis
    from ml_gmpi_amd import expand_depth_alpha
    orc = oracle.render(expand_depth_alpha(rgb1, depth, table, *zb, bg).numpy(), dhw, ray, eye, zd, view_to_mpi=v2m, threads=True)
    rgbd = torch.cat((rgb.to(dev), depth.to(dev)), 1)
    depth_v, rgb_v = rgbd[:, 3:], rgbd[:1, :3].expand(2, -1, -1, -1)
    assert not depth_v.is_contiguous() and rgb_v.stride(0) == 0
    got = render(rgb_v, depth_v, table, bg.to(dev), dhw, ray, eye, zd, zb, strict=True, on_device=True, **kw)
    assert abi["supports"] == [1] and abi["launched"] == ["window"], abi
    for k in KEYS:
        assert np.array_equal(got[k], orc[k]), k
    assert int(got["status"][0]) == 0


def test_transmittance_out_pm1_and_caller_outputs_behave_as_with_pixel(abi):
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = _case(seed=1, B=2, D=8, S=96, n_z_bins=4)
    rgb, depth, plane_z, bg, dhw, ray, eye, zd = (t.to(dev) for t in (rgb, depth, plane_z, bg, dhw, ray, eye, zd))
    res = {}
    for how in ("window", "pixel"):
        mpi = MPI(strict_order=True, on_out_of_plane="raise")
        out = dict(color=torch.full((2, 3, 96, 96), -7.0, device=dev), depth=torch.full((2, 1, 96, 96), -7.0, device=dev),
                   T=torch.full((2, 1, 96, 96), -7.0, device=dev))
        with torch.no_grad():
            plain = mpi.render_views_depth(rgb, depth, plane_z, zb, dhw, ray, eye, zd, background=bg, depth_forward=how)
            full = mpi.render_views_depth(rgb, depth, plane_z, zb, dhw, ray, eye, zd, background=bg, want_transmittance=True, out_pm1=True, out=out,
                                          depth_forward=how)
        assert plain["T"] is None
        assert full["color"] is out["color"] and full["depth"] is out["depth"] and full["T"] is out["T"]
        assert torch.equal(full["color"], 2.0 * plain["color"] - 1.0) and torch.equal(full["depth"], plain["depth"])
        res[how] = (plain, full)
    for a, b in zip(res["window"], res["pixel"]):
        for k in KEYS:
            assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k
    assert abi["launched"] == ["window", "window", "pixel", "pixel"]


@pytest.mark.parametrize("depth_backward", ["pixel", "tile"])
def test_autograd_through_the_window_forward(abi, depth_backward):
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    case = _case(seed=5, B=4, D=8, S=64, n_z_bins=4, M=2)
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = case
    g = np.random.default_rng(5)
    ups = [torch.as_tensor(g.standard_normal((4, c, 64, 64)).astype(np.float32)).to(dev) for c in (3, 1, 1)]
    t = lambda a: a.to(dev)
    got = {}
    for how in ("window", "pixel"):
        ins = [t(p).clone().requires_grad_(True) for p in (rgb, depth, bg)]
        out = MPI(on_out_of_plane="raise").render_views_depth(ins[0], ins[1], t(plane_z), zb, t(dhw), t(ray), t(eye), t(zd), background=ins[2],
                                                              views_per_mpi=2, want_transmittance=True, depth_forward=how,
                                                              depth_backward=depth_backward if how == "window" else "pixel")
        sum((out[k] * u).sum() for k, u in zip(KEYS, ups)).backward()
        torch.cuda.synchronize()
        got[how] = ([i.grad.double().cpu().numpy() for i in ins], {k: out[k].detach().clone() for k in KEYS})
    assert abi["launched"] == ["window", "pixel"], abi
    for x, y in zip(got["window"][0], got["pixel"][0]):   # the all-pixel path
        assert float(np.abs(y).max()) > 0
        assert np.abs(x - y).max() <= 1e-5 * np.abs(y).max() + 1e-7
    for k in KEYS:
        assert torch.equal(got["window"][1][k], got["pixel"][1][k]), k


def test_raw_abi_auto_and_gather_through_the_new_entry_and_the_refusals():
    from ml_gmpi_amd import _lib as L
    from ml_gmpi_amd.depth_alpha import ramp_constants
    lib = L.load_library()
    dev = torch.device(DEV)
    rgb, depth, plane_z, bg, dhw, ray, eye, zd, zb = _case(seed=3, B=1, D=3, S=32, n_z_bins=4)
    rgb, depth, bg = (t.to(dev) for t in (rgb, depth, bg))
    dhw, ray, eye, zd, plane_z = (t.to(dev).float().contiguous() for t in (dhw, ray, eye, zd, plane_z))
    color, dep = torch.empty((1, 3, 32, 32), device=dev), torch.empty((1, 1, 32, 32), device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    p = L.GmpiRenderParams()
    p.struct_size = ctypes.sizeof(L.GmpiRenderParams)
    p.flags, p.rgba_dtype = L.FLAG_ALIGN_CORNERS | L.FLAG_STRICT_ORDER, L.DTYPE_F32
    p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = 1, 1, 3, 32, 32, 32, 32, 1
    p.rgba = depth.data_ptr()
    p.rgba_stride[:] = [32 * 32, 0, 0, 32, 1]
    p.dhw, p.ray_dir, p.eye_pos, p.z_dir = dhw.data_ptr(), ray.data_ptr(), eye.data_ptr(), zd.data_ptr()
    p.rgb_out, p.depth_out, p.status = color.data_ptr(), dep.data_ptr(), status.data_ptr()
    s = L.GmpiSharedColor()
    s.struct_size = ctypes.sizeof(L.GmpiSharedColor)
    s.rgb, s.background = rgb.data_ptr(), bg.data_ptr()
    for i in range(3):
        s.rgb_stride[i], s.background_stride[i] = rgb.stride(i), bg.stride(i)
    d = L.GmpiDepthAlpha()
    d.struct_size = ctypes.sizeof(L.GmpiDepthAlpha)
    d.plane_z, d.plane_z_stride = plane_z.data_ptr(), 0
    d.z_lo, d.z_hi, d.z_den = ramp_constants(*zb)
    args = (ctypes.byref(p), ctypes.byref(s), ctypes.byref(d))
    results = {}
    for name, entry in (("old", lib.gmpi_mpi_render_depth_launch), ("gather", lib.gmpi_mpi_render_depth_window_launch),
                        ("auto", lib.gmpi_mpi_render_depth_window_launch)):
        p.variant = L.VARIANT_GATHER if name == "gather" else L.VARIANT_AUTO
        color.fill_(-7.0), dep.fill_(-7.0)
        assert lib.gmpi_render_depth_window_supports(*args) == 1, name
        assert entry(*args, None) == 0, name
        torch.cuda.synchronize()
        results[name] = (color.clone(), dep.clone())
    for name in ("gather", "auto"):
        assert torch.equal(results[name][0], results["old"][0]) and torch.equal(results[name][1], results["old"][1]), name
    assert float(results["auto"][0].min()) >= 0.0
    for name in ("wave", "band", "lds"):
        p.variant = L.VARIANTS[name]
        assert lib.gmpi_mpi_render_depth_window_launch(*args, None) == -6, name
        assert lib.gmpi_render_depth_window_supports(*args) == -6, name
        assert lib.gmpi_mpi_render_depth_launch(*args, None) == -6, name   # the old entry: as before
    # an unaligned base pointer: the query says 0 and the launch refuses; GATHER and the old entry still take it
    p.variant = L.VARIANT_AUTO
    p.rgba = depth.data_ptr() + 4
    p.Wt = 31
    assert lib.gmpi_render_depth_window_supports(*args) == 0 and lib.gmpi_mpi_render_depth_window_launch(*args, None) == -6
    assert lib.gmpi_mpi_render_depth_launch(*args, None) == 0
    p.variant = L.VARIANT_GATHER
    assert lib.gmpi_render_depth_window_supports(*args) == 1 and lib.gmpi_mpi_render_depth_window_launch(*args, None) == 0
    torch.cuda.synchronize()
    p.D = 0
    assert lib.gmpi_render_depth_window_supports(*args) == -2
    assert lib.gmpi_render_depth_window_supports(None, args[1], args[2]) == -1
    assert lib.gmpi_query(0) == 2 and lib.gmpi_query(25) == 1 and (lib.gmpi_query(26), lib.gmpi_query(27)) == (64, 32) and lib.gmpi_query(24) == -1
    assert int(status[0].item()) == 0
