"""CPU tests of the INPUTS of the deep-plane GPU tests (tests/_deep_cases.py, tests/_visible.py), against the oracle and the float64 / fp32
restatements only:

  * every listed plane of every thin / surface stack is visible: taking it out moves the colour (depth) of the reference render by at least
    100 x the bar the GPU test applies (colour 5e-6 -> 5e-4, depth 1e-5 -> 1e-3) -- a fault confined to one plane exceeds the bar, not merely
    touches it;
  * the blind spot these inputs exist for: on a white-noise stack the same measure is below the bar from plane 32 on;
  * the per-slab gradient bar of `slab_compare` is max(5e-5, 4 e_ref): e_ref <= 1e-4 in every slab of every committed backward case, and
    every slab's scale is >= 1e-3 of the tensor's maximum, so the bar calibrates itself within a factor 8 of the project's 5e-5 and no slab
    is an afterthought;
  * the same two conditions for the inputs of the chunked and shaded twins of the volume backward (`twin_case`), for the shading gradient per
    MPI image too; both ends of the clip are taken by at least 5 % of the colour products, fp32 and float64 agree on both gates, and the tile
    boxes of the 64 x 8 tile backward fit (or, for the minified case, do not fit) as the cases say."""
import numpy as np
import pytest
import torch

import oracle
import _deep_cases as C
from _visible import E_REF_CAP, listed_planes, make_alpha, plane_visibility, slab_stats, surface, thin
from test_hip_parity import TOL, _random_case

COLOUR_MIN = 100 * 0.5 * TOL   # 5e-4
DEPTH_MIN = 100 * TOL          # 1e-3


def _visibility(cfg, alpha, dtype=None, planes=None, bg_parts=False):
    rgba, dhw, ray, eye, zd = _random_case(alpha=alpha, **cfg)
    if dtype is not None:
        rgba = rgba.to(dtype).float()
    vol = rgba.numpy()
    if bg_parts:   # the shared-colour layout: one colour image in front, the background image on plane D - 1
        vol = np.concatenate([np.broadcast_to(vol[:, :1, :3], (vol.shape[0], vol.shape[1] - 1, 3, *vol.shape[-2:])), vol[:, -1:, :3]], 1)
        vol = np.concatenate([vol, rgba.numpy()[:, :, 3:]], 2)

    def fn(v):
        o = oracle.render(v, dhw, ray, eye, zd, threads=True)
        return o["color"], o["depth"]
    return plane_visibility(fn, vol, listed_planes(cfg["D"]) if planes is None else planes)


def _assert_visible(vis, label):
    c = min(v[0] for v in vis.values())
    z = min(v[1] for v in vis.values())
    print(f"{label}: planes {len(vis)} min colour change {c:.2e} ({c / (0.5 * TOL):.0f} x bar) min depth change {z:.2e} ({z / TOL:.0f} x bar)")
    bad = {k: v for k, v in vis.items() if v[0] < COLOUR_MIN or v[1] < DEPTH_MIN}
    assert not bad, (label, bad)


@pytest.mark.parametrize("cfg,alpha", C.small_cases(), ids=lambda c: c if isinstance(c, str) else f"D{c['D']}" + ("-tilted" if c.get("extreme") else ""))
def test_every_plane_of_the_tile_and_strip_cases_is_visible(cfg, alpha):
    if cfg.get("extreme"):
        cfg = dict(cfg, S=cfg["S"] // 2)   # (half the image size: the planes and the poses are the GPU test's)
    for dtype in (None, torch.bfloat16) if cfg["D"] == 97 else (None,):   # (bf16: the coarsest format the GPU tests round the stacks to)
        _assert_visible(_visibility(cfg, alpha, dtype), f"{alpha} {cfg} {dtype}")


@pytest.mark.parametrize("alpha", ["thin", "surface"])
@pytest.mark.parametrize("cfg", C.SPLIT_CASES + [C.TWO_WAVES_CASE], ids=lambda c: f"B{c['B']}-D{c['D']}-S{c['S']}")
def test_every_plane_of_the_plane_split_cases_is_visible(cfg, alpha):
    small = dict(cfg, S=cfg["S"] // 2)   # (half the image size: the planes and the poses are the GPU test's)
    _assert_visible(_visibility(small, alpha), f"{alpha} {small}")


@pytest.mark.parametrize("shape", C.FULL_SIZE + [C.SHARED_VIEWS, C.AUTO_SHARES], ids=lambda s: f"D{s['D']}-{str(s.get('dtype', ''))[6:]}" + ("-extreme" if s.get("extreme") else ""))
def test_every_listed_plane_of_the_full_size_thin_stacks_is_visible(shape):
    """The band-kernel shapes at 1/8 of the image size.  Thin stacks only: on a 64 x 64 window of a surface stack only the planes whose surface
    crosses the window are visible, so the window tests of the full-size shapes use the thin law (the surface law meets the band kernel at
    256^2, whole image: TWO_WAVES_CASE's shape)."""
    cfg = dict(seed=6, B=min(shape["B"], 2), D=shape["D"], S=shape["S"] // 8, preset=shape.get("preset", "FFHQ"), extreme=shape.get("extreme", False))
    _assert_visible(_visibility(cfg, "thin", shape.get("dtype")), f"thin {cfg}")


@pytest.mark.parametrize("cfg", C.SHARED_COLOUR, ids=lambda c: f"D{c['D']}")
def test_the_background_plane_of_the_shared_colour_cases_is_visible(cfg):
    for dtype in (None, torch.bfloat16):
        _assert_visible(_visibility(cfg, "thin", dtype, bg_parts=True), f"shared colour thin {cfg} {dtype}")


@pytest.mark.parametrize("alpha", ["thin", "surface"])
def test_every_plane_of_the_compute_depth_case_is_visible(alpha):
    c = C.DEPTH_CASE
    vol = make_alpha(oracle.synth_rgba(77, (c["B"], c["D"], 4, c["S"], c["S"])), alpha)
    ds = np.linspace(0.95, 1.12, c["D"]).astype(np.float32)
    base, _ = oracle.alpha_depth(vol[:, :, 3:], ds)
    for k in range(c["D"]):
        a = vol[:, :, 3:].copy()
        a[:, k] = 0
        z, _ = oracle.alpha_depth(a, ds)
        assert np.abs(z - base).max() >= DEPTH_MIN, (alpha, k, np.abs(z - base).max())


def test_white_noise_stack_is_blind_behind_plane_32():
    """The blind spot: with alpha ~ U[0,1) the transmittance falls by about e per plane, and from plane 32 on taking a plane out moves neither
    colour nor depth by as much as the bar -- the kernels' ring wrap, chunk boundary and split merge lie behind that.  The same planes of the
    thin stack are 100 x above it (the tests above)."""
    cfg = dict(seed=20 + 97, B=1, D=97, S=64)
    vis = _visibility(cfg, "noise", planes=range(97))
    assert vis[0][0] >= COLOUR_MIN                    # (the front plane is seen, of course)
    behind = [max(vis[k][0] / (0.5 * TOL), vis[k][1] / TOL) for k in range(32, 97)]
    print("white noise, D = 97: largest change / bar for planes 32..96:", max(behind), "; planes 16, 24:", vis[16], vis[24])
    assert max(behind) < 1.0
    assert all(vis[k] == (0.0, 0.0) for k in range(64, 97))   # behind plane 64 not one bit of the output depends on a plane


@pytest.mark.parametrize("name", list(C.GRAD_CASES))
def test_gradient_cases_keep_the_slab_bar_honest(name):
    case = C.grad_case(name)
    scale, e_ref = slab_stats(C.volume_grad_ref(case, torch.float64), C.volume_grad_ref(case, torch.float32))
    print(f"{name}: slab scale min {scale.min():.2e} max {scale.max():.2e}; e_ref max {e_ref.max():.2e} median {np.median(e_ref):.2e}")
    assert e_ref.max() <= E_REF_CAP, e_ref.max()
    assert scale.min() >= 1e-3 * scale.max(), (scale.min(), scale.max(), np.unravel_index(scale.argmin(), scale.shape))


TWIN_KEYS = C.twin_keys("chunk") + C.twin_keys("shaded")


def _assert_honest(label, refs, shaded):
    """refs = (float64, fp32) of tests/_deep_cases.py `twin_refs`: e_ref and the slab scales of the volume gradient and, shaded, of the shading's."""
    ref64, ref32 = refs
    pairs = [("volume", ref64[0], ref32[0]), ("shading", ref64[1], ref32[1])] if shaded else [("volume", ref64, ref32)]
    for what, r64, r32 in pairs:
        scale, e_ref = slab_stats(r64, r32)
        print(f"{label} {what}: slab scale min {scale.min():.2e} max {scale.max():.2e} (min / max {scale.min() / scale.max():.2e}); "
              f"e_ref max {e_ref.max():.2e} median {np.median(e_ref):.2e}")
        assert e_ref.max() <= E_REF_CAP, (what, e_ref.max())
        assert scale.min() >= 1e-3 * scale.max(), (what, scale.min(), scale.max(), np.unravel_index(scale.argmin(), scale.shape))


def test_the_further_references_of_the_shaded_twin_keep_the_slab_bar_honest():
    """The two references tests/test_hip_shaded_gradients.py uses beside the cases' own: colour written as 2 C - 1, and ONE shading image expanded
    over both MPIs (its gradient is the sum over them)."""
    _assert_honest("t12-ragged out_pm1", C.twin_refs("t12-ragged", True, out_pm1=True), True)
    _assert_honest("t12-views-vpm one shading image", C.twin_refs("t12-views-vpm", True, one_shading=True), True)


@pytest.mark.parametrize("name,shaded", TWIN_KEYS, ids=[n + ("-shaded" if s else "") for n, s in TWIN_KEYS])
def test_twin_gradient_cases_keep_the_slab_bar_honest(name, shaded):
    """The inputs of tests/test_hip_chunk_gradients.py and tests/test_hip_shaded_gradients.py: the two conditions above for the volume gradient and,
    per MPI image, for the shading gradient; both branches of the clip are taken by at least 5 % of the colour products, and fp32 and float64 agree
    on both gates for every texel (a texel they disagreed on would carry an O(1) difference no bar could absorb)."""
    case = C.twin_case(name, shaded)
    _assert_honest(name, C.twin_refs(name, shaded), shaded)
    if shaded:
        rgb, s = torch.from_numpy(case["rgba"][:, :, :3]), torch.from_numpy(case["shading"])
        p32, p64 = rgb * s[:, None], rgb.double() * s.double()[:, None]
        above, below = float((p64 > 1).double().mean()), float((p64 < 0).double().mean())
        print(f"{name}: products above 1 {above:.3f}, below 0 {below:.3f}")
        assert above >= 0.05 and below >= 0.05, (above, below)
        assert bool(((p32 > 1) == (p64 > 1)).all()) and bool(((p32 < 0) == (p64 < 0)).all())


def _tile_boxes(case, tw, th):
    """(columns, rows) of the texel box of every (view, tw x th pixel tile, plane): `item_box<1>` of gmpi_device.hpp over the images of the tile's four
    corner pixels, restated in float64 without its 1/64 texel of slack (the callers leave a texel of margin either way)."""
    dhw, ray, eye = (np.asarray(case[k], dtype=np.float64) for k in ("dhw", "ray", "eye"))
    Ht, Wt = case["rgba"].shape[-2:]
    out = []
    for n in range(case["N"]):
        for y0 in range(0, case["H"], th):
            for x0 in range(0, case["W"], tw):
                ys, xs = [y0, min(y0 + th - 1, case["H"] - 1)], [x0, min(x0 + tw - 1, case["W"] - 1)]
                r = ray[n][:, ys][:, :, xs].reshape(3, 4)
                for d, ph, pw in dhw[case["v2m"][n]]:
                    s = (d - eye[n, 2]) / r[2]
                    u, v = 2 * (eye[n, 0] + r[0] * s) / pw, 2 * (eye[n, 1] + r[1] * s) / ph
                    if case["ac"]:
                        ix, iy = (u + 1) * (Wt - 1) / 2, (v + 1) * (Ht - 1) / 2
                    else:
                        u, v = np.where(np.abs(u) <= 1, u * 0.95, u), np.where(np.abs(v) <= 1, v * 0.95, v)
                        ix, iy = ((u + 1) * Wt - 1) / 2, ((v + 1) * Ht - 1) / 2
                    out.append((np.floor(ix.max()) + 1 - np.floor(ix.min()) + 1, np.floor(iy.max()) + 1 - np.floor(iy.min()) + 1))
    return np.array(out)


def test_twin_frames_stage_or_scatter_as_their_cases_say():
    """The 64 x 8 tile backward stages a plane's scatter when the tile's texel box fits 80 columns x 19 rows (B2Wide, render_backward.hip).  On the
    20 x 150 frame over 36 x 52 (and 36 x 50) texels every box fits with a texel to spare: the staged path, the flush waves and the fixed-point sums
    run on every plane.  On t6-minified (250 x 190 texels under 24 x 40 pixels) no box fits by more than a texel: every plane scatters straight to
    global memory."""
    for name in ("t97-thin", "t129-surface-ac0", "t12-ragged", "t12-ragged-ac0", "t12-views-v2m", "t12-views-vpm"):
        b = _tile_boxes(C.twin_case(name), 64, 8)
        assert (b[:, 0] + 1 <= 80).all() and (b[:, 1] + 1 <= 19).all(), (name, b.max(0))
    b = _tile_boxes(C.twin_case("t6-minified"), 64, 8)
    print("t6-minified: smallest box", b.min(0))
    assert ((b[:, 0] - 1 > 80) | (b[:, 1] - 1 > 19)).all(), b.min(0)


@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("cfg", C.SHARED_GRAD, ids=lambda c: f"D{c['D']}")
def test_shared_colour_gradient_cases_keep_the_slab_bar_honest(cfg, with_bg):
    import test_hip_shared_color as shared
    parts, dhw, ray, eye, zd, v2m, gc, gd, gT = C.shared_grad_case(cfg, with_bg)
    r64 = shared._reference_grads(parts, dhw, ray, eye, zd, v2m, gc, gd, gT, False, torch.float64)
    r32 = shared._reference_grads(parts, dhw, ray, eye, zd, v2m, gc, gd, gT, False, torch.float32)
    scale, e_ref = slab_stats(r64[1], r32[1])   # the alpha gradient, per (MPI, plane)
    print(f"shared colour D={cfg['D']} bg={with_bg}: alpha slab scale min {scale.min():.2e} max {scale.max():.2e}; e_ref max {e_ref.max():.2e}")
    assert e_ref.max() <= E_REF_CAP and scale.min() >= 1e-3 * scale.max()
    if with_bg:   # the background gradient is worth comparing
        assert np.abs(r64[2]).max() >= 1e-2 * np.abs(r64[0]).max()


def test_geometry_cases_give_every_plane_row_weight():
    from _geometry_ref import geometry_grads
    for cfg in C.GEOMETRY:
        rgba, dhw, ray, eye, zd, v2m, gc, gd = C.geometry_case(cfg)
        row = np.abs(geometry_grads(rgba, dhw, ray, eye, zd, v2m, gc, gd, align_corners=True)[0]).max(axis=2)
        assert row.min() >= 1e-3 * row.max(), (cfg, row.min(), row.max())


def test_thin_and_surface_keep_the_transmittance_healthy():
    """thin: sum of alphas ~ budget whatever D is; surface: every plane nearly opaque somewhere, alpha within [0, 1]; both rounded to storage."""
    for D in (32, 97, 256):
        vol = oracle.synth_rgba(3, (1, D, 4, 24, 40))
        t = thin(vol)
        assert abs(float(t[:, :, 3].sum(1).mean()) - 1.5) < 0.1
        s = surface(vol)
        assert float(s[:, :, 3].max()) <= 1.0 and float(s[:, :, 3].min()) >= 0.0
        assert float(s[0, :, 3].reshape(D, -1).max(1).min()) >= 0.5
        b = thin(torch.from_numpy(vol), dtype=torch.bfloat16)
        assert b.dtype == torch.bfloat16 and torch.equal(b, torch.from_numpy(t).to(torch.bfloat16))
    assert np.array_equal(thin(vol[:, :2])[:, :, 3], vol[:, :2, 3])   # never scaled up
