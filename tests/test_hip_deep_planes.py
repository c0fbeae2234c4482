"""Forward kernels on stacks in which EVERY plane counts (tests/_visible.py: "thin" and "surface" alpha laws).  With the white-noise alpha of
the rest of the suite the transmittance falls by about e per plane and nothing behind plane ~30 moves an output by half an ulp: the 96-plane
chunks of the tile kernel, the strip kernel's 32-entry ring and its 3- / 6-way plane split, the band kernel's per-plane records at D = 96 / 256
and the background plane of the shared-colour layout are compared there against zeros.  Here the inputs are the ones
tests/test_visible_stacks_cpu.py holds to "taking any plane out moves the reference by >= 100 x the bar"; the bars are the project's own --
strict-order mode BIT-identical to the oracle (colour, depth, T), default mode within 0.5 TOL colour / TOL depth and transmittance, against the
fp32 oracle (same coordinates; float64 would be 1e-5 away on the surface stacks).  Run on the MI355X box:  python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch

import oracle
import _deep_cases as C
import test_hip_properties as props
import test_hip_shared_color as shared
from _visible import make_alpha
from test_hip_parity import TOL, _random_case, hip_render, variants

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
WORST = {}   # kernel variant -> worst default-mode error seen in this file (printed by every check: the last line holds the totals)


def _check(vol, dhw, ray, eye, zd, use, label, strict=True):
    """`vol` holds the STORED values (the oracle gets them upcast).  Strict mode bit for bit, default mode within the bars, every variant."""
    orc = oracle.render(vol.float(), dhw, ray, eye, zd, threads=True)
    for variant in use:
        if strict:
            out = hip_render(vol, dhw, ray, eye, zd, variant=variant, strict=True)
            for k in ("color", "depth", "T"):
                assert np.array_equal(out[k], orc[k]), (label, variant, k, float(np.abs(out[k] - orc[k]).max()))
        fast = hip_render(vol, dhw, ray, eye, zd, variant=variant)
        errs = {k: float(np.abs(fast[k] - orc[k]).max()) for k in ("color", "depth", "T")}
        w = WORST.setdefault(variant, dict(color=0.0, depth=0.0, T=0.0))
        for k in errs:
            w[k] = max(w[k], errs[k])
        print(f"default mode {label} {variant}: {errs}; worst so far {w}")
        assert errs["color"] <= 0.5 * TOL and errs["depth"] <= TOL and errs["T"] <= TOL, (label, variant, errs)
        assert int(fast["status"][0]) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("cfg,alpha", C.small_cases(), ids=lambda c: c if isinstance(c, str) else f"D{c['D']}" + ("-tilted" if c.get("extreme") else ""))
def test_every_kernel_on_visible_stacks_around_ring_and_chunk_boundaries(cfg, alpha, dtype):
    """D around the strip kernel's 32-entry table ring and the tile kernel's 96-plane chunks (and two chunks + 1), all storage types, every
    kernel variant; the tilted case crosses the chunk boundary on the half-tile path."""
    rgba, dhw, ray, eye, zd = _random_case(alpha=alpha, **cfg)
    _check(rgba.to(dtype), dhw, ray, eye, zd, variants(), f"{alpha} D={cfg['D']} {dtype}")


@pytest.mark.parametrize("alpha", ["thin", "surface"])
@pytest.mark.parametrize("cfg", C.SPLIT_CASES + [C.TWO_WAVES_CASE], ids=lambda c: f"B{c['B']}-D{c['D']}-S{c['S']}")
def test_strip_kernel_plane_split_merges_every_part(cfg, alpha):
    """The shapes of test_strip_kernel_plane_split_regimes (6-way, 3-way, unsplit, D not divisible by the split, fewer planes than parts) and the
    2-waves-per-SIMD instance at D = 96, on stacks whose LAST part still carries a visible share of the image: the in-order merge of every
    part is compared, not only of the first one or two.  fp32 and bf16 volumes; the 256^2 x 96 shapes also through the band kernel (whole image)."""
    rgba, dhw, ray, eye, zd = _random_case(alpha=alpha, **cfg)
    use = ("wave", "band", "lds") if cfg["D"] == 96 else ("wave",)
    _check(rgba, dhw, ray, eye, zd, use, f"{alpha} split {cfg}")
    _check(rgba.to(torch.bfloat16), dhw, ray, eye, zd, use, f"{alpha} split bf16 {cfg}")


@pytest.mark.parametrize("shape", C.FULL_SIZE, ids=lambda s: f"D{s['D']}-{str(s['dtype'])[6:]}" + ("-extreme" if s.get("extreme") else ""))
def test_full_size_windows_on_thin_stacks(shape):
    """The band kernel's shapes (1024^2 x 96 bf16 / fp16, 1024^2 x 256 fp32 MetFaces, the two tilted ones) with all 96 / 256 planes in every
    window.  (Thin law: a 64 x 64 window of a surface stack shows only the planes whose surface crosses it.)"""
    props.test_full_size_window_against_oracle(shape, alpha="thin")


def test_views_sharing_one_mpi_on_thin_stacks():
    """256^2 x 96 x 8 views and 8 camera-path views of ONE 512^2 x 96 MPI: band and tile side, every variant."""
    props.test_full_size_windows_config2_and_config4_against_oracle(alpha="thin")


def test_auto_shares_its_views_between_band_and_tile_kernel_on_a_thin_stack():
    props.test_config5_shape_auto_shares_the_views_between_band_and_tile_kernel(alpha="thin")


def test_plane_split_associativity_with_a_visible_back_half():
    """composite(planes[:40]) (+) composite(planes[40:]) == composite(all) where the front transmittance at the split is >= 0.1 (asserted) --
    on the white-noise stack it is ~1e-17.  Same bars."""
    props.test_plane_split_associativity_full_size(alpha="thin")


@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("cfg", C.SHARED_COLOUR, ids=lambda c: f"D{c['D']}")
def test_shared_colour_forward_reaches_the_background_plane(cfg, dtype, with_bg):
    """Shared-colour layout on a thin stack: the background image sits on plane D - 1, behind 31 / 95 planes that let it through."""
    rgba, dhw, ray, eye, zd = _random_case(alpha="thin", **cfg)
    rgb, alpha, bg = shared._parts(rgba, dtype)
    if with_bg:   # the condition of the CPU test, on these very inputs: the background's share of the image is far above the bar
        vol = shared._expand(rgb, alpha, bg).numpy()
        a, gone = oracle.render(vol, dhw, ray, eye, zd, threads=True), vol.copy()
        gone[:, -1, 3] = 0
        b = oracle.render(gone, dhw, ray, eye, zd, threads=True)
        assert np.abs(a["color"] - b["color"]).max() >= 100 * 0.5 * TOL
    shared._check_forward(rgb, alpha, bg if with_bg else None, dhw, ray, eye, zd, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("alpha", ["thin", "surface"])
def test_compute_depth_bit_exact_through_96_visible_planes(alpha, dtype):
    """LightRenderer.compute_depth (gmpi_alpha_depth_launch): depth and transmittance bit for bit, alpha planes as the strided view of a volume."""
    import ml_gmpi_amd
    c = C.DEPTH_CASE
    vol = torch.from_numpy(make_alpha(oracle.synth_rgba(77, (c["B"], c["D"], 4, c["S"], c["S"])), alpha)).cuda().to(dtype)
    ds = np.linspace(0.95, 1.12, c["D"]).astype(np.float32)
    a = vol[:, :, 3:]
    depth, T = ml_gmpi_amd.compute_depth(a, torch.from_numpy(ds).reshape(-1, 1), want_transmittance=True)
    want_d, want_T = oracle.alpha_depth(a.float().cpu().numpy(), ds)
    assert float(want_T.min()) > 1e-3 or alpha == "surface"
    assert np.array_equal(depth.cpu().numpy(), want_d) and np.array_equal(T.cpu().numpy(), want_T)
