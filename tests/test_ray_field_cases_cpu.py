"""CPU tests of the INPUTS of tests/test_hip_ray_fields.py (tests/_ray_field_cases.py), on the inputs and references alone: the conditions that
make the GPU comparisons mean something.

  * the tile shapes and staging limits are the ones the kernel sources state, and the fixed columns and rows are every tiling's corner lines;
  * the fixed pixels of every field carry the pinhole field's bits, so every tile's boxes are the pinhole field's; `pinhole` itself counts no
    footprint outside its box under any tiling;
  * per texture and tiling, on view 0 (15 000 pixel-plane pairs): `permuted` has at least 500 `far` pairs, `bulge` at least 100 `straddle` pairs
    on `twin` and `broad`, and at least one tile and plane holds in_box, straddle and far lanes together (a wave with mixed lanes: under
    `permuted` on every texture, under `bulge` on `twin` and `broad` -- on `coarse` a bulge of two texels never clears a box); at most 5 % of the
    pairs have every weight zero;
  * the references obey the rules of tests/_visible.py through every field: e_ref <= E_REF_CAP in every slab, every slab >= 1e-3 of its tensor's
    maximum, `slab_compare` passes the fp32 reference with nothing left out;
  * `permuted` under permuted upstream gradients has the pinhole field's float64 reference.

Counts with the kernels' constants (BULGE_A = 0.04, one free pixel in four exchanged; far / straddle of view 0, smallest to largest over the six
tilings): permuted twin 1585-2004 / 51-88, broad 653-2060 / 2-14, coarse 1612-1842 / 148-202; bulge twin 130-136 / 305-372, broad 190-262 /
288-397, coarse 0 / 318-327.  (`broad` under the 32 x 16 tilings with 27 box rows: 9520 of the 15 000 pairs lie in boxes that do not fit.)"""
import numpy as np
import pytest

import _ray_field_cases as F
import _upstream_cases as U
from _visible import E_REF_CAP, slab_compare, slab_stats

TEX = ("twin", "broad", "coarse")   # forward: twin, coarse; backward: all three
FAMILIES = ("normal", "same_sign")
TILINGS = list(F.tilings())
PAIRS = U.D * U.H * U.W


def test_constants_and_fixed_lines_are_the_kernels():
    t = F.tilings()
    assert {v[:2] for v in t.values()} == {(64, 8), (32, 16)}
    assert t["backward"] == (64, 8, 80, 19, 1) and t["backward1"] == t["alpha"] == (32, 16, 56, 27, 1) and t["window"] == (32, 16, 64, 32, 1)
    assert t["forward"] == (32, 16, 56, 27, 4) and t["u8"] == (32, 16, 64, 32, 4)
    assert F.fixed_axes() == ((0, 31, 32, 63, 64, 95, 96, 127, 128, 149), (0, 7, 8, 15, 16, 19))
    fixed = F.fixed_mask()
    for tiling in TILINGS:   # every corner pixel of every tile is fixed
        for y0, y1, x0, x1, _ in F.boxes("twin", "pinhole", tiling):
            assert fixed[[y0, y0, y1, y1], [x0, x1, x0, x1]].all()
    assert int((~fixed).sum()) == 14 * 140


@pytest.mark.parametrize("vpm", [None, 2])
@pytest.mark.parametrize("field", F.MOVED)
def test_fixed_pixels_keep_the_pinhole_bits_and_the_free_ones_move(field, vpm):
    base, moved = F.scene("twin", "pinhole", vpm)["ray"], F.scene("twin", field, vpm)["ray"]
    assert moved.dtype == np.float32 and moved.shape == base.shape
    fixed = F.fixed_mask()
    assert np.array_equal(moved[..., fixed].view(np.uint32), base[..., fixed].view(np.uint32))
    changed = (moved != base).any(1)   # [N,H,W]
    assert not changed[:, fixed].any()
    n_free = int((~fixed).sum())
    if field == "permuted":
        pi = F.permutation()
        assert np.array_equal(np.sort(pi), np.arange(U.H * U.W)) and int((pi != np.arange(U.H * U.W)).sum()) >= n_free // 4 - 5
        assert (changed.reshape(len(base), -1).sum(1) >= n_free // 4 - 5).all()
        assert np.array_equal(moved, F.permute_pixels(base))
    else:
        assert changed[:, ~fixed].all()   # every free pixel moves, by at most BULGE_A
        assert float(np.abs(moved - base).max()) <= F.BULGE_A * 1.0001 and np.array_equal(moved[:, 2], base[:, 2])
    a, b = F.scene("twin", field, vpm), F.scene("twin", "pinhole", vpm)   # nothing else differs
    assert all(np.array_equal(a[k], b[k]) for k in ("rgba", "dhw", "eye", "zd", "v2m"))


@pytest.mark.parametrize("tiling", TILINGS)
@pytest.mark.parametrize("tex", TEX)
def test_class_counts(tex, tiling):
    got = {field: F.counts(tex, field, tiling) for field in F.FIELDS}
    print("COUNTS", tex, tiling, {f: (c["in_box"], c["straddle"], c["far"], c["unstaged"], c["no_weight"]) for f, c in got.items()},
          "mixed tiles", {f: F.mixed_tiles(tex, f, tiling) for f in F.MOVED})
    for field, c in got.items():
        assert sum(c.values()) == PAIRS
        assert c["no_weight"] <= 0.05 * PAIRS, (field, c)
    assert got["pinhole"]["straddle"] == 0 and got["pinhole"]["far"] == 0
    assert got["pinhole"]["in_box"] >= 5000   # (`broad` under 27 box rows: most planes are not staged; the staged ones carry the test)
    assert got["permuted"]["far"] >= 500, got["permuted"]
    assert F.mixed_tiles(tex, "permuted", tiling) >= 1
    assert got["bulge"]["straddle"] >= 100, got["bulge"]   # (asked of `twin` and `broad`; `coarse` has 318 too)
    if tex in ("twin", "broad"):
        assert F.mixed_tiles(tex, "bulge", tiling) >= 1
    for field in F.MOVED:   # the boxes are the pinhole field's
        assert [b[4] for b in F.boxes(tex, field, tiling)] == [b[4] for b in F.boxes(tex, "pinhole", tiling)]


@pytest.mark.parametrize("tex", TEX)
def test_every_view_has_its_share(tex):
    """View 1 (another tilt) and, on `twin`, the four views of two per MPI: the counts are no accident of view 0."""
    for view in range(1, U.M):
        assert F.counts(tex, "permuted", "backward", view)["far"] >= 500
        assert F.counts(tex, "bulge", "backward", view)["straddle"] >= 100
    if tex == "twin":
        for view in range(4):
            assert F.counts(tex, "permuted", "backward", view, 2)["far"] >= 500
            assert F.counts(tex, "bulge", "backward", view, 2)["straddle"] >= 100


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("field", F.MOVED)
@pytest.mark.parametrize("tex", TEX)
def test_references_obey_the_rules_of_visible(tex, field, family):
    for label, _, r64, r32 in F.reference_sets(tex, field, family):
        for i, (a, b) in enumerate(zip(r64, r32)):
            scale, e_ref = slab_stats(a, b)
            assert np.isfinite(a).all() and np.isfinite(b).all()
            assert e_ref.max() <= E_REF_CAP, (label, i, e_ref.max())
            assert scale.min() >= 1e-3 * scale.max(), (label, i, scale.min(), scale.max())
            res = slab_compare(b, a, b, min_rel_scale=0, label=f"{tex} {field} {family} {label}[{i}]:")
            assert res["skipped"] == 0 and not res["failures"], (label, i, res["failures"][:3])


@pytest.mark.parametrize("shape", F.LINES, ids=[f"{h}x{w}" for h, w in F.LINES])
@pytest.mark.parametrize("kind", ["volume", "shared", "depth"])
def test_references_of_the_one_row_and_one_column_images(kind, shape):
    """The images that get no usable homography (W >= 2 && H >= 2 fails): the same rules, and every slab is reached by the forty pixels."""
    H, W = shape
    assert min(H, W) == 1 and max(H, W) == 40
    r64, r32 = F.line_refs(kind, H, W)
    for i, (a, b) in enumerate(zip(r64, r32)):
        scale, e_ref = slab_stats(a, b)
        assert e_ref.max() <= E_REF_CAP, (i, e_ref.max())
        assert scale.min() >= 1e-3 * scale.max(), (i, scale.min(), scale.max())
        res = slab_compare(b, a, b, min_rel_scale=0, label=f"line {kind} {H}x{W} [{i}]:")
        assert res["skipped"] == 0 and not res["failures"], (i, res["failures"][:3])


@pytest.mark.parametrize("tex", TEX)
def test_permuted_rays_under_permuted_gradients_have_the_pinhole_reference(tex):
    """float64 autograd: the same sum in another order -- equal to 1e-12 of the slab's maximum (the GPU test compares the two runs of a path)."""
    import torch
    import _deep_cases
    base = U.with_upstream(F.scene(tex, "pinhole"), "normal")
    perm = dict(F.scene(tex, "permuted"), **{k: F.permute_pixels(base[k]) for k in ("gc", "gd", "gT")})
    a, b = (_deep_cases.volume_grad_ref(c, torch.float64, align_corners=True) for c in (base, perm))
    scale, _ = slab_stats(a, a)
    assert float((np.abs(a - b).reshape(*scale.shape, -1).max(-1) / scale).max()) <= 1e-12
