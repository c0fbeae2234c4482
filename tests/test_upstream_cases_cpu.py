"""CPU tests of the INPUTS of tests/test_hip_upstream_gradients.py (tests/_upstream_cases.py), on the references alone: the conditions that keep
the GPU comparisons honest.

  * every texture takes the path of the 64 x 8 tile backward it was chosen for, on every plane and tile of view 0, with the headroom bits named;
  * scaling the upstream gradients by 2^-40 / 2^40 creates no denormal and no overflow in any reference;
  * under `same_sign` the fp32 chain stays within 1e-5 of float64 in every slab: the GPU bar there is the 5e-5 floor, not a loose 4 e_ref;
  * the `far` masks of `sparse` and the poisoned pixel leave out at most a tenth of a slab on the textures named for it and are nowhere empty,
    cover every other MPI, and the reference is exactly 0 (`sparse`) on them and non-zero on at least half of the rest (the clean run of a
    poisoned family; 4 / 25 on the texture finer than the image);
  * the right half of `two_scale` carries at least 2^-26 of the tensor's maximum;
  * `slab_compare` passes the fp32 reference itself for every finite family with nothing left out."""
import numpy as np
import pytest

import _upstream_cases as U
from _visible import slab_compare, slab_stats

TEX = list(U.TEXTURES)
DENSE = ("twin", "broad", "coarse", "wide")   # textures no finer than the image in both directions: under `normal` (nearly) every texel gets a gradient


@pytest.mark.parametrize("tex", TEX)
def test_every_texture_takes_the_path_it_was_chosen_for(tex):
    tp = U.tile_paths(tex)
    assert len(tp) == 3 * 3 * U.D
    if U.PATHS[tex] == "direct":
        assert not any(t["fits"] for t in tp) and min(t["margin"] for t in tp) >= 2, tp     # no box fits, by two texels or more
        return
    assert all(t["fits"] for t in tp) and min(t["margin"] for t in tp) >= 2                 # every box fits with two texels to spare
    lo, hi = U.HBITS[tex]
    hb = [t["hbits"] for t in tp]
    print(tex, "hbits", min(hb), "to", max(hb), "texels per box", min(t["area"] for t in tp), "to", max(t["area"] for t in tp))
    assert lo <= min(hb) and max(hb) <= hi, (min(hb), max(hb))
    assert all(t["wide"] == (U.PATHS[tex] == "wide") for t in tp)
    assert (U.PATHS[tex] == "wide") == (min(hb) >= 9)


@pytest.mark.parametrize("tex", TEX)
def test_scaling_by_2_to_the_40_creates_no_denormal_and_no_overflow(tex):
    """The fp32 references under `normal` have no non-zero element below 2^-80 or above 2^80; those of down40 / up40 are then the exact scalings."""
    for label, _, r64, r32 in U.reference_sets(tex, "normal"):
        for g in r32:
            a = np.abs(g[g != 0])
            assert a.min() >= 2.0 ** -80 and a.max() <= 2.0 ** 80, (label, a.min(), a.max())


@pytest.mark.parametrize("tex", U.SAME_SIGN_TIGHT)
def test_same_sign_keeps_the_fp32_chain_close(tex):
    for label, _, r64, r32 in U.reference_sets(tex, "same_sign"):
        for a, b in zip(r64, r32):
            scale, e_ref = slab_stats(a, b)
            print(f"{tex} {label}: e_ref max {e_ref.max():.2e}")
            assert e_ref.max() < 1e-5, (label, e_ref.max())


@pytest.mark.parametrize("family", list(U.FAR_TEXTURES))
def test_far_masks(family):
    """On the textures of FAR_TEXTURES the mask leaves out at most a tenth of a slab; on every texture it is not empty in any slab (the GPU test
    applies it wherever it exists), covers the other MPI, and the poisoned pixel's taps lie inside the texture on every plane."""
    for tex in TEX:
        case = U.scene(tex)
        far = U.far_mask(tex, family)
        touched = sorted({int(case["v2m"][n]) for n in U.nonzero_pixels(family, case["N"])})
        left_out = 1.0 - far.reshape(U.M, U.D, -1).mean(-1)
        union_out = 1.0 - far.all(1).reshape(U.M, -1).mean(-1)
        print(f"{family} {tex}: left out per plane at most {left_out.max():.3f}, of an image shared by the planes {union_out.max():.3f}")
        assert 0 < left_out[touched].min() and left_out[touched].max() < 1 and union_out[touched].max() < 1
        if tex in U.FAR_TEXTURES[family]:
            assert left_out[touched].max() <= 0.10 and union_out[touched].max() <= 0.10
        for m in range(U.M):
            if m not in touched:
                assert far[m].all()
        if family != "sparse":
            assert all(p[4] for p in U.peak_texels(tex)), U.peak_texels(tex)    # the poisoned pixel's taps lie inside the texture on every plane
        for label, vpm, r64, _ in U.reference_sets(tex, "sparse" if family == "sparse" else "normal"):
            if vpm is not None:
                continue
            for g in r64:
                mask = U.mask_for(far, g)
                if family == "sparse":
                    assert not np.any(g[mask]), label
                near = g[~mask]
                if label == "depth" and g.shape[1] == 1:   # (the depth image: a texel off every ramp has no gradient wherever it lies)
                    continue
                if family == "sparse":
                    # a pixel feeds the 2 x 2 texels under it, `far` starts more than 2 away: at most 4 of up to 25 cells of a footprint can be
                    # non-zero, so "half" cannot hold for isolated pixels; what is asserted is that every slab is reached at all
                    reached = np.abs(np.where(mask, 0.0, g)).reshape(*g.shape[:-2], -1).max(-1)
                    assert (reached[touched] > 0).all(), label
                else:
                    # the clean run of a poisoned family.  `fine` is finer than the image -- a pixel row feeds two texel rows of about eleven --:
                    # what must be non-zero there is the pixel's own 2 x 2 taps among the at most 5 x 5 cells of its footprint
                    least = 0.5 if tex in DENSE else 4.0 / 25.0
                    assert np.count_nonzero(near) >= least * near.size, (label, g.shape, np.count_nonzero(near), near.size)


def test_sparse_zero_view_and_single_channel_tiles():
    gc, gd, gT = U.upstream("sparse", 2, U.H, U.W, 5)
    assert not gc[U.SPARSE_ZERO_VIEW].any() and not gd[U.SPARSE_ZERO_VIEW].any() and not gT[U.SPARSE_ZERO_VIEW].any()
    for (y0, x0), which in (((8, 128), gd), ((16, 64), gT)):   # the tiles of the depth-only and the T-only pixel: no colour gradient, one other
        assert not gc[0, :, y0:y0 + 8, x0:x0 + 64].any() and np.count_nonzero(which[0, :, y0:y0 + 8, x0:x0 + 64]) == 1
    assert np.count_nonzero(gc[0, 0]) == 8


@pytest.mark.parametrize("tex", TEX)
def test_two_scale_right_half_is_not_trivial(tex):
    R = U.right_region(tex)
    assert R.any(3).any(2).all()   # some of every plane
    for label, vpm, r64, _ in U.reference_sets(tex, "two_scale"):
        if vpm is not None:
            continue
        for g in r64:
            mask = U.mask_for(R, g)
            top, right = np.abs(g).max(), np.abs(np.where(mask, g, 0.0)).max()
            print(f"{tex} {label} {g.shape}: max in R / max = 2^{np.log2(right / top):.1f}")
            assert right >= 2.0 ** -26 * top, (label, right, top)


@pytest.mark.parametrize("family", U.FINITE)
@pytest.mark.parametrize("tex", TEX)
def test_the_fp32_reference_passes_its_own_bar(tex, family):
    """The upper-bound arithmetic: (ref32 as `got`, ref64, ref32) has no failure and leaves nothing out."""
    for label, _, r64, r32 in U.reference_sets(tex, family):
        for a, b in zip(r64, r32):
            res = slab_compare(b, a, b, min_rel_scale=0, label=f"{tex} {family} {label}:")
            assert res["skipped"] == 0 and not res["failures"], (label, res["failures"][:3])


def test_upstream_makes_float64_and_strided_gradients_dense_fp32():
    """`_upstream` (hip_mpi.py), the one place the bridges take their outputs' gradients through: whatever dtype and strides come in, the entries
    get contiguous fp32 of the same values (colour always, depth and T or None).  A float64 gradient cannot be delivered through autograd -- the
    engine casts to the output's dtype first --, so it is handed over here; tests/test_hip_upstream_gradients.py delivers strided ones on the GPU."""
    import torch
    from ml_gmpi_amd.hip_mpi import _upstream
    gc, gd, gT = (torch.from_numpy(a) for a in U.upstream("normal", 2, U.H, U.W, 5))
    c64 = gc.double().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    d64 = torch.zeros((2, 1, U.H, 2 * U.W), dtype=torch.float64)
    d64[..., ::2] = gd
    d64 = d64[..., ::2]
    assert not c64.is_contiguous() and not d64.is_contiguous()
    out = _upstream(None, torch.device("cpu"), c64, d64, gT.expand(2, 1, U.H, U.W)[..., ::1])
    for got, want in zip(out, (gc, gd, gT)):
        assert got.dtype == torch.float32 and got.is_contiguous() and got.stride() == want.contiguous().stride() and torch.equal(got, want)
    assert _upstream(None, torch.device("cpu"), gc, None, None)[1:] == (None, None)
