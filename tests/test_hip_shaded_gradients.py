"""The shaded twins of the volume backward (render_backward_shaded_kernel, render_backward_tile2_shaded_kernel), the shading-only backward
(render_backward_shading_only_kernel) and the in-place chain rule through the clip (light_apply_backward_inplace_kernel) through
MPI.render_views_shaded, on the inputs of tests/_deep_cases.py `twin_case(name, shaded=True)`, compared PER SLAB.  tests/test_hip_shaded_render.py
runs them on square frames with image = texture, Wt % 4 == 0, align_corners=True, at most 16 planes, colours in [0, 1) and a per-tensor bar.  Here:
20 x 150 pixels over 36 x 52 texels (three ragged columns and rows of 64 x 8 tiles), 97 and 129 planes, both align_corners modes, the three storage
dtypes, a texture width that is no multiple of 4 and a texture of one column (the scalar instance of the chain rule; the one-pixel twin under
"auto"), a texture no tile box fits (the tile twin's direct scatter), shared MPIs, and colours in [-0.15, 1.15] so that BOTH ends of the clip are
taken (products above 1: 15 %, below 0: 12 %; the kernels run with range_check="off").

Bars: tests/_visible.py `slab_compare` against float64 -- max(5e-5, 4 e_ref) of the slab's own maximum, + half an ulp for a 16-bit gradient --
for every (MPI, plane, channel) slab of the volume gradient and every MPI image of the shading gradient, no slab left out
(tests/test_visible_stacks_cpu.py: e_ref <= 1e-4, every slab >= 1e-3 of the largest, fp32 and float64 agree on both gates for every texel); and
wherever float64 says the clip is closed the returned colour gradient is exactly 0."""
import numpy as np
import pytest
import torch

import _deep_cases as C
from _visible import slab_compare
from test_hip_shaded_render import _hip_grads

pytestmark = pytest.mark.gpu
VARIANTS = ("auto", "gather")   # the 64 x 8 tile twin (the one-pixel twin for a one-column texture) | the one-pixel twin
SHADED = [n for n, _ in C.twin_keys("shaded")]


def _grads(name, variant, needs=(True, True), out_pm1=False, prep=None, shading=None):
    """MPI.render_views_shaded + backward on the case -> the two leaves (volume in the case's dtype, shading fp32)."""
    case = C.twin_case(name, True)
    s = case["shading"] if shading is None else shading
    ins, _ = _hip_grads(torch.from_numpy(case["rgba"]), torch.from_numpy(s), case["dhw"], case["ray"], case["eye"], case["zd"], case["v2m"], case["gc"],
                        case["gd"], case["gT"], out_pm1, variant, case["dtype"], needs=needs, align_corners=case["ac"], range_check="off",
                        views_per_mpi=case["vpm"], prep=prep)
    assert torch.equal(ins[0].detach().float().cpu(), torch.from_numpy(case["rgba"]))   # the references were fed the stored values
    return ins


def _closed(case, s):
    """[M,D,3,Ht,Wt] bool: float64 says clip(rgb s) passes no gradient (the product lies outside [0, 1])."""
    p = torch.from_numpy(case["rgba"][:, :, :3]).double() * torch.from_numpy(s).double()[:, None]
    return ((p > 1) | (p < 0)).numpy()


def _check_volume(name, label, grad, refs, failures, s=None):
    case = C.twin_case(name, True)
    assert grad.dtype == case["dtype"] and grad.shape == case["rgba"].shape and grad.is_contiguous()
    got = grad.double().cpu().numpy()
    res = slab_compare(got, refs[0][0], refs[1][0], case["dtype"], min_rel_scale=0, label=f"{name} {label} volume:")
    assert res["skipped"] == 0
    if res["failures"]:
        failures[label, "volume"] = (len(res["failures"]), res["worst"], res["where"], res["failures"][:5])
    closed = _closed(case, case["shading"] if s is None else s)
    leaked = int(np.count_nonzero(got[:, :, :3][closed]))
    if leaked:
        failures[label, "gradient through a closed clip"] = (leaked, int(closed.sum()))


def _check_shading(name, label, grad, refs, failures):
    assert grad.dtype == torch.float32 and grad.shape == refs[0][1].shape
    res = slab_compare(grad.double().cpu().numpy(), refs[0][1], refs[1][1], min_rel_scale=0, label=f"{name} {label} shading:")
    assert res["skipped"] == 0
    if res["failures"]:
        failures[label, "shading"] = (len(res["failures"]), res["worst"], res["where"], res["failures"][:5])


@pytest.mark.parametrize("name", SHADED)
def test_shaded_gradients_per_slab(name):
    """Every shaded case, both variants, both gradients.  What each case is for: t97-thin / t129-surface-ac0 deep stacks across the tile twin's
    96-plane table (ac=False: the AC = false instances); -bf16 / -f16: 16-bit volumes and gradients; t12-ragged(-ac0): Wt = 50, the scalar chain
    rule and pair loads at an odd right border; t12-column(-ac0): Wt = 1, where launch_backward_shaded_t's guard `p.Wt >= 2` sends "auto" to the
    one-pixel twin; t6-minified: 250 x 190 texels under 24 x 40 pixels, no box fits and the tile twin scatters straight to global memory;
    t12-views-*: views that share an MPI, by index and by views_per_mpi."""
    refs = C.twin_refs(name, True)
    failures = {}
    for variant in VARIANTS:
        vol, s = _grads(name, variant)
        _check_volume(name, variant, vol.grad, refs, failures)
        _check_shading(name, variant, s.grad, refs, failures)
    assert not failures, failures


@pytest.mark.parametrize("needs", [(True, False), (False, True)], ids=["volume-only", "shading-only"])
@pytest.mark.parametrize("name", ["t129-surface-ac0", "t12-ragged-ac0", "t6-minified"])
def test_partial_needs_per_slab(name, needs):
    """Only the volume requires grad (the chain rule writes no shading gradient), then only the shading: render_backward_shading_only_kernel applies
    the chain rule per tap, whatever the variant, and must give the shading gradient of the full run -- the same float64 reference, the same rule."""
    refs = C.twin_refs(name, True)
    failures = {}
    for variant in VARIANTS:
        vol, s = _grads(name, variant, needs=needs)
        assert (vol.grad is not None) == needs[0] and (s.grad is not None) == needs[1]
        if needs[0]:
            _check_volume(name, f"{variant} needs={needs}", vol.grad, refs, failures)
        if needs[1]:
            _check_shading(name, f"{variant} needs={needs}", s.grad, refs, failures)
    assert not failures, failures


def test_colour_written_as_pm1():
    name = "t12-ragged"
    refs = C.twin_refs(name, True, out_pm1=True)
    failures = {}
    for variant in VARIANTS:
        vol, s = _grads(name, variant, out_pm1=True)
        _check_volume(name, f"{variant} pm1", vol.grad, refs, failures)
        _check_shading(name, f"{variant} pm1", s.grad, refs, failures)
        vol, s = _grads(name, variant, needs=(False, True), out_pm1=True)
        _check_shading(name, f"{variant} pm1 shading-only", s.grad, refs, failures)
    assert not failures, failures


@pytest.mark.parametrize("name", ["t12-views-v2m", "t12-views-vpm"])
def test_one_shading_image_expanded_over_both_mpis(name):
    """The leaf is ONE image [1,1,Ht,Wt], the render gets its `expand` over the two MPIs: the leaf's gradient is the sum over both, in the float64
    reference and through the kernels (full run and shading-only run)."""
    case = C.twin_case(name, True)
    one = case["shading"][:1]
    refs = C.twin_refs(name, True, one_shading=True)
    both = np.repeat(one, case["M"], 0)
    expand = lambda v, s: (v, s.expand(case["M"], -1, -1, -1))
    failures = {}
    for variant in VARIANTS:
        for needs in ((True, True), (False, True)):
            vol, s = _grads(name, variant, needs=needs, prep=expand, shading=one)
            assert s.shape == (1, 1) + case["rgba"].shape[-2:]
            if needs[0]:
                _check_volume(name, f"{variant} expanded", vol.grad, refs, failures, s=both)
            _check_shading(name, f"{variant} expanded needs={needs}", s.grad, refs, failures)
    assert not failures, failures


PAD = 6


def _padded_rows(x, fill):
    """A view of x's values inside rows of Wt + 6 elements, the padding filled with `fill`; differentiable w.r.t. x."""
    buf = torch.full(x.shape[:-1] + (x.shape[-1] + PAD,), fill, device=x.device, dtype=x.dtype)
    buf[..., :x.shape[-1]] = x
    v = buf[..., :x.shape[-1]]
    assert v.stride(-2) == x.shape[-1] + PAD and v.stride(-1) == 1
    return v


def test_row_padded_shading_and_row_padded_volume():
    """Wt = 50 in rows of 56 elements.  The shading as such a view, its padding NaN, requiring no grad: the volume gradient is finite and meets the
    rule (a kernel that read the shading at the gradient's or the volume's row stride would pick the NaNs up).  Then the volume as such a view (the
    shading contiguous, both gradients wanted): the gradient the backward returns for the view is contiguous, of the view's shape, and meets the rule."""
    name = "t12-ragged"
    refs = C.twin_refs(name, True)
    failures = {}
    for variant in VARIANTS:
        vol, s = _grads(name, variant, needs=(True, False), prep=lambda v, s: (v, _padded_rows(s, float("nan"))))
        assert s.grad is None and bool(torch.isfinite(vol.grad).all())
        _check_volume(name, f"{variant} padded shading", vol.grad, refs, failures)
        seen = []

        def padded_volume(v, s):
            view = _padded_rows(v, 7.0)
            view.register_hook(lambda g: seen.append((g.is_contiguous(), tuple(g.shape), g.dtype)))
            return view, s
        vol, s = _grads(name, variant, prep=padded_volume)
        assert seen == [(True, tuple(vol.shape), vol.dtype)], seen
        _check_volume(name, f"{variant} padded volume", vol.grad, refs, failures)
        _check_shading(name, f"{variant} padded volume", s.grad, refs, failures)
    assert not failures, failures
