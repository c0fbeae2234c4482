"""Backward kernels on stacks in which every plane counts, compared PER PLANE.  On the white-noise volumes of tests/test_hip_backward.py 79 of
98 gradient planes are smaller than the per-tensor bar, so a sweep that zeroed, doubled or misplaced planes 19-97 passes, and the backward always
takes the path that rebuilds an underflowed T_out.  Here (tests/_deep_cases.py) T_out is healthy through 32-129 planes and every (MPI, plane,
channel) slab of the gradient is held to max(5e-5, 4 e_ref) of ITS OWN maximum (tests/_visible.py `slab_compare`; e_ref = fp32 vs float64 of the
same chain on the CPU, <= 1e-4 and every slab >= 1e-3 of the tensor's maximum by tests/test_visible_stacks_cpu.py).
Run on the MI355X box:  python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch

import _deep_cases as C
import test_hip_shared_color as shared
from _geometry_ref import geometry_grads
from _visible import slab_compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# tile backward (one-pixel-per-lane kernel from D = 129 on), the all-atomic kernel, the atomics-free pixel-pass + texel-gather pair
PATHS = {"tile": dict(variant="auto"), "all-atomic": dict(variant="gather"), "gather-pair": dict(backward="gather")}


def _hip_volume_grad(case, path):
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    vol = t(case["rgba"]).to(case["dtype"]).requires_grad_(True)
    assert torch.equal(vol.detach().float().cpu(), torch.from_numpy(case["rgba"]))   # the references were fed the stored values
    mpi = MPI(align_corners=True, on_out_of_plane="raise", **PATHS[path])
    uniform = case["N"] == case["M"]
    kw = dict(views_per_mpi=1) if uniform else dict(view_to_mpi=t(case["v2m"]))
    out = mpi.render_views(vol, t(case["dhw"]), t(case["ray"]), t(case["eye"]), t(case["zd"]), check_last_plane=False, want_transmittance=True, **kw)
    assert float(out["T"].max()) > 1e-3   # the ordinary path: a T_out that did not underflow
    ((out["color"] * t(case["gc"])).sum() + (out["depth"] * t(case["gd"])).sum() + (out["T"] * t(case["gT"])).sum()).backward()
    assert vol.grad.dtype == case["dtype"]
    return vol.grad.double().cpu().numpy()


@pytest.mark.parametrize("name", list(C.GRAD_CASES))
def test_volume_gradient_per_slab(name):
    """D = 32, 97 (two table chunks), 129 on thin and surface stacks, 96 x 160 pixels (several tiles both ways), one rotated camera, one bf16
    and one fp16 volume, uniform views and one ragged view_to_mpi; loss over colour, depth and T; every backward path."""
    case = C.grad_case(name)
    ref64, ref32 = C.volume_grad_ref(case, torch.float64), C.volume_grad_ref(case, torch.float32)
    failures = {}
    for path in PATHS:
        res = slab_compare(_hip_volume_grad(case, path), ref64, ref32, case["dtype"], label=f"{name} {path}:")
        assert res["skipped"] == 0
        if res["failures"]:
            failures[path] = (len(res["failures"]), res["worst"], res["where"], res["failures"][:5])
    assert not failures, failures


@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("cfg", C.SHARED_GRAD, ids=lambda c: f"D{c['D']}")
def test_shared_colour_gradient_alpha_per_plane(cfg, with_bg):
    """rgb, alpha and background gradients of the shared-colour backward on a thin stack: rgb and background as tests/test_hip_shared_color.py
    compares them, the alpha gradient per (MPI, plane) slab."""
    parts, dhw, ray, eye, zd, v2m, gc, gd, gT = C.shared_grad_case(cfg, with_bg)
    ref64 = shared._reference_grads(parts, dhw, ray, eye, zd, v2m, gc, gd, gT, False, torch.float64)
    ref32 = shared._reference_grads(parts, dhw, ray, eye, zd, v2m, gc, gd, gT, False, torch.float32)
    failures = {}
    for variant in ("auto", "gather"):
        ins, out = shared._hip_grads(parts, dhw, ray, eye, zd, 2, gc, gd, gT, False, variant)
        assert float(out["T"].max()) > 1e-3
        got = [None if i is None else i.grad.double().cpu().numpy() for i in ins]
        shared._compare(got, ref64, ref32, torch.float32, f"thin D={cfg['D']} {variant}", True, with_bg)
        res = slab_compare(got[1], ref64[1], ref32[1], label=f"shared colour thin D={cfg['D']} bg={with_bg} {variant} alpha:")
        assert res["skipped"] == 0
        if res["failures"]:
            failures[variant] = (len(res["failures"]), res["worst"], res["where"], res["failures"][:5])
    assert not failures, failures


@pytest.mark.parametrize("cfg", C.GEOMETRY, ids=lambda c: f"D{c['D']}")
def test_geometry_pass_plane_gradient_per_row(cfg):
    """MPI(geometry_grad=True): dhw.grad is a per-plane quantity -- every (MPI, plane) row against the float64 oracle of tests/_geometry_ref.py
    with the bar of tests/test_hip_geometry_grad.py's `_check` (1e-4, strict-order mode) applied to the row's own maximum, on a thin smooth
    stack (every plane's row carries weight: asserted)."""
    import test_hip_geometry_grad as geo
    rgba, dhw, ray, eye, zd, v2m, gc, gd = C.geometry_case(cfg)
    got, stored = geo._run(rgba, dhw, ray, eye, zd, v2m, gc, gd, True, True, views_per_mpi=1)
    ref = geometry_grads(stored, dhw, ray, eye, zd, v2m, gc, gd, align_corners=True)
    geo._check(got, ref)
    g_dhw, r_dhw = got[0], ref[0]
    row_max = np.abs(r_dhw).max(axis=2)                          # [M,D]
    assert row_max.min() >= 1e-3 * row_max.max(), (row_max.min(), row_max.max())
    ratio = np.abs(g_dhw - r_dhw).max(axis=2) / (1e-4 * row_max)
    print(f"geometry D={cfg['D']}: row max min {row_max.min():.2e} max {row_max.max():.2e}; worst row ratio {ratio.max():.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}")
    assert ratio.max() <= 1.0, (ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))
