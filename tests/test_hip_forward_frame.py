"""The frame every forward kernel shares around its plane loop (gmpi_device.hpp: view_setup, check_camera_behind, leaves_last_plane,
store_pixel): the parts other tests reach through one variant or one shape only, on every kernel variant and on the smallest shapes that put
a partial tile behind a full one in each of them.  All expected values are exact."""
import functools

import numpy as np
import pytest
import torch

import oracle
from test_hip_edge_cases import _cam, _dhw
from test_hip_parity import variants

pytestmark = pytest.mark.gpu

N = M = 2
D = 3
T = 32  # texture height and width
# H x W: 19 x 130 is past two 64-pixel gather waves, four 32-pixel tiles / strips and one 128-pixel fp32 band, and past two 8-row strips /
# bands and one 16-row tile; 11 x 258 is past one 256-pixel 16-bit band.
CASES = {"f32_19x130": (19, 130, torch.float32), "bf16_11x258": (11, 258, torch.bfloat16)}
GRID = [(c, ac) for c in CASES for ac in (True, False)]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    H, W, dtype = CASES[case]
    rgba = oracle.synth_rgba(51, (M, D, 4, T, T), bf16_round=dtype == torch.bfloat16)
    ray, eye, zd = _cam(N, H, W, seed=6)
    return rgba, _dhw(M, D), ray, eye, zd


def _render(case, ac, variant, *, out_pm1=False, want_T=True, check_last=True, ray=None, dhw=None):
    from ml_gmpi_amd import MPI, GmpiError
    rgba, dhw0, ray0, eye, zd = _inputs(case)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = (t(rgba).to(CASES[case][2]), t(dhw0 if dhw is None else dhw), t(ray0 if ray is None else ray), t(eye), t(zd))
    kw = dict(views_per_mpi=1, check_last_plane=check_last, want_transmittance=want_T, out_pm1=out_pm1)
    mpi = MPI(align_corners=ac, variant=variant, range_check="touched", on_out_of_plane="raise")
    with torch.no_grad():
        try:
            out = mpi.render_views(*args, **kw)
        except GmpiError as e:  # a staged kernel that cannot take the shape refuses it; "auto" then renders (as test_hip_parity.hip_render)
            if variant not in ("lds", "wave", "band") or "GMPI_E_VARIANT" not in str(e):
                raise
            mpi.variant = "auto"
            out = mpi.render_views(*args, **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _base(case, ac, variant):
    """The plain render (colour in [0, 1], T wanted, last-plane check on): computed once, shared, never modified."""
    return _render(case, ac, variant)


@pytest.mark.parametrize("case,ac", GRID)
def test_out_pm1_is_two_c_minus_one(case, ac):
    for variant in variants():
        base, pm1 = _base(case, ac, variant), _render(case, ac, variant, out_pm1=True)
        assert int(base["status"][0]) == 0 and int(pm1["status"][0]) == 0
        # 2 c is exact, the subtraction rounds once -- on the device and here
        assert np.array_equal(pm1["color"], np.float32(2) * base["color"] - np.float32(1)), (case, ac, variant)
        assert np.array_equal(pm1["depth"], base["depth"]) and np.array_equal(pm1["T"], base["T"]), (case, ac, variant)


@pytest.mark.parametrize("case,ac", GRID)
def test_transmittance_not_wanted(case, ac):
    for variant in variants():
        base, out = _base(case, ac, variant), _render(case, ac, variant, want_T=False)
        assert out.get("T") is None, (case, ac, variant)
        assert np.array_equal(out["color"], base["color"]) and np.array_equal(out["depth"], base["depth"]), (case, ac, variant)


@pytest.mark.parametrize("corner", ["first", "last"])
@pytest.mark.parametrize("case,ac", GRID)
def test_one_pixel_leaves_the_last_plane(case, ac, corner):
    """One ray of view N - 1 bent far sideways -- pixel (0, 0), or (H - 1, W - 1) inside the partial tile of every kernel -- sets the bit."""
    H, W, _ = CASES[case]
    rgba, dhw, ray, eye, zd = _inputs(case)
    y, x = (0, 0) if corner == "first" else (H - 1, W - 1)
    bent = ray.copy()
    bent[N - 1, :, y, x] = np.array([0.8, 0.0, 0.6], np.float32)
    inside = lambda uv: (uv[:, 0] >= -1) & (uv[:, 1] <= 1) & (uv[:, 2] >= -1) & (uv[:, 3] <= 1)
    # what makes the test mean something: only the bend takes a view out of [-1, 1], and only view N - 1
    assert inside(oracle.render(rgba, dhw, ray, eye, zd, align_corners=ac)["uv_minmax"]).all()
    assert inside(oracle.render(rgba, dhw, bent, eye, zd, align_corners=ac)["uv_minmax"]).tolist() == [True] * (N - 1) + [False]
    for variant in variants():
        assert int(_base(case, ac, variant)["status"][0]) == 0, (case, ac, variant)
        with pytest.raises(RuntimeError, match="goes out of plane"):
            _render(case, ac, variant, ray=bent)


@pytest.mark.parametrize("case,ac", GRID)
def test_camera_behind_a_plane_of_the_last_mpi(case, ac):
    """mpi.py:70-72 compares every plane of every MPI with eye_z of the FIRST view: one plane of MPI M - 1 just below it, view 0's own MPI fine."""
    rgba, dhw, ray, eye, zd = _inputs(case)
    behind = dhw.copy()
    behind[M - 1, D - 1, 0] = np.nextafter(eye[0][2], np.float32(-np.inf))
    assert behind[M - 1, D - 1, 0] < eye[0][2] and (behind[0, :, 0] >= eye[0][2]).all()
    for variant in variants():
        with pytest.raises(AssertionError, match="Camera must be placed closer"):
            _render(case, ac, variant, dhw=behind, check_last=False)
        assert int(_render(case, ac, variant, check_last=False)["status"][0]) == 0, (case, ac, variant)  # the one value put back
