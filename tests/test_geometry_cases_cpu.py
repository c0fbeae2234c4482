"""The conditions under which tests/test_hip_geometry_outputs.py means something, checked without a GPU on the inputs of tests/_geometry_cases.py and
their float64 references alone: the frames' tile counts against the reducers' width (read out of render_backward_geometry.hip), the workspace
restatement, that no reference gradient is trivially zero, that every plane of the deep layout cases carries weight, that an MPI without a view has
an exactly zero reference row -- and, on the recording library, that the VOLUME path hands the C entry exactly the outputs that are wanted, for every
subset (tests/test_geometry_layouts_cpu.py pins the same for the two layouts)."""
import itertools

import numpy as np
import pytest

import _geometry_cases as G
from ml_gmpi_amd.hip_mpi import MPI
from test_geometry_layouts_cpu import GEO_NAMES, QUERY, _check_outputs, _with_grad, rec  # noqa: F401  (rec: the recorder fixture)

SUBSETS = [s for r in range(1, 5) for s in itertools.combinations(GEO_NAMES, r)]
UNUSED = [((2,), (0, 1)), ((2, 2, 0), (1,))]   # (view_to_mpi over M = 3, the MPIs no view points to)


# ---- the frames against the kernel's constants -----------------------------------------------------------------------------------------------------------
def test_tile_counts_reach_the_second_and_third_trip_of_the_reducers():
    c = G.constants()
    assert (c["kGTW"], c["kGTH"]) == (64, 4)   # (the counts below are stated for this tile)
    assert {f: G.tiles(*hw) for f, hw in G.FRAMES.items()} == dict(TALL=258 * 2, WIDE=5 * 52, ROW=1, COL=10, SMALL=3 * 2, DEEP=10 * 2)
    assert G.tiles(*G.FRAMES["TALL"]) > 2 * c["kGRed"] and G.tiles(*G.FRAMES["WIDE"]) > c["kGRed"]
    assert G.tiles(*G.FRAMES["TALL"]) % 8 != 0                                    # the tile remap's grid is padded
    for f in ("TALL", "WIDE", "SMALL"):                                            # ragged on both axes
        assert G.FRAMES[f][0] % c["kGTH"] != 0 and G.FRAMES[f][1] % c["kGTW"] != 0, f
    assert G.FRAMES["ROW"][0] == 1 and G.FRAMES["COL"][1] == 1
    assert max(G.DEEP_D) > c["kGChunk"] and 98 > c["kGChunk"]                      # the deep cases and SMALL / D = 98 cross the chunk boundary


def test_workspace_restatement():
    # (a frame of one tile can round both dhw forms up to the same 256 bytes: the plane_z part alone is rounded on its own)
    for (H, W), D, N in ((G.FRAMES["SMALL"], 98, 2), (G.FRAMES["TALL"], 4, 2), (G.FRAMES["SMALL"], 6, 2), (G.FRAMES["WIDE"], 4, 3)):
        f = lambda dhw, pz: G.workspace_floats(N, H, W, D, dhw, pz)
        assert f(False, False) < f(True, False) and f(False, True) < f(True, True)      # strictly increasing in dhw ...
        assert f(False, False) < f(False, True) and f(True, False) < f(True, True)      # ... and in plane_z
        pz_part = (4 * D * N * G.tiles(H, W) + 255) // 256 * 64
        assert f(True, True) == f(True, False) + pz_part and f(False, True) == f(False, False) + pz_part
        assert all(f(a, b) % 64 == 0 for a in (False, True) for b in (False, True))     # 256-byte parts
        assert f(False, False) >= 6 * N * G.tiles(H, W) and f(True, False) >= (6 + 3 * D) * N * G.tiles(H, W)


# ---- the references ---------------------------------------------------------------------------------------------------------------------------------------
def _frame_case(source, frame, **kw):
    if frame in ("TALL", "WIDE"):
        return G.case(source, frame, 4, M=1, v2m=(0, 0), vpm=2, **kw)
    return G.case(source, frame, 6, **kw)


@pytest.mark.parametrize("frame", ["TALL", "WIDE", "ROW", "COL", "SMALL"])
@pytest.mark.parametrize("source", G.SOURCES)
def test_every_reference_gradient_is_finite_and_non_zero(source, frame):
    c = _frame_case(source, frame)
    assert c.ray.shape == (c.N, 3) + G.FRAMES[frame] and c.ray.flags["C_CONTIGUOUS"]
    ref = G.reference(c)
    assert set(ref) == set(G.GEO) | ({"pz"} if source == "depth" else set())
    for k, r in ref.items():
        assert np.all(np.isfinite(r)) and np.abs(r).max() > 0, k
    for n in range(c.N):   # (`_check` holds eye and z_dir per view)
        assert np.linalg.norm(ref["eye"][n]) > 0 and np.linalg.norm(ref["zd"][n]) > 0


def test_the_line_frames_are_slices_of_one_camera():
    from test_hip_edge_cases import _cam
    full = _cam(2, G.LINE_CAMERA, G.LINE_CAMERA, seed=62, tilt=0.3)[0]
    assert np.array_equal(G.camera("ROW", 2)[0][:, :, 0], full[:, :, G.LINE_ROW]) and np.array_equal(G.camera("COL", 2)[0][:, :, :, 0], full[:, :, :, G.LINE_COL])


@pytest.mark.parametrize("D", G.DEEP_D)
@pytest.mark.parametrize("layout", ["shared", "depth"])
def test_every_plane_of_the_deep_layout_cases_carries_weight(layout, D):
    """The volume test's own condition (tests/test_hip_deep_gradients.py::test_geometry_pass_plane_gradient_per_row), with no exempt row."""
    c = G.layout_deep_case(layout, D)
    assert (c.H, c.W) == G.FRAMES["DEEP"] and c.images[0].shape[2:] == (G.HT, G.WT) and c.with_T == (layout == "depth")
    ref = G.reference(c)
    row_max = np.abs(ref["dhw"]).max(axis=2)
    print(f"{layout} D={D}: dhw row max, min / max = {row_max.min() / row_max.max():.3e}")
    assert row_max.min() >= 1e-3 * row_max.max(), (row_max.min(), row_max.max())
    if layout == "depth":
        vol = G.expanded(c)
        a = vol[:, :, 3]
        assert np.all((a > 0).any(axis=(2, 3)) & (a < 1).any(axis=(2, 3)))   # every plane is on the ramp somewhere
        pz = np.abs(ref["pz"])
        assert pz.shape == (c.M, D)
        print(f"depth D={D}: |plane_z.grad| min / max per MPI = {pz.min(axis=1) / pz.max(axis=1)}")
        assert np.all(pz.min(axis=1) >= 1e-3 * pz.max(axis=1)), (pz.min(axis=1), pz.max(axis=1))
        assert np.all(np.sign(ref["pz"]) == np.sign(ref["pz"][0, 0]))        # one sign: no plane's sum is a cancellation (see layout_deep_case)


@pytest.mark.parametrize("v2m,unused", UNUSED)
@pytest.mark.parametrize("source", G.SOURCES)
def test_an_mpi_without_a_view_has_an_exactly_zero_reference_row(source, v2m, unused):
    c = G.case(source, "SMALL", 6, M=3, v2m=v2m, pz_rows=source == "depth")
    ref = G.reference(c)
    used = sorted(set(v2m))
    assert np.all(ref["dhw"][list(unused)] == 0.0) and all(np.abs(ref["dhw"][m]).max() > 0 for m in used)
    if source == "depth":
        assert ref["pz"].shape == (3, 6) and np.all(ref["pz"][list(unused)] == 0.0) and all(np.abs(ref["pz"][m]).max() > 0 for m in used)
    nan = G.expanded(c, G.with_nan(c, unused))
    assert np.all(np.isnan(nan[list(unused)])) and np.array_equal(nan[used], G.expanded(c)[used])


# ---- the volume path on the recording library ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uses_T", [False, True])
@pytest.mark.parametrize("names", SUBSETS, ids="+".join)
def test_volume_bridge_hands_over_exactly_the_wanted_outputs(rec, names, uses_T):  # noqa: F811
    from test_marshal_cpu import make_inputs
    vol, *geo = make_inputs(2)
    geo = _with_grad(geo, names)
    res = MPI(geometry_grad=True).render_views(vol, *geo, want_transmittance=True)
    loss = (res["color"] * 0.5).sum() + res["depth"].sum()
    (loss + (res["T"] * 2.0).sum() if uses_T else loss).backward()
    slabs = any(n in names for n in ("dhw", "eye_pos", "z_dir"))
    entry = "gmpi_mpi_render_geometry_backward_ex_launch" if uses_T else "gmpi_mpi_render_geometry_backward_launch"
    assert [c.name for c in rec.calls] == ["gmpi_mpi_render_launch"] + ([QUERY] if slabs else []) + [entry]
    bwd = rec.calls[-1]
    _check_outputs(bwd, 4 if uses_T else 3, geo, names)
    assert (bwd.args[0].workspace is not None) == slabs           # only `ray_dir` wanted: no workspace, no query
    if slabs:
        assert rec.named(QUERY)[0].args[1] == int("dhw" in names)   # want_dhw
    assert vol.grad is None
