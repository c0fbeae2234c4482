"""The geometry pass (render_backward_geometry.hip), one output at a time and past one trip of its reductions, on the inputs of
tests/_geometry_cases.py (conditions on them: tests/test_geometry_cases_cpu.py).  Every comparison is with the float64 oracle of
tests/_geometry_ref.py (tests/_transmittance_ref.py where the loss reaches T, tests/test_hip_plane_z_grad.py `_reference` for plane_z) under the bars
of tests/test_hip_geometry_grad.py `_check`, unchanged: strict-order mode on white noise, x 10 in the default mode on smooth inputs.
  (a) every non-empty subset of the outputs on the three tap sources: an unwanted input gets no gradient, a wanted one meets its own bar and is, bit
      for bit, what the run that wants everything gives (the DHW = false instances, the launch without a slab, the launch without g_ray);
  (b) frames of 516 and 260 tiles: the reducers' second and third trip, the padded tile remap, two views adding into one dhw row;
  (c) frames one pixel high and one pixel wide;
  (d) MPIs no view points to: their rows are exactly 0, whatever their images hold;
  (e) the workspace through the C entry: exactly the queried bytes are enough, nothing behind them is written, every summed slot was written;
  (f) per-plane bars for the shared-colour and depth-alpha sources, dhw per (MPI, plane) row and plane_z per element.
Run on the MI355X box:  python -m pytest tests -m gpu"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _geometry_cases as G
from test_hip_geometry_grad import _check
from test_hip_geometry_layouts import _render
from test_hip_plane_z_grad import _bar

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GEO = G.GEO
E_WORKSPACE = -8


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _names(source):
    return GEO + (("pz",) if source == "depth" else ())


def _subsets(names):
    return [s for r in range(1, len(names) + 1) for s in itertools.combinations(names, r)]


# ---- the device side ----------------------------------------------------------------------------------------------------------------------------------
def _run(c, needs, ac=True, strict=True, dtype=torch.float32, with_T=None, images=None):
    """One render and backward of case `c`; `needs`: the names among dhw, ray, eye, zd, pz that require grad -> {name: gradient as numpy or None}."""
    from ml_gmpi_amd import MPI
    images = c.images if images is None else images
    with_T = c.with_T if with_T is None else with_T
    geo = [_t(c[k]).requires_grad_(k in needs) for k in GEO]
    kw = dict(views_per_mpi=c.vpm) if c.vpm is not None else dict(view_to_mpi=_t(c.v2m))
    pz = None
    if c.source == "volume":
        mpi = MPI(align_corners=ac, strict_order=strict, on_out_of_plane="raise", geometry_grad=True)
        out = mpi.render_views(_t(images[0]).to(dtype), *geo, check_last_plane=False, want_transmittance=with_T, **kw)
    else:
        rgb, mid, bg, pz = (None if a is None else _t(a) for a in images)
        if pz is not None:
            pz.requires_grad_("pz" in needs)
        mpi = MPI(align_corners=ac, strict_order=strict, on_out_of_plane="raise", geometry_grad="all")
        out = _render(mpi, c.source, rgb.to(dtype), mid.to(dtype), bg.to(dtype), pz, c.zb, geo, want_transmittance=with_T, **kw)
    loss = (out["color"] * _t(c.gc)).sum() + (out["depth"] * _t(c.gd)).sum()
    if with_T:
        loss = loss + (out["T"] * _t(c.gT)).sum()
    loss.backward()
    torch.cuda.synchronize()
    got = {k: None if t.grad is None else t.grad.cpu().numpy() for k, t in zip(GEO, geo)}
    got["pz"] = None if pz is None or pz.grad is None else pz.grad.cpu().numpy()
    return got


_ALL = {}


def _all_wanted(c, ac=True, strict=True, dtype=torch.float32, with_T=None):
    """The run that wants every output of the case (once per configuration)."""
    key = (c.key, ac, strict, dtype, with_T)
    if key not in _ALL:
        _ALL[key] = _run(c, _names(c.source), ac, strict, dtype, with_T)
    return _ALL[key]


def _ratios(got, ref, needs):
    """{name: error / `_check`'s allowance} of the wanted outputs (printed; the assertions are `_check`'s and `_bar`'s own)."""
    out = {}
    for k in needs:
        g, r = got[k].astype(np.float64), ref[k]
        if k == "ray":
            out[k] = np.abs(g - r).max() / (1e-4 * np.abs(r).max())
        elif k in ("eye", "zd"):
            out[k] = max(np.linalg.norm(g[n] - r[n]) / (1e-4 * np.linalg.norm(r[n])) for n in range(g.shape[0]))
        else:
            out[k] = np.linalg.norm(g - r) / (1e-4 * np.linalg.norm(r))
    return out


def _check_wanted(label, got, ref, needs, scale=1.0):
    """`_check` and, for plane_z, `_bar` on the wanted outputs, each against its own reference tensor alone (an unwanted one is replaced by its
    reference: it adds no scale and no error)."""
    for k in _names("depth"):
        assert (got[k] is not None) == (k in needs), (label, k)
    print(f"{label}: error / allowed " + ", ".join(f"{k} {v / scale:.3f}" for k, v in _ratios(got, ref, needs).items()))
    for k in needs:
        assert got[k].shape == ref[k].shape and np.all(np.isfinite(got[k])), (label, k)
    _check([got[k] if k in needs else ref[k] for k in GEO], [ref[k] for k in GEO], scale)
    if "pz" in needs:
        _bar(got["pz"], ref["pz"], scale)


def _assert_same_bits(label, got, want, names):
    for k in names:
        assert np.array_equal(got[k], want[k]), (label, k, float(np.abs(got[k] - want[k]).max()))


# ---- (a) every subset of the outputs --------------------------------------------------------------------------------------------------------------------
def _subset_test(c, needs, ac=True, dtype=torch.float32, with_T=False):
    label = f"{c.source} {c.frame} D={c.D} ac={int(ac)} {'+'.join(needs)}"
    ref = G.reference(c, ac, with_T)
    got = _run(c, needs, ac, True, dtype, with_T)
    _check_wanted(label, got, ref, needs)
    _assert_same_bits(label, got, _all_wanted(c, ac, True, dtype, with_T), needs)


SUBSET_CASES = [(s, ac, needs) for s in G.SOURCES for ac in (True, False) for needs in _subsets(_names(s))]


@pytest.mark.parametrize("source,ac,needs", SUBSET_CASES, ids=lambda v: "+".join(v) if isinstance(v, tuple) else (f"ac{int(v)}" if isinstance(v, bool) else v))
def test_every_subset_of_the_outputs(source, ac, needs):
    """SMALL / D = 6, strict-order mode.  15 subsets of (dhw, ray, eye, zd) on the volume and the shared-colour source, 31 with plane_z on the
    depth-alpha source: DHW on and off, the slab with and without g_ray, no slab at all, the PZ instances with and without the (d, h, w) components."""
    _subset_test(G.case(source, "SMALL", 6), needs, ac)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("needs", [("ray",), ("eye",), ("dhw",), ("eye", "zd")], ids="+".join)
def test_volume_subsets_past_the_plane_chunk(needs, dtype):
    """D = 98: the second chunk of 96 planes with and without the per-plane sums; once on a bf16 volume."""
    bf16 = dtype == "bf16"
    _subset_test(G.case("volume", "SMALL", 98, bf16=bf16), needs, True, torch.bfloat16 if bf16 else torch.float32)


@pytest.mark.parametrize("needs", [("ray",), ("dhw",), ("eye", "zd")], ids="+".join)
def test_volume_subsets_with_a_loss_through_T(needs):
    """The `_ex` entry: S starts at gT T_out."""
    _subset_test(G.case("volume", "SMALL", 6), needs, True, with_T=True)


# ---- (b) long reductions ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["strict", "default"])
@pytest.mark.parametrize("source,pz_rows", [("volume", False), ("shared", False), ("depth", False), ("depth", True)],
                         ids=["volume", "shared", "depth", "depth-pz_rows"])
@pytest.mark.parametrize("frame", ["TALL", "WIDE"])
def test_frames_of_hundreds_of_tiles(frame, source, pz_rows, mode):
    """516 and 260 tiles, two views of one MPI (their slabs add into one dhw row, in view order), D = 4: strict-order mode on white noise, the default
    mode on smooth inputs at x 10; two runs give the same bits.  depth: plane_z as [D] and as [M, D]."""
    strict = mode == "strict"
    c = G.case(source, frame, 4, M=1, v2m=(0, 0), vpm=2, smooth=not strict, pz_rows=pz_rows)
    names = _names(source)
    a, b = _run(c, names, True, strict), _run(c, names, True, strict)
    if source == "depth":
        assert a["pz"].shape == ((1, 4) if pz_rows else (4,))
    label = f"{source}{' pz_rows' if pz_rows else ''} {frame} {mode}"
    _check_wanted(label, a, G.reference(c, True), names, scale=1.0 if strict else 10.0)
    _assert_same_bits(label, a, b, names)


# ---- (c) one-pixel frames -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ac", [True, False], ids=["ac1", "ac0"])
@pytest.mark.parametrize("source", G.SOURCES)
@pytest.mark.parametrize("frame", ["ROW", "COL"])
def test_frames_one_pixel_high_or_wide(frame, source, ac):
    """1 x 40: three of the four waves hold no pixel, 24 lanes of the fourth neither; 40 x 1: 63 inactive lanes in every wave."""
    c = G.case(source, frame, 6)
    names = _names(source)
    label = f"{source} {frame} ac={int(ac)}"
    full = _all_wanted(c, ac)
    _check_wanted(label, full, G.reference(c, ac), names)
    eye = _run(c, ("eye",), ac)
    assert all(eye[k] is None for k in names if k != "eye")
    _assert_same_bits(label, eye, full, ("eye",))


# ---- (d) MPIs without views ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", G.SOURCES)
@pytest.mark.parametrize("v2m,unused", [((2,), (0, 1)), ((2, 2, 0), (1,))], ids=["N1-v2m2", "N3-v2m220"])
def test_mpis_without_views_get_exactly_zero_rows(v2m, unused, source):
    """M = 3.  The reducer's grid is max(N, M) high so that these rows are written: they are exactly 0.0 (the outputs are torch.empty), the used rows
    meet the oracle bar, and NaN in the unused MPIs' images changes no bit (plane_z [M, D] on the depth-alpha source)."""
    c = G.case(source, "SMALL", 6, M=3, v2m=v2m, pz_rows=source == "depth")
    names = _names(source)
    label = f"{source} v2m={list(v2m)}"
    # (fill the caching allocator's free blocks with NaN first: an output row nobody writes then shows)
    junk = [torch.full((n,), float("nan"), device=DEV) for n in (3 * 6 * 3, 3 * 6, 128, 512)]
    del junk
    got = _run(c, names)
    for k in ("dhw",) + (("pz",) if source == "depth" else ()):
        assert got[k].shape[0] == 3
        assert np.all(got[k][list(unused)] == 0.0), (label, k, got[k][list(unused)])
    _check_wanted(label, got, G.reference(c), names)
    nan = _run(c, names, images=G.with_nan(c, unused))
    _assert_same_bits(label + " NaN in the unused MPIs", nan, got, names)


# ---- (e) the workspace, through the C entry -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_dhw,want_pz", [(False, False), (True, False), (False, True), (True, True)], ids=["eye-zd", "dhw", "pz", "dhw-pz"])
@pytest.mark.parametrize("frame,D", [("SMALL", 98), ("TALL", 4)])
def test_exactly_the_queried_workspace_is_enough_and_nothing_behind_it_is_written(frame, D, want_dhw, want_pz):
    """gmpi_mpi_render_depth_geometry_backward_pz_launch (grad_plane_z NULL: the entry without it) with the four forms of its workspace query.  The
    workspace is the first `need` bytes of a buffer of need + 4096 bytes of 0xFF (every float a NaN), the outputs are prefilled with NaN: afterwards
    the last 4096 bytes are untouched, every output is finite (a slot that is summed and was never written is a NaN) and equals the autograd run's
    bits.  With one byte less the entry refuses and writes nothing."""
    from ml_gmpi_amd import MPI, _lib
    from ml_gmpi_amd.hip_mpi import _Keep, _Scalars, _depth_alpha, _render_params, _shared_color
    lib = _lib.load_library()
    c = G.case("depth", frame, D) if frame == "SMALL" else G.case("depth", frame, D, M=1, v2m=(0, 0), vpm=2)
    rgb, depth, bg, pz = (_t(a) for a in c.images)
    dhw, ray, eye, zd = (_t(c[k]) for k in GEO)
    v2m = _t(c.v2m)
    with torch.no_grad():
        fwd = MPI(align_corners=True, strict_order=True, on_out_of_plane="raise").render_views_depth(
            rgb, depth, pz, c.zb, dhw, ray, eye, zd, background=bg, check_last_plane=False, want_transmittance=True, view_to_mpi=v2m)
    T = fwd["T"].contiguous()
    flags = _lib.FLAG_ALIGN_CORNERS | _lib.FLAG_STRICT_ORDER
    p = _render_params(_Scalars(flags, _lib.VARIANT_AUTO, _lib.DTYPE_F32, c.N, c.M, D, G.HT, G.WT, c.H, c.W, 1),
                       _Keep(depth.unsqueeze(1), dhw, ray, eye, zd, v2m), T=T)
    sc, da = _shared_color(rgb, bg), _depth_alpha(pz, *c.zb)
    need = int(lib.gmpi_render_depth_geometry_backward_workspace_bytes(ctypes.byref(p), int(want_dhw), int(want_pz)))
    assert need == 4 * G.workspace_floats(c.N, c.H, c.W, D, want_dhw, want_pz)
    if not want_pz:
        assert need == int(lib.gmpi_render_geometry_backward_workspace_bytes(ctypes.byref(p), int(want_dhw)))
    GUARD = 4096
    buf = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    gc, gd = _t(c.gc), _t(c.gd)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    shapes = dict(ray=(c.N, 3, c.H, c.W), eye=(c.N, 3), zd=(c.N, 3), dhw=(c.M, D, 3), pz=tuple(pz.shape))
    needs = ("ray", "eye", "zd") + (("dhw",) if want_dhw else ()) + (("pz",) if want_pz else ())

    def launch(nbytes):
        o = {k: torch.full(shapes[k], float("nan"), device=DEV) for k in needs}
        p.workspace, p.workspace_bytes = buf.data_ptr(), nbytes
        ptr = lambda k: o[k].data_ptr() if k in o else None
        rc = lib.gmpi_mpi_render_depth_geometry_backward_pz_launch(ctypes.byref(p), ctypes.byref(sc), ctypes.byref(da), gc.data_ptr(), gd.data_ptr(), None,
                                                                   ptr("ray"), ptr("eye"), ptr("zd"), ptr("dhw"), ptr("pz"), stream)
        torch.cuda.synchronize()
        return rc, {k: v.cpu().numpy() for k, v in o.items()}

    rc, untouched = launch(need - 1)
    assert rc == E_WORKSPACE
    assert all(np.all(np.isnan(v)) for v in untouched.values()) and bool((buf == 0xFF).all())
    rc, got = launch(need)
    _lib.check(rc, "gmpi_mpi_render_depth_geometry_backward_pz_launch")
    assert bool((buf[need:] == 0xFF).all()), "bytes behind the lent workspace were written"
    for k in needs:
        assert np.all(np.isfinite(got[k])), (k, int((~np.isfinite(got[k])).sum()))
    want = _run(c, needs)
    _assert_same_bits(f"depth {frame} D={D} {'+'.join(needs)}", got, want, needs)


# ---- (f) per-plane bars for the two layouts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", G.DEEP_D)
@pytest.mark.parametrize("layout", ["shared", "depth"])
def test_layout_gradients_per_plane(layout, D):
    """tests/_geometry_cases.py `layout_deep_case`, strict-order mode.  dhw.grad: every (MPI, plane) row within 1e-4 of ITS OWN maximum, the rule of
    tests/test_hip_deep_gradients.py::test_geometry_pass_plane_gradient_per_row.  plane_z.grad, per element: within
    1e-4 max(|ref[m, k]|, 1e-2 max_k |ref[m, :]|) -- the pass's 1e-4, with a floor that keeps a plane's scalar sum from setting a bar below fp32
    summation error; 100 times tighter than the norm over all planes.  (The depth case's loss reaches T, with upstream gradients of one sign each:
    why, in `layout_deep_case`.)"""
    c = G.layout_deep_case(layout, D)
    names = _names(layout)
    ref = G.reference(c)
    got = _run(c, names)
    _check_wanted(f"{layout} deep D={D}", got, ref, names)
    row_max = np.abs(ref["dhw"]).max(axis=2)
    assert row_max.min() >= 1e-3 * row_max.max()
    ratio = np.abs(got["dhw"] - ref["dhw"]).max(axis=2) / (1e-4 * row_max)
    where = np.unravel_index(ratio.argmax(), ratio.shape)
    print(f"{layout} deep D={D}: dhw worst row ratio {ratio.max():.3f} at (MPI, plane) {tuple(int(i) for i in where)}")
    assert ratio.max() <= 1.0, (ratio.max(), where)
    if layout == "depth":
        r = ref["pz"]
        allowed = 1e-4 * np.maximum(np.abs(r), 1e-2 * np.abs(r).max(axis=1, keepdims=True))
        ratio = np.abs(got["pz"] - r) / allowed
        where = np.unravel_index(ratio.argmax(), ratio.shape)
        print(f"depth deep D={D}: plane_z worst element ratio {ratio.max():.3f} at (MPI, plane) {tuple(int(i) for i in where)}")
        assert ratio.max() <= 1.0, (ratio.max(), where)
