"""The window forward of the depth-alpha layout without a GPU: what `hip_mpi` hands the two new C entries (the recorder of test_depth_alpha_cpu), the
entries' argument errors and the queries on the host, their declaration, the driver methods, and the resources of the new kernels read from their
kernel descriptors."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

from test_depth_alpha_cpu import DEPTH_ENTRIES, HIPCC, ROOT, depth_inputs, rec  # noqa: F401  (rec: the recorder fixture)
from test_marshal_cpu import Call, loss_of, scalars_of

PIXEL, WINDOW, SUPPORTS = "gmpi_mpi_render_depth_launch", "gmpi_mpi_render_depth_window_launch", "gmpi_render_depth_window_supports"
BWD_PIXEL, BWD_TILE = "gmpi_mpi_render_depth_backward_launch", "gmpi_mpi_render_depth_backward_tile_launch"


@pytest.fixture
def rec2(rec):
    """The recorder of test_depth_alpha_cpu, which also knows the new entries; `rec.answer` is what the support query returns (the recorder itself
    answers 0 to everything)."""
    rec.entries = tuple(rec.entries) + (WINDOW, BWD_TILE)
    rec.answer = 1

    def supports(*args):
        rec.calls.append(Call(SUPPORTS, tuple(rec._copy(a) for a in args), None))
        return rec.answer
    rec.__dict__[SUPPORTS] = supports   # (found before Recorder.__getattr__ is asked)
    return rec


@pytest.fixture
def fresh_warning(monkeypatch):
    from ml_gmpi_amd import hip_mpi
    monkeypatch.setattr(hip_mpi, "_WINDOW_FALLBACK_WARNED", False)


def _render(rec, how="absent", dtype=torch.float32, background=True, mpi=None, **kw):
    from ml_gmpi_amd.hip_mpi import MPI
    rgb, depth, pz, bg, geo = depth_inputs(dtype, background, per_mpi_table=True)
    del rec.calls[:]
    mpi = mpi or MPI()
    with torch.no_grad():
        res = mpi.render_views_depth(rgb, depth, pz, (-2 / 10, 2 / 10), *geo, background=bg, **({} if how == "absent" else {"depth_forward": how}), **kw)
    return list(rec.calls), res, mpi


def _same_structs(a, b):
    """GmpiRenderParams up to addresses; GmpiSharedColor and GmpiDepthAlpha up to their pointers (every run has its own tensors)."""
    assert scalars_of(a.args[0]) == scalars_of(b.args[0])
    assert list(a.args[0].rgba_stride) == list(b.args[0].rgba_stride)
    sa, sb = a.args[1], b.args[1]
    assert bytes(sa)[:8] == bytes(sb)[:8] and list(sa.rgb_stride) == list(sb.rgb_stride) and list(sa.background_stride) == list(sb.background_stride)
    assert (sa.background is None) == (sb.background is None) and ctypes.sizeof(sa) == ctypes.sizeof(sb) == 72
    da, db = a.args[2], b.args[2]
    assert (da.struct_size, da.plane_z_stride, da.z_lo, da.z_hi, da.z_den) == (db.struct_size, db.plane_z_stride, db.z_lo, db.z_hi, db.z_den)


@pytest.mark.parametrize("background", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_window_records_the_query_then_the_new_entry_with_the_default_paths_structs(rec2, dtype, background):
    (default,), _, _ = _render(rec2, dtype=dtype, background=background)
    (by_name,), _, _ = _render(rec2, "pixel", dtype=dtype, background=background)
    (by_none,), _, _ = _render(rec2, None, dtype=dtype, background=background)
    assert default.name == by_name.name == by_none.name == PIXEL == DEPTH_ENTRIES[0]   # None or "pixel": today's entry only
    (query, launch), res, mpi = _render(rec2, "window", dtype=dtype, background=background)
    assert (query.name, launch.name) == (SUPPORTS, WINDOW)
    assert len(query.args) == 3 and len(launch.args) == 4 and launch.args[3] == 0
    for i in range(3):   # the query saw the structs the launch got, byte for byte
        assert bytes(query.args[i]) == bytes(launch.args[i]), i
    for other in (default, by_name, by_none):
        _same_structs(launch, other)
    assert launch.args[0].variant == 0 and mpi.depth_window_fallbacks == 0
    assert launch.args[0].rgb_out == res["color"].data_ptr()


def test_a_zero_answer_takes_todays_entry_counts_and_warns_once(rec2, fresh_warning):
    rec2.answer = 0
    with pytest.warns(RuntimeWarning, match="depth_forward") as w:
        calls, _, mpi = _render(rec2, "window")
    assert [c.name for c in calls] == [SUPPORTS, PIXEL] and mpi.depth_window_fallbacks == 1 and len(w) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # the warning is given once per process
        calls, _, _ = _render(rec2, "window", mpi=mpi)
    assert [c.name for c in calls] == [SUPPORTS, PIXEL] and mpi.depth_window_fallbacks == 2
    rec2.answer = -4
    from ml_gmpi_amd import _lib
    with pytest.raises(_lib.GmpiError, match=SUPPORTS):
        _render(rec2, "window")


def test_tight_storage_behind_the_last_row_falls_back(rec2, fresh_warning):
    """A width that is no multiple of 4: the loader reads the padding of the last row, which a view that ends with its storage does not have."""
    from ml_gmpi_amd.hip_mpi import MPI
    _, _, pz, _, geo = depth_inputs(background=False)
    M, Ht, Wt = 2, 6, 8
    g = torch.Generator().manual_seed(5)
    wide = torch.rand((M, 4, Ht, Wt), generator=g)
    rgb, depth = wide[:, :3, :, :7], wide[:, 3:, :, :7]          # rows of 7 in a pitch of 8: the padding exists
    dhw, ray, eye, zd = geo
    with torch.no_grad():
        MPI().render_views_depth(rgb, depth, pz, (-0.2, 0.2), dhw, ray, eye, zd, depth_forward="window")
    assert [c.name for c in rec2.calls] == [SUPPORTS, WINDOW]
    del rec2.calls[:]
    tight = torch.rand((M * 4 * Ht * 8 - 1,), generator=g).as_strided((M, 4, Ht, 7), (4 * Ht * 8, Ht * 8, 8, 1))   # ... and here it does not
    mpi = MPI()
    with torch.no_grad(), pytest.warns(RuntimeWarning):
        mpi.render_views_depth(tight[:, :3], tight[:, 3:], pz, (-0.2, 0.2), dhw, ray, eye, zd, depth_forward="window")
    assert [c.name for c in rec2.calls] == [SUPPORTS, PIXEL] and mpi.depth_window_fallbacks == 1


def test_unknown_names_are_refused_before_any_call(rec2):
    from ml_gmpi_amd import make_renderer
    from ml_gmpi_amd.hip_mpi import MPI
    rgb, depth, pz, bg, geo = depth_inputs()
    for name in ("windows", "lds", "tile", "", 1):
        with pytest.raises(ValueError, match="depth_forward"):
            MPI().render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg, depth_forward=name)
    for variant in ("lds", "wave", "band"):   # variant= keeps its refusals next to the new argument
        with pytest.raises(ValueError, match="not built"):
            MPI().render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, variant=variant, depth_forward="window")
    r = make_renderer("FFHQ", n_planes=4, device=torch.device("cpu"), ray_backend="torch")
    g = torch.Generator().manual_seed(0)
    with pytest.raises(ValueError, match="depth_forward"):
        r.render_depth(torch.rand((1, 3, 8, 8), generator=g), torch.rand((1, 1, 8, 8), generator=g), 8, 8, z_range=1, n_z_bins=4, depth_forward="box")
    assert rec2.calls == []


def test_renderer_passes_the_argument_through(rec2):
    from ml_gmpi_amd import make_renderer
    r = make_renderer("FFHQ", n_planes=4, device=torch.device("cpu"), ray_backend="torch")
    g = torch.Generator().manual_seed(0)
    rgb, depth = torch.rand((1, 3, 8, 8), generator=g), torch.rand((1, 1, 8, 8), generator=g)
    for how, want in (("absent", [PIXEL]), (None, [PIXEL]), ("pixel", [PIXEL]), ("window", [SUPPORTS, WINDOW])):
        del rec2.calls[:]
        torch.manual_seed(0)
        with torch.no_grad():
            r.render_depth(rgb, depth, 8, 8, z_range=1, n_z_bins=4, **({} if how == "absent" else {"depth_forward": how}))
        assert [c.name for c in rec2.calls] == want, how


@pytest.mark.parametrize("depth_backward,entry", [("pixel", BWD_PIXEL), ("tile", BWD_TILE)])
@pytest.mark.parametrize("uses_T", [False, True])
def test_backward_entry_does_not_depend_on_the_forward(rec2, depth_backward, entry, uses_T):
    from ml_gmpi_amd.hip_mpi import MPI
    recs = {}
    for how in ("pixel", "window"):
        rgb, depth, pz, bg, geo = depth_inputs(torch.float32, True, per_mpi_table=True)
        for t in (rgb, depth, bg):
            t.requires_grad_(True)
        del rec2.calls[:]
        res = MPI().render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg, want_transmittance=True, depth_forward=how,
                                       depth_backward=depth_backward)
        loss_of(res, uses_T).backward()
        recs[how] = list(rec2.calls)
        assert all(t.grad is not None and t.grad.shape == t.shape for t in (rgb, depth, bg))
    assert [c.name for c in recs["pixel"]] == [PIXEL, entry] and [c.name for c in recs["window"]] == [SUPPORTS, WINDOW, entry]
    fwd, bwd = recs["window"][1:]
    assert bytes(bwd.args[1]) == bytes(fwd.args[1]) and bytes(bwd.args[2]) == bytes(fwd.args[2])   # the backward rebuilds the forward's structs
    assert bwd.args[0].transmittance_out == fwd.args[0].transmittance_out and bwd.args[0].variant == fwd.args[0].variant == 0
    a, b = recs["pixel"][1], bwd
    assert scalars_of(a.args[0]) == scalars_of(b.args[0]) and len(a.args) == len(b.args) == 13
    for i in (7, 9, 11):
        assert a.args[i] == b.args[i], i
    assert (b.args[5] is not None) == uses_T


# ---- the C entries on the host -------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_window_entries_as_plain_c(tmp_path):
    src = tmp_path / "w.c"
    src.write_text(
        '#include "gmpi_render.h"\n'
        "typedef int (*fwd_t)(const GmpiRenderParams *, const GmpiSharedColor *, const GmpiDepthAlpha *, void *);\n"
        "typedef int (*sup_t)(const GmpiRenderParams *, const GmpiSharedColor *, const GmpiDepthAlpha *);\n"
        "int main(void) {\n"
        "    fwd_t pixel = gmpi_mpi_render_depth_launch, window = gmpi_mpi_render_depth_window_launch;\n"
        "    sup_t sup = gmpi_render_depth_window_supports;\n"
        "    return (pixel == 0) + (window == 0) + (sup == 0) + (GMPI_ABI_VERSION != 2) + (sizeof(GmpiRenderParams) != 184)\n"
        "           + (sizeof(GmpiSharedColor) != 72) + (sizeof(GmpiDepthAlpha) != 40);\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "w.o")], check=True)


def test_library_exports_the_window_entries_and_keeps_the_abi():
    from ml_gmpi_amd import _lib
    assert WINDOW in _lib.EXPORTS and SUPPORTS in _lib.EXPORTS and PIXEL in _lib.EXPORTS
    assert _lib.ABI_VERSION == 2 and ctypes.sizeof(_lib.GmpiRenderParams) == 184 and ctypes.sizeof(_lib.GmpiSharedColor) == 72
    assert ctypes.sizeof(_lib.GmpiDepthAlpha) == 40
    lib = _lib.load_library()
    assert list(lib.gmpi_mpi_render_depth_window_launch.argtypes) == list(lib.gmpi_mpi_render_depth_launch.argtypes)
    assert len(lib.gmpi_render_depth_window_supports.argtypes) == 3
    q = lib.gmpi_query
    assert q(25) == 1 and (q(26), q(27)) == (64, 32) and q(28) > 0
    assert q(24) == q(21) == q(19) == q(15) == -1 and q(29) == -1 and q(22) == 1 and q(23) == 128 and q(0) == 2


def test_argument_error_codes_equal_the_one_pixel_entrys_on_the_host():
    """test_depth_alpha_tile_cpu's table for the forward: the new entry, its support query and the one-pixel entry give the same code for the same
    bad arguments.  Every call is refused (or has no views) before anything is launched: no device is needed, the pointers are never followed."""
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    host = np.zeros(64 + 4, dtype=np.float32)
    fake = (host.ctypes.data + 15) & ~15   # (a non-NULL address, 16-byte aligned)

    def params(N=1):
        p = L.GmpiRenderParams()
        p.struct_size = ctypes.sizeof(L.GmpiRenderParams)
        p.flags, p.variant, p.rgba_dtype = L.FLAG_ALIGN_CORNERS, L.VARIANT_AUTO, L.DTYPE_F32
        p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = N, 1, 3, 4, 4, 4, 4, 1
        p.rgba = fake
        p.rgba_stride[:] = [16, 0, 0, 4, 1]   # [1], [2]: ignored
        p.dhw = p.ray_dir = p.eye_pos = p.z_dir = p.rgb_out = p.depth_out = fake
        return p

    def shared(with_bg=True):
        s = L.GmpiSharedColor()
        s.struct_size = ctypes.sizeof(L.GmpiSharedColor)
        s.rgb, s.background = fake, (fake if with_bg else None)
        s.rgb_stride[:] = [48, 16, 4]
        s.background_stride[:] = [48, 16, 4]
        return s

    def ramp(lo=-0.25, hi=0.25, den=0.5):
        d = L.GmpiDepthAlpha()
        d.struct_size = ctypes.sizeof(L.GmpiDepthAlpha)
        d.plane_z, d.plane_z_stride, d.z_lo, d.z_hi, d.z_den = fake, 0, lo, hi, den
        return d

    ref = lambda x: None if x is None else ctypes.byref(x)
    seen = []

    def call(p, s, d):
        """The three entries on arguments that are refused; they must agree.  Returns the window entry's code."""
        rc = [lib.gmpi_mpi_render_depth_window_launch(ref(p), ref(s), ref(d), None), lib.gmpi_mpi_render_depth_launch(ref(p), ref(s), ref(d), None)]
        assert rc[0] == rc[1], rc
        sup = lib.gmpi_render_depth_window_supports(ref(p), ref(s), ref(d))
        assert sup == (rc[0] if rc[0] < 0 else 1), (sup, rc)
        seen.append(rc[0])
        return rc[0]

    assert call(params(N=0), shared(), ramp()) == 0                                              # no views: nothing to launch
    assert call(None, shared(), ramp()) == -1 and call(params(), None, ramp()) == -1 and call(params(), shared(), None) == -1   # GMPI_E_NULL
    d = ramp(); d.plane_z = None
    assert call(params(), shared(), d) == -1
    s = shared(); s.rgb = None
    assert call(params(), s, ramp()) == -1
    p = params(); p.rgba = None
    assert call(p, shared(), ramp()) == -1
    p = params(); p.rgb_out = None
    assert call(p, shared(), ramp()) == -1                                                       # the forward needs its outputs
    p = params(); p.rgba_dtype = L.DTYPE_U8
    assert call(p, shared(), ramp()) == -3                                                       # GMPI_E_DTYPE
    for lo, hi, den in ((0.25, 0.25, 0.5), (0.3, 0.25, 0.5), (-0.25, 0.25, 0.0), (-0.25, 0.25, -0.5), (float("nan"), 0.25, 0.5)):
        assert call(params(), shared(), ramp(lo, hi, den)) == -2, (lo, hi, den)                  # bad bounds: GMPI_E_SHAPE
    d = ramp(); d.plane_z_stride = -3
    assert call(params(), shared(), d) == -4                                                     # GMPI_E_STRIDE
    p = params(); p.rgba_stride[4] = 2
    assert call(p, shared(), ramp()) == -4
    s = shared(); s.rgb_stride[2] = 3
    assert call(params(), s, ramp()) == -4                                                       # rows shorter than the texture
    d = ramp(); d.struct_size += 8
    assert call(params(), shared(), d) == -5                                                     # GMPI_E_ABI
    p = params(); p.struct_size -= 8
    assert call(p, shared(), ramp()) == -5
    for v in (L.VARIANT_LDS, L.VARIANT_WAVE, L.VARIANT_DMA, L.VARIANT_BAND, 9):
        p = params(); p.variant = v
        assert call(p, shared(), ramp()) == -6, v                                                # GMPI_E_VARIANT: the old entry too
    p = params(); p.flags |= 1 << 30
    assert call(p, shared(), ramp()) == -7                                                       # GMPI_E_FLAGS
    p = params(N=0); p.variant = L.VARIANT_GATHER
    assert call(p, shared(), ramp()) == 0
    p = params(N=65536); p.variant = L.VARIANT_GATHER
    assert call(p, shared(), ramp()) == -2                                                       # GATHER: the view index is a grid dimension
    assert len(seen) >= 27

    # what only the window kernel's loader refuses: a base pointer or an outer stride that is no multiple of 16 bytes -> supports 0, launch -6
    def window_only(p, s, d):
        return lib.gmpi_render_depth_window_supports(ref(p), ref(s), ref(d)), lib.gmpi_mpi_render_depth_window_launch(ref(p), ref(s), ref(d), None)
    assert lib.gmpi_render_depth_window_supports(ref(params()), ref(shared()), ref(ramp())) == 1
    p = params(); p.rgba = fake + 4
    assert window_only(p, shared(), ramp()) == (0, -6)
    s = shared(); s.rgb = fake + 8
    assert window_only(params(), s, ramp()) == (0, -6)
    s = shared(); s.background = fake + 4
    assert window_only(params(), s, ramp()) == (0, -6)
    s = shared(with_bg=False); s.background_stride[:] = [7, 7, 7]   # (no background: its strides are not looked at)
    assert lib.gmpi_render_depth_window_supports(ref(params()), ref(s), ref(ramp())) == 1
    p = params(); p.Wt = 3; p.rgba_stride[:] = [16, 0, 0, 6, 1]
    s = shared(); s.rgb_stride[:] = [48, 16, 4]; s.background_stride[:] = [48, 16, 4]
    assert window_only(p, s, ramp()) == (0, -6)                                                  # a row stride of 6 floats
    p = params(); p.Wt = 3                                                                        # any Wt with aligned rows is taken
    assert lib.gmpi_render_depth_window_supports(ref(p), ref(shared()), ref(ramp())) == 1
    p = params(); p.rgba_dtype = L.DTYPE_BF16; p.rgba_stride[:] = [16, 0, 0, 4, 1]               # 16-bit storage: 4 texels are 8 bytes
    assert window_only(p, shared(), ramp()) == (0, -6)
    p.rgba_stride[:] = [32, 0, 0, 8, 1]
    s = shared(); s.rgb_stride[:] = [96, 32, 8]; s.background_stride[:] = [96, 32, 8]
    assert lib.gmpi_render_depth_window_supports(ref(p), ref(s), ref(ramp())) == 1
    p = params(); p.rgba = fake + 4; p.variant = L.VARIANT_GATHER                                # GATHER by name: the one-pixel kernel takes anything
    assert lib.gmpi_render_depth_window_supports(ref(p), ref(shared()), ref(ramp())) == 1


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------------
def test_driver_methods_exist_and_share_their_bodies():
    from ml_gmpi_amd import ViewBatchDriver
    from ml_gmpi_amd import driver
    sig = inspect.signature(ViewBatchDriver.render_path_depth)
    assert list(sig.parameters)[1:] == ["rgb", "depth", "render_size", "yaws", "pitches", "z_range", "n_z_bins", "plane_z", "background", "indices",
                                        "to_uint8", "depth_range", "want_transmittance", "to_host", "depth_forward"]
    kinds = {n: q.kind for n, q in sig.parameters.items()}
    assert all(kinds[n] is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[6:])
    assert sig.parameters["depth_forward"].default == driver.DEPTH_FORWARD_DEFAULT and driver.DEPTH_FORWARD_DEFAULT in ("pixel", "window")
    sig = inspect.signature(ViewBatchDriver.render_seeds_depth)
    assert list(sig.parameters)[1:] == ["rgb", "depth", "render_size", "z_range", "n_z_bins", "plane_z", "background", "views_per_mpi", "depth_forward",
                                        "render_kwargs"]
    assert sig.parameters["depth_forward"].default == driver.DEPTH_FORWARD_DEFAULT
    for mine, plain in (("render_path_depth", "render_path"), ("render_seeds_depth", "render_seeds")):
        a, b = inspect.getsource(getattr(ViewBatchDriver, mine)), inspect.getsource(getattr(ViewBatchDriver, plain))
        helper = "_" + plain
        assert helper + "(" in a and helper + "(" in b, (mine, plain)   # one body for all three layouts
        assert "for s in range" not in a, mine                          # ... and no third copy of the loop


# ---- the kernels' resources, from their descriptors ----------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_window_kernels_have_no_scratch_and_three_workgroups_of_lds(tmp_path):
    csrc = os.path.join(ROOT, "ml-gmpi_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
             "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]   # = ml-gmpi_amd/csrc/Makefile
    mk = open(os.path.join(csrc, "Makefile")).read()
    for f in ("-ffp-contract=off", "-fno-slp-vectorize", "-O3", "render_depth_window.hip"):
        assert f in mk, f"the Makefile no longer has {f}: keep this test in step with it"
    res = subprocess.run([HIPCC, *flags, "-save-temps", "-c", os.path.join(csrc, "render_depth_window.hip"), "-o", "render_depth_window.o"], cwd=tmp_path,
                         capture_output=True, timeout=900)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    asm = open(os.path.join(tmp_path, "render_depth_window-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    kernels = {}
    for name, meta in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel", asm, flags=re.M | re.S):   # the descriptors only
        field = lambda key: int(re.search(r"\.amdhsa_" + key + r"\s+(\d+)", meta).group(1))
        kernels[name] = (field("private_segment_fixed_size"), field("group_segment_fixed_size"))
    window = {n: v for n, v in kernels.items() if "render_depth_window_kernel" in n}
    assert len(window) >= 12 and len(kernels) == len(window), sorted(kernels)   # 3 storage types x align_corners x order, and nothing else in the file
    for name, (scratch, lds) in sorted(window.items()):
        print(name, "scratch", scratch, "lds", lds)
        assert scratch == 0, (name, scratch)
        assert 32768 <= lds <= 53 * 1024, (name, lds)   # the 32 KiB window is there; three workgroups fit the 160 KB of a CU
    shutil.rmtree(tmp_path, ignore_errors=True)
