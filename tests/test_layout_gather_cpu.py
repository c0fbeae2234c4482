"""The atomics-free backward of the shared-colour and depth-alpha layouts without a GPU: what `hip_mpi` hands the C ABI for
`shared_backward="gather"` / `depth_backward="gather"` (the recorder of test_depth_alpha_cpu, extended with the new entry names and a workspace
query that answers), that every other name records what it records today, the entries' refusals on the host, their declarations as plain C, and the
resources of the new kernels read from their kernel descriptors."""
import ctypes
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

from test_depth_alpha_cpu import DEPTH_ENTRIES, HIPCC, ROOT, depth_inputs, rec  # noqa: F401  (rec: the recorder fixture)
from test_marshal_cpu import Call, Recorder, loss_of, make_inputs, M, D, Ht, Wt

QUERY = "gmpi_render_layout_backward_gather_workspace_bytes"
SET_RUNS = "gmpi_render_layout_backward_gather_set_runs"
SHARED = ("gmpi_mpi_render_shared_launch", "gmpi_mpi_render_shared_backward_launch", "gmpi_mpi_render_shared_backward_gather_launch")
DEPTH = (DEPTH_ENTRIES[0], DEPTH_ENTRIES[1], "gmpi_mpi_render_depth_backward_gather_launch")
TILE = "gmpi_mpi_render_depth_backward_tile_launch"
WS_BYTES = 4096


class _AnsweringRecorder(Recorder):
    """test_marshal_cpu's recorder; the layouts' workspace query is recorded like any entry and answers `ws_bytes` (0: the pair cannot take
    the launch)."""
    ws_bytes = WS_BYTES

    def __getattr__(self, name):
        call = Recorder.__getattr__(self, name)
        if name != QUERY:
            return call

        def query(*args):
            call(*args)
            return self.ws_bytes
        return query


@pytest.fixture
def rec3(rec, monkeypatch):
    """The recorder of test_depth_alpha_cpu, which also knows the tile entry, the two gather entries, their query and the test hook."""
    from ml_gmpi_amd import _lib
    r = _AnsweringRecorder(tuple(rec.entries) + (TILE, SHARED[2], DEPTH[2], QUERY, SET_RUNS))
    monkeypatch.setattr(_lib, "load_library", lambda: r)
    return r


def _shared_inputs(dtype=torch.float32, background=True):
    vol, dhw, ray, eye, zd = make_inputs(2, dtype)
    g = torch.Generator().manual_seed(2)
    rgb = torch.rand((M, 3, Ht, Wt), generator=g).to(dtype)
    bg = torch.rand((M, 3, Ht, Wt), generator=g).to(dtype) if background else None
    return rgb, vol[:, :, 3:].contiguous(), bg, (dhw, ray, eye, zd)


def _record(r, layout, uses_T=False, background=True, dtype=torch.float32, mpi_kw=None, **kw):
    """One forward + backward through `MPI`; returns the recorded calls and the three inputs."""
    from ml_gmpi_amd.hip_mpi import MPI
    del r.calls[:]
    mpi = MPI(**(mpi_kw or {}))
    if layout == "shared":
        rgb, alpha, bg, geo = _shared_inputs(dtype, background)
        ins = (rgb, alpha, bg)
    else:
        rgb, depth, pz, bg, geo = depth_inputs(dtype, background, per_mpi_table=True)
        ins = (rgb, depth, bg)
    for t in ins:
        if t is not None:
            t.requires_grad_(True)
    if layout == "shared":
        res = mpi.render_views_shared(rgb, alpha, *geo, background=bg, want_transmittance=True, **kw)
    else:
        res = mpi.render_views_depth(rgb, depth, pz, (-2 / 10, 2 / 10), *geo, background=bg, want_transmittance=True, **kw)
    loss_of(res, uses_T).backward()
    return list(r.calls), ins, mpi


ARG = {"shared": "shared_backward", "depth": "depth_backward"}
NAMES = {"shared": SHARED, "depth": DEPTH}


@pytest.mark.parametrize("uses_T", [False, True])
@pytest.mark.parametrize("background", [False, True])
@pytest.mark.parametrize("layout", ["shared", "depth"])
def test_gather_records_the_query_then_the_gather_entry_with_a_lent_workspace(rec3, layout, background, uses_T):
    from ml_gmpi_amd import _lib
    fwd_name, atomic_name, gather_name = NAMES[layout]
    calls, ins, mpi = _record(rec3, layout, uses_T, background, **{ARG[layout]: "gather"})
    assert [c.name for c in calls] == [fwd_name, QUERY, gather_name]
    fwd, query, bwd = calls
    n_structs = 2 if layout == "shared" else 3
    # the query sees the launch's structs: no workspace yet, no overwrite flag; the shared-colour one passes NULL for the ramp
    assert len(query.args) == 3 and (query.args[2] is None) == (layout == "shared")
    qp, bp = query.args[0], bwd.args[0]
    assert qp.workspace is None and qp.workspace_bytes == 0 and not qp.flags & _lib.FLAG_GRAD_OVERWRITE
    assert bp.workspace is not None and bp.workspace_bytes == WS_BYTES
    assert bp.flags == fwd.args[0].flags | _lib.FLAG_GRAD_OVERWRITE and bp.variant == _lib.VARIANT_AUTO
    for i in range(1, n_structs):   # the layout's structs: those of the forward, byte for byte
        assert bytes(bwd.args[i]) == bytes(fwd.args[i]) == bytes(query.args[i])
    for name in ("rgba", "dhw", "ray_dir", "eye_pos", "z_dir", "transmittance_out"):
        assert getattr(bp, name) == getattr(fwd.args[0], name) == getattr(qp, name), name
    # the gradient arguments: the pattern of the atomic entry
    a_calls, _, _ = _record(rec3, layout, uses_T, background)
    assert [c.name for c in a_calls] == [fwd_name, atomic_name]
    a = a_calls[1]
    assert len(bwd.args) == len(a.args)
    g0 = n_structs + 3
    assert (bwd.args[n_structs + 2] is not None) == uses_T
    for i in range(n_structs, len(a.args)):
        assert (bwd.args[i] is None) == (a.args[i] is None), i
    for i in (g0 + 1, g0 + 3, g0 + 5):
        assert bwd.args[i] == a.args[i], i
    assert a.args[0].workspace is None and not a.args[0].flags & _lib.FLAG_GRAD_OVERWRITE
    assert mpi.layout_gather_fallbacks == 0
    for t in ins:
        assert t is None or (t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype)


@pytest.mark.parametrize("layout", ["shared", "depth"])
def test_every_other_name_records_what_it_records_today(rec3, layout):
    fwd_name, atomic_name, _ = NAMES[layout]
    today = [fwd_name, atomic_name]
    names = lambda calls: [c.name for c in calls]
    assert names(_record(rec3, layout)[0]) == today                                               # the default
    assert names(_record(rec3, layout, mpi_kw=dict(backward="gather"))[0]) == today              # MPI(backward="gather") names the volume entry only
    if layout == "shared":
        assert names(_record(rec3, layout, shared_backward="tile")[0]) == today
    else:
        assert names(_record(rec3, layout, depth_backward="pixel")[0]) == today
        assert names(_record(rec3, layout, depth_backward="tile")[0]) == [fwd_name, TILE]
    # MPI(backward="gather") next to the per-call name: the per-call name decides
    assert names(_record(rec3, layout, mpi_kw=dict(backward="gather"), **{ARG[layout]: "gather"})[0]) == [fwd_name, QUERY, NAMES[layout][2]]


@pytest.mark.parametrize("layout", ["shared", "depth"])
def test_a_query_of_zero_takes_the_atomic_entry_counts_and_warns_once(rec3, layout, monkeypatch):
    from ml_gmpi_amd import _lib, hip_mpi
    fwd_name, atomic_name, _ = NAMES[layout]
    rec3.ws_bytes = 0
    monkeypatch.setattr(hip_mpi, "_GATHER_FALLBACK_WARNED", False)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        calls, ins, mpi = _record(rec3, layout, **{ARG[layout]: "gather"})
        calls2, _, _ = _record(rec3, layout, **{ARG[layout]: "gather"})
    assert [c.name for c in calls] == [fwd_name, QUERY, atomic_name] == [c.name for c in calls2]
    p = calls[2].args[0]
    assert p.workspace is None and p.workspace_bytes == 0 and not p.flags & _lib.FLAG_GRAD_OVERWRITE
    assert mpi.layout_gather_fallbacks == 1
    hits = [w for w in seen if issubclass(w.category, RuntimeWarning) and "layout_gather_fallbacks" in str(w.message)]
    assert len(hits) == 1


def test_the_test_hook_brackets_the_query_and_the_launch(rec3):
    calls, _, _ = _record(rec3, "shared", shared_backward="gather", _gather_runs=3)
    assert [c.name for c in calls] == [SHARED[0], SET_RUNS, QUERY, SHARED[2], SET_RUNS]
    assert calls[1].args == (3,) and calls[4].args == (0,)


def test_unknown_names_are_refused_before_any_call(rec3):
    from ml_gmpi_amd import make_renderer
    from ml_gmpi_amd.hip_mpi import MPI
    rgb, alpha, bg, geo = _shared_inputs()
    for name in ("pixel", "atomic", "gathers", "", None, 1):
        with pytest.raises(ValueError, match="shared_backward"):
            MPI().render_views_shared(rgb, alpha, *geo, background=bg, shared_backward=name)
    rgb, depth, pz, bg, geo = depth_inputs()
    for name in ("gathers", "atomic", "", None, 1):
        with pytest.raises(ValueError, match='"pixel", "tile" or "gather"'):
            MPI().render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg, depth_backward=name)
    r = make_renderer("FFHQ", n_planes=4, device=torch.device("cpu"), ray_backend="torch")
    g = torch.Generator().manual_seed(0)
    with pytest.raises(ValueError, match="shared_backward"):
        r.render_shared(torch.rand((1, 3, 8, 8), generator=g), torch.rand((1, 4, 1, 8, 8), generator=g), 8, 8, shared_backward="box")
    with pytest.raises(ValueError, match="depth_backward"):
        r.render_depth(torch.rand((1, 3, 8, 8), generator=g), torch.rand((1, 1, 8, 8), generator=g), 8, 8, z_range=1, n_z_bins=4, depth_backward="box")
    assert rec3.calls == []


def test_renderer_passes_both_arguments_through(rec3):
    from ml_gmpi_amd import make_renderer
    r = make_renderer("FFHQ", n_planes=4, device=torch.device("cpu"), ray_backend="torch")
    g = torch.Generator().manual_seed(0)
    rgb = torch.rand((1, 3, 8, 8), generator=g)
    alpha = torch.rand((1, 4, 1, 8, 8), generator=g).requires_grad_(True)
    depth = torch.rand((1, 1, 8, 8), generator=g).requires_grad_(True)
    backward = lambda: [c.name for c in rec3.calls if "backward" in c.name and c.name != SET_RUNS]
    for how, want in ((None, [SHARED[1]]), ("tile", [SHARED[1]]), ("gather", [QUERY, SHARED[2]])):
        del rec3.calls[:]
        torch.manual_seed(0)
        r.render_shared(rgb, alpha, 8, 8, **({} if how is None else {"shared_backward": how}))[0].sum().backward()
        assert backward() == want, how
    for how, want in ((None, [DEPTH[1]]), ("pixel", [DEPTH[1]]), ("tile", [TILE]), ("gather", [QUERY, DEPTH[2]])):
        del rec3.calls[:]
        torch.manual_seed(0)
        r.render_depth(rgb, depth, 8, 8, z_range=1, n_z_bins=4, **({} if how is None else {"depth_backward": how}))[0].sum().backward()
        assert backward() == want, how


# ---- the C entries on the host -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_gather_entries_as_plain_c(tmp_path):
    src = tmp_path / "g.c"
    src.write_text(
        '#include "gmpi_render.h"\n'
        "typedef int (*sbwd_t)(const GmpiRenderParams *, const GmpiSharedColor *, const float *, const float *, const float *, float *,\n"
        "                      const int64_t *, float *, const int64_t *, float *, const int64_t *, void *);\n"
        "typedef int (*dbwd_t)(const GmpiRenderParams *, const GmpiSharedColor *, const GmpiDepthAlpha *, const float *, const float *, const float *,\n"
        "                      float *, const int64_t *, float *, const int64_t *, float *, const int64_t *, void *);\n"
        "typedef uint64_t (*query_t)(const GmpiRenderParams *, const GmpiSharedColor *, const GmpiDepthAlpha *);\n"
        "int main(void) {\n"
        "    sbwd_t s0 = gmpi_mpi_render_shared_backward_launch, s1 = gmpi_mpi_render_shared_backward_gather_launch;\n"
        "    dbwd_t d0 = gmpi_mpi_render_depth_backward_launch, d1 = gmpi_mpi_render_depth_backward_gather_launch;\n"
        "    query_t q = gmpi_render_layout_backward_gather_workspace_bytes;\n"
        "    return (s0 == 0) + (s1 == 0) + (d0 == 0) + (d1 == 0) + (q == 0) + (GMPI_ABI_VERSION != 2) + (sizeof(GmpiRenderParams) != 184)\n"
        "           + (sizeof(GmpiSharedColor) != 72) + (sizeof(GmpiDepthAlpha) != 40);\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "g.o")], check=True)


def test_library_exports_the_gather_entries_and_keeps_the_abi():
    from ml_gmpi_amd import _lib
    for name in (SHARED[2], DEPTH[2], QUERY, SET_RUNS, "gmpi_render_layout_backward_gather_runs"):
        assert name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 2 and ctypes.sizeof(_lib.GmpiRenderParams) == 184 and ctypes.sizeof(_lib.GmpiSharedColor) == 72
    assert ctypes.sizeof(_lib.GmpiDepthAlpha) == 40
    lib = _lib.load_library()
    assert list(lib.gmpi_mpi_render_depth_backward_gather_launch.argtypes) == list(lib.gmpi_mpi_render_depth_backward_launch.argtypes)
    assert list(lib.gmpi_mpi_render_shared_backward_gather_launch.argtypes) == list(lib.gmpi_mpi_render_shared_backward_launch.argtypes)
    assert lib.gmpi_query(34) == 1 and lib.gmpi_query(33) == -1 and lib.gmpi_query(35) == -1 and lib.gmpi_query(0) == 2


def test_refusals_and_the_query_on_the_host():
    """Every call is refused (or has no views) before anything is launched: no device is needed, the pointers are never followed.  The argument
    errors are those of the layouts' atomic entries, side by side; the query is 0 exactly where the gather launch answers GMPI_E_VARIANT or an
    argument error, and the workspace codes come after both."""
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    host = np.zeros(4096, dtype=np.float32)
    fake = host.ctypes.data   # (a non-NULL address)

    def params(N=1, flags=L.FLAG_ALIGN_CORNERS, ws=None, ws_bytes=0):
        p = L.GmpiRenderParams()
        p.struct_size = ctypes.sizeof(L.GmpiRenderParams)
        p.flags, p.variant, p.rgba_dtype = flags, L.VARIANT_AUTO, L.DTYPE_F32
        p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = N, 1, 3, 4, 4, 4, 4, 1
        p.rgba = fake
        p.rgba_stride[:] = [48, 16, 0, 4, 1]
        p.dhw = p.ray_dir = p.eye_pos = p.z_dir = fake
        p.workspace, p.workspace_bytes = ws, ws_bytes
        return p

    def shared(with_bg=True):
        s = L.GmpiSharedColor()
        s.struct_size = ctypes.sizeof(L.GmpiSharedColor)
        s.rgb, s.background = fake, (fake if with_bg else None)
        s.rgb_stride[:] = [48, 16, 4]
        s.background_stride[:] = [48, 16, 4]
        return s

    def ramp():
        d = L.GmpiDepthAlpha()
        d.struct_size = ctypes.sizeof(L.GmpiDepthAlpha)
        d.plane_z, d.plane_z_stride, d.z_lo, d.z_hi, d.z_den = fake, 0, -0.25, 0.25, 0.5
        return d

    ref = lambda x: None if x is None else ctypes.byref(x)
    s3 = (ctypes.c_int64 * 3)(48, 16, 4)
    seen = []

    def both(p, s, d, go=fake, gr=fake, gm=fake, gb=fake, atomic_too=True):
        """(code of the shared-colour gather entry, code of the depth-alpha one); with `atomic_too` each must equal its atomic entry's code."""
        out = []
        for depth in (False, True):
            mid = (ref(d),) if depth else ()
            tail = (go, None, None, gr, s3, gm, s3, gb, s3, None)
            fn = lib.gmpi_mpi_render_depth_backward_gather_launch if depth else lib.gmpi_mpi_render_shared_backward_gather_launch
            at = lib.gmpi_mpi_render_depth_backward_launch if depth else lib.gmpi_mpi_render_shared_backward_launch
            rc = fn(ref(p), ref(s), *mid, *tail)
            if atomic_too:
                assert rc == at(ref(p), ref(s), *mid, *tail), (depth, rc)
            out.append(rc)
        seen.append(out)
        return tuple(out)

    query = lambda p, s, d: (lib.gmpi_render_layout_backward_gather_workspace_bytes(ref(p), ref(s), None),
                             lib.gmpi_render_layout_backward_gather_workspace_bytes(ref(p), ref(s), ref(d)))
    # argument errors: the atomic entries' codes (GMPI_E_NULL, _DTYPE, _STRIDE, _ABI, _FLAGS, _SHAPE), and a query of 0
    assert both(params(N=0), shared(), ramp()) == (0, 0) and query(params(N=0), shared(), ramp()) == (0, 0)
    assert both(None, shared(), ramp()) == (-1, -1) and both(params(), None, ramp()) == (-1, -1)
    assert lib.gmpi_mpi_render_depth_backward_gather_launch(ref(params()), ref(shared()), None, fake, None, None, fake, s3, fake, s3, fake, s3, None) == -1
    p = params(); p.rgba_dtype = L.DTYPE_U8
    assert both(p, shared(), ramp()) == (-3, -3) and query(p, shared(), ramp()) == (0, 0)
    p = params(); p.rgba_stride[4] = 2
    assert both(p, shared(), ramp()) == (-4, -4) and query(p, shared(), ramp()) == (0, 0)
    p = params(); p.struct_size -= 8
    assert both(p, shared(), ramp()) == (-5, -5) and query(p, shared(), ramp()) == (0, 0)
    p = params(); p.flags |= 1 << 30
    assert both(p, shared(), ramp()) == (-7, -7)
    assert both(params(), shared(), ramp(), go=None) == (-1, -1)
    assert both(params(), shared(), ramp(), gr=None, gm=None, gb=None) == (-1, -1)                 # all three NULL
    assert both(params(), shared(with_bg=False), ramp()) == (-1, -1)                                 # a background gradient without a background
    assert both(params(N=65536), shared(), ramp()) == (-2, -2)
    # any variant but AUTO: GMPI_E_VARIANT, the query 0 (GATHER runs the atomic entries' one-pixel kernels: no error there)
    for v in (L.VARIANT_GATHER, L.VARIANT_LDS, L.VARIANT_WAVE, L.VARIANT_DMA, L.VARIANT_BAND, 9):
        p = params(); p.variant = v
        assert both(p, shared(), ramp(), atomic_too=False) == (-6, -6), v
        assert query(p, shared(), ramp()) == (0, 0), v
    # launches the pair does not support: GMPI_E_VARIANT exactly where the query is 0
    v2m = np.zeros(1, dtype=np.int32)
    unsupported = []
    p = params(flags=0); unsupported.append(p)                                   # align_corners = False
    p = params(); p.view_to_mpi = v2m.ctypes.data; unsupported.append(p)          # a view list
    p = params(); p.Wt = 1; unsupported.append(p)                                 # Wt < 2
    p = params(); p.H, p.W = 1 << 16, 1 << 15; unsupported.append(p)              # H W = 2^31
    for p in unsupported:
        assert query(p, shared(), ramp()) == (0, 0)
        assert both(p, shared(), ramp(), atomic_too=False) == (-6, -6)
    # a supported launch: the query is records + 24 bytes per pixel and plane (+ slabs), a multiple of 256 ...
    need = query(params(), shared(), ramp())
    runs = lib.gmpi_render_layout_backward_gather_runs(ref(params()), ref(shared()), None)
    assert runs == 3                                                             # one tile: a plane per run
    records, pixels = 256, 1 * 3 * 4 * 4 * 24
    assert need == tuple((records + pixels + 1 * runs * c * 4 * 4 * 4 + 255) // 256 * 256 for c in (3, 4))
    lib.gmpi_render_layout_backward_gather_set_runs(1)
    try:
        assert lib.gmpi_render_layout_backward_gather_runs(ref(params()), ref(shared()), ref(ramp())) == 1
        assert query(params(), shared(), ramp()) == ((records + pixels + 255) // 256 * 256,) * 2
    finally:
        lib.gmpi_render_layout_backward_gather_set_runs(0)
    assert query(params(), shared(), ramp()) == need
    # ... and the launch refuses a workspace that is missing, too small or misaligned: GMPI_E_WORKSPACE
    base = (fake + 255) // 256 * 256
    assert both(params(), shared(), ramp(), atomic_too=False) == (-8, -8)
    assert both(params(ws=base, ws_bytes=min(need) - 1), shared(), ramp(), atomic_too=False) == (-8, -8)
    assert both(params(ws=base + 128, ws_bytes=max(need)), shared(), ramp(), atomic_too=False) == (-8, -8)
    assert len(seen) >= 24


# ---- the kernels' resources, from their descriptors ----------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_layout_gather_kernels_have_no_scratch(tmp_path):
    csrc = os.path.join(ROOT, "ml-gmpi_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
             "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]   # = ml-gmpi_amd/csrc/Makefile
    mk = open(os.path.join(csrc, "Makefile")).read()
    for f in ("-ffp-contract=off", "-fno-slp-vectorize", "-O3", "render_backward_gather.hip"):
        assert f in mk, f"the Makefile no longer has {f}: keep this test in step with it"
    res = subprocess.run([HIPCC, *flags, "-save-temps", "-c", os.path.join(csrc, "render_backward_gather.hip"), "-o", "render_backward_gather.o"],
                         cwd=tmp_path, capture_output=True, timeout=900)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    asm = open(os.path.join(tmp_path, "render_backward_gather-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    kernels = {}
    for name, meta in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel", asm, flags=re.M | re.S):   # the descriptors only
        field = lambda key: int(re.search(r"\.amdhsa_" + key + r"\s+(\d+)", meta).group(1))
        kernels[name] = (field("private_segment_fixed_size"), field("group_segment_fixed_size"), field("next_free_vgpr"))
    new = {n: v for n, v in kernels.items() if "layout_" in n}
    count = lambda part: sum(part in n for n in new)
    # pixel pass: 3 storage types x 2 layouts; texel pass and reduce: overwrite x layout
    assert (count("layout_pixel_pass_kernel"), count("layout_texel_gather_kernel"), count("layout_reduce_kernel")) == (6, 4, 4), sorted(new)
    for name, (scratch, lds, vgpr) in sorted(new.items()):
        print(name, "scratch", scratch, "lds", lds, "vgpr", vgpr)
        assert scratch == 0, (name, scratch)
        if "layout_texel_gather_kernel" in name:
            assert 49152 <= lds <= 53248 and vgpr <= 128, (name, lds, vgpr)   # the volume kernel's staging buffers + the sink's parameters; two workgroups per CU
        else:
            assert lds == 0, (name, lds)
    shutil.rmtree(tmp_path, ignore_errors=True)
