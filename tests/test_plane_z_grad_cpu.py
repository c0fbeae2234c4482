"""The gradient w.r.t. plane_z of the depth-alpha layout without a GPU: what the bridge hands the C ABI when plane_z requires grad under
geometry_grad="all" (through test_marshal_cpu's recorder: the new workspace query and the new entry, once), the new entry's refusals on the host
library, the two workspace queries against each other, and the compiler's report for the PZ instances of render_backward_geometry.hip."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from ml_gmpi_amd import _lib
from ml_gmpi_amd.hip_mpi import MPI
from test_depth_alpha_cpu import check_depth_alpha, depth_inputs
from test_marshal_cpu import BACKWARD_ENTRIES, FORWARD_ENTRIES, Recorder, check_backward_struct, check_shared_color

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FORWARD = "gmpi_mpi_render_depth_launch"
IMAGE = "gmpi_mpi_render_depth_backward_launch"
OLD_GEO, OLD_QUERY = "gmpi_mpi_render_depth_geometry_backward_launch", "gmpi_render_geometry_backward_workspace_bytes"
PZ_GEO, PZ_QUERY = "gmpi_mpi_render_depth_geometry_backward_pz_launch", "gmpi_render_depth_geometry_backward_workspace_bytes"
GEO_NAMES = ("dhw", "ray_dir", "eye_pos", "z_dir")


@pytest.fixture
def rec(monkeypatch):
    r = Recorder(FORWARD_ENTRIES + BACKWARD_ENTRIES + (FORWARD, IMAGE, "gmpi_mpi_render_depth_backward_tile_launch", OLD_GEO, OLD_QUERY, PZ_GEO, PZ_QUERY))
    monkeypatch.setattr(_lib, "load_library", lambda: r)
    return r


def _with_grad(geo, names):
    return tuple(t.clone().requires_grad_(name in names) for t, name in zip(geo, GEO_NAMES))


def _check_pz_call(call, pz, geo, names):
    """The five output pointers of the new entry (ray, eye, z_dir, dhw, plane_z from argument 6 on): plane_z's is never NULL, the others follow
    needs_input_grad; the gradient has plane_z's shape and dtype."""
    ray_p, eye_p, zd_p, dhw_p, pz_p = call.args[6:11]
    assert pz_p is not None
    assert [p is not None for p in (dhw_p, ray_p, eye_p, zd_p)] == [n in names for n in GEO_NAMES]
    assert call.args[11] == 0 and len(call.args) == 12   # the stream
    for t, name in zip(geo, GEO_NAMES):
        assert (t.grad is not None) == (name in names), name
    assert pz.grad is not None and pz.grad.shape == pz.shape and pz.grad.dtype == pz.dtype and pz.grad.device == pz.device
    assert call.args[0].workspace is not None   # (the plane_z sums go through slabs)


@pytest.mark.parametrize("pz_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("per_mpi_table", [False, True])
@pytest.mark.parametrize("names", [(), ("dhw",), ("ray_dir",), ("eye_pos", "z_dir"), GEO_NAMES])
def test_plane_z_alone_is_the_new_query_and_the_new_entry(rec, names, per_mpi_table, pz_dtype):
    rgb, depth, pz, bg, geo = depth_inputs(per_mpi_table=per_mpi_table)
    pz = pz.to(pz_dtype).requires_grad_(True)
    geo = _with_grad(geo, names)
    res = MPI(geometry_grad="all").render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg)
    ((res["color"] * 0.5).sum() + res["depth"].sum()).backward()
    assert [c.name for c in rec.calls] == [FORWARD, PZ_QUERY, PZ_GEO]   # once, whatever else is wanted; never the old pair
    fwd, q, bwd = rec.calls
    assert q.args[1:] == (int("dhw" in names), 1)   # want_dhw, want_plane_z
    b, f = bwd.args[0], fwd.args[0]
    for k, _ in _lib.GmpiRenderParams._fields_:
        if k in ("rgb_out", "depth_out", "status"):
            assert getattr(b, k) is None, k
        elif k == "rgba_stride":
            assert list(b.rgba_stride) == list(f.rgba_stride)
        elif k not in ("workspace", "workspace_bytes"):
            assert getattr(b, k) == getattr(f, k), k
    assert bytes(bwd.args[1]) == bytes(fwd.args[1]) and bytes(bwd.args[2]) == bytes(fwd.args[2])   # GmpiSharedColor, GmpiDepthAlpha: the forward's
    check_shared_color(bwd.args[1], rgb, bg)
    assert bwd.args[2].plane_z_stride == (pz.shape[1] if per_mpi_table else 0)
    if pz_dtype is torch.float32:
        check_depth_alpha(bwd.args[2], pz, -0.2, 0.2)   # (fp32 on the device already: the kernels read the caller's table)
    assert bwd.args[3] is not None and bwd.args[4] is not None and bwd.args[5] is None   # gC, gZ, no gT
    _check_pz_call(bwd, pz, geo, names)
    assert rgb.grad is None and depth.grad is None and bg.grad is None


@pytest.mark.parametrize("depth_backward", ["pixel", "tile"])
def test_images_and_plane_z_are_the_image_backward_and_the_new_pair(rec, depth_backward):
    rgb, depth, pz, bg, geo = depth_inputs()
    rgb.requires_grad_(True), depth.requires_grad_(True), pz.requires_grad_(True)
    geo = _with_grad(geo, ("ray_dir", "dhw"))
    res = MPI(geometry_grad="all").render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg, depth_backward=depth_backward, want_transmittance=True)
    (res["color"].sum() + (res["T"] * 2.0).sum()).backward()
    image = IMAGE if depth_backward == "pixel" else "gmpi_mpi_render_depth_backward_tile_launch"
    assert [c.name for c in rec.calls] == [FORWARD, image, PZ_QUERY, PZ_GEO]
    check_backward_struct(rec.calls[1], rec.calls[0], False)
    assert rec.calls[1].args[0].workspace is None   # the image entry runs exactly as it did
    assert rec.calls[2].args[1:] == (1, 1)
    assert rec.calls[3].args[5] is not None         # gT: the loss reaches T
    _check_pz_call(rec.calls[3], pz, geo, ("ray_dir", "dhw"))
    assert rgb.grad is not None and depth.grad is not None and bg.grad is None


def test_without_plane_z_the_old_pair_and_without_all_nothing_new(rec):
    rgb, depth, pz, bg, geo = depth_inputs()
    geo = _with_grad(geo, ("dhw",))
    res = MPI(geometry_grad="all").render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg)   # plane_z needs no gradient
    res["color"].sum().backward()
    assert [c.name for c in rec.calls] == [FORWARD, OLD_QUERY, OLD_GEO]
    assert len(rec.calls[2].args) == 11 and rec.calls[1].args[1:] == (1,)   # the old arguments
    for gg in (False, True):   # geometry_grad False / True: plane_z is detached as ever
        rec.calls.clear()
        rgb, depth, pz, bg, geo = depth_inputs()
        pz.requires_grad_(True)
        out = MPI(geometry_grad=gg).render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg)
        assert not out["color"].requires_grad and [c.name for c in rec.calls] == [FORWARD]
        rec.calls.clear()
        rgb.requires_grad_(True)
        MPI(geometry_grad=gg).render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg)["color"].sum().backward()
        assert [c.name for c in rec.calls] == [FORWARD, IMAGE] and pz.grad is None and rgb.grad is not None
    rec.calls.clear()
    with torch.no_grad():
        MPI(geometry_grad="all").render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg)
    assert [c.name for c in rec.calls] == [FORWARD]


def test_an_unused_output_launches_nothing(rec):
    rgb, depth, pz, bg, geo = depth_inputs()
    pz.requires_grad_(True)
    res = MPI(geometry_grad="all").render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg)
    (res["color"].detach().sum() + pz.sum()).backward()
    assert [c.name for c in rec.calls] == [FORWARD]


# ---- the C ABI on the host -------------------------------------------------------------------------------------------------------------------------
def test_exports_and_query_ids():
    assert PZ_GEO in _lib.EXPORTS and PZ_QUERY in _lib.EXPORTS
    lib = _lib.load_library()
    assert lib.gmpi_query(40) == 1 and lib.gmpi_query(39) == -1
    assert lib.gmpi_query(0) == 2 and lib.gmpi_query(1) == 184   # GMPI_ABI_VERSION and GmpiRenderParams: unchanged
    header = open(os.path.join(ROOT, "include", "gmpi_render.h")).read()
    assert re.search(r"\bint\s+" + PZ_GEO + r"\s*\(", header) and re.search(r"\buint64_t\s+" + PZ_QUERY + r"\s*\(", header)


def test_argument_errors_need_no_device():
    """Every refusal of the new entry is decided on the host, before any launch: host pointers are enough."""
    from ml_gmpi_amd.hip_mpi import _Keep, _Scalars, _depth_alpha, _render_params, _shared_color
    lib = _lib.load_library()
    rgb, depth, pz, bg, (dhw, ray, eye, zd) = depth_inputs()
    Mn, _, Ht, Wt = depth.shape
    N, _, H, W = ray.shape
    D = dhw.shape[1]
    depth5 = depth.unsqueeze(1)
    T, gc = torch.ones((N, 1, H, W)), torch.ones((N, 3, H, W))
    g_ray, g_pz = torch.empty((N, 3, H, W)), torch.empty((D,))
    sc, da = _shared_color(rgb, bg), _depth_alpha(pz, -0.2, 0.2)
    ref = lambda x: None if x is None else ctypes.byref(x)
    ptr = lambda t: None if t is None else t.data_ptr()

    def params(dtype=_lib.DTYPE_F32, variant=_lib.VARIANT_AUTO):
        return _render_params(_Scalars(1, variant, dtype, N, Mn, D, Ht, Wt, H, W, 1), _Keep(depth5, dhw, ray, eye, zd, None), T=T)

    def call(p, sc_=sc, da_=da, gc_=gc, ray_=g_ray, pz_=None):
        return lib.gmpi_mpi_render_depth_geometry_backward_pz_launch(ref(p), ref(sc_), ref(da_), ptr(gc_), None, None, ptr(ray_), None, None, None, ptr(pz_), None)
    E_NULL, E_SHAPE, E_DTYPE, E_STRIDE, E_ABI, E_VARIANT, E_WORKSPACE = -1, -2, -3, -4, -5, -6, -8
    assert call(None) == E_NULL and call(params(), sc_=None) == E_NULL and call(params(), da_=None) == E_NULL
    assert call(params(), gc_=None) == E_NULL
    assert call(params(dtype=_lib.DTYPE_U8)) == E_DTYPE
    assert call(params(variant=_lib.VARIANT_WAVE)) == E_VARIANT
    bad = _depth_alpha(pz, -0.2, 0.2)
    bad.z_den = 0.0
    assert call(params(), da_=bad) == E_SHAPE
    bad = _depth_alpha(pz, -0.2, 0.2)
    bad.plane_z_stride = -1
    assert call(params(), da_=bad) == E_STRIDE
    p = params()
    p.struct_size = 180
    assert call(p) == E_ABI
    assert call(params(), ray_=None) == 0                               # nothing wanted: nothing launched
    assert call(params(), pz_=g_pz) == E_WORKSPACE                      # plane_z wanted without a workspace
    assert call(params(), ray_=None, pz_=g_pz) == E_WORKSPACE
    query = lambda p, d, z: int(lib.gmpi_render_depth_geometry_backward_workspace_bytes(ctypes.byref(p), d, z))
    old = lambda p, d: int(lib.gmpi_render_geometry_backward_workspace_bytes(ctypes.byref(p), d))
    for d in (0, 1):   # too small by one 256-byte step: what the launch without plane_z needs (never dereferenced)
        p = params()
        p.workspace, p.workspace_bytes = 256, query(params(), d, 1) - 256
        assert call(p, pz_=g_pz) == E_WORKSPACE
    p = params()
    p.workspace, p.workspace_bytes = 256 + 4, query(params(), 0, 1)   # not 256-byte aligned
    assert call(p, pz_=g_pz) == E_WORKSPACE
    p = params()
    p.N = 0
    assert call(p, pz_=g_pz) == 0                                       # no views
    # the two queries
    p = params()
    assert query(p, 1, 1) - query(p, 1, 0) >= D * N * 4 and query(p, 0, 1) - query(p, 0, 0) >= D * N * 4
    assert query(p, 0, 0) == old(p, 0) > 0 and query(p, 1, 0) == old(p, 1) > 0
    assert query(p, 1, 1) >= (6 + 4 * D) * N * 4
    assert query(params(dtype=_lib.DTYPE_U8), 1, 1) == 0 == old(params(dtype=_lib.DTYPE_U8), 1)


# ---- the compiler's report -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_the_plane_z_instances_compile_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "ml-gmpi_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
             "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]   # = ml-gmpi_amd/csrc/Makefile
    mk = open(os.path.join(csrc, "Makefile")).read()
    for f in ("-ffp-contract=off", "-fno-slp-vectorize", "-O3", "render_backward_geometry.hip"):
        assert f in mk, f"the Makefile no longer has {f}: keep this test in step with it"
    res = subprocess.run([HIPCC, *flags, "-save-temps", "-c", os.path.join(csrc, "render_backward_geometry.hip"), "-o", "render_backward_geometry.o"],
                         cwd=tmp_path, capture_output=True, timeout=900)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    asm = open(os.path.join(tmp_path, "render_backward_geometry-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    seen = set()
    for name in sorted(set(re.findall(r"^(_Z\w*(?:geometry_pixel_kernel\w*PlaneZGrad\w*|plane_z_reduce_kernel\w*)):", asm, flags=re.M))):
        meta = asm[asm.index(".amdhsa_kernel " + name):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1)) == 0, name
        seen.add(name)
    assert len(seen) == 24 + 1, sorted(seen)   # 3 storage types x align_corners x order x dhw, and the reducer
