"""geometry_grad="all" over the volume as STORED, without a GPU: what the uint8 bridge (`render_views`) and the float-layers bridge
(`render_views_layers`) hand the C ABI when a camera tensor or dhw requires grad (through test_marshal_cpu's recorder) -- the forward, the workspace
query of the in-place entries, the in-place geometry entry over the SAVED storage with NULL for every output nobody wants, and no volume backward
unless the layers themselves need a gradient -- and the refusals of the two C entries on host pointers."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from ml_gmpi_amd import _lib
from ml_gmpi_amd.hip_mpi import MPI
from ml_gmpi_amd.layers import layer_strides
from test_geometry_layouts_cpu import GEO_NAMES, WANTS, _check_outputs, _with_grad
from test_marshal_cpu import BACKWARD_ENTRIES, FORWARD_ENTRIES, Recorder, make_inputs
from test_u8_storage_cpu import u8_inputs

U8_GEO = "gmpi_mpi_render_u8_geometry_backward_launch"
LAYERS_GEO = "gmpi_mpi_render_layers_geometry_backward_launch"
QUERY = "gmpi_render_geometry_inplace_workspace_bytes"
OLD_QUERY = "gmpi_render_geometry_backward_workspace_bytes"
LAYERS_ENTRIES = ("gmpi_mpi_render_layers_launch", "gmpi_render_layers_supports", "gmpi_mpi_render_layers_backward_launch",
                  "gmpi_render_layers_backward_supports")
VOLUME_BACKWARDS = ("gmpi_mpi_render_backward_launch", "gmpi_mpi_render_backward_ex_launch", "gmpi_mpi_render_geometry_backward_launch",
                    "gmpi_mpi_render_geometry_backward_ex_launch")


@pytest.fixture
def rec(monkeypatch):
    r = Recorder(FORWARD_ENTRIES + BACKWARD_ENTRIES + LAYERS_ENTRIES + (U8_GEO, LAYERS_GEO, QUERY))
    monkeypatch.setattr(_lib, "load_library", lambda: r)
    return r


def _same_launch(b, f):
    """The struct a geometry entry gets is the forward's, rebuilt: field by field (outputs and status: a backward names none; T: the node's)."""
    for k, _ in _lib.GmpiRenderParams._fields_:
        if k in ("rgb_out", "depth_out", "status"):
            assert getattr(b, k) is None, k
        elif k == "rgba_stride":
            assert list(b.rgba_stride) == list(f.rgba_stride)
        elif k not in ("workspace", "workspace_bytes"):
            assert getattr(b, k) == getattr(f, k), k
    assert b.transmittance_out is not None and b.transmittance_out == f.transmittance_out


# ---- uint8 volumes -------------------------------------------------------------------------------------------------------------------------------
def _u8_volume(layout):
    q, *geo = u8_inputs(2)
    if layout == "u8cl":   # channels-last codes: the view [M,D,4,Ht,Wt] of layers [M,D,Ht,Wt,4]
        q = q.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    return q, geo


@pytest.mark.parametrize("uses_T", [False, True])
@pytest.mark.parametrize("names", WANTS)
@pytest.mark.parametrize("layout", ["u8", "u8cl"])
def test_uint8_bridge_launches_the_in_place_geometry_entry_alone(rec, layout, names, uses_T):
    q, geo = _u8_volume(layout)
    geo = _with_grad(geo, names)
    res = MPI(geometry_grad="all").render_views(q, *geo, want_transmittance=True)
    loss = (res["color"] * 0.5).sum() + res["depth"].sum()
    (loss + (res["T"] * 2.0).sum() if uses_T else loss).backward()
    slabs = any(n in names for n in ("dhw", "eye_pos", "z_dir"))
    assert [c.name for c in rec.calls] == ["gmpi_mpi_render_launch"] + ([QUERY] if slabs else []) + [U8_GEO]   # no volume backward, no old query
    fwd, bwd = rec.calls[0], rec.calls[-1]
    b = bwd.args[0]
    _same_launch(b, fwd.args[0])
    M, D, _, Ht, Wt = q.shape
    assert b.rgba_dtype == _lib.DTYPE_U8 and b.rgba == q.data_ptr()   # the codes themselves
    want_strides = [D * 4 * Ht * Wt, 4 * Ht * Wt, Ht * Wt, Wt, 1] if layout == "u8" else [D * Ht * Wt * 4, Ht * Wt * 4, 1, Wt * 4, 4]
    assert list(b.rgba_stride) == want_strides
    assert bwd.args[1] is not None and bwd.args[2] is not None and (bwd.args[3] is not None) == uses_T   # gC, gZ, gT (always an argument)
    assert len(bwd.args) == 9
    _check_outputs(bwd, 4, geo, names)
    assert (b.workspace is not None) == slabs
    if slabs:
        assert rec.named(QUERY)[0].args[1] == int("dhw" in names)   # want_dhw
    assert q.grad is None and not q.requires_grad


def test_uint8_true_still_raises_and_nothing_that_requires_grad_is_the_forward_alone(rec):
    q, geo = _u8_volume("u8")
    with pytest.raises(NotImplementedError, match="dequantize_volume"):
        MPI(geometry_grad=True).render_views(q, *_with_grad(geo, ("ray_dir",)))
    assert rec.calls == []
    MPI(geometry_grad="all").render_views(q, *geo)
    assert [c.name for c in rec.calls] == ["gmpi_mpi_render_launch"]
    rec.calls.clear()
    with torch.no_grad():
        MPI(geometry_grad="all").render_views(q, *_with_grad(geo, ("ray_dir",)))
    assert [c.name for c in rec.calls] == ["gmpi_mpi_render_launch"]
    rec.calls.clear()
    ray = geo[1].clone().requires_grad_(True)   # geometry_grad False: no gradient, nothing recorded
    res = MPI().render_views(q, geo[0], ray, geo[2], geo[3])
    assert not res["color"].requires_grad and [c.name for c in rec.calls] == ["gmpi_mpi_render_launch"]


def test_the_float_volume_entry_is_what_it_was(rec):
    vol, *geo = make_inputs(2)
    geo = _with_grad(geo, GEO_NAMES)
    MPI(geometry_grad="all").render_views(vol, *geo)["color"].sum().backward()
    assert [c.name for c in rec.calls] == ["gmpi_mpi_render_launch", OLD_QUERY, "gmpi_mpi_render_geometry_backward_launch"]


# ---- float layers --------------------------------------------------------------------------------------------------------------------------------
def _layers(dtype=torch.float32, sliced=False):
    vol, *geo = make_inputs(2)
    M, D, _, Ht, Wt = vol.shape
    if sliced:   # padded rows and a column offset: a texel starts at any element
        big = torch.rand((M, D, Ht + 3, Wt + 5, 4)).to(dtype)
        return big[:, :, 2:-1, 3:-2], geo
    return vol.permute(0, 1, 3, 4, 2).contiguous().to(dtype), geo


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("names", WANTS)
@pytest.mark.parametrize("mode", ["planar", "texel"])
def test_layers_bridge_without_a_layer_gradient_is_the_geometry_launch_alone(rec, mode, names, sliced):
    layers, geo = _layers(sliced=sliced)
    geo = _with_grad(geo, names)
    res = MPI(geometry_grad="all").render_views_layers(layers, *geo, layers_backward=mode)
    ((res["color"] * 0.5).sum() + res["depth"].sum()).backward()
    slabs = any(n in names for n in ("dhw", "eye_pos", "z_dir"))
    assert [c.name for c in rec.calls] == ["gmpi_mpi_render_layers_launch"] + ([QUERY] if slabs else []) + [LAYERS_GEO]
    fwd, bwd = rec.calls[0], rec.calls[-1]
    b = bwd.args[0]
    _same_launch(b, fwd.args[0])
    assert b.rgba == layers.data_ptr() and list(b.rgba_stride) == layer_strides(layers)   # the layers in place, as the volume they are a view of
    assert bwd.args[1] is not None and bwd.args[2] is not None and bwd.args[3] is None and len(bwd.args) == 9
    _check_outputs(bwd, 4, geo, names)
    assert (b.workspace is not None) == slabs
    if slabs:
        q = rec.named(QUERY)[0]
        assert q.args[1] == int("dhw" in names) and list(q.args[0].rgba_stride) == layer_strides(layers)
    assert layers.grad is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("uses_T", [False, True])
@pytest.mark.parametrize("mode", ["planar", "texel"])
def test_layers_and_geometry_together_are_the_layers_backward_then_the_geometry_entry(rec, mode, uses_T, dtype):
    layers, geo = _layers(dtype)
    layers.requires_grad_(True)
    names = ("dhw", "ray_dir")
    geo = _with_grad(geo, names)
    res = MPI(geometry_grad="all").render_views_layers(layers, *geo, layers_backward=mode, want_transmittance=True)
    loss = res["color"].sum()
    (loss + res["T"].sum() if uses_T else loss).backward()
    first = ("gmpi_mpi_render_backward_ex_launch" if uses_T else "gmpi_mpi_render_backward_launch") if mode == "planar" else "gmpi_mpi_render_layers_backward_launch"
    assert [c.name for c in rec.calls] == ["gmpi_mpi_render_layers_launch", first, QUERY, LAYERS_GEO]
    b = rec.calls[-1].args[0]
    _same_launch(b, rec.calls[0].args[0])
    assert b.rgba == layers.data_ptr() and list(b.rgba_stride) == layer_strides(layers)   # never the planar copy, in either mode
    if mode == "planar":
        assert rec.calls[1].args[0].rgba != layers.data_ptr()
    assert (rec.calls[-1].args[3] is not None) == uses_T
    _check_outputs(rec.calls[-1], 4, geo, names)
    assert layers.grad is not None and layers.grad.shape == layers.shape and layers.grad.dtype == dtype


def test_layers_that_had_to_be_copied_take_the_same_path_over_the_copy(rec):
    layers, geo = _layers()
    odd = layers.permute(0, 1, 2, 4, 3).contiguous().permute(0, 1, 2, 4, 3)   # the right shape, texels not contiguous
    geo = _with_grad(geo, ("eye_pos",))
    mpi = MPI(geometry_grad="all")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # (the once-per-process warning of a copy: tests/test_float_layers_cpu.py checks it)
        res = mpi.render_views_layers(odd, *geo)
    res["color"].sum().backward()
    assert mpi.layers_copies == 1
    assert [c.name for c in rec.calls] == ["gmpi_mpi_render_layers_launch", QUERY, LAYERS_GEO]
    b, f = rec.calls[-1].args[0], rec.calls[0].args[0]
    assert b.rgba == f.rgba and b.rgba != odd.data_ptr() and list(b.rgba_stride) == list(f.rgba_stride)


def test_layers_true_still_raises_and_the_other_entries_still_refuse(rec):
    layers, geo = _layers()
    with pytest.raises(NotImplementedError, match="float layers"):
        MPI(geometry_grad=True).render_views_layers(layers, *_with_grad(geo, ("ray_dir",)))
    vol = layers.permute(0, 1, 4, 2, 3).contiguous()
    with pytest.raises(NotImplementedError):
        MPI(geometry_grad="all").render_views_shaded(vol, torch.ones((2, 1) + tuple(vol.shape[3:])), *_with_grad(geo, ("ray_dir",)))
    with pytest.raises(NotImplementedError):
        MPI(geometry_grad="all").render_views_chunks([vol[:, :2], vol[:, 2:]], *_with_grad(geo, ("ray_dir",)))
    assert rec.calls == []


# ---- the C ABI on the host -------------------------------------------------------------------------------------------------------------------------
def _library():
    import os
    if not os.path.isfile(_lib.library_path()):
        pytest.skip("library not built")
    return _lib.load_library()


def test_exports_binding_and_query_id():
    for name in (U8_GEO, LAYERS_GEO, QUERY):
        assert name in _lib.EXPORTS
    lib = _library()
    assert lib.gmpi_query(48) == 1 and lib.gmpi_query(47) == -1 and lib.gmpi_query(49) == -1
    assert lib.gmpi_query(0) == 2 and lib.gmpi_query(1) == 184   # GMPI_ABI_VERSION and GmpiRenderParams: unchanged
    assert lib.gmpi_mpi_render_u8_geometry_backward_launch.argtypes == lib.gmpi_mpi_render_geometry_backward_ex_launch.argtypes


M_, D_, Ht_, Wt_, H_, W_, N_ = 1, 2, 8, 8, 4, 70, 2   # two 64 x 4 tiles per view


def _host_params(kind, dtype=None):
    """A launch over HOST buffers (only what is validated before a launch may be asked of it).  kind: "u8" planar codes, "u8cl" channels-last codes,
    "layers" channels-last float layers, "planar" a planar float volume."""
    esize = 1 if kind in ("u8", "u8cl") else 4
    bufs = dict(rgba=np.zeros(M_ * D_ * 4 * Ht_ * Wt_ * esize + 16, np.uint8), dhw=np.ones((M_, D_, 3), np.float32), ray=np.ones((N_, 3, H_, W_), np.float32),
                eye=np.zeros((N_, 3), np.float32), zd=np.ones((N_, 3), np.float32), T=np.ones((N_, 1, H_, W_), np.float32),
                gc=np.ones((N_, 3, H_, W_), np.float32))
    p = _lib.GmpiRenderParams()
    p.struct_size = ctypes.sizeof(_lib.GmpiRenderParams)
    p.flags, p.variant = 1, 0
    p.rgba_dtype = dtype if dtype is not None else (_lib.DTYPE_U8 if esize == 1 else _lib.DTYPE_F32)
    p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = N_, M_, D_, Ht_, Wt_, H_, W_, 2
    p.rgba = bufs["rgba"].ctypes.data
    planar, texel = [D_ * 4 * Ht_ * Wt_, 4 * Ht_ * Wt_, Ht_ * Wt_, Wt_, 1], [D_ * Ht_ * Wt_ * 4, Ht_ * Wt_ * 4, 1, Wt_ * 4, 4]
    p.rgba_stride[:] = planar if kind in ("u8", "planar") else texel
    p.dhw, p.ray_dir, p.eye_pos, p.z_dir = (bufs[k].ctypes.data for k in ("dhw", "ray", "eye", "zd"))
    p.transmittance_out = bufs["T"].ctypes.data
    return p, bufs


class _Outputs:
    """The four outputs as host arrays of a sentinel, and the check that a refusal wrote none of them."""
    def __init__(self):
        self.ray, self.eye = np.full((N_, 3, H_, W_), 7.0, np.float32), np.full((N_, 3), 7.0, np.float32)
        self.zd, self.dhw = np.full((N_, 3), 7.0, np.float32), np.full((M_, D_, 3), 7.0, np.float32)

    def untouched(self):
        return all(np.all(a == 7.0) for a in (self.ray, self.eye, self.zd, self.dhw))


def _call(lib, name, p, b, out, gc=True, ray=True, eye=False, zd=False, dhw=False, gT=False):
    h = lambda a, on=True: a.ctypes.data if on else None
    return getattr(lib, name)(ctypes.byref(p) if p is not None else None, h(b["gc"], gc), None, h(b["T"], gT), h(out.ray, ray), h(out.eye, eye), h(out.zd, zd),
                              h(out.dhw, dhw), None)


E_NULL, E_SHAPE, E_DTYPE, E_STRIDE, E_ABI, E_WORKSPACE = -1, -2, -3, -4, -5, -8


@pytest.mark.parametrize("name,kinds", [(U8_GEO, ("u8", "u8cl")), (LAYERS_GEO, ("layers",))])
def test_the_two_entries_refuse_on_the_host_and_write_nothing(name, kinds):
    lib = _library()
    query = lambda p, want_dhw: int(lib.gmpi_render_geometry_inplace_workspace_bytes(ctypes.byref(p), want_dhw))
    old = lambda p, want_dhw: int(lib.gmpi_render_geometry_backward_workspace_bytes(ctypes.byref(p), want_dhw))
    out = _Outputs()
    for kind in kinds:
        p, b = _host_params(kind)
        assert _call(lib, name, None, b, out) == E_NULL
        assert _call(lib, name, p, b, out, gc=False) == E_NULL                         # no grad_rgb
        assert _call(lib, name, p, b, out, ray=False) == 0                             # no output wanted: GMPI_OK, nothing launched
        for sums in (dict(eye=True), dict(zd=True), dict(dhw=True)):                   # a sum that goes through the slabs, without a workspace
            assert _call(lib, name, p, b, out, **sums) == E_WORKSPACE
        for want_dhw in (0, 1):
            need = query(p, want_dhw)
            assert need >= (6 + 3 * D_ * want_dhw) * N_ * 2 * 4 and need % 256 == 0    # per component: N views x 2 tiles of 64 x 4 pixels
            assert old(p, want_dhw) == 0                                               # the volume entry's query keeps refusing these params
            pp, _ = _host_params("planar")
            assert need == old(pp, want_dhw) == query(pp, want_dhw)                    # N, H, W and D only
            p.workspace, p.workspace_bytes = 256, need - 1                             # short by one byte (never dereferenced)
            assert _call(lib, name, p, b, out, eye=True, dhw=bool(want_dhw)) == E_WORKSPACE
            p.workspace, p.workspace_bytes = 256 + 4, need                             # not 256-byte aligned
            assert _call(lib, name, p, b, out, eye=True, dhw=bool(want_dhw)) == E_WORKSPACE
        p, b = _host_params(kind)
        p.struct_size = 180
        assert _call(lib, name, p, b, out) == E_ABI and query(p, 1) == 0
        p, b = _host_params(kind)
        p.N = 0
        assert _call(lib, name, p, b, out, eye=True, dhw=True) == 0 and query(p, 1) == 0   # no views: GMPI_OK at once, before any other check
        p, b = _host_params(kind)
        p.N = 65536
        p.views_per_mpi = 65536
        assert _call(lib, name, p, b, out) == E_SHAPE
        p, b = _host_params(kind)
        p.dhw = None
        assert _call(lib, name, p, b, out) == E_NULL
        p, b = _host_params(kind)
        p.rgba = None
        assert _call(lib, name, p, b, out) == E_NULL
        p, b = _host_params(kind)
        p.rgba_stride[3] = (1 if kind == "u8" else 4) * Wt_ - 1                        # rows that overlap
        assert _call(lib, name, p, b, out) == E_STRIDE
    if name == U8_GEO:
        for dtype in (_lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16, 4, -1):         # GMPI_DTYPE_U8 only, whatever the strides
            for kind in ("u8", "u8cl"):
                p, b = _host_params(kind, dtype)
                assert _call(lib, name, p, b, out) == E_DTYPE
        p, b = _host_params("u8")
        p.rgba_stride[4] = 2                                                           # neither planar nor channels-last
        assert _call(lib, name, p, b, out) == E_STRIDE
        p, b = _host_params("u8cl")
        p.rgba += 3                                                                    # a base pointer at any byte is no refusal
        assert _call(lib, name, p, b, out, ray=False) == 0
    else:
        p, b = _host_params("layers", _lib.DTYPE_U8)
        assert _call(lib, name, p, b, out) == E_DTYPE                                  # channels-last codes belong to the other entry
        p, b = _host_params("layers", 4)
        assert _call(lib, name, p, b, out) == E_DTYPE
        for dtype in (_lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16):
            p, b = _host_params("planar", dtype)
            assert _call(lib, name, p, b, out) == E_STRIDE                             # planar strides
            p, b = _host_params("layers", dtype)
            assert _call(lib, name, p, b, out, ray=False) == 0 and query(p, 1) > 0
        p, b = _host_params("planar", _lib.DTYPE_U8)
        assert _call(lib, name, p, b, out) == E_STRIDE                                 # (the strides are looked at first, as in the layers backward)
    assert out.untouched()
    # the volume entries keep refusing both: pinned by tests/test_u8_storage_cpu.py and tests/test_float_layers_cpu.py, restated for the new params
    for kind, want in (("u8", E_DTYPE), ("u8cl", E_DTYPE), ("layers", E_STRIDE)):
        p, b = _host_params(kind)
        assert _call(lib, "gmpi_mpi_render_geometry_backward_ex_launch", p, b, out) == want
    assert out.untouched()
