"""What `hip_mpi` hands the C ABI, pinned field by field without a GPU: the library is replaced by a recorder (`records_only`, as in
test_install_reference.py) that copies the structs of every call it is given.  Forward: every field of GmpiRenderParams / GmpiSharedColor
against literals and the tensors it must name.  Backward: the struct each bridge rebuilds must be the forward's (tests/test_hip_marshal.py
asserts the same on the device, through a recorder that forwards to the real library)."""
import collections
import ctypes

import pytest
import torch

from ml_gmpi_amd import _lib
from ml_gmpi_amd.hip_mpi import MPI

M, D, Ht, Wt, H, W = 2, 3, 6, 8, 4, 5

FORWARD_ENTRIES = ("gmpi_mpi_render_launch", "gmpi_mpi_render_shared_launch", "gmpi_rgba_range_check_launch")
BACKWARD_ENTRIES = ("gmpi_mpi_render_backward_launch", "gmpi_mpi_render_backward_ex_launch", "gmpi_mpi_render_geometry_backward_launch",
                    "gmpi_mpi_render_geometry_backward_ex_launch", "gmpi_mpi_render_shared_backward_launch",
                    "gmpi_render_geometry_backward_workspace_bytes")

Call = collections.namedtuple("Call", "name args v2m")   # v2m: the values behind GmpiRenderParams.view_to_mpi during the call (host tensors only)


class Recorder:
    """Stands in for libgmpi_render.so.  A call to one of `entries` is recorded with copies of its structs and arrays; with `real` (the
    loaded library) it is then forwarded, without it it returns GMPI_OK (0 bytes for a workspace query).  Every other name goes to `real`,
    or does not exist: a recorder without `real` sees exactly the entries it lists."""

    def __init__(self, entries=FORWARD_ENTRIES, real=None):
        self.entries, self.real, self.calls = entries, real, []
        self.records_only = real is None

    @staticmethod
    def _copy(a):
        a = getattr(a, "_obj", a)   # (ctypes.byref(x)._obj is x)
        if isinstance(a, ctypes.Structure):
            return type(a).from_buffer_copy(a)
        return list(a) if isinstance(a, ctypes.Array) else a

    def __getattr__(self, name):
        if name.startswith("__") or name not in self.entries:
            if name.startswith("__") or self.real is None:
                raise AttributeError(name)
            return getattr(self.real, name)

        def call(*args):
            copies = tuple(self._copy(a) for a in args)
            v2m = None
            if self.real is None and isinstance(copies[0], _lib.GmpiRenderParams) and copies[0].view_to_mpi:
                v2m = list((ctypes.c_int32 * copies[0].N).from_address(copies[0].view_to_mpi))
            self.calls.append(Call(name, copies, v2m))
            return 0 if self.real is None else getattr(self.real, name)(*args)
        return call

    def named(self, *names):
        return [c for c in self.calls if c.name in names]


@pytest.fixture
def rec(monkeypatch):
    r = Recorder(FORWARD_ENTRIES + BACKWARD_ENTRIES)
    monkeypatch.setattr(_lib, "load_library", lambda: r)
    return r


def make_inputs(n_views, dtype=torch.float32, device="cpu", seed=0):
    g = torch.Generator().manual_seed(seed)
    vol = torch.rand((M, D, 4, Ht, Wt), generator=g).to(dtype).to(device)
    # a scene a kernel can render (the device test launches it): planes at depth 1.. in front of eyes near z = -1 that look along +z
    dhw = torch.rand((M, D, 3), generator=g) * 0.5 + torch.tensor([1.0, 2.0, 2.0]) + torch.arange(D).view(1, D, 1) * torch.tensor([1.0, 0.0, 0.0])
    ray = torch.rand((n_views, 3, H, W), generator=g) * 0.2 - 0.1
    ray[:, 2] = 1.0
    eye = torch.rand((n_views, 3), generator=g) * 0.2 - 0.1 - torch.tensor([0.0, 0.0, 1.0])
    zd = torch.rand((n_views, 3), generator=g) * 0.1 + torch.tensor([0.0, 0.0, 1.0])
    return vol, dhw.to(device), ray.to(device), eye.to(device), zd.to(device)


POINTERS = ("rgba", "view_to_mpi", "dhw", "ray_dir", "eye_pos", "z_dir", "rgb_out", "depth_out", "transmittance_out", "status", "workspace")
SCALARS = dict(struct_size=184, flags=9, variant=0, rgba_dtype=0, N=2, M=2, D=3, Ht=6, Wt=8, H=4, W=5, views_per_mpi=1,
               rgba_stride=[576, 192, 48, 8, 1], workspace_bytes=0)


def scalars_of(p):
    return {k: (list(getattr(p, k)) if k == "rgba_stride" else getattr(p, k)) for k in SCALARS}


def check_struct(p, res, inputs, view_to_mpi=None, T=None, **literal):
    """Every non-pointer field against SCALARS overridden by `literal`; every pointer against the tensor it must name (None: NULL)."""
    assert scalars_of(p) == dict(SCALARS, **literal)
    vol, dhw, ray, eye, zd = inputs
    want = dict(rgba=vol, view_to_mpi=view_to_mpi, dhw=dhw, ray_dir=ray, eye_pos=eye, z_dir=zd, rgb_out=res["color"], depth_out=res["depth"],
                transmittance_out=T, status=res["status"], workspace=None)
    assert set(want) == set(POINTERS)
    for k, t in want.items():
        assert getattr(p, k) == (None if t is None else t.data_ptr()), k


def render(mpi, inputs, **kw):
    with torch.no_grad():
        return mpi.render_views(*inputs, **kw)


# ---- forward -----------------------------------------------------------------------------------------------------------------------------

def test_padded_rows_are_passed_without_a_copy(rec):
    big = torch.rand((M, D, 4, Ht, 2 * Wt))
    inputs = (big[..., :Wt],) + make_inputs(2)[1:]
    res = render(MPI(), inputs)
    (c,) = rec.calls
    assert c.name == "gmpi_mpi_render_launch" and c.args[1] == 0
    check_struct(c.args[0], res, inputs, rgba_stride=[1152, 384, 96, 16, 1])
    assert c.args[0].rgba == big.data_ptr()


def test_ragged_views_per_mpi_become_a_view_index(rec):
    inputs = make_inputs(3)
    res = render(MPI(), inputs, views_per_mpi=[1, 2])
    (c,) = rec.calls
    p = c.args[0]
    assert p.view_to_mpi is not None and c.v2m == [0, 1, 1]
    assert scalars_of(p) == dict(SCALARS, N=3, views_per_mpi=1)
    assert (p.rgba, p.rgb_out, p.status) == (inputs[0].data_ptr(), res["color"].data_ptr(), res["status"].data_ptr())


@pytest.mark.parametrize("views_per_mpi", [2, [2, 2]])
def test_uniform_views_per_mpi_need_no_view_index(rec, views_per_mpi):
    inputs = make_inputs(4)
    res = render(MPI(), inputs, views_per_mpi=views_per_mpi)
    (c,) = rec.calls
    check_struct(c.args[0], res, inputs, N=4, views_per_mpi=2)


def test_an_explicit_view_index_is_passed(rec):
    inputs = make_inputs(3)
    res = render(MPI(), inputs, view_to_mpi=torch.tensor([1, 0, 1], dtype=torch.int32))
    (c,) = rec.calls
    assert c.v2m == [1, 0, 1] and scalars_of(c.args[0]) == dict(SCALARS, N=3)
    assert res["color"].shape == (3, 3, H, W)


def test_flags_of_a_strict_lds_launch_with_every_option(rec):
    inputs = make_inputs(2)
    res = render(MPI(variant="lds", strict_order=True), inputs, out_pm1=True, check_last_plane=True, oblique_hint=True)
    (c,) = rec.calls
    check_struct(c.args[0], res, inputs, flags=287, variant=2)


@pytest.mark.parametrize("ctor,kw,flags", [
    ({}, dict(frontal_hint=True), 9 | 32),
    ({}, dict(tilted_hint=True), 9 | 64),
    (dict(range_check="off"), {}, 1),
    (dict(align_corners=False), {}, 8),
    ({}, dict(out_pm1=True), 9 | 2),
    ({}, dict(check_last_plane=True), 9 | 4),
    (dict(strict_order=True), {}, 9 | 16),
    ({}, dict(oblique_hint=True), 9 | 256),
])
def test_each_flag_bit(rec, ctor, kw, flags):
    inputs = make_inputs(2)
    res = render(MPI(**ctor), inputs, **kw)
    (c,) = rec.calls
    check_struct(c.args[0], res, inputs, flags=flags)


@pytest.mark.parametrize("name,value", [("auto", 0), ("gather", 1), ("lds", 2), ("wave", 3), ("band", 5)])
def test_variant_field(rec, name, value):
    assert set(_lib.VARIANTS) == {"auto", "gather", "lds", "wave", "band"}
    inputs = make_inputs(2)
    res = render(MPI(variant=name), inputs)
    check_struct(rec.calls[0].args[0], res, inputs, variant=value)


def test_transmittance_out_names_the_returned_T(rec):
    inputs = make_inputs(2)
    res = render(MPI(), inputs)
    assert res["T"] is None
    check_struct(rec.calls[0].args[0], res, inputs, T=None)
    res = render(MPI(), inputs, want_transmittance=True)
    assert res["T"].shape == (2, 1, H, W)
    check_struct(rec.calls[1].args[0], res, inputs, T=res["T"])


def test_caller_supplied_outputs_are_written_in_place(rec):
    inputs = make_inputs(2)
    out = dict(color=torch.empty((2, 3, H, W)), depth=torch.empty((2, 1, H, W)), T=torch.empty((2, 1, H, W)))
    status = torch.zeros(_lib.STATUS_WORDS, dtype=torch.int32)
    res = render(MPI(), inputs, want_transmittance=True, out=out, status=status)
    assert res["color"] is out["color"] and res["depth"] is out["depth"] and res["T"] is out["T"] and res["status"] is status
    check_struct(rec.calls[0].args[0], res, inputs, T=out["T"])


@pytest.mark.parametrize("dtype,code", [(torch.float32, 0), (torch.bfloat16, 1), (torch.float16, 2)])
def test_rgba_dtype_field(rec, dtype, code):
    inputs = make_inputs(2, dtype)
    res = render(MPI(), inputs)
    check_struct(rec.calls[0].args[0], res, inputs, rgba_dtype=code)


def test_a_dtype_the_kernels_do_not_store_becomes_fp32(rec):
    inputs = make_inputs(2, torch.float64)
    render(MPI(), inputs)
    p = rec.calls[0].args[0]
    assert p.rgba_dtype == 0 and p.rgba != inputs[0].data_ptr() and list(p.rgba_stride) == SCALARS["rgba_stride"]


def test_a_non_unit_innermost_stride_is_copied(rec):
    inputs = make_inputs(2)
    vol = torch.rand((M, D, 4, Wt, Ht)).transpose(3, 4)
    assert vol.shape == inputs[0].shape and vol.stride(4) != 1
    render(MPI(), (vol,) + inputs[1:])
    p = rec.calls[0].args[0]
    assert p.rgba != vol.data_ptr() and scalars_of(p) == SCALARS   # (contiguous: innermost stride 1)


def test_full_range_check_runs_before_the_render(rec):
    inputs = make_inputs(2)
    res = render(MPI(range_check="full"), inputs)
    assert [c.name for c in rec.calls] == ["gmpi_rgba_range_check_launch", "gmpi_mpi_render_launch"]
    assert rec.calls[0].args == (inputs[0].data_ptr(), 0, inputs[0].numel(), res["status"].data_ptr(), 0)
    check_struct(rec.calls[1].args[0], res, inputs)


def test_off_device_tensors_need_a_recorder(monkeypatch):
    class NoRecorder:
        pass
    monkeypatch.setattr(_lib, "load_library", lambda: NoRecorder())
    with pytest.raises(_lib.GmpiError, match="no CPU path"):
        render(MPI(), make_inputs(2))


class _LaunchingLibrary:
    """A library that is NOT a recorder, as the real one: every entry it is asked for counts as a launch."""

    def __init__(self):
        self.launched = []

    def __getattr__(self, name):
        if not name.startswith("gmpi_"):
            raise AttributeError(name)
        return lambda *args: self.launched.append(name) or 0


def test_no_entry_is_launched_on_host_tensors_without_a_recorder(monkeypatch):
    """The one helper for C-ABI calls refuses tensors that are not on a ROCm device unless the library only records: the real entries would
    run kernels on host pointers.  Through the helper itself and through the public paths that have no device check of their own."""
    from ml_gmpi_amd import hip_mpi
    from ml_gmpi_amd.light import LightRenderer
    lib = _LaunchingLibrary()
    monkeypatch.setattr(_lib, "load_library", lambda: lib)
    cpu = torch.device("cpu")
    with pytest.raises(_lib.GmpiError, match="gmpi_light_blur_launch needs tensors on a ROCm device"):
        hip_mpi._call("gmpi_light_blur_launch", cpu, 0, 0, 1, 4, 5, 0, 9)
    light = LightRenderer(sphere_center_z=1.0, sphere_r=1.0)
    with pytest.raises(_lib.GmpiError, match="ROCm device"):
        light.blurrer_func(torch.rand((2, 1, 12, 12)))
    with pytest.raises(_lib.GmpiError, match="ROCm device"):
        light.shading(torch.rand((2, 1, 12, 12)), torch.rand((12, 12, 3)), torch.rand((2, 3)), 0.5, 0.5)
    status = torch.tensor([_lib.STATUS_OUT_OF_LAST_PLANE, 0, 0, 0], dtype=torch.int32)
    params = _lib.GmpiRenderParams()
    params.N = 2
    with pytest.raises(_lib.GmpiError, match="gmpi_last_plane_uv_minmax_launch needs tensors on a ROCm device"):
        MPI(on_out_of_plane="raise").raise_on_status(status, params=params, keep=None)
    assert lib.launched == []


# ---- forward, shared colour ----------------------------------------------------------------------------------------------------------------

def shared_inputs(dtype=torch.float32, background=True, device="cpu"):
    vol, dhw, ray, eye, zd = make_inputs(2, dtype, device)
    g = torch.Generator().manual_seed(1)
    alpha = torch.rand((M, D, 1, Ht, Wt), generator=g).to(dtype).to(device)
    rgb = torch.rand((M, 3, Ht, Wt), generator=g).to(dtype).to(device)
    bg = torch.rand((M, 3, Ht, Wt), generator=g).to(dtype).to(device) if background else None
    return rgb, alpha, bg, (dhw, ray, eye, zd)


def render_shared(mpi, rgb, alpha, bg, geo, **kw):
    with torch.no_grad():
        return mpi.render_views_shared(rgb, alpha, *geo, background=bg, **kw)


def check_shared_color(sc, rgb, bg):
    assert sc.struct_size == 72 and sc.rgb == rgb.data_ptr() and list(sc.rgb_stride) == [144, 48, 8]
    if bg is None:
        assert sc.background is None and list(sc.background_stride) == [0, 0, 0]
    else:
        assert sc.background == bg.data_ptr() and list(sc.background_stride) == [144, 48, 8]


def test_shared_colour_bf16_with_background(rec):
    rgb, alpha, bg, geo = shared_inputs(torch.bfloat16)
    res = render_shared(MPI(), rgb, alpha, bg, geo)
    (c,) = rec.calls
    assert c.name == "gmpi_mpi_render_shared_launch" and c.args[2] == 0
    check_struct(c.args[0], res, (alpha,) + geo, variant=0, rgba_dtype=1, rgba_stride=[144, 48, 48, 8, 1])
    check_shared_color(c.args[1], rgb, bg)


def test_shared_colour_without_background(rec):
    rgb, alpha, bg, geo = shared_inputs(background=False)
    res = render_shared(MPI(variant="lds"), rgb, alpha, bg, geo)   # (every variant but "gather": the library chooses)
    (c,) = rec.calls
    check_struct(c.args[0], res, (alpha,) + geo, variant=0, rgba_stride=[144, 48, 48, 8, 1])
    check_shared_color(c.args[1], rgb, None)


def test_shared_colour_gather_variant(rec):
    rgb, alpha, bg, geo = shared_inputs()
    res = render_shared(MPI(variant="gather"), rgb, alpha, bg, geo)
    check_struct(rec.calls[0].args[0], res, (alpha,) + geo, variant=1, rgba_stride=[144, 48, 48, 8, 1])


def test_shared_colour_mixed_dtypes_raise(rec):
    rgb, alpha, bg, geo = shared_inputs()
    with pytest.raises(TypeError, match="one storage dtype"):
        render_shared(MPI(), rgb.bfloat16(), alpha, bg.bfloat16(), geo)
    assert rec.calls == []


def test_shared_colour_full_range_check_covers_the_three_tensors(rec):
    rgb, alpha, bg, geo = shared_inputs()
    res = render_shared(MPI(range_check="full"), rgb, alpha, bg, geo)
    assert [c.name for c in rec.calls] == ["gmpi_rgba_range_check_launch"] * 3 + ["gmpi_mpi_render_shared_launch"]
    st = res["status"].data_ptr()
    assert [c.args for c in rec.calls[:3]] == [(t.data_ptr(), 0, t.numel(), st, 0) for t in (alpha, rgb, bg)]


# ---- backward: the rebuilt struct is the forward's -------------------------------------------------------------------------------------

VOLUME_BACKWARD = ("gmpi_mpi_render_backward_launch", "gmpi_mpi_render_backward_ex_launch")
GEOMETRY_BACKWARD = ("gmpi_mpi_render_geometry_backward_launch", "gmpi_mpi_render_geometry_backward_ex_launch")
SAME_POINTERS = ("view_to_mpi", "dhw", "ray_dir", "eye_pos", "z_dir", "rgba")
# the image backwards of the two layouts: one entry each for a loss with and without T (the T gradient is an argument, NULL when unused)
LAYOUT_BACKWARD = ("gmpi_mpi_render_shared_backward_launch", "gmpi_mpi_render_depth_backward_launch", "gmpi_mpi_render_depth_backward_tile_launch")


def check_backward_struct(bwd: Call, fwd: Call, uses_T: bool, overwrite: bool = False, user_T=None):
    """`bwd`: a recorded backward call; `fwd`: the forward call of the same node.  overwrite: FLAG_GRAD_OVERWRITE is expected (the
    backward="gather" path of the volume gradient, with a workspace)."""
    b, f = bwd.args[0], fwd.args[0]
    assert bwd.name.endswith("_ex_launch") == uses_T or bwd.name in LAYOUT_BACKWARD, bwd.name
    got, want = scalars_of(b), scalars_of(f)
    assert got.pop("workspace_bytes") == (b.workspace_bytes if b.workspace else 0)
    want.pop("workspace_bytes")
    want["flags"] |= _lib.FLAG_GRAD_OVERWRITE if overwrite else 0
    assert got == want
    for k in SAME_POINTERS:
        assert getattr(b, k) == getattr(f, k), k
    assert b.rgb_out is None and b.depth_out is None and b.status is None
    assert b.transmittance_out is not None and b.transmittance_out == f.transmittance_out
    if user_T is not None:
        assert b.transmittance_out != user_T.data_ptr()


def loss_of(res, uses_T):
    loss = (res["color"] * 0.5).sum() + res["depth"].sum()
    return loss + (res["T"] * 2.0).sum() if uses_T else loss


@pytest.mark.parametrize("uses_T", [False, True])
@pytest.mark.parametrize("mode", ["atomic", "gather"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_volume_backward_rebuilds_the_forward_struct(rec, dtype, mode, uses_T):
    vol, *geo = make_inputs(2, dtype)
    vol.requires_grad_(True)
    user_T = torch.empty((2, 1, H, W))
    res = MPI(backward=mode, variant="lds", strict_order=True).render_views(
        vol, *geo, out_pm1=True, check_last_plane=True, want_transmittance=True, out={"T": user_T})
    # (filled by a copy of the node's private buffer -- which no kernel wrote here: compared as bits)
    assert torch.equal(user_T.view(torch.int32), res["T"].detach().view(torch.int32)) and user_T.data_ptr() != res["T"].data_ptr()
    loss_of(res, uses_T).backward()
    fwd, bwd = rec.calls
    assert fwd.name == "gmpi_mpi_render_launch" and bwd.name in VOLUME_BACKWARD
    assert fwd.args[0].flags == 31 and fwd.args[0].rgba == vol.data_ptr()
    check_backward_struct(bwd, fwd, uses_T, user_T=user_T)   # (a recorder answers no workspace query: no scratch, no overwrite)
    assert bwd.args[0].workspace is None
    assert vol.grad.shape == vol.shape and vol.grad.dtype == dtype
    gptr = [bwd.args[1], bwd.args[2]] + ([bwd.args[3]] if uses_T else [])
    assert all(gptr) and bwd.args[-2] == [576, 192, 48, 8, 1] and bwd.args[-1] == 0


@pytest.mark.parametrize("uses_T", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_geometry_backward_rebuilds_the_forward_struct(rec, dtype, uses_T):
    vol, *geo = make_inputs(3, dtype)
    for t in [vol] + geo:
        t.requires_grad_(True)
    res = MPI(geometry_grad=True).render_views(vol, *geo, views_per_mpi=[1, 2], want_transmittance=True)
    loss_of(res, uses_T).backward()
    assert [c.name for c in rec.calls][0] == "gmpi_mpi_render_launch"
    fwd = rec.calls[0]
    (vb,), (gb,) = rec.named(*VOLUME_BACKWARD), rec.named(*GEOMETRY_BACKWARD)
    assert fwd.v2m == vb.v2m == gb.v2m == [0, 1, 1]
    check_backward_struct(vb, fwd, uses_T)
    check_backward_struct(gb, fwd, uses_T)
    assert gb.args[0].workspace is not None   # (slabs of the per-view and per-plane sums: at least one byte is lent)
    for t in geo:
        assert t.grad is not None and t.grad.shape == t.shape


@pytest.mark.parametrize("uses_T", [False, True])
@pytest.mark.parametrize("background", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_shared_backward_rebuilds_the_forward_structs(rec, dtype, background, uses_T):
    rgb, alpha, bg, geo = shared_inputs(dtype, background)
    for t in (rgb, alpha, bg):
        if t is not None:
            t.requires_grad_(True)
    res = MPI().render_views_shared(rgb, alpha, *geo, background=bg, want_transmittance=True)
    loss_of(res, uses_T).backward()
    fwd, bwd = rec.calls
    assert (fwd.name, bwd.name) == ("gmpi_mpi_render_shared_launch", "gmpi_mpi_render_shared_backward_launch")
    check_backward_struct(bwd, fwd, uses_T)
    assert bytes(bwd.args[1]) == bytes(fwd.args[1])   # GmpiSharedColor: the same struct
    check_shared_color(bwd.args[1], rgb, bg)
    assert (bwd.args[4] is not None) == uses_T and bwd.args[-1] == 0
    assert rgb.grad.shape == rgb.shape and alpha.grad.shape == alpha.shape and (bg is None or bg.grad.shape == bg.shape)
