"""The shaded render of an RGBA volume without a GPU: what `MPI.render_views_shaded` hands the C ABI (a recorder stands in for the library, as in
tests/test_marshal_cpu.py), the error codes of the three C entries on pointers that are never followed (as in tests/test_chunks_cpu.py), and
`apply_shading`, the executable definition, against the LightRenderer fixture the reference made.

Not here: that `LightRenderer.shading_image` advances `step`, `cur_ka`, `cur_kd` and the torch RNG exactly as `render` does.  Neither method has a CPU
path (both refuse tensors that are not on the device before they advance anything), so that comparison -- both run from one seed, the state compared
afterwards -- is tests/test_hip_shaded_render.py::test_shading_image_then_render_views_shaded_equals_light_render_then_render_views."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from _util import load_npz
from ml_gmpi_amd import _lib, apply_shading
from ml_gmpi_amd.hip_mpi import MPI
from test_marshal_cpu import BACKWARD_ENTRIES, FORWARD_ENTRIES, Recorder, check_struct, make_inputs, M, D, Ht, Wt

SHADED_ENTRIES = ("gmpi_mpi_render_shaded_launch", "gmpi_render_shaded_supports", "gmpi_mpi_render_shaded_backward_launch")


@pytest.fixture
def rec(monkeypatch):
    r = Recorder(FORWARD_ENTRIES + BACKWARD_ENTRIES + SHADED_ENTRIES)
    monkeypatch.setattr(_lib, "load_library", lambda: r)
    return r


def shading(seed=1):
    return 0.4 + 1.2 * torch.rand((M, 1, Ht, Wt), generator=torch.Generator().manual_seed(seed))


# ---- marshalling ---------------------------------------------------------------------------------------------------------------------------------
def test_forward_structs_name_the_callers_tensors(rec):
    inputs, s = make_inputs(2), shading()
    with torch.no_grad():
        res = MPI().render_views_shaded(inputs[0], s, *inputs[1:], want_transmittance=True)
    (c,) = rec.calls
    assert c.name == "gmpi_mpi_render_shaded_launch" and c.args[2] == 0
    check_struct(c.args[0], res, inputs, T=res["T"])                     # AUTO: a host tensor is never asked about the staged kernel
    sh = c.args[1]
    assert isinstance(sh, _lib.GmpiShading) and sh.struct_size == ctypes.sizeof(_lib.GmpiShading) == 32
    assert sh.shading == s.data_ptr() and list(sh.shading_stride) == [Ht * Wt, Wt]
    rec.calls.clear()
    with torch.no_grad():
        MPI(variant="gather").render_views_shaded(inputs[0], s, *inputs[1:])
    assert rec.calls[0].args[0].variant == _lib.VARIANT_GATHER


def test_padded_expanded_and_non_contiguous_shadings(rec):
    inputs = make_inputs(2)
    buf = torch.rand((M, 1, Ht, Wt + 5)) + 0.5
    padded = buf[..., :Wt]
    with torch.no_grad():
        MPI().render_views_shaded(inputs[0], padded, *inputs[1:])
    sh = rec.calls[-1].args[1]
    assert sh.shading == padded.data_ptr() and list(sh.shading_stride) == [Ht * (Wt + 5), Wt + 5]      # read as it is: no copy
    # an expanded image over TWO MPIs has an MPI stride of 0, which the entry takes for one MPI only: copied
    one = torch.rand((1, 1, Ht, Wt)) + 0.5
    with torch.no_grad():
        MPI().render_views_shaded(inputs[0], one.expand(M, -1, -1, -1), *inputs[1:])
    sh = rec.calls[-1].args[1]
    assert sh.shading != one.data_ptr() and list(sh.shading_stride) == [Ht * Wt, Wt]
    # ... and is read as it is for one MPI
    vol1, dhw1 = inputs[0][:1], inputs[1][:1]
    e = torch.as_strided(one, (1, 1, Ht, Wt), (0, 0, Wt, 1))   # (what `expand` of one image over a batch leaves)
    with torch.no_grad():
        MPI().render_views_shaded(vol1, e, dhw1, *inputs[2:], views_per_mpi=2)
    sh = rec.calls[-1].args[1]
    assert sh.shading == one.data_ptr() and list(sh.shading_stride) == [0, Wt]
    # innermost stride 2, and a float64 image: contiguous fp32 copies
    wide = torch.rand((M, 1, Ht, 2 * Wt)) + 0.5
    for s in (wide[..., ::2], shading().double()):
        with torch.no_grad():
            MPI().render_views_shaded(inputs[0], s, *inputs[1:])
        sh = rec.calls[-1].args[1]
        assert sh.shading != s.data_ptr() and list(sh.shading_stride) == [Ht * Wt, Wt]


@pytest.mark.parametrize("needs", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("uses_T", [False, True])
def test_backward_is_one_launch_on_the_forwards_struct_with_null_for_what_is_not_needed(rec, needs, uses_T):
    inputs, s = make_inputs(2), shading()
    vol = inputs[0].clone().requires_grad_(needs[0])
    s = s.requires_grad_(needs[1])
    out = MPI().render_views_shaded(vol, s, *inputs[1:], want_transmittance=True)
    fwd = rec.named("gmpi_mpi_render_shaded_launch")[0]
    loss = out["color"].sum() + (out["T"].sum() if uses_T else 0)
    loss.backward()
    (b,) = rec.named("gmpi_mpi_render_shaded_backward_launch")
    assert not rec.named(*BACKWARD_ENTRIES)
    p, sh, g_rgb, g_depth, g_T, g_rgba, g_stride, g_sh, g_sh_stride, stream = b.args
    f = fwd.args[0]
    for k in ("flags", "variant", "rgba_dtype", "N", "M", "D", "Ht", "Wt", "H", "W", "views_per_mpi", "rgba", "dhw", "ray_dir", "eye_pos", "z_dir"):
        assert getattr(p, k) == getattr(f, k), k
    assert list(p.rgba_stride) == list(f.rgba_stride) and p.transmittance_out == f.transmittance_out and not p.rgb_out and not p.workspace
    assert sh.shading == fwd.args[1].shading and list(sh.shading_stride) == list(fwd.args[1].shading_stride)
    assert g_rgb and g_depth is None and (g_T is not None) == uses_T
    # what needs no gradient gets no buffer: NULL pointer, NULL strides
    assert (g_rgba is not None) == needs[0] and (g_stride == [D * 4 * Ht * Wt, 4 * Ht * Wt, Ht * Wt, Wt, 1] if needs[0] else g_stride is None)
    assert (g_sh is not None) == needs[1] and (g_sh_stride == [Ht * Wt, Wt] if needs[1] else g_sh_stride is None)
    assert (vol.grad is not None) == needs[0] and (s.grad is not None) == needs[1]
    if needs[0]:
        assert vol.grad.data_ptr() == g_rgba                                      # fp32 input: the buffer IS rgba.grad


def test_refusals(rec):
    inputs, s = make_inputs(2), shading()
    with pytest.raises(TypeError):
        MPI().render_views_shaded((inputs[0] * 255).to(torch.uint8), s, *inputs[1:])
    for bad in (s[:, 0], s[:1], torch.rand((M, 3, Ht, Wt)), torch.rand((M, 1, Ht, Wt + 1))):
        with pytest.raises(ValueError):
            MPI().render_views_shaded(inputs[0], bad, *inputs[1:])
    for i in (1, 2, 3, 4):   # dhw, ray_dir, eye_pos, z_dir
        geo = list(inputs)
        geo[i] = geo[i].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError):
            MPI(geometry_grad=True).render_views_shaded(geo[0], s, *geo[1:])
    assert not rec.calls


def test_full_range_check_sees_only_the_alpha_channel(rec):
    inputs, s = make_inputs(2), shading()
    with torch.no_grad():
        MPI(range_check="full").render_views_shaded(inputs[0], s, *inputs[1:])
    names = [c.name for c in rec.calls]
    assert names == ["gmpi_rgba_range_check_launch", "gmpi_mpi_render_shaded_launch"]
    ptr, dtype, count = rec.calls[0].args[:3]
    assert count == M * D * Ht * Wt and dtype == 0                               # a quarter of the volume: the alpha planes
    assert ptr != inputs[0].data_ptr()                                           # (a contiguous copy of the strided alpha view)


# ---- error codes of the C entries ------------------------------------------------------------------------------------------------------------------
def test_c_entry_error_codes():
    """Every call is refused (or has no views) before anything is launched: no device is needed, the pointers are never followed."""
    lib = _lib.load_library()
    assert lib.gmpi_query(38) == 1 and lib.gmpi_query(37) == -1
    host = np.zeros(4096, dtype=np.float32)
    fake = (host.ctypes.data + 63) & ~63   # (a non-NULL address, aligned as a device allocation is)

    def params(N=1, variant=_lib.VARIANT_GATHER, dtype=_lib.DTYPE_F32, outputs=True):
        p = _lib.GmpiRenderParams()
        p.struct_size = ctypes.sizeof(_lib.GmpiRenderParams)
        p.flags, p.variant, p.rgba_dtype = _lib.FLAG_ALIGN_CORNERS, variant, dtype
        p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = N, 1, 3, 4, 4, 4, 4, 1
        p.rgba = fake
        p.rgba_stride[:] = [192, 64, 16, 4, 1]
        p.dhw = p.ray_dir = p.eye_pos = p.z_dir = fake
        if outputs:
            p.rgb_out = p.depth_out = fake
        return p

    def shade(size=None, ptr=fake, strides=(16, 4)):
        sh = _lib.GmpiShading()
        sh.struct_size = ctypes.sizeof(_lib.GmpiShading) if size is None else size
        sh.shading = ptr
        sh.shading_stride[:] = strides
        return sh

    by = lambda x: None if x is None else ctypes.byref(x)
    s5, s2 = (ctypes.c_int64 * 5)(192, 64, 16, 4, 1), (ctypes.c_int64 * 2)(16, 4)
    fwd = lambda p, sh: lib.gmpi_mpi_render_shaded_launch(by(p), by(sh), None)
    sup = lambda p, sh: lib.gmpi_render_shaded_supports(by(p), by(sh))
    bwd = lambda p, sh, g=fake, out=fake, st=s5, gs=fake, gst=s2: lib.gmpi_mpi_render_shaded_backward_launch(by(p), by(sh), g, None, None, out, st, gs, gst, None)
    for entry in (fwd, sup, bwd):
        assert entry(None, shade()) == -1 and entry(params(), None) == -1                      # GMPI_E_NULL
        assert entry(params(), shade(ptr=None)) == -1
        assert entry(params(), shade(size=16)) == -5                                            # GMPI_E_ABI
        p = params(); p.struct_size -= 8
        assert entry(p, shade()) == -5
        assert entry(params(dtype=_lib.DTYPE_U8), shade()) == -3                                # GMPI_E_DTYPE
        assert entry(params(), shade(strides=(16, -4))) == -4 and entry(params(), shade(strides=(16, 3))) == -4   # GMPI_E_STRIDE
        assert entry(params(), shade(strides=(-16, 4))) == -4
        p = params(); p.M = 2
        assert entry(p, shade(strides=(0, 4))) == -4                                            # an MPI stride of 0 only for M = 1
        p = params(); p.flags |= 1 << 30
        assert entry(p, shade()) == -7
    assert fwd(params(N=0), shade()) == 0 and bwd(params(N=0), shade()) == 0 and sup(params(N=0), shade()) == 0   # no views: GMPI_OK at once
    for v in (_lib.VARIANT_WAVE, _lib.VARIANT_BAND, _lib.VARIANT_DMA, 9):
        assert fwd(params(variant=v), shade()) == -6, v                                         # GMPI_E_VARIANT
    assert fwd(params(outputs=False), shade()) == -1
    assert fwd(params(N=65536), shade()) == -2
    # the staged kernel's loader wants 16-byte aligned bases: an explicit LDS launch over a misaligned one is refused, and the query says 0
    odd = shade(ptr=fake + 4)
    assert sup(params(variant=_lib.VARIANT_LDS), odd) == 0 and fwd(params(variant=_lib.VARIANT_LDS), odd) == -6
    assert sup(params(variant=_lib.VARIANT_LDS), shade()) == 1
    # backward
    # either gradient may be NULL when the other is not (never launched here: such a call would run); both NULL, or one without its strides: GMPI_E_NULL
    assert bwd(params(), shade(), g=None) == -1 and bwd(params(), shade(), out=None, gs=None) == -1 and bwd(params(), shade(), st=None) == -1
    assert bwd(params(), shade(), gst=None) == -1 and bwd(params(), shade(), out=None, st=None, gst=None) == -1
    assert bwd(params(), shade(), out=None, st=None, gst=(ctypes.c_int64 * 2)(16, 3)) == -4   # the shading-only form checks its strides too
    assert bwd(params(N=65536), shade()) == -2
    assert bwd(params(), shade(), st=(ctypes.c_int64 * 5)(192, 64, 16, 4, 2)) == -4 and bwd(params(), shade(), st=(ctypes.c_int64 * 5)(192, 64, 16, 3, 1)) == -4
    assert bwd(params(), shade(), gst=(ctypes.c_int64 * 2)(16, 3)) == -4


def test_header_declares_the_entries():
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gmpi_render.h")).read()
    for name in SHADED_ENTRIES + ("typedef struct GmpiShading",):
        assert name in src, name
    assert set(SHADED_ENTRIES) <= set(_lib.EXPORTS)


# ---- apply_shading -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kd", "ambient"])
def test_apply_shading_is_the_references_light_apply_on_the_golden_fixture(name):
    """The fixture holds the reference's shaded volume; its shading image is the numpy oracle's (which tests/test_light_render.py pins to the same
    fixture within 5e-6).  apply_shading of the two must be the fixture's volume within 1e-5, alpha bit for bit."""
    fx = load_npz("light_render.npz")
    ka, kd = fx[f"ka_kd_{name}"]
    out, s = oracle.light_shade(fx["rgba"], fx["dhw"][:, 0], fx["xyz"][-1], fx[f"light_dir_{name}"], ka, kd)
    s = torch.from_numpy(np.asarray(s, dtype=np.float32)).reshape(2, 1, 32, 32)
    vol = torch.from_numpy(fx["rgba"])
    got = apply_shading(vol, s)
    assert got.dtype == torch.float32 and got.shape == vol.shape
    assert float((got - torch.from_numpy(fx[f"ref_{name}"])).abs().max()) <= 1e-5
    assert torch.equal(got, torch.from_numpy(out))                               # the oracle's own apply step: the same fp32 product and clip
    assert torch.equal(got[:, :, 3], vol[:, :, 3])
    for dtype in (torch.bfloat16, torch.float16):                                # 16-bit storage: the product is formed in fp32
        v = vol.to(dtype)
        assert torch.equal(apply_shading(v, s), apply_shading(v.float(), s))
    with pytest.raises(ValueError):
        apply_shading(vol, s[:, 0])
    # differentiable w.r.t. both
    v, sg = vol.clone().requires_grad_(True), s.clone().requires_grad_(True)
    apply_shading(v, sg).sum().backward()
    assert v.grad is not None and sg.grad is not None and float(v.grad[:, :, 3].min()) == 1.0
