"""Interleaved (channels-last) uint8 RGBA volumes without a GPU: `[M, D, Ht, Wt, 4]` layers seen as `[M, D, 4, Ht, Wt]` -- channel stride 1, texel
stride 4 -- reach the C ABI in place, as GMPI_DTYPE_U8 with those strides; what does not fit the layout is still made contiguous; the helpers of
quantized.py; what the C ABI accepts and refuses for the layout before a launch; the resources of the new kernel instances."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from ml_gmpi_amd import _lib
from ml_gmpi_amd.hip_mpi import MPI
from test_marshal_cpu import BACKWARD_ENTRIES, FORWARD_ENTRIES, Recorder, check_struct, make_inputs, render
from test_u8_storage_cpu import HIPCC, ROOT, _library, _params

M, D, Ht, Wt = 2, 3, 6, 8          # make_inputs' volume
E_STRIDE, E_DTYPE, E_VARIANT = -4, -3, -6


@pytest.fixture
def rec(monkeypatch):
    r = Recorder(FORWARD_ENTRIES + BACKWARD_ENTRIES)
    monkeypatch.setattr(_lib, "load_library", lambda: r)
    return r


def layers(shape, seed=0):
    return torch.randint(0, 256, tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


# ---- 1. marshalling: the layout reaches the struct in place --------------------------------------------------------------------------------

def test_error_codes_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "gmpi_render.h")).read()
    for name, value in (("GMPI_E_STRIDE", E_STRIDE), ("GMPI_E_DTYPE", E_DTYPE), ("GMPI_E_VARIANT", E_VARIANT)):
        assert re.search(rf"{name} = (-\d+)", hdr).group(1) == str(value), name


def test_permuted_layers_reach_the_struct_in_place(rec):
    rest = make_inputs(2)[1:]
    lay = layers((M, D, Ht, Wt, 4))
    vol = lay.permute(0, 1, 4, 2, 3)
    res = render(MPI(), (vol,) + rest)
    (c,) = rec.calls                                                                # that one launch: no copy kernel, no range pass
    assert c.name == "gmpi_mpi_render_launch"
    check_struct(c.args[0], res, (vol,) + rest, rgba_dtype=3, rgba_stride=[D * Ht * Wt * 4, Ht * Wt * 4, 1, 4 * Wt, 4])
    assert c.args[0].rgba == lay.data_ptr()


def test_padded_rows_slices_and_an_expanded_batch_stay_in_place(rec):
    rest = make_inputs(2)[1:]
    wide = layers((M, D, Ht, 2 * Wt, 4), seed=1)
    view = wide[:, :, :, 3:3 + Wt].permute(0, 1, 4, 2, 3)                           # rows padded, first texel 3: the pointer moves by 12 bytes
    render(MPI(), (view,) + rest)
    (c,) = rec.calls
    p = c.args[0]
    assert p.rgba == wide.data_ptr() + 12 and p.rgba_dtype == 3
    assert list(p.rgba_stride) == [D * Ht * 2 * Wt * 4, Ht * 2 * Wt * 4, 1, 8 * Wt, 4]
    rec.calls.clear()
    one = layers((1, D, Ht, Wt, 4), seed=2)
    render(MPI(), (one.permute(0, 1, 4, 2, 3).expand(M, -1, -1, -1, -1),) + rest)   # a batch stride of 0
    (c,) = rec.calls
    p = c.args[0]
    assert p.rgba == one.data_ptr() and list(p.rgba_stride) == [0, Ht * Wt * 4, 1, 4 * Wt, 4]
    rec.calls.clear()
    deep = layers((M, 2 * D, Ht, Wt, 4), seed=3)
    render(MPI(range_check="full"), (deep[:, ::2].permute(0, 1, 4, 2, 3),) + rest)  # every other plane; "full" has nothing to pass over
    assert [c.name for c in rec.calls] == ["gmpi_mpi_render_launch"]
    p = rec.calls[0].args[0]
    assert p.rgba == deep.data_ptr() and list(p.rgba_stride) == [2 * D * Ht * Wt * 4, 2 * Ht * Wt * 4, 1, 4 * Wt, 4]


def test_forward_and_renderer_entry_points_pass_the_layout_on(rec):
    vol, dhw, ray, eye, zd = make_inputs(2)
    lay = layers((M, D, Ht, Wt, 4), seed=4)
    q = lay.permute(0, 1, 4, 2, 3)
    with torch.no_grad():
        MPI().forward(batch_rgba=q, batch_dhw=dhw, batch_ray_dir=[ray[:1], ray[1:]], batch_eye_pos=[eye[:1], eye[1:]], batch_z_dir=[zd[:1], zd[1:]],
                      separate_background=None)
    (c,) = rec.calls
    assert c.args[0].rgba == lay.data_ptr() and list(c.args[0].rgba_stride) == [D * Ht * Wt * 4, Ht * Wt * 4, 1, 4 * Wt, 4]


# ---- 2. what is not the layout keeps today's path ----------------------------------------------------------------------------------------------

def test_other_strided_views_are_still_made_contiguous(rec):
    rest = make_inputs(2)[1:]
    planar = [D * 4 * Ht * Wt, 4 * Ht * Wt, Ht * Wt, Wt, 1]
    f = torch.rand((M, D, Ht, Wt, 4)).permute(0, 1, 4, 2, 3)                        # float channels-last
    five = layers((M, D, Ht, Wt, 5), seed=5)[..., :4].permute(0, 1, 4, 2, 3)        # texel stride 5
    assert five.stride(4) == 5 and five.stride(2) == 1
    for vol, dtype in ((f, 0), (five, 3)):                                          # (a negative stride: the predicate test below -- torch builds none)
        rec.calls.clear()
        render(MPI(), (vol,) + rest)
        (c,) = rec.calls
        p = c.args[0]
        assert p.rgba_dtype == dtype and list(p.rgba_stride) == planar and p.rgba != vol.data_ptr()


def test_the_predicate_refuses_negative_strides_and_other_texel_strides():
    """torch builds no tensor with a negative stride, so the predicate is asked directly (a stand-in with the tensor attributes it reads)."""
    from ml_gmpi_amd.quantized import is_interleaved

    class Fake:
        dtype, ndim = torch.uint8, 5

        def __init__(self, shape, strides):
            self.shape, self._s = shape, strides

        def stride(self, i=None):
            return self._s if i is None else self._s[i]

    shape = (M, D, 4, Ht, Wt)
    assert is_interleaved(Fake(shape, (D * Ht * Wt * 4, Ht * Wt * 4, 1, 4 * Wt, 4)))
    assert is_interleaved(layers((M, D, Ht, Wt, 4)).permute(0, 1, 4, 2, 3))
    assert not is_interleaved(Fake(shape, (D * Ht * Wt * 4, -Ht * Wt * 4, 1, 4 * Wt, 4)))     # a negative plane stride
    assert not is_interleaved(Fake(shape, (D * Ht * Wt * 4, Ht * Wt * 4, 1, -4 * Wt, 4)))
    assert not is_interleaved(Fake(shape, (D * Ht * Wt * 4, Ht * Wt * 4, 1, 4 * Wt - 4, 4)))  # rows that overlap
    assert not is_interleaved(Fake(shape, (D * Ht * Wt * 5, Ht * Wt * 5, 1, 5 * Wt, 5)))
    assert not is_interleaved(Fake(shape, (D * Ht * Wt * 8, Ht * Wt * 8, 2, 8 * Wt, 4)))      # channel stride 2
    assert not is_interleaved(layers((M, D, 4, Ht, Wt)))                                      # planar
    assert not is_interleaved(torch.rand((M, D, Ht, Wt, 4)).permute(0, 1, 4, 2, 3))           # float


# ---- 3. helpers ------------------------------------------------------------------------------------------------------------------------------

def test_layer_helpers_share_storage_and_round_trip():
    import ml_gmpi_amd
    from ml_gmpi_amd import layers_as_volume, volume_as_layers
    assert "layers_as_volume" in ml_gmpi_amd.__all__ and "volume_as_layers" in ml_gmpi_amd.__all__
    lay = layers((M, D, Ht, Wt, 4), seed=7)
    q = layers_as_volume(lay)
    assert tuple(q.shape) == (M, D, 4, Ht, Wt) and q.stride() == (D * Ht * Wt * 4, Ht * Wt * 4, 1, 4 * Wt, 4)
    assert q.data_ptr() == lay.data_ptr() and torch.equal(q, lay.permute(0, 1, 4, 2, 3))
    back = volume_as_layers(q)
    assert back.data_ptr() == lay.data_ptr() and back.stride() == lay.stride() and torch.equal(back, lay)
    lay[1, 2, 3, 4, 1] ^= 0xFF                                                       # one storage: a write through the layers shows in the volume
    assert q[1, 2, 1, 3, 4] == lay[1, 2, 3, 4, 1]
    sub = lay[:, 1:, 2:, 1:5]                                                        # slices along D, rows and columns stay layers
    assert volume_as_layers(layers_as_volume(sub)).data_ptr() == sub.data_ptr()
    with pytest.raises(TypeError):
        layers_as_volume(lay.float())
    with pytest.raises(ValueError):
        layers_as_volume(lay[..., :3])
    with pytest.raises(ValueError):
        layers_as_volume(lay[0])
    with pytest.raises(ValueError):
        layers_as_volume(layers((M, D, Ht, Wt, 5))[..., :4])                         # texel stride 5
    with pytest.raises(ValueError):
        volume_as_layers(layers((M, D, 4, Ht, Wt)))                                  # planar
    with pytest.raises(TypeError):
        volume_as_layers(q.float())
    with pytest.raises(ValueError):
        volume_as_layers(q[:, :, :3])


def test_quantize_interleaved_has_the_same_codes_in_the_other_order():
    from ml_gmpi_amd import dequantize_volume, quantize_volume, volume_as_layers
    x = torch.rand((M, D, 4, Ht, Wt), generator=torch.Generator().manual_seed(8))
    planar, inter = quantize_volume(x), quantize_volume(x, interleaved=True)
    assert planar.is_contiguous() and torch.equal(quantize_volume(x, interleaved=False), planar)
    assert inter.dtype is torch.uint8 and tuple(inter.shape) == tuple(planar.shape) and torch.equal(inter, planar)
    assert inter.stride() == (D * Ht * Wt * 4, Ht * Wt * 4, 1, 4 * Wt, 4) and volume_as_layers(inter).is_contiguous()
    assert torch.equal(dequantize_volume(inter), dequantize_volume(planar))
    assert dequantize_volume(inter, torch.bfloat16).dtype is torch.bfloat16
    with pytest.raises(ValueError):
        quantize_volume(torch.rand((D, 4, Ht, Wt)), interleaved=True)
    with pytest.raises(ValueError):
        quantize_volume(x + 1, interleaved=True)


# ---- 4. the C ABI: what is accepted and refused before a launch ----------------------------------------------------------------------------------

def _interleaved_params(variant=0, dtype=3):
    """test_u8_storage_cpu._params (1 x 2 x 4 x 8 x 8 over host buffers, 4 x 4 pixels) with the interleaved strides."""
    p, bufs = _params(dtype=dtype, variant=variant)
    p.rgba_stride[:] = [p.D * p.Ht * p.Wt * 4, p.Ht * p.Wt * 4, 1, 4 * p.Wt, 4]
    return p, bufs


def test_query_reports_the_layout():
    lib = _library()
    assert lib.gmpi_query(20) == 1
    assert lib.gmpi_query(19) == -1 and lib.gmpi_query(21) == -1 and lib.gmpi_query(15) == -1


def test_the_abi_validates_the_layout_before_a_launch():
    lib = _library()
    ref = ctypes.byref
    # accepted: the workspace query validates the struct and wants nothing
    for variant in (0, 1, 2):
        p, b = _interleaved_params(variant)
        assert lib.gmpi_render_workspace_bytes(ref(p)) == 0
    # variants the type does not have
    for variant in (3, 5, 4, 9):
        p, b = _interleaved_params(variant)
        assert lib.gmpi_mpi_render_launch(ref(p), None) == E_VARIANT
    # the staged kernel by name, over tensors its 16-byte items cannot take
    p, b = _interleaved_params(2)
    p.Wt, p.rgba_stride[3] = 6, 24
    assert lib.gmpi_mpi_render_launch(ref(p), None) == E_VARIANT
    p, b = _interleaved_params(2)
    p.rgba += 1
    assert lib.gmpi_mpi_render_launch(ref(p), None) == E_VARIANT
    p, b = _interleaved_params(2)
    p.rgba_stride[1] = 4 * p.Ht * p.Wt + 2
    assert lib.gmpi_mpi_render_launch(ref(p), None) == E_VARIANT
    # stride combinations that are not the layout: refused by every variant, AUTO and GATHER included
    for variant in (0, 1, 2):
        p, b = _interleaved_params(variant, dtype=0)                                # fp32 with a texel stride of 4
        assert lib.gmpi_mpi_render_launch(ref(p), None) == E_STRIDE
        p, b = _interleaved_params(variant, dtype=1)
        assert lib.gmpi_mpi_render_launch(ref(p), None) == E_STRIDE
        p, b = _interleaved_params(variant)
        p.rgba_stride[2] = 2                                                        # channel stride 2
        assert lib.gmpi_mpi_render_launch(ref(p), None) == E_STRIDE
        p, b = _interleaved_params(variant)
        p.rgba_stride[3] = 4 * p.Wt - 4                                             # rows that overlap
        assert lib.gmpi_mpi_render_launch(ref(p), None) == E_STRIDE
        for texel in (2, 8, 5, 3):
            p, b = _interleaved_params(variant)
            p.rgba_stride[4] = texel
            assert lib.gmpi_mpi_render_launch(ref(p), None) == E_STRIDE
        p, b = _interleaved_params(variant)
        p.rgba_stride[1] = -p.rgba_stride[1]
        assert lib.gmpi_mpi_render_launch(ref(p), None) == E_STRIDE
    p, b = _interleaved_params(dtype=4)
    assert lib.gmpi_mpi_render_launch(ref(p), None) == E_DTYPE


def test_every_other_entry_still_refuses_the_type():
    lib = _library()
    p, b = _interleaved_params()
    ref = ctypes.byref
    host = lambda a: a.ctypes.data
    stride5 = (ctypes.c_int64 * 5)(*[b["g"].strides[i] // 4 for i in range(5)])
    g = host(b["g"])
    assert lib.gmpi_mpi_render_backward_launch(ref(p), host(b["rgb"]), host(b["dep"]), g, stride5, None) == E_DTYPE
    assert lib.gmpi_mpi_render_backward_ex_launch(ref(p), host(b["rgb"]), host(b["dep"]), host(b["dep"]), g, stride5, None) == E_DTYPE
    assert lib.gmpi_mpi_render_geometry_backward_launch(ref(p), host(b["rgb"]), host(b["dep"]), host(b["ray"]), None, None, None, None) == E_DTYPE
    assert lib.gmpi_mpi_render_geometry_backward_ex_launch(ref(p), host(b["rgb"]), host(b["dep"]), host(b["dep"]), host(b["ray"]), None, None, None, None) == E_DTYPE
    assert lib.gmpi_render_backward_workspace_bytes(ref(p)) == 0 and lib.gmpi_render_geometry_backward_workspace_bytes(ref(p), 1) == 0
    sc = _lib.GmpiSharedColor()
    sc.struct_size = ctypes.sizeof(_lib.GmpiSharedColor)
    sc.rgb = host(b["rgba"])
    sc.rgb_stride[:] = [3 * 64, 64, 8]
    for variant in (0, 1, 2):
        p.variant = variant
        assert lib.gmpi_mpi_render_shared_launch(ref(p), ref(sc), None) == E_DTYPE
        assert lib.gmpi_render_shared_supports(ref(p), ref(sc)) == E_DTYPE
    p.variant = 0
    s3 = (ctypes.c_int64 * 3)(3 * 64, 64, 8)
    assert lib.gmpi_mpi_render_shared_backward_launch(ref(p), ref(sc), host(b["rgb"]), None, None, g, s3, None, None, None, None, None) == E_DTYPE
    p.rgba_dtype = 0                                                                # ... and the layout under a float type is a stride error there as well
    assert lib.gmpi_mpi_render_backward_launch(ref(p), host(b["rgb"]), host(b["dep"]), g, stride5, None) == E_STRIDE
    assert lib.gmpi_mpi_render_shared_launch(ref(p), ref(sc), None) == E_STRIDE


# ---- 5. resources of the new instances -----------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("unit,kernel,lds_cap", [("render_u8", "render_rgba8_kernel", 40 * 1024), ("render_gather", "render_gather_kernel", 0)])
def test_interleaved_instances_compile_for_gfx950_without_scratch(tmp_path, unit, kernel, lds_cap):
    """The compiler's own report (the .amdhsa_* directives of -save-temps): zero scratch in the four staged and the four gather instances over
    rgba8_t, the staged ones within four workgroups per CU, their loader without a byte permute and with one 16-byte buffer load per plane."""
    csrc = os.path.join(ROOT, "ml-gmpi_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
             "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]   # = ml-gmpi_amd/csrc/Makefile
    mk = open(os.path.join(csrc, "Makefile")).read()
    for f in ("-ffp-contract=off", "-fno-slp-vectorize", "-O3", unit + ".hip"):
        assert f in mk, f"the Makefile no longer has {f}: keep this test in step with it"
    res = subprocess.run([HIPCC, *flags, "-save-temps", "-c", os.path.join(csrc, unit + ".hip"), "-o", unit + ".o"], cwd=tmp_path, capture_output=True, timeout=900)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    asm = open(os.path.join(tmp_path, unit + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    names = sorted(n for n in set(re.findall(rf"^(_Z\w*{kernel}\w*):", asm, flags=re.M)) if kernel == "render_rgba8_kernel" or "7rgba8_t" in n)
    assert len(names) == 4, names                                                    # align_corners x order
    for name in names:
        meta = asm[asm.index(".amdhsa_kernel " + name):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", meta).group(1)) <= lds_cap, name
        body = asm[asm.index("\n" + name + ":"):]
        body = body[:body.index("s_endpgm")]
        if kernel == "render_rgba8_kernel":
            assert "v_perm_b32" not in body, name                                    # the memory image is the LDS image
            assert "buffer_load_dwordx4" in body and "ds_write_b128" in body, name
        else:
            assert "global_load_ubyte" not in body and "global_load_dword" in body, name   # one texel load per tap, none by the byte
            assert "v_cvt_f32_ubyte3" in body, name
