"""Channels-last FLOAT layers without a GPU: `[M, D, Ht, Wt, 4]` fp32 / bf16 / fp16 reach gmpi_mpi_render_layers_launch in place, with the strides
[s_M, s_D, 1, s_row, 4]; what is not the layout is made contiguous as layers, counted and warned of; uint8 layers keep their own path; the permuted
float VIEW handed to `render_views` is still copied; what the C ABI accepts and refuses for the layout before a launch; the predicate; the resources of
the new kernel instances."""
import ctypes
import os
import re
import subprocess
import warnings

import pytest
import torch

from ml_gmpi_amd import _lib
from ml_gmpi_amd.hip_mpi import MPI
from test_marshal_cpu import BACKWARD_ENTRIES, FORWARD_ENTRIES, Recorder, check_struct, make_inputs, render
from test_u8_storage_cpu import HIPCC, ROOT, _library, _params

M, D, Ht, Wt = 2, 3, 6, 8          # make_inputs' volume
E_STRIDE, E_DTYPE, E_VARIANT = -4, -3, -6
LAYERS = "gmpi_mpi_render_layers_launch"
RANGE = "gmpi_rgba_range_check_launch"
DTYPES = [(torch.float32, 0), (torch.bfloat16, 1), (torch.float16, 2)]


@pytest.fixture
def rec(monkeypatch):
    r = Recorder(FORWARD_ENTRIES + BACKWARD_ENTRIES + (LAYERS,))
    monkeypatch.setattr(_lib, "load_library", lambda: r)
    return r


def layers(shape, dtype=torch.float32, seed=0):
    return torch.rand(tuple(shape), generator=torch.Generator().manual_seed(seed)).to(dtype)


def render_layers(mpi, lay, rest, **kw):
    with torch.no_grad():
        return mpi.render_views_layers(lay, *rest, **kw)


# ---- 1. marshalling: the layers reach the struct in place --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,code", DTYPES)
def test_layers_reach_the_new_entry_in_place(rec, dtype, code):
    rest = make_inputs(2)[1:]
    lay = layers((M, D, Ht, Wt, 4), dtype)
    res = render_layers(MPI(), lay, rest)
    (c,) = rec.calls                                                                # that one launch: no copy kernel, no range pass
    assert c.name == LAYERS
    check_struct(c.args[0], res, (lay,) + rest, rgba_dtype=code, rgba_stride=[D * Ht * Wt * 4, Ht * Wt * 4, 1, 4 * Wt, 4])
    assert c.args[0].rgba == lay.data_ptr()


@pytest.mark.parametrize("name,value", [("auto", 0), ("gather", 1), ("lds", 2)])
def test_variant_names(rec, name, value):
    rest = make_inputs(2)[1:]
    lay = layers((M, D, Ht, Wt, 4))
    render_layers(MPI(), lay, rest, variant=name)
    render_layers(MPI(variant=name), lay, rest)
    assert [c.args[0].variant for c in rec.calls] == [value, value]
    for bad in ("wave", "band", "dma", ""):
        with pytest.raises(ValueError):
            render_layers(MPI(), lay, rest, variant=bad)
    with pytest.raises(ValueError):
        render_layers(MPI(variant="band"), lay, rest)                              # the module's own variant, when the layout does not have it
    with pytest.raises(ValueError):
        render_layers(MPI(), lay[0], rest)
    with pytest.raises(ValueError):
        render_layers(MPI(), lay[..., :3], rest)
    with pytest.raises(TypeError):
        render_layers(MPI(), lay, rest, _layout=None)
    assert len(rec.calls) == 2


def test_slices_padded_rows_and_an_expanded_batch_stay_in_place(rec):
    rest = make_inputs(2)[1:]
    wide = layers((M, D, Ht, 2 * Wt, 4), torch.bfloat16, seed=1)
    mpi = MPI()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        render_layers(mpi, wide[:, :, :, 3:3 + Wt], rest)                           # rows padded, first texel 3: the pointer moves by 3 texels of 8 bytes
        (c,) = rec.calls
        p = c.args[0]
        assert c.name == LAYERS and p.rgba == wide.data_ptr() + 24 and p.rgba_dtype == 1
        assert list(p.rgba_stride) == [D * Ht * 2 * Wt * 4, Ht * 2 * Wt * 4, 1, 8 * Wt, 4]
        rec.calls.clear()
        one = layers((1, D, Ht, Wt, 4), seed=2)
        render_layers(mpi, one.expand(M, -1, -1, -1, -1), rest)                     # a batch stride of 0
        (c,) = rec.calls
        assert c.args[0].rgba == one.data_ptr() and list(c.args[0].rgba_stride) == [0, Ht * Wt * 4, 1, 4 * Wt, 4]
        rec.calls.clear()
        deep = layers((M + 1, 2 * D, Ht + 2, Wt, 4), torch.float16, seed=3)
        view = deep[1:, ::2, 2:]                                                    # slices along M and rows, every other plane
        render_layers(mpi, view, rest)
        (c,) = rec.calls
        assert c.args[0].rgba == view.data_ptr() == deep.data_ptr() + 2 * (2 * D * (Ht + 2) * Wt * 4 + 2 * Wt * 4)
        assert list(c.args[0].rgba_stride) == [2 * D * (Ht + 2) * Wt * 4, 2 * (Ht + 2) * Wt * 4, 1, 4 * Wt, 4]
    assert mpi.layers_copies == 0


def test_full_range_check_passes_over_the_layers_own_storage(rec):
    rest = make_inputs(2)[1:]
    lay = layers((M, D, Ht, Wt, 4), seed=4)
    render_layers(MPI(range_check="full"), lay, rest)
    assert [c.name for c in rec.calls] == [RANGE, LAYERS]
    assert rec.calls[0].args[0] == lay.data_ptr() and rec.calls[0].args[2] == lay.numel()    # in place: any order serves a min/max
    rec.calls.clear()
    one = layers((1, D, Ht, Wt, 4), seed=5)
    render_layers(MPI(range_check="full"), one.expand(M, -1, -1, -1, -1), rest)
    assert [c.name for c in rec.calls] == [RANGE, LAYERS]
    assert rec.calls[0].args[0] == one.data_ptr() and rec.calls[0].args[2] == one.numel()    # an expanded batch: once
    rec.calls.clear()
    render_layers(MPI(range_check="off"), lay, rest)
    assert [c.name for c in rec.calls] == [LAYERS] and not (rec.calls[0].args[0].flags & _lib.FLAG_CHECK_RANGE)


def test_other_strides_are_copied_as_layers_counted_and_warned_of_once(rec, monkeypatch):
    from ml_gmpi_amd import hip_mpi
    monkeypatch.setattr(hip_mpi, "_LAYERS_COPY_WARNED", False)
    rest = make_inputs(2)[1:]
    planar = layers((M, D, 4, Ht, Wt), seed=6).permute(0, 1, 3, 4, 2)               # layers by shape, planar in memory: last strides (1, Ht Wt)
    five = layers((M, D, Ht, Wt, 5), seed=7)[..., :4]                               # texel stride 5
    mpi = MPI()
    with pytest.warns(RuntimeWarning, match="layers_copies"):
        render_layers(mpi, planar, rest)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                              # ... once
        render_layers(mpi, five, rest)
    assert mpi.layers_copies == 2 and [c.name for c in rec.calls] == [LAYERS, LAYERS]
    for c, src in zip(rec.calls, (planar, five)):
        p = c.args[0]
        assert list(p.rgba_stride) == [D * Ht * Wt * 4, Ht * Wt * 4, 1, 4 * Wt, 4] and p.rgba != src.data_ptr()


def test_float64_becomes_fp32_and_uint8_takes_the_existing_path(rec):
    rest = make_inputs(2)[1:]
    render_layers(MPI(), layers((M, D, Ht, Wt, 4)).double(), rest)
    (c,) = rec.calls
    assert c.name == LAYERS and c.args[0].rgba_dtype == 0 and list(c.args[0].rgba_stride) == [D * Ht * Wt * 4, Ht * Wt * 4, 1, 4 * Wt, 4]
    rec.calls.clear()
    codes = torch.randint(0, 256, (M, D, Ht, Wt, 4), dtype=torch.uint8)
    render_layers(MPI(), codes, rest)
    (c,) = rec.calls
    assert c.name == "gmpi_mpi_render_launch" and c.args[0].rgba_dtype == 3 and c.args[0].rgba == codes.data_ptr()
    assert list(c.args[0].rgba_stride) == [D * Ht * Wt * 4, Ht * Wt * 4, 1, 4 * Wt, 4]
    with pytest.raises(TypeError):
        render_layers(MPI(), torch.zeros((M, D, Ht, Wt, 4), dtype=torch.int32), rest)


def test_render_views_of_the_permuted_float_view_still_copies(rec):
    """What `render_views` did before the layout had an entry, restated: nothing is routed to the new one."""
    rest = make_inputs(2)[1:]
    lay = layers((M, D, Ht, Wt, 4), seed=8)
    vol = lay.permute(0, 1, 4, 2, 3)
    render(MPI(), (vol,) + rest)
    (c,) = rec.calls
    p = c.args[0]
    assert c.name == "gmpi_mpi_render_launch" and list(p.rgba_stride) == [D * 4 * Ht * Wt, 4 * Ht * Wt, Ht * Wt, Wt, 1] and p.rgba != lay.data_ptr()
    from ml_gmpi_amd import layers_as_volume
    with pytest.raises(TypeError):
        layers_as_volume(lay)


def test_renderer_and_driver_entry_points_pass_the_layout_on(rec):
    from ml_gmpi_amd import ViewBatchDriver, make_renderer
    r = make_renderer("FFHQ", n_planes=D, device=torch.device("cpu"), ray_backend="torch")
    lay = layers((M, D, Ht, Wt, 4), torch.bfloat16, seed=9)
    strides = [D * Ht * Wt * 4, Ht * Wt * 4, 1, 4 * Wt, 4]
    with torch.no_grad():
        torch.manual_seed(0)
        out = r.render_layers(lay, 8, 8, variant="gather")
        torch.manual_seed(0)
        ref = r.render(lay.permute(0, 1, 4, 2, 3), 8, 8)
    assert len(out) == 4 and torch.equal(out[2], ref[2]) and torch.equal(out[3], ref[3])      # the same poses from the same seed
    a, b = rec.calls
    assert a.name == LAYERS and a.args[0].rgba == lay.data_ptr() and list(a.args[0].rgba_stride) == strides and a.args[0].variant == 1
    assert b.name == "gmpi_mpi_render_launch" and b.args[0].rgba != lay.data_ptr()
    assert (a.args[0].N, a.args[0].H, a.args[0].W, a.args[0].flags & ~(32 | 64 | 256)) == (b.args[0].N, b.args[0].H, b.args[0].W, b.args[0].flags & ~(32 | 64 | 256))
    rec.calls.clear()
    drv = ViewBatchDriver(r, batch=2)
    res = drv.render_path_layers(lay[:1], 8, [0.0, 0.1, 0.2], [0.0, 0.0, 0.1])
    assert tuple(res["rgb"].shape) == (3, 3, 8, 8)
    assert [c.name for c in rec.calls] == [LAYERS, LAYERS] and [c.args[0].N for c in rec.calls] == [2, 1]
    assert all(c.args[0].rgba == lay.data_ptr() and list(c.args[0].rgba_stride) == strides for c in rec.calls)
    rec.calls.clear()
    out = drv.render_seeds_layers(lay, 8, defer_status=True)
    assert tuple(out[0].shape) == (M, 3, 8, 8) and [c.name for c in rec.calls] == [LAYERS]
    assert rec.calls[0].args[0].rgba == lay.data_ptr() and list(rec.calls[0].args[0].rgba_stride) == strides


def test_the_node_saves_the_layers_and_the_backward_launches_over_a_planar_copy(rec):
    vol, dhw, ray, eye, zd = make_inputs(2)
    lay = layers((M, D, Ht, Wt, 4), torch.bfloat16, seed=10).requires_grad_(True)
    res = MPI().render_views_layers(lay, dhw, ray, eye, zd)
    (f,) = rec.calls
    assert f.name == LAYERS and f.args[0].rgba == lay.data_ptr()
    saved = [t for t in res["color"].grad_fn.saved_tensors if t.dim() == 5]
    assert len(saved) == 1 and saved[0].data_ptr() == lay.data_ptr() and tuple(saved[0].shape) == (M, D, Ht, Wt, 4)
    res["color"].sum().backward()
    (b,) = rec.named("gmpi_mpi_render_backward_launch")
    assert list(b.args[0].rgba_stride) == [D * 4 * Ht * Wt, 4 * Ht * Wt, Ht * Wt, Wt, 1] and b.args[0].rgba != lay.data_ptr() and b.args[0].rgba_dtype == 1
    assert tuple(lay.grad.shape) == (M, D, Ht, Wt, 4) and lay.grad.dtype is torch.bfloat16 and lay.grad.is_contiguous()
    with pytest.raises(NotImplementedError):
        MPI(geometry_grad=True).render_views_layers(lay, dhw.clone().requires_grad_(True), ray, eye, zd)


# ---- 2. the predicate -------------------------------------------------------------------------------------------------------------------------

def test_the_predicate():
    import ml_gmpi_amd
    from ml_gmpi_amd import is_float_layers
    from ml_gmpi_amd.quantized import is_interleaved
    assert "is_float_layers" in ml_gmpi_amd.__all__

    class Fake:
        ndim = 5

        def __init__(self, shape, strides, dtype=torch.float32):
            self.shape, self._s, self.dtype = shape, strides, dtype

        def stride(self, i=None):
            return self._s if i is None else self._s[i]

    shape = (M, D, Ht, Wt, 4)
    for dtype, _ in DTYPES:
        lay = layers(shape, dtype)
        assert is_float_layers(lay) and is_float_layers(lay[1:, 1:, 2:, 1:5]) and is_float_layers(lay[:1].expand(3, -1, -1, -1, -1))
        assert not is_interleaved(lay.permute(0, 1, 4, 2, 3))                       # quantized.is_interleaved stays uint8-only
    assert is_float_layers(Fake(shape, (D * Ht * Wt * 4, Ht * Wt * 4, Wt * 4, 4, 1)))
    assert not is_float_layers(Fake(shape, (D * Ht * Wt * 4, -Ht * Wt * 4, Wt * 4, 4, 1)))    # a negative plane stride
    assert not is_float_layers(Fake(shape, (D * Ht * Wt * 4, Ht * Wt * 4, -Wt * 4, 4, 1)))
    assert not is_float_layers(Fake(shape, (D * Ht * Wt * 4, Ht * Wt * 4, Wt * 4 - 4, 4, 1)))  # rows that overlap
    assert not is_float_layers(Fake(shape, (D * Ht * Wt * 5, Ht * Wt * 5, Wt * 5, 5, 1)))      # texel stride 5
    assert not is_float_layers(Fake(shape, (D * Ht * Wt * 8, Ht * Wt * 8, Wt * 8, 4, 2)))      # channel stride 2
    assert not is_float_layers(layers((M, D, 4, Ht, Wt)).permute(0, 1, 3, 4, 2))               # planar
    assert not is_float_layers(layers(shape)[..., :3]) and not is_float_layers(layers(shape)[0])
    assert not is_float_layers(torch.zeros(shape, dtype=torch.uint8)) and not is_float_layers(torch.zeros(shape, dtype=torch.float64))


# ---- 3. the C ABI: what is accepted and refused before a launch ----------------------------------------------------------------------------------

def _layer_params(variant=0, dtype=0):
    """test_u8_storage_cpu._params (1 x 2 x 4 x 8 x 8 over host buffers of 2 KiB, 4 x 4 pixels) with the layers' strides; fp32 fits the buffer with D = 1."""
    p, bufs = _params(dtype=dtype, variant=variant)
    p.D = 1 if dtype == 0 else 2
    p.rgba_stride[:] = [p.D * p.Ht * p.Wt * 4, p.Ht * p.Wt * 4, 1, 4 * p.Wt, 4]
    return p, bufs


def test_header_and_binding_name_the_entries():
    hdr = open(os.path.join(ROOT, "include", "gmpi_render.h")).read()
    assert "int gmpi_mpi_render_layers_launch(const GmpiRenderParams *params, void *stream);" in hdr
    assert "int gmpi_render_layers_supports(const GmpiRenderParams *params);" in hdr
    assert "gmpi_mpi_render_layers_launch" in _lib.EXPORTS and "gmpi_render_layers_supports" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 2 and ctypes.sizeof(_lib.GmpiRenderParams) == 184    # struct, size and ABI version stay


def test_query_reports_the_layout():
    lib = _library()
    assert lib.gmpi_query(42) == 1 and lib.gmpi_query(41) == -1 and lib.gmpi_query(43) == -1


def test_the_abi_validates_the_layout_before_a_launch():
    lib = _library()
    ref = ctypes.byref
    # accepted: the support query validates the struct as the launch does, and launches nothing
    for dtype in (0, 1, 2):
        for variant in (0, 1, 2):
            p, b = _layer_params(variant, dtype)
            assert lib.gmpi_render_layers_supports(ref(p)) == 1
            p.N = 0
            assert lib.gmpi_mpi_render_layers_launch(ref(p), None) == 0            # no views: nothing to launch
        # variants the layout does not have
        for variant in (3, 5, 4, 9, -1):
            p, b = _layer_params(variant, dtype)
            assert lib.gmpi_mpi_render_layers_launch(ref(p), None) == E_VARIANT
    # the support rule, both ways: fp32 takes any width and any element-aligned pointer
    p, b = _layer_params(2, 0)
    p.Wt, p.rgba_stride[3] = 7, 32
    assert lib.gmpi_render_layers_supports(ref(p)) == 1
    p.rgba += 4
    p.Ht = 7
    assert lib.gmpi_render_layers_supports(ref(p)) == 1
    for dtype in (1, 2):
        # ... 16-bit texels go two per item: an odd width, a pointer or a stride that is no multiple of 4 bytes -> 0, and LDS by name is refused
        p, b = _layer_params(2, dtype)
        p.Wt = 7
        assert lib.gmpi_render_layers_supports(ref(p)) == 0 and lib.gmpi_mpi_render_layers_launch(ref(p), None) == E_VARIANT
        p, b = _layer_params(2, dtype)
        p.rgba += 2
        p.Ht = 7
        assert lib.gmpi_render_layers_supports(ref(p)) == 0 and lib.gmpi_mpi_render_layers_launch(ref(p), None) == E_VARIANT
        for i in (0, 1, 3):
            p, b = _layer_params(2, dtype)
            p.Wt = 6
            p.rgba_stride[i] = p.rgba_stride[i] - 1 if i != 3 else 4 * p.Wt + 1   # an odd element stride: 2 bytes off
            assert lib.gmpi_render_layers_supports(ref(p)) == 0 and lib.gmpi_mpi_render_layers_launch(ref(p), None) == E_VARIANT
        p, b = _layer_params(2, dtype)
        p.rgba += 4                                                                # one column further: a multiple of 4 bytes, still staged
        p.Wt = 6
        assert lib.gmpi_render_layers_supports(ref(p)) == 1
    # in-box byte offsets below 2^31
    p, b = _layer_params(2, 0)
    p.rgba_stride[3] = 1 << 24
    assert lib.gmpi_render_layers_supports(ref(p)) == 0
    # stride combinations that are not the layout: refused by every variant, AUTO and GATHER included, by both entries
    for dtype in (0, 1, 2):
        for variant in (0, 1, 2):
            def refused(change):
                p, b = _layer_params(variant, dtype)
                change(p)
                assert lib.gmpi_mpi_render_layers_launch(ref(p), None) == E_STRIDE
                assert lib.gmpi_render_layers_supports(ref(p)) == E_STRIDE
            refused(lambda p: p.rgba_stride.__setitem__(slice(None), [p.D * 4 * p.Ht * p.Wt, 4 * p.Ht * p.Wt, p.Ht * p.Wt, p.Wt, 1]))   # planar
            refused(lambda p: p.rgba_stride.__setitem__(2, 2))                      # channel stride 2
            for texel in (2, 3, 5, 8):
                refused(lambda p: p.rgba_stride.__setitem__(4, texel))
            refused(lambda p: p.rgba_stride.__setitem__(3, 4 * p.Wt - 4))           # rows that overlap
            refused(lambda p: p.rgba_stride.__setitem__(1, -p.rgba_stride[1]))      # a negative stride
            refused(lambda p: p.rgba_stride.__setitem__(0, -1))
            # the existing entry keeps refusing the layout for the float types
            p, b = _layer_params(variant, dtype)
            assert lib.gmpi_mpi_render_launch(ref(p), None) == E_STRIDE
    p, b = _layer_params(dtype=4)
    assert lib.gmpi_mpi_render_layers_launch(ref(p), None) == E_DTYPE and lib.gmpi_render_layers_supports(ref(p)) == E_DTYPE
    # uint8 with these strides: the existing path's answers
    p, b = _layer_params(3, dtype=3)
    assert lib.gmpi_mpi_render_layers_launch(ref(p), None) == E_VARIANT
    p, b = _layer_params(2, dtype=3)
    assert lib.gmpi_render_layers_supports(ref(p)) == 1
    p.Wt, p.rgba_stride[3] = 6, 24
    assert lib.gmpi_render_layers_supports(ref(p)) == 0 and lib.gmpi_mpi_render_layers_launch(ref(p), None) == E_VARIANT
    p.struct_size -= 8
    assert lib.gmpi_render_layers_supports(ref(p)) == -5 and lib.gmpi_mpi_render_layers_launch(ref(p), None) == -5
    assert lib.gmpi_render_layers_supports(None) == -1 and lib.gmpi_mpi_render_layers_launch(None, None) == -1


# ---- 4. resources of the new instances -----------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("unit,kernel", [("render_layers", "render_layers_kernel"), ("render_gather", "render_gather_kernel")])
def test_layer_instances_compile_for_gfx950_without_scratch(tmp_path, unit, kernel):
    """The compiler's own report (the .amdhsa_* directives of -save-temps): zero scratch in the twelve staged and the twelve gather instances over the
    three texel types; LDS of the staged ones within 72 KB (fp32: two workgroups per CU) / 40 KB (16-bit)."""
    csrc = os.path.join(ROOT, "ml-gmpi_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
             "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]   # = ml-gmpi_amd/csrc/Makefile
    mk = open(os.path.join(csrc, "Makefile")).read()
    for f in ("-ffp-contract=off", "-fno-slp-vectorize", "-O3", unit + ".hip"):
        assert f in mk, f"the Makefile no longer has {f}: keep this test in step with it"
    res = subprocess.run([HIPCC, *flags, "-save-temps", "-c", os.path.join(csrc, unit + ".hip"), "-o", unit + ".o"], cwd=tmp_path, capture_output=True, timeout=900)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    asm = open(os.path.join(tmp_path, unit + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    for tag, lds_cap in (("9rgba32f_t", 72 * 1024), ("9rgba16h_t", 40 * 1024), ("9rgba16b_t", 40 * 1024)):
        names = sorted(n for n in set(re.findall(rf"^(_Z\w*{kernel}\w*):", asm, flags=re.M)) if tag in n)
        assert len(names) == 4, (tag, names)                                         # align_corners x order
        for name in names:
            meta = asm[asm.index(".amdhsa_kernel " + name):]
            meta = meta[:meta.index(".end_amdhsa_kernel")]
            assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1)) == 0, name
            lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", meta).group(1))
            assert lds <= (lds_cap if unit == "render_layers" else 0), (name, lds)
