"""The in-place backward of channels-last float layers (gmpi_mpi_render_layers_backward_launch, gmpi_render_layers_backward_supports;
`layers_backward="texel"`) without a GPU: the real library is asked with fake, aligned pointers (as test_big_strides_cpu.py does), and the launch entry
is only called on arguments that must be refused before anything is launched."""
import ctypes

import numpy as np
import pytest

LAUNCH, SUPPORTS = "gmpi_mpi_render_layers_backward_launch", "gmpi_render_layers_backward_supports"
DTYPES = {"f32": (0, 4), "bf16": (1, 2), "f16": (2, 2)}
E_NULL, E_DTYPE, E_STRIDE = -1, -3, -4
D, HT, WT, H, W = 3, 32, 40, 19, 130


@pytest.fixture(scope="module")
def env():
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    host = np.zeros(1024, dtype=np.uint8)
    fake = (host.ctypes.data + 511) & ~255   # a non-NULL address, 256-byte aligned; never followed
    return L, lib, fake, host


def layer_stride(ht=HT, wt=WT, d=D, s_row=None):
    s_row = 4 * wt if s_row is None else s_row
    return [d * ht * s_row, ht * s_row, 1, s_row, 4]


def _params(env, dtype="f32", stride=None, *, n=2, ht=HT, wt=WT, variant=None):
    L, lib, fake, _ = env
    p = L.GmpiRenderParams()
    p.struct_size = ctypes.sizeof(L.GmpiRenderParams)
    p.flags = L.FLAG_ALIGN_CORNERS
    p.variant, p.rgba_dtype = (L.VARIANT_AUTO if variant is None else variant), (dtype if isinstance(dtype, int) else DTYPES[dtype][0])
    p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = n, 2, D, ht, wt, H, W, max(1, -(-n // 2))
    p.rgba = fake
    p.rgba_stride[:] = layer_stride(ht, wt) if stride is None else stride
    p.dhw = p.ray_dir = p.eye_pos = p.z_dir = p.transmittance_out = fake   # (a backward: no rgb_out / depth_out / status)
    return p


def i64(v):
    return (ctypes.c_int64 * 5)(*v)


def supports(env, p, gst):
    return int(getattr(env[1], SUPPORTS)(ctypes.byref(p), i64(gst)))


def launch(env, p, gst, grad_rgb="fake", grad_layers="fake"):
    fake = env[2]
    return int(getattr(env[1], LAUNCH)(ctypes.byref(p), fake if grad_rgb == "fake" else grad_rgb, None, None,
                                       fake if grad_layers == "fake" else grad_layers, i64(gst) if gst is not None else None, None))


def test_entries_are_exported_and_announced(env):
    L, lib, _, _ = env
    assert LAUNCH in L.EXPORTS and SUPPORTS in L.EXPORTS
    assert lib.gmpi_query(44) == 1 and lib.gmpi_query(43) == -1 and lib.gmpi_query(42) == 1


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_supports_takes_a_plain_case(env, dtype):
    assert supports(env, _params(env, dtype), layer_stride()) == 1
    assert supports(env, _params(env, dtype, layer_stride(s_row=4 * WT + 12)), layer_stride(s_row=4 * WT + 8)) == 1   # padded rows, either tensor
    assert supports(env, _params(env, dtype, variant=env[0].VARIANT_GATHER), layer_stride()) == 1   # (the query does not look at the variant)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_supports_answers_zero_where_a_tile_guard_fails(env, dtype):
    _, es = DTYPES[dtype]
    assert supports(env, _params(env, dtype, wt=1), layer_stride(wt=1)) == 0                        # no pair of columns
    assert supports(env, _params(env, dtype, n=65536), layer_stride()) == 0                         # the view index in grid.y
    assert supports(env, _params(env, dtype, n=65535), layer_stride()) == 1
    # the layers' byte offsets: (Ht s_row + 4 Wt) es = 2^31 exactly is refused, one element per row less is taken
    s_row = (2 ** 31 // es - 4 * WT) // HT
    assert (HT * s_row + 4 * WT) * es == 2 ** 31, "choose Ht, Wt so that the sum can be hit"
    assert supports(env, _params(env, dtype, layer_stride(s_row=s_row)), layer_stride()) == 0
    assert supports(env, _params(env, dtype, layer_stride(s_row=s_row - 1)), layer_stride()) == 1
    # the gradient's dword offsets: Ht gs_row + 4 Wt = 2^31
    gs_row = (2 ** 31 - 4 * WT) // HT
    assert HT * gs_row + 4 * WT == 2 ** 31
    assert supports(env, _params(env, dtype), layer_stride(s_row=gs_row)) == 0
    assert supports(env, _params(env, dtype), layer_stride(s_row=gs_row - 1)) == 1


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_bad_strides_are_refused_by_both_entries(env, dtype):
    planar = [D * 4 * HT * WT, 4 * HT * WT, HT * WT, WT, 1]
    texel8 = [D * HT * 8 * WT, HT * 8 * WT, 1, 8 * WT, 8]
    short = layer_stride(s_row=4 * WT - 4)
    for bad in (planar, texel8, short):
        p = _params(env, dtype, bad)
        assert supports(env, p, layer_stride()) == E_STRIDE, bad
        assert launch(env, p, layer_stride()) == E_STRIDE, bad
    for bad in ([D * HT * 4 * WT, HT * 4 * WT, 2, 4 * WT, 4], planar, texel8, short, [D * HT * 4 * WT, 0, 1, 4 * WT, 4], [-1, HT * 4 * WT, 1, 4 * WT, 4]):
        p = _params(env, dtype)
        assert supports(env, p, bad) == E_STRIDE, bad
        assert launch(env, p, bad) == E_STRIDE, bad


def test_uint8_layers_have_no_gradient(env):
    L = env[0]
    p = _params(env, L.DTYPE_U8)
    assert supports(env, p, layer_stride()) == E_DTYPE
    assert launch(env, p, layer_stride()) == E_DTYPE


def test_null_pointers_are_refused(env):
    p = _params(env)
    assert launch(env, p, layer_stride(), grad_layers=None) == E_NULL
    assert launch(env, p, layer_stride(), grad_rgb=None) == E_NULL
    assert launch(env, p, None) == E_NULL
    assert int(getattr(env[1], SUPPORTS)(ctypes.byref(p), None)) == E_NULL
    assert int(getattr(env[1], SUPPORTS)(None, i64(layer_stride()))) == E_NULL
    q = _params(env)
    q.rgba = None
    assert launch(env, q, layer_stride()) == E_NULL and supports(env, q, layer_stride()) == E_NULL


def test_no_views_is_ok_before_anything_else(env):
    p = _params(env, n=0)
    assert launch(env, p, layer_stride(), grad_rgb=None, grad_layers=None) == 0


def test_the_keyword_takes_two_values():
    import torch
    from ml_gmpi_amd import MPI, make_renderer
    lay = torch.zeros((1, 2, 8, 8, 4))
    geo = (torch.zeros((1, 2, 3)), torch.zeros((1, 3, 4, 4)), torch.zeros((1, 3)), torch.zeros((1, 3)))
    with pytest.raises(ValueError, match="layers_backward"):
        MPI().render_views_layers(lay, *geo, layers_backward="nope")
    r = make_renderer("FFHQ", n_planes=2, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="layers_backward"):
        r.render_layers(lay, 4, 4, layers_backward="nope")
    assert MPI().layers_backward_fallbacks == 0
