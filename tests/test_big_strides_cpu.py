"""The host-side guards of the kernels that keep in-plane offsets in 32 bits, on the strides of tests/_big_strides.py, without a GPU: the real
library is asked with fake, aligned pointers (as test_depth_alpha_window_cpu.py does), and launch entries are only called on arguments that must be
refused before anything is launched."""
import ctypes

import numpy as np
import pytest

import _big_strides as big

DTYPES = {"f32": (0, 4), "bf16": (1, 2), "f16": (2, 2)}
H, W = 19, 130
E_VARIANT = -6


@pytest.fixture(scope="module")
def env():
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    host = np.zeros(1024, dtype=np.uint8)
    fake = (host.ctypes.data + 511) & ~255   # a non-NULL address, 256-byte aligned; never followed
    return L, lib, fake, host


def _params(env, dtype, stride, *, wt=None, variant=None, D=3, flags=None):
    L, lib, fake, _ = env
    code, es = DTYPES[dtype]
    p = L.GmpiRenderParams()
    p.struct_size = ctypes.sizeof(L.GmpiRenderParams)
    p.flags = L.FLAG_ALIGN_CORNERS if flags is None else flags
    p.variant, p.rgba_dtype = (L.VARIANT_AUTO if variant is None else variant), code
    p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = 2, 2, D, big.HT, (big.wt_of(es) if wt is None else wt), H, W, 1
    p.rgba = fake
    p.rgba_stride[:] = list(stride) + [1]
    p.dhw = p.ray_dir = p.eye_pos = p.z_dir = p.rgb_out = p.depth_out = fake
    return p


def _contiguous(D, wt):
    return (D * 4 * big.HT * wt, 4 * big.HT * wt, big.HT * wt, wt)


def test_layout_strides_are_where_the_docstring_says():
    for dtype, (_, es) in DTYPES.items():
        a, b, c = (3 * big.chan_stride(k, es) * es for k in ("chanA", "chanB", "chanC"))
        assert 2 ** 31 - 2 ** 24 - 192 <= a <= 2 ** 31 - 2 ** 24 and 2 ** 31 + 2 ** 24 <= b < 2 ** 31 + 2 ** 24 + 256 and 2 ** 32 + 2 ** 24 <= c < 2 ** 32 + 2 ** 24 + 256
        rb, rc = ((big.HT - 1) * big.row_stride(k, es) * es for k in ("rowB", "rowC"))
        assert 2 ** 31 <= rb < 2 ** 32 and rc >= 2 ** 32 + 2 ** 24
        assert big.S_PLANE * es > (2 ** 32 if es == 4 else 2 ** 31) and big.S_MPI > 2 ** 31
        for layout in big.FLOAT_LAYOUTS:
            assert all(s % (64 // es) == 0 or s == big.PITCH for s in big.strides(layout, es)), (layout, dtype)   # 16-byte items stay aligned
            assert (big.plane_bytes(layout, es) < 2 ** 31) == (layout in big.FITS_32), (layout, dtype)
    assert big.U8_S_PLANE > 2 ** 31 and big.U8_S_MPI > 2 ** 32
    # the fp32 outer layout is the largest buffer: about 18 GiB
    top = big.LEAD + (big.span((2, 2, 4, big.HT, 36), big.strides("outer", 4) + (1,)) + 1) * 4 + big.TAIL
    assert 18 * 2 ** 30 <= top < 18.01 * 2 ** 30 < big.NEED_FREE


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_backward_workspace_query_is_zero_where_a_planes_offsets_leave_32_bits(env, dtype):
    """gmpi_render_backward_workspace_bytes: non-zero = the atomics-free pair takes the launch.  Its pixel pass (fetch_pair_taps) adds 32-bit byte
    offsets to the plane pointer, so a volume with (3 s_chan + Ht s_row + Wt) es >= 2^31 must take the atomic kernels: the query answers 0."""
    L, lib, _, _ = env
    _, es = DTYPES[dtype]
    wt = big.wt_of(es)
    q = lambda p: int(lib.gmpi_render_backward_workspace_bytes(ctypes.byref(p)))
    assert q(_params(env, dtype, _contiguous(3, wt))) >= 2 * 3 * H * W * 24   # N D H W 24 bytes behind the homography records
    for layout in big.FLOAT_LAYOUTS:
        got = q(_params(env, dtype, big.strides(layout, es), D=big.planes_of(layout)))
        if layout in big.FITS_32:
            assert got >= 2 * big.planes_of(layout) * H * W * 24, (layout, dtype, got)
        else:
            assert got == 0, (layout, dtype, got)
    # the boundary itself: (3 s_chan + Ht s_row + Wt) es = 2^31 exactly is refused, one item below is taken
    s_row = big.PITCH
    s_chan = (2 ** 31 // es - big.HT * s_row - wt) // 3
    assert (3 * s_chan + big.HT * s_row + wt) * es == 2 ** 31, "choose Wt so that the sum can be hit"
    at = (3 * big.HT * big.PITCH, big.HT * big.PITCH, s_chan, s_row)
    below = (3 * big.HT * big.PITCH, big.HT * big.PITCH, s_chan - 1, s_row)
    assert q(_params(env, dtype, at)) == 0
    assert q(_params(env, dtype, below)) > 0
    # a row stride alone can leave 32 bits too
    s_chan = next(c for c in range(big.PITCH, big.PITCH + big.HT) if (2 ** 31 // es - wt - 3 * c) % big.HT == 0)
    s_row = (2 ** 31 // es - wt - 3 * s_chan) // big.HT
    assert (3 * s_chan + big.HT * s_row + wt) * es == 2 ** 31
    assert q(_params(env, dtype, (12 * s_chan, 4 * s_chan, s_chan, s_row))) == 0 and q(_params(env, dtype, (12 * s_chan, 4 * s_chan, s_chan, s_row - 1))) > 0
    # what was refused before stays refused, whatever the strides
    assert q(_params(env, dtype, _contiguous(3, wt), flags=0)) == 0                       # align_corners=False
    assert q(_params(env, dtype, _contiguous(3, wt), variant=L.VARIANT_GATHER)) == 0      # the all-atomic cross-check


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_explicit_staged_variants_refuse_strides_they_cannot_address(env, dtype):
    """GMPI_VARIANT_LDS and _BAND keep channel and row offsets of a box in 32 bits: GMPI_E_VARIANT for chanC and rowC.  GMPI_VARIANT_WAVE gives
    every channel image a buffer descriptor of its own (64-bit base) and keeps only row offsets in 32 bits: it refuses rowC, and takes chanC --
    which only a GPU can show (tests/test_hip_big_strides.py)."""
    L, lib, fake, _ = env
    _, es = DTYPES[dtype]
    launch = lambda p: int(lib.gmpi_mpi_render_launch(ctypes.byref(p), None))
    # (wave_variant_supports, render_wave.hip, bounds (Ht + 64) s_row es alone -- s_chan does not enter it: an explicit WAVE on chanC would be
    #  launched, which this host cannot do; lds_variant_supports and band_variant_supports bound 3 s_chan + rows s_row)
    for layout, variants in (("chanC", (L.VARIANT_LDS, L.VARIANT_BAND)), ("rowC", (L.VARIANT_LDS, L.VARIANT_WAVE, L.VARIANT_BAND))):
        for variant in variants:
            if variant == L.VARIANT_BAND and dtype == "f16" and lib.gmpi_query(8) <= 0:
                continue
            p = _params(env, dtype, big.strides(layout, es), variant=variant)
            if variant == L.VARIANT_BAND:   # the band kernel's first question is its workspace: lend one, so that the strides decide
                c = _params(env, dtype, _contiguous(3, p.Wt), variant=variant)
                need = int(lib.gmpi_render_workspace_bytes(ctypes.byref(c)))
                assert need > 0
                p.workspace, p.workspace_bytes = fake, 1 << 40
            assert launch(p) == E_VARIANT, (layout, dtype, variant)


def test_shared_forward_supports_answers_zero_for_a_row_stride_over_its_bound(env):
    L, lib, fake, _ = env
    rows = lib.gmpi_query(14)   # kSFRows: box rows of the staged shared-colour forward
    assert rows > 0

    def ask(dtype, s_row, rgb_row=big.PITCH, bg_row=big.PITCH):
        _, es = DTYPES[dtype]
        p = _params(env, dtype, (3 * big.HT * big.PITCH, big.HT * big.PITCH, 1, s_row), variant=L.VARIANT_LDS)
        s = L.GmpiSharedColor()
        s.struct_size = ctypes.sizeof(L.GmpiSharedColor)
        s.rgb, s.background = fake, fake
        s.rgb_stride[:] = [3 * big.HT * big.PITCH, big.HT * big.PITCH, rgb_row]
        s.background_stride[:] = [3 * big.HT * big.PITCH, big.HT * big.PITCH, bg_row]
        return int(lib.gmpi_render_shared_supports(ctypes.byref(p), ctypes.byref(s)))

    for dtype, (_, es) in DTYPES.items():
        assert ask(dtype, big.PITCH) == 1
        assert ask(dtype, big.row_stride("rowC", es)) == 0
        # the bound: (kSFRows + 1) row + 128 < 2^31 / es, on whichever of the three tensors has the longest rows (multiples of the 4-texel item)
        first_bad = -(-(2 ** 31 // es - 128) // (rows + 1))
        first_bad = -(-first_bad // 4) * 4
        last_good = first_bad - 4
        assert (rows + 1) * last_good + 128 < 2 ** 31 // es <= (rows + 1) * first_bad + 128
        assert ask(dtype, last_good) == 1 and ask(dtype, first_bad) == 0
        assert ask(dtype, big.PITCH, rgb_row=first_bad) == 0 and ask(dtype, big.PITCH, bg_row=first_bad) == 0
        assert ask(dtype, big.PITCH, rgb_row=last_good, bg_row=last_good) == 1
