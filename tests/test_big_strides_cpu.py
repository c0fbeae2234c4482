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
QUERY_SF_ROWS = 14   # gmpi_query: kSFRows, the box rows of the staged shared-colour and shaded forwards (shared_forward_query, render_shared_forward.hip)


@pytest.fixture(scope="module")
def env():
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    host = np.zeros(1024, dtype=np.uint8)
    fake = (host.ctypes.data + 511) & ~255   # a non-NULL address, 256-byte aligned; never followed
    return L, lib, fake, host


def _params(env, dtype, stride, *, wt=None, variant=None, D=3, flags=None):
    L, lib, fake, _ = env
    code, es = DTYPES[dtype] if dtype != "u8" else (L.DTYPE_U8, 1)
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


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_cameras_of_the_gpu_modules_reach_the_first_and_last_texel_row(dtype):
    """The row layouts put the row whose offset passes 2^31 or 2^32 last (31 s_row), so the cameras of tests/test_hip_big_strides.py (`_geo`) must
    put weight on it: with the oracle, halving texel row 0, row HT - 1 or column WT - 1 of the front plane changes the image, for both
    image sizes and both plane counts -- and no ray leaves the stack (T < 1 everywhere), so the planes' borders lie inside the image."""
    import oracle
    import test_hip_big_strides as G
    for D in (2, 3):
        v = G._volume(dtype, D).float().numpy()
        geo = G._geo(dtype, D)
        base = oracle.render(v, *geo, align_corners=True)
        assert base["status"] == 0 and float(base["T"].max()) < 1
        for axis, index in ((3, 0), (3, big.HT - 1), (4, v.shape[-1] - 1)):
            w = v.copy()
            cut = [slice(None)] * 5
            cut[1], cut[axis] = 0, index
            w[tuple(cut)] *= 0.5
            seen = int((oracle.render(w, *geo, align_corners=True)["color"] != base["color"]).any(1).sum())
            assert seen >= 8, (dtype, D, axis, index, seen)


def _layer_params(env, dtype, stride3, *, D=3, backward=False):
    """Float layers [2, D, HT, WT, 4] with (s_mpi, s_plane, s_row) = stride3, as `render_views_layers` hands them to the layers entries."""
    L, _, fake, _ = env
    s_mpi, s_plane, s_row = stride3
    p = _params(env, dtype, (s_mpi, s_plane, 1, s_row), D=D)
    p.rgba_stride[:] = [s_mpi, s_plane, 1, s_row, 4]
    if backward:   # (a backward: the forward's T, no outputs)
        p.rgb_out = p.depth_out = None
        p.transmittance_out = fake
    return p


def _dense_layers(D, wt):
    return (D * big.HT * 4 * wt, big.HT * 4 * wt, 4 * wt)


def _i64(v):
    return (ctypes.c_int64 * len(v))(*v)


def test_layer_gradient_and_shading_strides_are_where_the_docstring_says():
    for dtype, (_, es) in DTYPES.items():
        wt = big.wt_of(es)
        for layout in big.LAYER_LAYOUTS:
            s_mpi, s_plane, s_row = big.layer_strides(layout, es)
            D = big.planes_of(layout)
            assert s_row * es % 64 == 0 and s_plane * es % 64 == 0 and s_mpi * es % 64 == 0, (layout, dtype)
            dims = sorted([(4, wt), (s_row, big.HT), (s_plane, D), (s_mpi, 2)])
            assert all(b[0] >= a[0] * a[1] for a, b in zip(dims, dims[1:])), (layout, dtype, "the window's texels must not overlap")
        a, t, b, c = (big.layer_row_stride(k, es) * es for k in ("L-rowA", "L-rowT", "L-rowB", "L-rowC"))
        assert 33 * a + 16 * 64 + 128 < 2 ** 31 <= 33 * (a + 64) + 16 * 64 + 128
        assert 33 * (t - 64) < 2 ** 31 <= 33 * t and 32 * t + 4 * wt * es < 2 ** 31
        assert 2 ** 31 + 2 ** 24 <= 31 * b < 2 ** 31 + 2 ** 25 and 2 ** 32 + 2 ** 24 <= 31 * c < 2 ** 32 + 2 ** 25
        _, _, g_byte = big.grad_strides("G-byte", wt)
        _, _, g_past = big.grad_strides("G-past", wt)
        assert big.HT * g_byte + 4 * wt < 2 ** 31 and 31 * g_byte * 4 >= 2 ** 32 + 2 ** 24
        assert big.HT * (g_past - 1) + 4 * wt < 2 ** 31 <= big.HT * g_past + 4 * wt
        (_, ra), (_, rb) = big.shading_strides("S-rowA", wt), big.shading_strides("S-rowB", wt)
        assert rb - ra == 16 and big.HT * ra + wt < 2 ** 29 <= big.HT * rb + wt
        # SHADING_TILE: the layouts inside the shaded tile backward's third guard, plane_offsets_fit_32(0, s_row, HT, WT, 4) -- no query of the
        # library answers for that guard, so the list is held to the guard's arithmetic here
        for layout in big.SHADING_LAYOUTS:
            assert (big.HT * big.shading_strides(layout, wt)[1] + wt < 2 ** 29) == (layout in big.SHADING_TILE), (layout, dtype)
    # the dword margins are four times the byte margins; the largest buffers: 28 GiB (G-byte) and 32 GiB (G-past)
    assert (big.GRAD_LEAD, big.GRAD_TAIL) == (4 * big.LEAD, 4 * big.TAIL)
    for layout, lo in (("G-byte", 28), ("G-past", 31.7)):
        gs = big.grad_strides(layout, 36)
        top = big.GRAD_LEAD + (big.span((2, 3, big.HT, 36, 4), gs + (4, 1)) + 1) * 4 + big.GRAD_TAIL
        assert lo * 2 ** 30 <= top < (lo + 0.1) * 2 ** 30, (layout, top / 2 ** 30)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_layer_layouts_lie_on_the_side_of_each_guard_the_table_claims(env, dtype):
    """gmpi_render_layers_supports (the staged forward of render_layers.hip) and gmpi_render_layers_backward_supports (the texel tile backward), as
    compiled: outer and A are taken by both, T by the backward alone, B and C by neither; one 64-byte step above A the forward refuses."""
    _, lib, _, _ = env
    _, es = DTYPES[dtype]
    wt = big.wt_of(es)
    fwd = lambda p: int(lib.gmpi_render_layers_supports(ctypes.byref(p)))
    bwd = lambda p, gs: int(lib.gmpi_render_layers_backward_supports(ctypes.byref(p), _i64([gs[0], gs[1], 1, gs[2], 4])))
    for layout in big.LAYER_LAYOUTS:
        D = big.planes_of(layout)
        st = big.layer_strides(layout, es)
        assert fwd(_layer_params(env, dtype, st, D=D)) == (1 if layout in big.LAYERS_STAGED else 0), (layout, dtype)
        assert bwd(_layer_params(env, dtype, st, D=D, backward=True), _dense_layers(D, wt)) == (1 if layout in big.LAYERS_TILE else 0), (layout, dtype)
    s_mpi, s_plane, a = big.layer_strides("L-rowA", es)
    assert fwd(_layer_params(env, dtype, (s_mpi, s_plane, a + 64 // es))) == 0                       # A is the LARGEST the staged forward takes
    assert bwd(_layer_params(env, dtype, (s_mpi, s_plane, a + 64 // es), backward=True), _dense_layers(3, wt)) == 1
    # the gradient's layouts over dense layers: G-byte is taken, G-past is the FIRST row stride refused
    dense = _layer_params(env, dtype, _dense_layers(3, wt), backward=True)
    g_mpi, g_plane, g_past = big.grad_strides("G-past", wt)
    assert bwd(dense, big.grad_strides("G-byte", wt)) == 1
    assert bwd(dense, (g_mpi, g_plane, g_past)) == 0 and bwd(dense, (g_mpi, g_plane, g_past - 1)) == 1


def test_channels_last_codes_outer_is_staged_and_the_row_layout_is_not(env):
    """u8_variant_supports through gmpi_render_layers_supports: it decides which forward renders channels-last codes and, in default mode, whether
    the in-place geometry backward uses the forward's transmittance (gmpi_abi.hip).  `outer` is taken; rows of row_stride("rowC", 1) bytes are not."""
    L, lib, _, _ = env
    ask = lambda st, D: int(lib.gmpi_render_layers_supports(ctypes.byref(_layer_params(env, "u8", st, D=D))))
    assert ask((big.U8_S_MPI, big.U8_S_PLANE, 4 * big.PITCH), 2) == 1
    assert ask((3 * 4 * big.PITCH, 4 * big.PITCH, big.row_stride("rowC", 1)), 3) == 0
    assert (big.HT - 1) * big.row_stride("rowC", 1) >= 2 ** 32 + 2 ** 24


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_shaded_forward_takes_every_layout_of_the_shaded_cases(env, dtype):
    """gmpi_render_shaded_supports: the staged shaded forward gives every channel image a 64-bit base and keeps only row offsets in 32 bits, at
    (27 + 1) rows of the volume and of the shading image: it takes the volume on `outer` and on `chanB`, and the shading image on all three of its
    layouts -- rows of 2^24 floats are inside ITS bound.  (S-rowA and S-rowB straddle the third guard of the shaded tile BACKWARD, for which the
    library has no query: test_layer_gradient_and_shading_strides_are_where_the_docstring_says holds them to that guard's arithmetic.)  A shading
    row stride past the forward's own bound is refused."""
    L, lib, fake, _ = env
    _, es = DTYPES[dtype]
    wt = big.wt_of(es)
    rows = lib.gmpi_query(QUERY_SF_ROWS)
    assert rows > 0

    def ask(vol_stride, D, sh_stride):
        p = _params(env, dtype, vol_stride, D=D, variant=L.VARIANT_LDS)
        sh = L.GmpiShading()
        sh.struct_size = ctypes.sizeof(L.GmpiShading)
        sh.shading = fake
        sh.shading_stride[:] = list(sh_stride)
        return int(lib.gmpi_render_shaded_supports(ctypes.byref(p), ctypes.byref(sh)))

    dense_sh = (big.HT * wt, wt)
    for layout in ("outer", "chanB"):
        assert ask(big.strides(layout, es), big.planes_of(layout), dense_sh) == 1, (layout, dtype)
    for layout in big.SHADING_LAYOUTS:
        assert ask(_contiguous(3, wt), 3, big.shading_strides(layout, wt)) == 1, (layout, dtype)
    first_bad = -(-(2 ** 29 - 128) // ((rows + 1) * 4)) * 4
    assert ask(_contiguous(3, wt), 3, (big.PITCH, first_bad)) == 0 and ask(_contiguous(3, wt), 3, (big.PITCH, first_bad - 4)) == 1


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
    rows = lib.gmpi_query(QUERY_SF_ROWS)
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
