"""The kernels that read a texture IN PLACE and the fused shaded render, on strides past 2^31 bytes, 2^32 bytes and 2^31 elements: the layouts of
tests/_big_strides.py for channels-last float layers, their fp32 gradient and the shading image, next to the volume layouts of
tests/test_hip_big_strides.py, whose rules hold here: small textures as windows of one NaN-filled (uint8: 255-filled, gradients: zero-filled) device
buffer whose margins keep every 32-bit mistake inside the allocation; every strided run against the same call on a contiguous copy, the contiguous copy
against a reference that does not run the code under test; view 1 differs from view 0 and T.max() > 1e-3 in every test.

  float layers, forward     render_layers.hip (staged) and the one-pixel texel instances, tests/test_hip_big_strides.py's forward rules
  float layers, backward    the texel instances of render_backward.hip: the 64 x 8 tile kernel and the one-pixel kernel, the gradient in fp32 through
                            the C ABI at the fp32 bars (2e-5 max + 1e-6 against float64, 1e-5 max strided against contiguous); then into a strided gradient
  geometry, in place        MPI(geometry_grad="all") over uint8 codes (planar, channels-last) and float layers, `_check`'s bars against float64
  the fused shaded render   render_shaded.hip and the shaded instances of render_backward.hip, the bars of tests/test_hip_shaded_render.py

Which kernel ran is read from the library's supports queries on the launch's own struct and from the module's fallback counters, and asserted:
tests/test_big_strides_cpu.py shows the same answers without a device.  A module that asks for "lds" over layers the staged forward refuses counts
that launch in `layers_lds_fallbacks`: the counter is 0 on the layouts the table calls staged and 1 per such launch on the others."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
import _big_strides as big
import _transmittance_ref
from _geometry_ref import geometry_grads
from test_hip_big_strides import DEV, DTYPES, KEYS, M, N, _d, _default_bars, _es, _forward, _geo, _means_something, _mpi, _upstream, _volume

pytestmark = pytest.mark.gpu
FORWARD_VARIANTS = ("gather", "lds", "auto")


def _peak():
    return f"peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB"


def _layers_of(planar):
    """[M, D, 4, HT, WT] -> contiguous layers [M, D, HT, WT, 4]."""
    return planar.permute(0, 1, 3, 4, 2).contiguous()


def _layer_window(layers, layout, es, **kw):
    return big.Window(layers, big.layer_strides(layout, es, D=layers.shape[1]) + (4, 1), **kw)


def _layers_query(query, p, *more):
    from ml_gmpi_amd import _lib
    rc = int(getattr(_lib.load_library(), query)(ctypes.byref(p), *more))
    assert rc in (0, 1), (query, rc)
    return rc


# ---- float layers, forward ----------------------------------------------------------------------------------------------------------------------
def _layers_forward(lay, geo, variant, strict):
    """(colour, depth, T on the host, `layers_lds_fallbacks`): `render_views_layers` reads `lay` where it lies (`layers_copies` stays 0)."""
    mpi = _mpi(strict_order=strict)
    with torch.no_grad():
        out = mpi.render_views_layers(lay, *geo, variant=variant, views_per_mpi=1, check_last_plane=False, want_transmittance=True)
    torch.cuda.synchronize()
    assert int(out["status"][0].item()) == 0 and mpi.layers_copies == 0
    return {k: out[k].cpu() for k in KEYS}, mpi.layers_lds_fallbacks


def _launch_struct(lay, geo, variant="auto"):
    """The forward's launch struct over `lay` (what the supports queries are asked with), its keep-alive tensors and its outputs."""
    mpi = _mpi(variant=variant)
    with torch.no_grad():
        fwd = mpi.render_views(lay, *geo, _layers=variant, views_per_mpi=1, check_last_plane=False, want_transmittance=True, defer_status=True,
                               _in_autograd_fn=True)
    mpi.raise_on_status(fwd["status"])   # a NaN the forward sampled raises here
    return fwd


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("layout", big.LAYER_LAYOUTS)
def test_layers_forward_every_variant(layout, name):
    """tests/test_hip_big_strides.py `_forward_all`'s rules: strict mode -- copy == oracle (on the planar float copy) and strided == copy, bit for bit;
    default mode -- equal bits where the same kernel ran on both (variant "gather"; "lds" and "auto" on the layouts the staged kernel takes), else
    (the strided layers ran the one-pixel kernel, the copy the staged one) the parity bars against the oracle and, bit for bit, the strided "gather"
    result."""
    D, es = big.planes_of(layout), _es(name)
    planar = _volume(name, D)
    dhw, ray, eye, zd = _geo(name, D)
    orc = oracle.render(planar.float().numpy(), dhw, ray, eye, zd, align_corners=True)
    geo = tuple(_d(a) for a in (dhw, ray, eye, zd))
    staged = layout in big.LAYERS_STAGED
    with _layer_window(_layers_of(planar), layout, es) as w:
        assert w.view.stride() == big.layer_strides(layout, es) + (4, 1) and not w.view.is_contiguous()
        fwd = _launch_struct(w.view, geo)
        assert _layers_query("gmpi_render_layers_supports", fwd["_bwd"][0]) == (1 if staged else 0), (layout, name)
        assert _layers_query("gmpi_render_layers_supports", _launch_struct(w.copy, geo)["_bwd"][0]) == 1
        del fwd
        gathered = None
        for variant in FORWARD_VARIANTS:
            for strict in (True, False):
                label = ("layers", layout, name, variant, strict)
                got, fallbacks = _layers_forward(w.view, geo, variant, strict)
                alone, fallbacks_alone = _layers_forward(w.copy, geo, variant, strict)
                assert fallbacks_alone == 0 and fallbacks == (1 if variant == "lds" and not staged else 0), label
                for k in KEYS:
                    assert torch.isfinite(got[k]).all(), label + (k,)
                if strict:
                    for k in KEYS:
                        assert np.array_equal(alone[k].numpy(), orc[k]), label + (k, "contiguous copy against the oracle")
                        assert torch.equal(got[k], alone[k]), label + (k,)
                elif variant == "gather" or staged:
                    for k in KEYS:
                        assert torch.equal(got[k], alone[k]), label + (k,)
                    if variant == "gather":
                        gathered = got
                else:
                    _default_bars(got, orc, label)
                    _default_bars(alone, orc, label + ("contiguous copy",))
                    assert all(torch.equal(got[k], gathered[k]) for k in KEYS), label + ("not the one-pixel kernel's bits",)
                _means_something(got)
    print(f"BIGSTRIDES layers forward {layout} {name}: staged kernel {'ran' if staged else 'refused, one-pixel kernel ran'}; {_peak()}")


# ---- float layers, the texel backward -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layers_reference(name, D):
    """float64 autograd of the loss over colour, depth and T, in the layers' order (host, shared, never written to)."""
    dhw, ray, eye, zd = _geo(name, D)
    gc, gd, gT = _upstream(name)
    ref = _transmittance_ref.grads(_volume(name, D).float().numpy(), dhw, ray, eye, zd, np.arange(N), gc, gd, gT)[0]
    ref = np.ascontiguousarray(np.transpose(ref, (0, 1, 3, 4, 2)))
    assert np.abs(ref[:, :, big.HT - 1]).max() > 1e-3 * np.abs(ref).max()   # the last row, whose offsets are the largest, takes part
    ref.setflags(write=False)
    return ref


def _abi_layers_backward(lay, geo, name, variant, grad=None):
    """The gradient w.r.t. the layers in fp32 through gmpi_mpi_render_layers_backward_launch, as `_LayersRenderFunction._backward_texel` calls it:
    the forward's struct over the layers in place, upstream gradients on colour, depth and T, ONE zero-filled fp32 tensor in the layers' order (grad:
    this one instead).  variant "auto": the 64 x 8 tile kernel where gmpi_render_layers_backward_supports says so; "gather": the one-pixel kernel.
    Returns (gradient on the host, the query's answer)."""
    from ml_gmpi_amd import _lib
    lib = _lib.load_library()
    fwd = _launch_struct(lay, geo, variant)
    p, keep = fwd["_bwd"]
    p.rgb_out = p.depth_out = p.status = None
    gc, gd, gT = (_d(a) for a in _upstream(name))
    if grad is None:
        grad = torch.zeros(tuple(lay.shape), dtype=torch.float32, device=DEV)
    gst = (ctypes.c_int64 * 5)(grad.stride(0), grad.stride(1), 1, grad.stride(2), 4)
    takes = _layers_query("gmpi_render_layers_backward_supports", p, gst)
    _lib.check(lib.gmpi_mpi_render_layers_backward_launch(ctypes.byref(p), gc.data_ptr(), gd.data_ptr(), gT.data_ptr(), grad.data_ptr(), gst,
                                                          torch.cuda.current_stream(DEV).cuda_stream), "layers backward")
    torch.cuda.synchronize()
    _means_something({k: fwd[k] for k in KEYS})
    del keep
    return grad.cpu().numpy(), takes


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("layout", big.LAYER_LAYOUTS)
def test_layers_backward_tile_and_one_pixel(layout, name):
    D, es = big.planes_of(layout), _es(name)
    planar = _volume(name, D)
    ref = _layers_reference(name, D)
    scale = float(np.abs(ref).max())
    assert scale > 0
    geo = tuple(_d(a) for a in _geo(name, D))
    tile = layout in big.LAYERS_TILE
    worst = {}
    with _layer_window(_layers_of(planar), layout, es) as w:
        for variant in ("auto", "gather"):
            got, takes = _abi_layers_backward(w.view, geo, name, variant)
            alone, takes_alone = _abi_layers_backward(w.copy, geo, name, variant)
            label = ("layers backward", layout, name, variant)
            assert takes == (1 if tile else 0) and takes_alone == 1, label   # (the query does not look at the variant)
            assert np.isfinite(got).all() and np.isfinite(alone).all(), label
            e64, e64a = float(np.abs(got - ref).max()), float(np.abs(alone - ref).max())
            assert e64a <= 2e-5 * scale + 1e-6, label + ("contiguous copy against float64", e64a, scale)
            assert e64 <= 2e-5 * scale + 1e-6, label + ("against float64", e64, scale)
            esc = float(np.abs(got - alone).max())
            assert esc <= 1e-5 * float(np.abs(alone).max()), label + ("strided against contiguous", esc)
            worst[variant] = (esc / (1e-5 * float(np.abs(alone).max())), e64 / (2e-5 * scale + 1e-6))
        if name == "f32":   # layers_backward="texel" under autograd: the same routing through hip_mpi, counted
            gc, gd, gT = (_d(a) for a in _upstream(name))

            def through_autograd(v):
                lay = v.detach().requires_grad_(True)
                mpi = _mpi()
                out = mpi.render_views_layers(lay, *geo, layers_backward="texel", views_per_mpi=1, check_last_plane=False, want_transmittance=True)
                ((out["color"] * gc).sum() + (out["depth"] * gd).sum() + (out["T"] * gT).sum()).backward()
                torch.cuda.synchronize()
                return lay.grad.cpu().numpy(), mpi.layers_backward_fallbacks, mpi.layers_copies
            (a, fallbacks, copies), (b, fallbacks_alone, _) = through_autograd(w.view), through_autograd(w.copy)
            assert fallbacks == (0 if tile else 1) and fallbacks_alone == 0 and copies == 0, (layout, "autograd")
            assert np.abs(a - ref).max() <= 2e-5 * scale + 1e-6 and np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), (layout, "autograd")
    print(f"BIGSTRIDES layers backward {layout} {name}: {'tile kernel' if tile else 'one-pixel fallback'} under auto; (strided vs contiguous, strided vs "
          "float64) as fractions of their bars: " + ", ".join(f"{k} {v[0]:.3f} {v[1]:.3f}" for k, v in worst.items()) + f"; {_peak()}")


@pytest.mark.parametrize("layout", big.GRAD_LAYOUTS)
def test_layers_backward_into_a_strided_gradient(layout):
    """Contiguous fp32 layers, the gradient written into a window of a zero-filled buffer whose offsets the tile kernel counts in dwords (margins of
    8 and 16 GiB: tests/_big_strides.py).  G-byte: the tile kernel takes it -- every dword offset of a plane is below 2^31 -- and the cells lie past
    2^32 bytes; G-past: the first row stride its guard refuses, the one-pixel kernel runs.  Nothing but the window's cells may be written."""
    name, D = "f32", 3
    planar = _volume(name, D)
    ref = _layers_reference(name, D)
    scale = float(np.abs(ref).max())
    geo = tuple(_d(a) for a in _geo(name, D))
    lay = _layers_of(planar).to(DEV)
    want = {variant: _abi_layers_backward(lay, geo, name, variant)[0] for variant in ("auto", "gather")}
    stride = big.grad_strides(layout, planar.shape[-1], D=D) + (4, 1)
    with big.Window(torch.zeros(tuple(lay.shape)), stride, fill=0.0, lead=big.GRAD_LEAD, tail=big.GRAD_TAIL) as w:
        assert w.view.stride(2) == stride[2] and (big.HT - 1) * stride[2] * 4 >= 2 ** 32
        for variant in ("auto", "gather"):
            w.view.zero_()
            got, takes = _abi_layers_backward(lay, geo, name, variant, grad=w.view)
            label = ("strided gradient", layout, variant)
            assert takes == (1 if layout == "G-byte" else 0), label
            assert np.isfinite(got).all() and np.count_nonzero(got[:, :, big.HT - 1]) > 0, label   # (row HT - 1: the cells past 2^32 bytes)
            e64, esc = float(np.abs(got - ref).max()), float(np.abs(got - want[variant]).max())
            assert e64 <= 2e-5 * scale + 1e-6, label + ("against float64", e64, scale)
            assert esc <= 1e-5 * float(np.abs(want[variant]).max()), label + ("against the contiguous gradient", esc)
            base = w.view._base   # (counted in pieces: the comparison's temporary stays small next to the buffer)
            written = sum(int(base[i:i + 2 ** 28].ne(0).sum()) for i in range(0, base.numel(), 2 ** 28))
            del base
            assert written == int(np.count_nonzero(got)) > 0, label   # no write outside the window, by either kernel
    print(f"BIGSTRIDES layers strided gradient {layout}: {'tile kernel' if layout == 'G-byte' else 'one-pixel fallback'} under auto; {_peak()}")


# ---- the in-place geometry backward ---------------------------------------------------------------------------------------------------------------
def _geometry_run(render, geo_host, name, strict):
    """(gradients w.r.t. dhw, ray_dir, eye_pos, z_dir on the host) of the loss over colour and depth through MPI(geometry_grad="all")."""
    gc, gd, _ = _upstream(name)
    geo = [_d(a).requires_grad_(True) for a in geo_host]
    mpi = _mpi(strict_order=strict, geometry_grad="all")
    out = render(mpi, geo)
    ((out["color"] * _d(gc)).sum() + (out["depth"] * _d(gd)).sum()).backward()
    torch.cuda.synchronize()
    _means_something({k: out[k].detach() for k in KEYS})
    assert mpi.layers_copies == 0
    return [g.grad.cpu().numpy() for g in geo]


def _geometry_reference(values, geo_host, name):
    gc, gd, _ = _upstream(name)
    return geometry_grads(values, *geo_host, np.arange(N), gc, gd, align_corners=True)


def _geometry_pair(run, view, copy, ref, strict, same_bits, label):
    """The strided and the contiguous run against float64 at `_check`'s bars (strict mode on white noise; x 10 in default mode on smooth inputs);
    same_bits: strided == copy bit for bit -- the pass has no atomics, so always in strict mode, and in default mode where the forward that saved T
    ran the same kernel on both."""
    from test_hip_geometry_grad import _check
    got, alone = run(view, strict), run(copy, strict)
    assert all(np.isfinite(g).all() for g in got), label
    _check(alone, ref, scale=1.0 if strict else 10.0)
    _check(got, ref, scale=1.0 if strict else 10.0)
    if same_bits:
        for a, b in zip(got, alone):
            assert np.array_equal(a, b), label


@functools.lru_cache(maxsize=None)
def _opaque_codes(D, smooth):
    """The code volumes of tests/test_hip_geometry_inplace.py (`_codes`: white noise, or `_smooth_rgba` rounded to codes) with exactly opaque texels:
    alpha 255 on the left half of the LAST plane (the forward's T is 1e-10 times what lies in front of it: in default mode a sweep started from the
    staged forward's T would be off by orders of magnitude there) and on a patch of plane 0, in front of everything."""
    from test_hip_geometry_inplace import _codes
    codes = _codes(161, (M, D, 4, big.HT, big.wt_of(1)), smooth=smooth).clone()
    codes[:, -1, 3, :, :big.wt_of(1) // 2] = 255
    codes[:, 0, 3, 8:16, 20:28] = 255
    return codes


U8_GEOMETRY = [("outer", "planar"), ("chanC", "planar"), ("outer", "channels_last"), ("rowC", "channels_last")]


@pytest.mark.parametrize("layout,storage", U8_GEOMETRY)
def test_geometry_backward_over_uint8_codes(layout, storage):
    """In default mode the uint8 entry drops the forward's transmittance where u8_variant_supports takes the tensors (`outer`) and uses it where it
    does not (chanC; rows of row_stride("rowC", 1) bytes): the strided and the contiguous launch may take different sides of that branch, so each is
    held to the float64 bar and equal bits are asserted in strict mode only."""
    from ml_gmpi_amd import dequantize_volume
    from ml_gmpi_amd.quantized import layers_as_volume
    D = big.planes_of(layout)
    geo_host = _geo("f32", D)
    codes = {strict: _opaque_codes(D, not strict) for strict in (True, False)}
    ref_of = {strict: _geometry_reference(dequantize_volume(q).numpy(), geo_host, "f32") for strict, q in codes.items()}   # (divided on the host)
    if storage == "planar":
        stride = big.strides(layout, 1, u8=True) + (1,)
        values, as_volume = codes, (lambda t: t)
    else:   # layers [M, D, HT, WT, 4] of 4-byte texels
        s_mpi, s_plane, s_row = (big.U8_S_MPI, big.U8_S_PLANE, 4 * big.PITCH) if layout == "outer" else (D * 4 * big.PITCH, 4 * big.PITCH, big.row_stride(layout, 1))
        stride = (s_mpi, s_plane, s_row, 4, 1)
        values, as_volume = {k: _layers_of(q) for k, q in codes.items()}, layers_as_volume
    staged = layout == "outer"
    run = lambda vol, strict: _geometry_run(lambda mpi, geo: mpi.render_views(vol, *geo, views_per_mpi=1, check_last_plane=False, want_transmittance=True),
                                            geo_host, "f32", strict)
    # (one window at a time: the strict pair, then the default pair)
    for strict in (True, False):
        with big.Window(values[strict], stride, fill=255) as w:
            vol, copy = as_volume(w.view), as_volume(w.copy)
            assert torch.equal(vol.cpu(), codes[strict])
            if strict:   # which side of the branch the strides choose: an explicit "lds" is refused where u8_variant_supports says no
                geo = tuple(_d(a) for a in geo_host)
                assert _forward(vol, geo, "lds", False)[1] == (not staged) and not _forward(copy, geo, "lds", False)[1], (layout, storage)
            _geometry_pair(run, vol, copy, ref_of[strict], strict, strict, ("geometry uint8", layout, storage, strict))
            del vol, copy
    print(f"BIGSTRIDES geometry uint8 {layout} {storage}: default mode {'walks the alpha texels (T_out dropped)' if staged else 'starts from the forward T'}; {_peak()}")


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("layout", ["L-outer", "L-rowA", "L-rowC"])
def test_geometry_backward_over_float_layers(layout, name):
    from test_hip_geometry_grad import _smooth_rgba
    D, es = big.planes_of(layout), _es(name)
    geo_host = _geo(name, D)
    smooth = torch.from_numpy(_smooth_rgba(162, (M, D, 4, big.HT, big.wt_of(es)))).to(DTYPES[name])
    planar = {True: _volume(name, D), False: smooth}
    ref_of = {strict: _geometry_reference(v.float().numpy(), geo_host, name) for strict, v in planar.items()}
    run = lambda lay, strict: _geometry_run(lambda mpi, geo: mpi.render_views_layers(lay, *geo, views_per_mpi=1, check_last_plane=False,
                                                                                     want_transmittance=True), geo_host, name, strict)
    for strict in (True, False):
        with _layer_window(_layers_of(planar[strict]), layout, es) as w:
            # (default mode: the staged forward saved T on both where it takes the strides)
            _geometry_pair(run, w.view, w.copy, ref_of[strict], strict, strict or layout in big.LAYERS_STAGED, ("geometry layers", layout, name, strict))
    print(f"BIGSTRIDES geometry layers {layout} {name}: {_peak()}")


# ---- the fused shaded render ----------------------------------------------------------------------------------------------------------------------
SHADED_CASES = [("volume", "outer"), ("volume", "chanB")] + [("shading", k) for k in big.SHADING_LAYOUTS]


@functools.lru_cache(maxsize=None)
def _shaded_scene(name, D):
    """Stored values, the shading image, the oracle's render of the shaded volume and the float64 / fp32 autograd gradients (host, shared)."""
    from test_hip_shaded_render import _reference_grads, make_shading, shaded_volume
    vol = _volume(name, D, seed=55).float()
    s = make_shading(55, vol)
    dhw, ray, eye, zd = _geo(name, D)
    orc = oracle.render(shaded_volume(vol, s).numpy(), dhw, ray, eye, zd, align_corners=True)
    gc, gd, gT = _upstream(name)
    refs = [_reference_grads(vol, s, dhw, ray, eye, zd, np.arange(N), gc, gd, gT, False, dt) for dt in (torch.float64, torch.float32)]
    return s, orc, refs


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("which,layout", SHADED_CASES)
def test_shaded_render_forward_and_backward(which, layout, name):
    """The volume on `outer` and `chanB` under a contiguous shading image, then a contiguous volume under the shading image on its three layouts.
    Forward: strict mode == oracle on apply_shading's volume and strided == copy, bit for bit; default mode: the staged forward takes every one of
    these (gmpi_render_shaded_supports on the launch's struct; `shaded_lds_fallbacks` stays 0), so the same kernel ran on both: equal bits, and the
    parity bars.  Backward (volume and shading): float64 autograd through apply_shading at tests/test_hip_shaded_render.py's bars, the tile twin
    ("auto") where its three guards hold -- `outer`, S-outer, S-rowA -- and the one-pixel twin elsewhere and under "gather"."""
    from ml_gmpi_amd import _lib, hip_mpi
    from test_hip_shaded_render import _compare
    from test_hip_shared_color import _half_ulp
    D = big.planes_of(layout) if which == "volume" else 3
    es, dtype = _es(name), DTYPES[name]
    vol_host = _volume(name, D, seed=55)
    s_host, orc, refs = _shaded_scene(name, D)
    geo = tuple(_d(a) for a in _geo(name, D))
    gc, gd, gT = (_d(a) for a in _upstream(name))
    wt = vol_host.shape[-1]
    kw = dict(views_per_mpi=1, check_last_plane=False, want_transmittance=True)

    def forward(vol, s, variant, strict):
        mpi = _mpi(variant=variant, strict_order=strict)
        with torch.no_grad():
            out = mpi.render_views_shaded(vol, s, *geo, **kw)
        torch.cuda.synchronize()
        assert int(out["status"][0].item()) == 0
        return {k: out[k].cpu() for k in KEYS}, mpi.shaded_lds_fallbacks

    def staged_takes(vol, s):
        mpi = _mpi()
        with torch.no_grad():
            fwd = mpi.render_views(vol, *geo, _shading=s, defer_status=True, _in_autograd_fn=True, **kw)
        mpi.raise_on_status(fwd["status"])
        p, keep, images = fwd["_bwd"]
        return int(_lib.load_library().gmpi_render_shaded_supports(ctypes.byref(p), ctypes.byref(hip_mpi._shading_struct(images[0]))))

    def backward(vol, s, variant):
        leaves = [vol.detach().requires_grad_(True), s.detach().requires_grad_(True)]
        out = _mpi(variant=variant).render_views_shaded(*leaves, *geo, **kw)
        ((out["color"] * gc).sum() + (out["depth"] * gd).sum() + (out["T"] * gT).sum()).backward()
        torch.cuda.synchronize()
        assert leaves[0].grad.dtype == dtype and leaves[1].grad.dtype == torch.float32
        return [x.grad.double().cpu().numpy() for x in leaves]

    if which == "volume":
        window = big.Window(vol_host, big.strides(layout, es) + (1,))
    else:
        s_mpi, s_row = big.shading_strides(layout, wt)
        window = big.Window(s_host, (s_mpi, big.HT * s_row, s_row, 1))
    with window as w:
        assert not w.view.is_contiguous()
        copies = (vol_host.to(DEV), s_host.to(DEV))
        strided = (w.view, copies[1]) if which == "volume" else (copies[0], w.view)
        assert staged_takes(*strided) == 1 and staged_takes(*copies) == 1, (which, layout, name)
        for variant in FORWARD_VARIANTS:
            for strict in (True, False):
                label = ("shaded", which, layout, name, variant, strict)
                got, fallbacks = forward(*strided, variant, strict)
                alone, _ = forward(*copies, variant, strict)
                assert fallbacks == 0, label
                for k in KEYS:
                    assert torch.equal(got[k], alone[k]), label + (k,)
                    if strict:
                        assert np.array_equal(alone[k].numpy(), orc[k]), label + (k, "contiguous copy against the oracle")
                if not strict:
                    _default_bars(alone, orc, label)
                _means_something(got)
        worst = {}
        for variant in ("auto", "gather"):
            label = ("shaded backward", which, layout, name, variant)
            got, alone = backward(*strided, variant), backward(*copies, variant)
            for g in got + alone:   # (`_compare` does not see a NaN: NaN > 0 is False)
                assert np.isfinite(g).all(), label
            _compare(alone, refs[0], refs[1], (dtype, torch.float32), f"shaded backward contiguous {name} {variant}")
            _compare(got, refs[0], refs[1], (dtype, torch.float32), f"shaded backward {which} {layout} {name} {variant}")
            # strided against contiguous, element by element: the module's 1e-5 of the largest gradient between two fp32 sums whose atomics came in
            # another order, and, for the 16-bit volume gradient, the half ulp by which the one rounding of each of the two can move it
            for what, a, b, dt in zip(("volume", "shading"), got, alone, (dtype, torch.float32)):
                bar = 1e-5 * float(np.abs(b).max()) + _half_ulp(a, dt) + _half_ulp(b, dt)
                assert float(np.abs(b).max()) > 0 and (np.abs(a - b) <= bar).all(), label + (what, "strided against contiguous", float(np.abs(a - b).max()))
                worst[variant, what] = float((np.abs(a - b) / bar).max())
        del strided
    # (the tile twin's guards -- a plane's offsets in 31 bits for the volume, its gradient and the shading image -- have no query in the library: the
    #  side each layout lies on is tests/_big_strides.py's FITS_32 and SHADING_TILE, which tests/test_big_strides_cpu.py holds to the guards' arithmetic)
    tile = layout in (big.FITS_32 if which == "volume" else big.SHADING_TILE)
    print(f"BIGSTRIDES shaded {which} {layout} {name}: staged forward ran; backward under auto: {'tile twin' if tile else 'one-pixel twin'} (no query: by "
          "the guard's arithmetic); strided vs contiguous as fractions of the bar: " + ", ".join(f"{k[0]} {k[1]} {v:.3f}" for k, v in worst.items())
          + f"; {_peak()}")
