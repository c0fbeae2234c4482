"""Every kernel that reads a texture, on strides past 2^31 bytes, 2^32 bytes and 2^31 elements (tests/_big_strides.py): small textures as windows of
one NaN-filled device buffer, on both sides of every host-side guard that keeps a kernel with 32-bit in-plane offsets off a launch it cannot address.

Every strided result is compared with the same call on a contiguous copy, and the contiguous copy with a reference that does not run the code under
test (the CPU oracle, float64 autograd).  A truncated or wrapped offset lands on NaN inside the allocation (the margins of _big_strides.py): the
range check raises, or the comparison fails.  Each test also asserts that view 1 differs from view 0 (the MPIs hold different noise: a dropped MPI
stride shows) and that T.max() > 1e-3 (the planes behind plane 0 count: a dropped plane stride shows).

Forward, what "equal" means: strict-order mode is bit-identical across all kernels, so strided == contiguous == oracle always.  In default mode two
different kernels differ in the last bits, so strided == contiguous bit for bit is asserted where the same kernel ran on both -- an explicit variant
that was not refused, and "auto" on the layouts every guard passes -- and the default-mode bars against the oracle (colour 0.5e-5, depth and T 1e-5)
where a staged kernel refused the strides and "auto" rendered instead.  "auto" on strides outside a guard may choose another kernel than for the
copy: its default-mode result must then be, bit for bit, that of one of the explicit variants that took the strided volume (`_forward_all`).

Gradients: under autograd they come back in the storage dtype, and two fp32 sums that agree to 1e-5 can round one 16-bit ulp apart.  So the volume
gradient and the image gradients of the two layouts are taken in fp32 through the C ABI for every dtype, at the fp32 bars (2e-5 max + 1e-6 against
float64, 1e-5 max strided against contiguous); the autograd path is run next to it where the storage is fp32, at the same bars."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
import _big_strides as big
import _transmittance_ref
from _geometry_ref import geometry_grads
from test_hip_edge_cases import _cam, _dhw
from test_hip_parity import TOL, variants

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SIZES = {"f32": (19, 130), "f16": (19, 130), "bf16": (11, 258)}   # test_hip_forward_frame.py: a partial tile behind a full one in every kernel
N = M = 2
KEYS = ("color", "depth", "T")
STAGED = ("lds", "wave", "band")


def _d(a):
    return a.to(DEV) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _es(name):
    return 4 if name == "f32" else 2


@functools.lru_cache(maxsize=None)
def _geo(name, D):
    """(dhw, ray, eye, zd) as numpy: cameras of test_hip_backward.py (tilt 0.3), one view per MPI, over planes 0.9 times the size of `_dhw`'s.
    Under `_dhw`'s own planes these cameras sample texel rows 1 .. HT - 2 only, and the row layouts put the row whose offset passes 2^31 or 2^32 LAST
    (31 s_row): a one-pixel kernel never formed that offset.  At 0.9 the front planes' rows 0 and HT - 1 and first and last columns carry weight
    (tests/test_big_strides_cpu.py shows it with the oracle), and no ray leaves the last plane.  Shared, never written to."""
    H, W = SIZES[name]
    ray, eye, zd = _cam(N, H, W, seed=6, tilt=0.3)
    dhw = _dhw(M, D)
    dhw[..., 1:] *= np.float32(0.9)
    return dhw, ray, eye, zd


@functools.lru_cache(maxsize=None)
def _volume(name, D, seed=51):
    """White noise [M, D, 4, HT, WT] in the storage dtype (host).  Shared, never written to."""
    v = oracle.synth_rgba(seed, (M, D, 4, big.HT, big.wt_of(_es(name))), bf16_round=name == "bf16")
    return torch.from_numpy(v).to(DTYPES[name])


@functools.lru_cache(maxsize=None)
def _upstream(name, seed=5):
    H, W = SIZES[name]
    g = np.random.default_rng(seed)
    return tuple(g.standard_normal((N, c, H, W)).astype(np.float32) for c in (3, 1, 1))


def _means_something(out):
    """View 1 differs from view 0, and the planes behind the first count."""
    c = out["color"]
    assert not torch.equal(torch.as_tensor(c[0]), torch.as_tensor(c[1]))
    assert float(torch.as_tensor(out["T"]).max()) > 1e-3


def _mpi(**kw):
    from ml_gmpi_amd import MPI
    return MPI(align_corners=True, range_check="touched", on_out_of_plane="raise", **kw)


def _forward(vol, geo, variant, strict):
    """(colour, depth, T on the host, refused): an explicit staged variant that answers GMPI_E_VARIANT is rendered by "auto", as test_hip_parity.hip_render does."""
    from ml_gmpi_amd import GmpiError
    mpi = _mpi(variant=variant, strict_order=strict)
    kw = dict(views_per_mpi=1, check_last_plane=False, want_transmittance=True)
    refused = False
    with torch.no_grad():
        try:
            out = mpi.render_views(vol, *geo, **kw)
        except GmpiError as e:
            if variant not in STAGED or "GMPI_E_VARIANT" not in str(e):
                raise
            refused = True
            mpi.variant = "auto"
            out = mpi.render_views(vol, *geo, **kw)
    torch.cuda.synchronize()
    assert int(out["status"][0].item()) == 0
    return {k: out[k].cpu() for k in KEYS}, refused


def _default_bars(got, orc, label):
    errs = {k: float(np.abs(got[k].numpy() - orc[k]).max()) for k in KEYS}
    assert errs["color"] <= 0.5 * TOL and errs["depth"] <= TOL and errs["T"] <= TOL, (label, errs)


def _forward_all(vol, copy, geo, orc, names, layout, label0):
    """Every variant of `names` ("auto" last), strict and default mode, on the strided volume and on its contiguous copy.
      * the copy is never refused; strides inside every guard (FITS_32) neither: the staged kernel really ran;
      * strict mode: copy == oracle and strided == copy, bit for bit, whatever kernel rendered;
      * default mode, an explicit variant that ran: strided == copy bit for bit (the same kernel on both);
      * default mode, a refused variant ("auto" rendered instead): the parity bars against the oracle;
      * default mode, "auto" on strides outside a guard: it may choose another kernel than for the copy, so its result must be, bit for bit,
        that of one of the explicit variants that took the strided volume (each of which equals the copy's) -- and inside the bars.
    Returns the variants that refused the strided volume."""
    assert names[-1] == "auto"
    refusals, ran = [], {}
    for variant in names:
        for strict in (True, False):
            got, refused = _forward(vol, geo, variant, strict)
            alone, refused_alone = _forward(copy, geo, variant, strict)
            label = label0 + (variant, strict)
            assert not refused_alone, label
            if layout in big.FITS_32:
                assert not refused, label
            if refused and strict:
                refusals.append(variant)
            for k in KEYS:
                assert torch.isfinite(got[k]).all(), label + (k,)
            if strict:
                for k in KEYS:
                    assert np.array_equal(alone[k].numpy(), orc[k]), label + (k, "contiguous copy against the oracle")
                    assert torch.equal(got[k], alone[k]), label + (k,)
            elif refused:
                _default_bars(got, orc, label)
            elif variant == "auto" and layout not in big.FITS_32:
                _default_bars(got, orc, label)
                assert any(all(torch.equal(got[k], r[k]) for k in KEYS) for r in ran.values()), label + ("equals no explicit variant", sorted(ran))
            else:
                for k in KEYS:
                    assert torch.equal(got[k], alone[k]), label + (k,)
                ran[variant] = got
            _means_something(got)
    return refusals


# ---- forward, float volumes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("layout", big.FLOAT_LAYOUTS)
def test_forward_every_variant(layout, name):
    big.need_memory()
    D, es = big.planes_of(layout), _es(name)
    vals = _volume(name, D)
    dhw, ray, eye, zd = _geo(name, D)
    orc = oracle.render(vals.float().numpy(), dhw, ray, eye, zd, align_corners=True)
    geo = tuple(_d(a) for a in (dhw, ray, eye, zd))
    names = [v for v in variants() if not (v == "band" and name == "f16")]   # (band x fp16 is refused whatever the strides)
    with big.Window(vals, big.strides(layout, es) + (1,)) as w:
        assert w.view.stride()[:4] == big.strides(layout, es) and not w.view.is_contiguous()
        refusals = _forward_all(w.view, w.copy, geo, orc, names, layout, (layout, name))
    print(f"BIGSTRIDES forward {layout} {name}: refused by {refusals or 'none'}; peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


# ---- forward, uint8 -----------------------------------------------------------------------------------------------------------------------------
U8_CASES = [("outer", "planar"), ("outer", "channels_last"), ("chanA", "planar"), ("chanB", "planar"), ("chanC", "planar")]


@pytest.mark.parametrize("layout,storage", U8_CASES)
def test_forward_uint8(layout, storage):
    """Codes c = c / 255: "gather", "lds" and "auto" against the oracle on q.float() / 255, strict mode bit for bit (test_hip_u8_storage.py).  The
    fill is 255 -- an opaque white texel: a read outside the window changes colour, depth and T."""
    from ml_gmpi_amd.quantized import layers_as_volume
    big.need_memory()
    D = big.planes_of(layout)
    wt = big.wt_of(1)
    q = torch.randint(0, 256, (M, D, 4, big.HT, wt), generator=torch.Generator().manual_seed(101), dtype=torch.uint8)
    dhw, ray, eye, zd = _geo("f32", D)
    orc = oracle.render((q.float() / 255).numpy(), dhw, ray, eye, zd, align_corners=True)
    geo = tuple(_d(a) for a in (dhw, ray, eye, zd))
    s_mpi, s_plane, s_chan, s_row = big.strides(layout, 1, u8=True)
    if storage == "planar":
        values, stride = q, (s_mpi, s_plane, s_chan, s_row, 1)
        as_volume = lambda t: t
    else:   # layers [M, D, HT, WT, 4]: texels of 4 bytes in rows of 4 PITCH bytes
        values, stride = q.permute(0, 1, 3, 4, 2).contiguous(), (s_mpi, s_plane, 4 * big.PITCH, 4, 1)
        as_volume = layers_as_volume
    with big.Window(values, stride, fill=255) as w:
        vol, copy = as_volume(w.view), as_volume(w.copy)
        assert vol.shape == q.shape and torch.equal(vol.cpu(), q)
        refusals = _forward_all(vol, copy, geo, orc, ["gather", "lds", "auto"], layout, (layout, storage))
        del vol, copy
    print(f"BIGSTRIDES uint8 {layout} {storage}: refused by {refusals or 'none'}; peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


# ---- backward, the volume -----------------------------------------------------------------------------------------------------------------------
PATHS = ("tile", "atomic", "pair")   # variant="auto" | variant="gather" (one pixel per lane, all atomics) | backward="gather" (the atomics-free pair)


def _abi_backward(vol, geo, name, path, grad=None):
    """The gradient w.r.t. the volume in fp32 through the C ABI (as test_gather_backward_falls_back_and_accumulates drives it): the forward of
    `render_views`, then gmpi_mpi_render_backward_ex_launch with upstream gradients on colour, depth and T.  path "pair" lends the workspace the
    query asks for and sets GMPI_FLAG_GRAD_OVERWRITE over a NaN-filled gradient when the query is non-zero, and is the tile path over zeros when it
    is 0 -- what `MPI(backward="gather")` does.  grad: write into this (zero-filled) tensor instead.  Returns (gradient on the host, workspace bytes)."""
    from ml_gmpi_amd import _lib
    lib = _lib.load_library()
    mpi = _mpi(variant="gather" if path == "atomic" else "auto")
    with torch.no_grad():
        fwd = mpi.render_views(vol, *geo, views_per_mpi=1, check_last_plane=False, want_transmittance=True, defer_status=True, _in_autograd_fn=True)
    mpi.raise_on_status(fwd["status"])   # a NaN the forward sampled raises here
    p, keep = fwd["_bwd"]
    p.rgb_out = p.depth_out = p.status = None
    gc, gd, gT = (_d(a) for a in _upstream(name))
    need = 0
    ws = None
    if path == "pair":
        need = int(lib.gmpi_render_backward_workspace_bytes(ctypes.byref(p)))
        if need:
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            p.workspace, p.workspace_bytes = ws.data_ptr(), need
            p.flags |= _lib.FLAG_GRAD_OVERWRITE
    if grad is None:
        grad = torch.full(tuple(vol.shape), float("nan") if need else 0.0, dtype=torch.float32, device=DEV)
    gs = (ctypes.c_int64 * 5)(*grad.stride())
    _lib.check(lib.gmpi_mpi_render_backward_ex_launch(ctypes.byref(p), gc.data_ptr(), gd.data_ptr(), gT.data_ptr(), grad.data_ptr(), gs,
                                                      torch.cuda.current_stream(DEV).cuda_stream), "backward")
    torch.cuda.synchronize()
    _means_something({k: fwd[k] for k in KEYS})
    del ws
    return grad.cpu().numpy(), need


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("layout", big.FLOAT_LAYOUTS)
def test_volume_backward_three_paths(layout, name):
    """Loss over colour, depth and T.  On the layouts outside the 32-bit guards the tile path takes the round-1 tile kernel (the `v1` test of
    launch_backward_t) and the pair must not take the launch: the workspace query answers 0."""
    big.need_memory()
    D, es = big.planes_of(layout), _es(name)
    vals = _volume(name, D)
    dhw, ray, eye, zd = _geo(name, D)
    gc, gd, gT = _upstream(name)
    ref = _transmittance_ref.grads(vals.float().numpy(), dhw, ray, eye, zd, np.arange(N), gc, gd, gT)[0]
    scale = float(np.abs(ref).max())
    assert scale > 0
    geo = tuple(_d(a) for a in (dhw, ray, eye, zd))
    worst = {}
    with big.Window(vals, big.strides(layout, es) + (1,)) as w:
        for path in PATHS:
            got, need = _abi_backward(w.view, geo, name, path)
            alone, need_alone = _abi_backward(w.copy, geo, name, path)
            label = (layout, name, path)
            assert np.isfinite(got).all() and np.isfinite(alone).all(), label
            e64, e64a = float(np.abs(got - ref).max()), float(np.abs(alone - ref).max())
            assert e64a <= 2e-5 * scale + 1e-6, label + ("contiguous copy against float64", e64a, scale)
            assert e64 <= 2e-5 * scale + 1e-6, label + ("against float64", e64, scale)
            esc = float(np.abs(got - alone).max())
            assert esc <= 1e-5 * float(np.abs(alone).max()), label + ("strided against contiguous", esc)
            if path == "pair":
                assert need_alone >= N * D * SIZES[name][0] * SIZES[name][1] * 24, label
                if layout in big.FITS_32:
                    assert need == need_alone, label              # the pair takes the launch ...
                    assert np.array_equal(got, alone), label      # ... and writes every cell once, in a fixed order
                else:
                    assert need == 0, label                       # a plane's byte offsets leave 32 bits: the atomic path
            worst[path] = (esc / (1e-5 * float(np.abs(alone).max())), e64 / (2e-5 * scale + 1e-6))
        if name == "f32":   # `MPI(backward="gather")` under autograd: the same routing through hip_mpi
            def through_autograd(v):
                vol = v.detach().requires_grad_(True)
                out = _mpi(backward="gather").render_views(vol, *geo, views_per_mpi=1, check_last_plane=False, want_transmittance=True)
                ((out["color"] * _d(gc)).sum() + (out["depth"] * _d(gd)).sum() + (out["T"] * _d(gT)).sum()).backward()
                return vol.grad.cpu().numpy()
            a, b = through_autograd(w.view), through_autograd(w.copy)
            assert np.abs(a - ref).max() <= 2e-5 * scale + 1e-6 and np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), (layout, "autograd")
            if layout in big.FITS_32:
                assert np.array_equal(a, b), (layout, "autograd")
    print(f"BIGSTRIDES backward {layout} {name}: (strided vs contiguous, strided vs float64) as fractions of their bars: "
          + ", ".join(f"{k} {v[0]:.3f} {v[1]:.3f}" for k, v in worst.items()) + f"; peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


def test_volume_backward_into_a_strided_gradient():
    """The gradient-side half of the `v1` test: a contiguous volume, the gradient written into a channel-major window (3 gs_chan 4 bytes past 2^32)
    of a zero-filled buffer.  The tile path must leave the 64 x 8 kernel (32-bit gradient offsets); the pair addresses the gradient in 64 bits.
    Nothing but the window's cells may be written."""
    big.need_memory()
    name, layout = "f32", "chanC"
    D = big.planes_of(layout)
    vals = _volume(name, D)
    geo = tuple(_d(a) for a in _geo(name, D))
    vol = vals.to(DEV)
    want = {path: _abi_backward(vol, geo, name, path)[0] for path in PATHS}
    for path in PATHS:
        with big.Window(torch.zeros(tuple(vals.shape)), big.strides(layout, 4) + (1,), fill=0.0) as w:
            assert 3 * w.view.stride(2) * 4 >= 2 ** 32
            got, need = _abi_backward(vol, geo, name, path, grad=w.view)
            assert need == 0 or path == "pair"
            scale = float(np.abs(want[path]).max())
            assert np.isfinite(got).all() and np.abs(got - want[path]).max() <= 1e-5 * scale, (path, float(np.abs(got - want[path]).max()), scale)
            base = w.view._base   # (counted in pieces: the comparison's temporary stays small next to the buffer)
            written = sum(int(base[i:i + 2 ** 28].ne(0).sum()) for i in range(0, base.numel(), 2 ** 28))
            del base
            assert written == int(np.count_nonzero(got)) > 0, path   # no write outside the window
        print(f"BIGSTRIDES strided gradient {path}: peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


# ---- geometry backward --------------------------------------------------------------------------------------------------------------------------
def _geometry_check(got, ref):
    from test_hip_geometry_grad import _check
    _check(got, ref)


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("layout", ["outer", "chanC"])
def test_geometry_backward(layout, name):
    big.need_memory()
    D, es = big.planes_of(layout), _es(name)
    vals = _volume(name, D)
    dhw, ray, eye, zd = _geo(name, D)
    gc, gd, _ = _upstream(name)
    ref = geometry_grads(vals.float().numpy(), dhw, ray, eye, zd, np.arange(N), gc, gd, align_corners=True)

    def run(vol):
        geo = [_d(a).requires_grad_(True) for a in (dhw, ray, eye, zd)]
        out = _mpi(strict_order=True, geometry_grad=True).render_views(vol, *geo, views_per_mpi=1, check_last_plane=False, want_transmittance=True)
        ((out["color"] * _d(gc)).sum() + (out["depth"] * _d(gd)).sum()).backward()
        _means_something({k: out[k].detach() for k in KEYS})
        return [g.grad.cpu().numpy() for g in geo]

    with big.Window(vals, big.strides(layout, es) + (1,)) as w:
        got, alone = run(w.view), run(w.copy)
    print(f"BIGSTRIDES geometry {layout} {name}: peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    _geometry_check(alone, ref)
    for a, b in zip(got, alone):
        assert np.array_equal(a, b), (layout, name)   # the pass has no atomics


# ---- the two image layouts ------------------------------------------------------------------------------------------------------------------------
IMAGE_CASES = [("first", "outer"), ("rgb", "outer"), ("background", "outer"), ("rgb", "chanC"), ("background", "chanC")]


def _image_window(which, layout, tensors, es):
    """Window over tensors[which] ("first": the alpha planes [M, D, 1, ..] / the depth image [M, 1, ..]); the others stay contiguous."""
    t = tensors[which]
    if t.dim() == 5:
        s_mpi, s_plane, s_chan, s_row = big.strides(layout, es, D=t.shape[1], C=1)
        return big.Window(t, (s_mpi, s_plane, s_chan, s_row, 1))
    return big.Window(t, big.image_strides(layout, es) + (1,))


def _abi_image_grads(mpi, fwd, entry, name, depth_struct=None):
    """The fp32 gradients of (rgb, the alpha planes / the depth image, background) through the C ABI, as `_LayoutRenderFunction.backward` calls the
    entry: `fwd` is the layout's forward under `_in_autograd_fn=True` (its parameter struct and operands), the upstream gradients are on colour,
    depth and T.  Nothing is rounded to a 16-bit storage dtype on the way: the bar is the fp32 one for every dtype."""
    from ml_gmpi_amd import hip_mpi
    mpi.raise_on_status(fwd["status"])   # a NaN the forward sampled raises here
    p, keep, (rgb, bg) = fwd["_bwd"]
    p.rgb_out = p.depth_out = p.status = None
    sc = hip_mpi._shared_color(rgb, bg)
    structs = (ctypes.byref(sc),) if depth_struct is None else (ctypes.byref(sc), ctypes.byref(depth_struct))
    image = (p.M, 3, p.Ht, p.Wt)
    mid_shape, mid_dims = ((p.M, p.D, 1, p.Ht, p.Wt), (0, 1, 3)) if depth_struct is None else ((p.M, 1, p.Ht, p.Wt), (0, 1, 2))
    grads = dict(rgb=torch.zeros(image, device=DEV), first=torch.zeros(mid_shape, device=DEV), background=torch.zeros(image, device=DEV))
    gc, gd, gT = (_d(a) for a in _upstream(name))
    hip_mpi._call(entry, DEV, ctypes.byref(p), *structs, gc.data_ptr(), gd.data_ptr(), gT.data_ptr(), *hip_mpi._ptr_stride(grads["rgb"], (0, 1, 2)),
                  *hip_mpi._ptr_stride(grads["first"], mid_dims), *hip_mpi._ptr_stride(grads["background"], (0, 1, 2)))
    torch.cuda.synchronize()
    _means_something({k: fwd[k] for k in KEYS})
    return {k: g.cpu() for k, g in grads.items()}


def _image_grads_close(got, alone, label):
    """Strided against contiguous: 1e-5 of the gradient's maximum (the adds of the two runs come in another order)."""
    for k in got:
        a, b = got[k].float().numpy(), alone[k].float().numpy()
        scale = float(np.abs(b).max())
        assert np.isfinite(a).all() and scale > 0, label + (k,)
        assert np.abs(a - b).max() <= 1e-5 * scale, label + (k, float(np.abs(a - b).max()), scale)


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("which,layout", IMAGE_CASES)
def test_shared_colour(which, layout, name):
    from ml_gmpi_amd import expand_shared_color
    big.need_memory()
    D, es = (big.planes_of(layout) if which == "first" else 3), _es(name)   # (the outer layout's MPI stride has room for two planes)
    v = _volume(name, D, seed=52)
    host = dict(rgb=v[:, 0, :3].contiguous(), first=v[:, :, 3:].contiguous(), background=v[:, -1, :3].contiguous())
    dhw, ray, eye, zd = _geo(name, D)
    gc, gd, gT = _upstream(name)
    orc = oracle.render(expand_shared_color(host["rgb"].float(), host["first"].float(), host["background"].float()).numpy(), dhw, ray, eye, zd, align_corners=True)
    geo = tuple(_d(a) for a in (dhw, ray, eye, zd))

    def forward(t, variant, strict):
        mpi = _mpi(variant=variant, strict_order=strict)
        with torch.no_grad():
            out = mpi.render_views_shared(t["rgb"], t["first"], *geo, background=t["background"], views_per_mpi=1, check_last_plane=False, want_transmittance=True)
        torch.cuda.synchronize()
        assert int(out["status"][0].item()) == 0
        return {k: out[k].cpu() for k in KEYS}, mpi.shared_lds_fallbacks

    def backward(t, variant, geometry=False):
        leaves = {k: x.detach().requires_grad_(True) for k, x in t.items()}
        g = [a.clone().requires_grad_(geometry) for a in geo]
        mpi = _mpi(variant=variant, geometry_grad="all" if geometry else False)
        out = mpi.render_views_shared(leaves["rgb"], leaves["first"], *g, background=leaves["background"], views_per_mpi=1, check_last_plane=False,
                                      want_transmittance=True)
        ((out["color"] * _d(gc)).sum() + (out["depth"] * _d(gd)).sum() + (out["T"] * _d(gT)).sum()).backward()
        return {k: x.grad.cpu() for k, x in leaves.items()}, [a.grad.cpu() for a in g] if geometry else None

    def backward_abi(t, variant):
        mpi = _mpi(variant=variant)
        with torch.no_grad():
            fwd = mpi.render_views_shared(t["rgb"], t["first"], *geo, background=t["background"], views_per_mpi=1, check_last_plane=False,
                                          want_transmittance=True, defer_status=True, _in_autograd_fn=True)
        return _abi_image_grads(mpi, fwd, "gmpi_mpi_render_shared_backward_launch", name)

    with _image_window(which, layout, host, es) as w:
        copies = {k: x.to(DEV) for k, x in host.items()}
        strided = dict(copies)
        strided[which] = w.view
        assert not w.view.is_contiguous()
        for variant in ("gather", "auto", "lds"):
            for strict in (True, False):
                label = ("shared colour", which, layout, name, variant, strict)
                got, fallbacks = forward(strided, variant, strict)
                alone, _ = forward(copies, variant, strict)
                # gmpi_render_shared_supports: every in-box offset of these cases fits (rows of PITCH texels, 64-bit channel and plane bases)
                assert fallbacks == 0, label
                for k in KEYS:
                    assert torch.equal(got[k], alone[k]), label + (k,)
                    if strict:
                        assert np.array_equal(alone[k].numpy(), orc[k]), label + (k, "contiguous copy against the oracle")
                _means_something(got)
        for variant in ("auto", "gather"):
            _image_grads_close(backward_abi(strided, variant), backward_abi(copies, variant), ("shared colour backward", which, layout, name, variant))
        if name == "f32":   # under autograd the gradients come back in the storage dtype: the same bar where that is fp32
            for variant in ("auto", "gather"):
                _image_grads_close(backward(strided, variant)[0], backward(copies, variant)[0], ("shared colour autograd", which, layout, variant))
            # ... and one geometry_grad="all" pass: no atomics, the same bits
            (_, ga), (_, gb) = backward(strided, "auto", geometry=True), backward(copies, "auto", geometry=True)
            for a, b in zip(ga, gb):
                assert torch.equal(a, b) and torch.isfinite(a).all() and float(a.abs().max()) > 0, ("shared colour geometry", which, layout)
        del strided
    print(f"BIGSTRIDES shared colour {which} {layout} {name}: peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("which,layout", IMAGE_CASES)
def test_depth_alpha(which, layout, name):
    from ml_gmpi_amd import expand_depth_alpha
    from test_hip_depth_alpha import _bounds, _depth_image
    big.need_memory()
    D, es = 3, _es(name)
    wt = big.wt_of(es)
    v = _volume(name, D, seed=53)
    depth, plane_z = _depth_image(M, 36, D, 4, DTYPES[name])   # smooth, no texel on a ramp bound; cropped to the window
    zb = _bounds(4)
    host = dict(rgb=v[:, 0, :3].contiguous(), first=depth[:, :, :big.HT, :wt].contiguous(), background=v[:, -1, :3].contiguous())
    dhw, ray, eye, zd = _geo(name, D)
    gc, gd, gT = _upstream(name)
    vol = expand_depth_alpha(host["rgb"].float(), host["first"].float(), plane_z, zb[0], zb[1], host["background"].float())
    orc = oracle.render(vol.numpy(), dhw, ray, eye, zd, align_corners=True)
    geo = tuple(_d(a) for a in (dhw, ray, eye, zd))
    pz = plane_z.to(DEV)

    def forward(t, how, strict):
        mpi = _mpi(strict_order=strict)
        with torch.no_grad():
            out = mpi.render_views_depth(t["rgb"], t["first"], pz, zb, *geo, background=t["background"], views_per_mpi=1, check_last_plane=False,
                                         want_transmittance=True, depth_forward=how)
        torch.cuda.synchronize()
        assert int(out["status"][0].item()) == 0
        return {k: out[k].cpu() for k in KEYS}, mpi.depth_window_fallbacks

    def backward(t, how, geometry=False):
        leaves = {k: x.detach().requires_grad_(True) for k, x in t.items()}
        g = [a.clone().requires_grad_(geometry) for a in geo]
        mpi = _mpi(geometry_grad="all" if geometry else False)
        out = mpi.render_views_depth(leaves["rgb"], leaves["first"], pz, zb, *g, background=leaves["background"], views_per_mpi=1,
                                     check_last_plane=False, want_transmittance=True, depth_backward=how)
        ((out["color"] * _d(gc)).sum() + (out["depth"] * _d(gd)).sum() + (out["T"] * _d(gT)).sum()).backward()
        return {k: x.grad.cpu() for k, x in leaves.items()}, [a.grad.cpu() for a in g] if geometry else None

    def backward_abi(t, how):
        from ml_gmpi_amd import hip_mpi
        mpi = _mpi()
        with torch.no_grad():
            fwd = mpi.render_views_depth(t["rgb"], t["first"], pz, zb, *geo, background=t["background"], views_per_mpi=1, check_last_plane=False,
                                         want_transmittance=True, depth_backward=how, defer_status=True, _in_autograd_fn=True)
        return _abi_image_grads(mpi, fwd, hip_mpi._DEPTH_BACKWARD_ENTRIES[how], name, depth_struct=hip_mpi._depth_alpha(pz, *zb))

    with _image_window(which, layout, host, es) as w:
        copies = {k: x.to(DEV) for k, x in host.items()}
        strided = dict(copies)
        strided[which] = w.view
        for how in ("pixel", "window"):
            for strict in (True, False):
                label = ("depth alpha", which, layout, name, how, strict)
                got, fallbacks = forward(strided, how, strict)
                alone, _ = forward(copies, how, strict)
                assert fallbacks == 0, label   # aligned bases and strides: the window kernel took the launch
                for k in KEYS:
                    assert torch.equal(got[k], alone[k]), label + (k,)
                    if strict:
                        assert np.array_equal(alone[k].numpy(), orc[k]), label + (k, "contiguous copy against the oracle")
                _means_something(got)
        for how in ("pixel", "tile"):
            _image_grads_close(backward_abi(strided, how), backward_abi(copies, how), ("depth alpha backward", which, layout, name, how))
        if name == "f32":
            for how in ("pixel", "tile"):
                _image_grads_close(backward(strided, how)[0], backward(copies, how)[0], ("depth alpha autograd", which, layout, how))
            (_, ga), (_, gb) = backward(strided, "pixel", geometry=True), backward(copies, "pixel", geometry=True)
            for a, b in zip(ga, gb):
                assert torch.equal(a, b) and torch.isfinite(a).all() and float(a.abs().max()) > 0, ("depth alpha geometry", which, layout)
        del strided
    print(f"BIGSTRIDES depth alpha {which} {layout} {name}: peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


# ---- shading --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DTYPES))
def test_shading_kernels_on_the_outer_layout(name):
    """`compute_depth` on the strided alpha view, the apply kernel and its backward on the strided volume, against their contiguous runs: all three
    are deterministic, so the same bits (test_hip_light_shapes.py has the callers and the references of the contiguous runs)."""
    from ml_gmpi_amd import _lib, light
    big.need_memory()
    lib = _lib.load_library()
    D, es = big.planes_of("outer"), _es(name)
    vals = _volume(name, D, seed=54)
    Ht, Wt = vals.shape[-2:]
    ds = _d(_dhw(1, D)[0, :, 0].copy())
    code = {"f32": _lib.DTYPE_F32, "bf16": _lib.DTYPE_BF16, "f16": _lib.DTYPE_F16}[name]
    rng = np.random.default_rng(21)
    s = _d(rng.uniform(0.25, 1.75, size=(M, Ht, Wt)).astype(np.float32))
    g = _d(rng.standard_normal((M, D, 4, Ht, Wt)).astype(np.float32))
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def run(vol):
        alpha = vol[:, :, 3:]
        with torch.no_grad():
            depth, T = light.compute_depth(alpha, ds, want_transmittance=True)
        a = alpha.detach().requires_grad_(True)
        d2, T2 = light.compute_depth(a, ds, want_transmittance=True)
        (d2.sum() + 0.5 * T2.sum()).backward()
        st = (ctypes.c_int64 * 5)(*vol.stride())
        out = torch.full((M, D, 4, Ht, Wt), float("nan"), dtype=torch.float32, device=DEV)
        _lib.check(lib.gmpi_light_apply_launch(vol.data_ptr(), code, st, s.data_ptr(), out.data_ptr(), M, D, Ht, Wt, stream), "apply")
        g_rgba = torch.full((M, D, 4, Ht, Wt), float("nan"), dtype=torch.float32, device=DEV)
        g_s = torch.full((M, Ht, Wt), float("nan"), dtype=torch.float32, device=DEV)
        _lib.check(lib.gmpi_light_apply_backward_launch(vol.data_ptr(), code, st, s.data_ptr(), g.data_ptr(), g_rgba.data_ptr(), g_s.data_ptr(), M, D,
                                                        Ht, Wt, stream), "apply backward")
        torch.cuda.synchronize()
        return dict(depth=depth.cpu(), T=T.cpu(), g_alpha=a.grad.float().cpu(), applied=out.cpu(), g_rgba=g_rgba.cpu(), g_shading=g_s.cpu())

    with big.Window(vals, big.strides("outer", es) + (1,)) as w:
        got, alone = run(w.view), run(w.copy)
    for k in got:
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], alone[k]), (name, k)
    assert not torch.equal(got["depth"][0], got["depth"][1]) and float(got["T"].max()) > 1e-3
    # the contiguous run against the definition: one fp32 product and a clamp (test_apply_entry_is_bit_exact)
    v = vals.float().numpy()
    want = v.copy()
    want[:, :, :3] = np.clip(v[:, :, :3] * s.cpu().numpy()[:, None, None], np.float32(0), np.float32(1))
    assert np.array_equal(alone["applied"].numpy(), want)
    d64, T64 = _transmittance_ref.alpha_depth(torch.from_numpy(v[:, :, 3:]).double(), ds.cpu().double())
    assert float((alone["depth"].double() - d64).abs().max()) <= 1e-5 and float((alone["T"].double() - T64).abs().max()) <= 1e-5
