"""The in-place backward of channels-last float layers on the device: `layers_backward="texel"` of `MPI.render_views_layers` /
`MPIRenderer.render_layers` (gmpi_mpi_render_layers_backward_launch: the texel instances of the one-pixel and of the 64 x 8 tile backward, which read
the saved layers where they lie and accumulate into one fp32 tensor of the layers' own order).

The reference of every comparison but one is the PLANAR backward on the planar copy of the same stored values -- `render_views(layers.permute(0, 1,
4, 2, 3).contiguous())` with the default backward: bit for bit where a launch is one tile per view and one view per MPI (both kernels stage the
same integer sums and every cell receives one flush atomic onto zero), to test_hip_backward.py's bar between two of the project's kernels,
max|diff| <= 1e-5 x the largest gradient, everywhere else.  One case goes against float64 autograd (tests/_torch_ref.py).  The tests that look at the
C entries and at the allocator are the ones a build that transposes the layers or their gradient fails.

The bar and 16-bit layers (`within_bar`): the kernels accumulate in fp32 and the bridge rounds the finished gradient to the layers' type ONCE.  Two
fp32 sums that differ in their last bit -- atomics that arrived in another order -- can round to neighbouring 16-bit numbers, 2^-8 (bf16) or 2^-11
(fp16) of the value apart: a hundred times the bar, with nothing wrong (seen on the first device run: 4.9e-4 of 3.98 for bf16).  So the reference of a
16-bit case is the planar backward over the fp32 upcast of the same stored values (an exact upcast: the 16-bit kernels compute with exactly these
fp32 taps), and the assertion is the bar itself on what a 16-bit output can tell: every element of the result is the rounding of SOME fp32 value
within 1e-5 x the largest gradient of the reference, i.e. it lies in [rn16(ref - tol), rn16(ref + tol)].  fp32 layers: the plain difference.
Run on the MI355X box:  python -m pytest tests/test_hip_float_layers_backward.py -m gpu"""
import functools
import warnings

import numpy as np
import pytest
import torch

from _torch_ref import torch_render
from test_hip_float_layers import DTYPES, DTYPE_IDS, camera_case, on_device, values
from test_hip_parity import _random_case

pytestmark = pytest.mark.gpu
BAR = 1e-5   # of the largest gradient: test_hip_backward.py's bar between two of the project's kernels
LAUNCH, SUPPORTS = "gmpi_mpi_render_layers_backward_launch", "gmpi_render_layers_backward_supports"
PLANAR_ENTRIES = ("gmpi_mpi_render_backward_launch", "gmpi_mpi_render_backward_ex_launch")


@functools.lru_cache(maxsize=None)
def cameras(seed, B, D, H, W):
    """camera_case, computed once per shape and left unchanged."""
    return camera_case(seed, B, D, H, W)


def upstream(seed, N, H, W):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(s, generator=g).cuda() for s in ((N, 3, H, W), (N, 1, H, W), (N, 1, H, W)))


def _loss(res, ups, uses_T):
    assert int(res["status"][0].item()) == 0                                         # the forward's status word
    return (res["color"] * ups[0]).sum() + (res["depth"] * ups[1]).sum() + ((res["T"] * ups[2]).sum() if uses_T else 0.0)


def _kw(view_to_mpi=None, views_per_mpi=1, out_pm1=False):
    v2m = None if view_to_mpi is None else torch.as_tensor(np.asarray(view_to_mpi), dtype=torch.int32).cuda()
    return dict(views_per_mpi=views_per_mpi, view_to_mpi=v2m, out_pm1=out_pm1, want_transmittance=True)


def texel_grad(lay_dev, geo, ups, *, ac=True, variant="auto", uses_T=False, mpi=None, **kw):
    """layers.grad through layers_backward="texel"; lay_dev keeps its strides."""
    from ml_gmpi_amd import MPI
    mpi = mpi or MPI(align_corners=ac, variant=variant, on_out_of_plane="raise")
    lay = lay_dev.detach().requires_grad_(True)
    assert lay.stride() == lay_dev.stride() and lay.data_ptr() == lay_dev.data_ptr()
    _loss(mpi.render_views_layers(lay, *geo, layers_backward="texel", **_kw(**kw)), ups, uses_T).backward()
    torch.cuda.synchronize()
    assert tuple(lay.grad.shape) == tuple(lay.shape) and lay.grad.dtype is lay.dtype
    return lay.grad


def planar_grad(lay_dev, geo, ups, *, ac=True, variant="auto", uses_T=False, upcast=True, **kw):
    """The planar backward on the planar copy, in the layers' order; upcast: of the stored values as fp32 (the unrounded gradient: see `within_bar`)."""
    from ml_gmpi_amd import MPI
    planar = lay_dev.detach().permute(0, 1, 4, 2, 3).contiguous()
    planar = (planar.float() if upcast else planar).requires_grad_(True)
    _loss(MPI(align_corners=ac, variant=variant, on_out_of_plane="raise").render_views(planar, *geo, **_kw(**kw)), ups, uses_T).backward()
    torch.cuda.synchronize()
    return planar.grad.permute(0, 1, 3, 4, 2)


def within_bar(got, ref, label):
    """got: the gradient in the layers' type; ref: the fp32 reference (module docstring)."""
    assert ref.dtype is torch.float32
    a, b = got.double(), ref.double()
    scale, err = float(b.abs().max()), float((a - b).abs().max())
    assert np.isfinite(scale) and scale > 0, (label, scale)
    tol = BAR * scale
    if got.dtype is torch.float32:
        print(f"{label}: max|grad diff| {err:.3e} of {scale:.3e} = {err / scale:.2e} (bar {BAR:g})")
        assert err <= tol, (label, err, scale)
        return
    lo, hi = (b - tol).to(got.dtype).double(), (b + tol).to(got.dtype).double()
    outside = int(((a < lo) | (a > hi)).sum())
    print(f"{label}: max|rounded grad - fp32 reference| {err:.3e} of {scale:.3e}; elements outside [rn(ref - tol), rn(ref + tol)], tol = {tol:.3e}: {outside}")
    assert outside == 0, (label, outside, err, scale)


@pytest.fixture
def entries(monkeypatch):
    """Spies on the C entries: every call of the texel launch (struct fields, gradient strides), the answers of its supports query, the names of the
    planar backward entries that were called."""
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    seen = dict(launch=[], supports=[], planar=[])
    real_launch, real_supports = getattr(lib, LAUNCH), getattr(lib, SUPPORTS)

    def launch(params, g_rgb, g_depth, g_T, grad, gst, stream):
        p = params._obj                                                              # (ctypes.byref(struct))
        seen["launch"].append(dict(rgba=int(p.rgba), rgba_stride=list(p.rgba_stride), dtype=int(p.rgba_dtype), variant=int(p.variant), grad=int(grad), gst=list(gst),
                                   g_T=g_T is not None))
        return real_launch(params, g_rgb, g_depth, g_T, grad, gst, stream)

    def supports(params, gst):
        rc = real_supports(params, gst)
        seen["supports"].append(int(rc))
        return rc
    monkeypatch.setattr(lib, LAUNCH, launch)
    monkeypatch.setattr(lib, SUPPORTS, supports)
    for name in PLANAR_ENTRIES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (seen["planar"].append(_name), _real(*a))[1])
    return seen


# 1. one tile per view, one view per MPI: the staged sums are integers and every cell receives one flush atomic onto zero -- equal bits
@pytest.mark.parametrize("uses_T", [False, True], ids=["noT", "T"])
@pytest.mark.parametrize("ac", [True, False], ids=["ac", "noac"])
@pytest.mark.parametrize("H,W", [(8, 64), (5, 50)])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_one_tile_has_the_planar_kernels_bits(entries, dtype, H, W, ac, uses_T):
    D = 5
    dhw, ray, eye, zd = cameras(401, 2, D, H, W)
    geo = tuple(t.cuda() for t in (dhw, ray, eye, zd))
    wide = values(401, (2, D, 40, 48, 4), dtype).cuda()
    lay = wide[:, :, :, 4:44]                                                        # rows padded: [2, 5, 40, 40, 4] inside [2, 5, 40, 48, 4]
    assert lay.stride(2) == 4 * 48
    ups = upstream(402, 2, H, W)
    got = texel_grad(lay, geo, ups, ac=ac, uses_T=uses_T)
    assert entries["supports"] == [1] and len(entries["launch"]) == 1 and entries["launch"][0]["g_T"] == uses_T and entries["planar"] == []
    ref = planar_grad(lay, geo, ups, ac=ac, uses_T=uses_T, upcast=False)                   # the same storage type: equal bits, rounded alike
    assert float(ref.float().abs().max()) > 0
    diff = float((got.float() - ref.float()).abs().max())
    print(f"{dtype} {H}x{W} ac={ac} T={uses_T}: max|diff| {diff:.3e}, cells that differ {int((got != ref).sum())}")
    assert torch.equal(got, ref)


# 2. many tiles (3 x 3 ragged ones of 64 x 8 pixels), views that share MPIs, the 96-plane table chunk: the project's bar
def _many_tiles(dtype, D, shared):
    H, W = 19, 130
    dhw, ray, eye, zd = cameras(403, 4, D, H, W)
    lay = values(404, (2, D, 36, 44, 4), dtype)
    if D > 3:
        lay[..., 3] *= 0.05                                                          # thin planes: the stack never goes opaque, every plane counts
    kw = dict(views_per_mpi=2) if shared == "vpm2" else dict(view_to_mpi=[0, 0, 1, 0])
    geo = tuple(t.cuda() for t in (dhw[:2].contiguous(), ray, eye, zd))
    return lay.cuda(), geo, upstream(405, 4, H, W), kw


@pytest.mark.parametrize("out_pm1", [False, True], ids=["01", "pm1"])
@pytest.mark.parametrize("shared", ["vpm2", "v2m"])
@pytest.mark.parametrize("D", [1, 3, 97])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_many_tiles_within_the_projects_bar(entries, dtype, D, shared, out_pm1):
    lay, geo, ups, kw = _many_tiles(dtype, D, shared)
    got = texel_grad(lay, geo, ups, uses_T=True, out_pm1=out_pm1, **kw)
    assert entries["supports"] == [1]
    within_bar(got, planar_grad(lay, geo, ups, uses_T=True, out_pm1=out_pm1, **kw), f"{dtype} D={D} {shared} pm1={out_pm1}")


# 3. against float64 autograd on the planar permutation: test_backward_matches_autograd's bar for its same-sized cases
def test_against_float64_autograd():
    B, D, S = 2, 4, 40
    rgba, dhw, ray, eye, zd = _random_case(seed=406, B=B, D=D, S=S)
    lay = rgba.permute(0, 1, 3, 4, 2).contiguous()
    ups = upstream(407, B, S, S)
    got = texel_grad(lay.cuda(), tuple(t.cuda() for t in (dhw, ray, eye, zd)), ups).cpu().numpy()
    vol = rgba.double().requires_grad_(True)
    color, depth = torch_render(vol, dhw.double(), ray.double(), eye.double(), zd.double(), np.arange(B), align_corners=True)
    ((color * ups[0].cpu().double()).sum() + (depth * ups[1].cpu().double()).sum()).backward()
    ref = vol.grad.permute(0, 1, 3, 4, 2).numpy()
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print(f"float64 autograd: max|grad diff| {err:.3e} of {scale:.3e}")
    assert err <= 2e-5 * scale + 1e-6, (err, scale)
    big = np.abs(ref) > 1e-3 * scale
    assert np.max(np.abs(got[big] - ref[big]) / np.abs(ref[big])) <= 2e-3


# 4. texture scale: a texture much coarser than the image (many taps per texel: the wide two-word cells) and one much finer (no box fits: the cold
#    scatter at texel addresses)
@pytest.mark.parametrize("S,T", [(64, 16), (16, 256)])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_texture_scale(dtype, S, T):
    _, dhw, ray, eye, zd = _random_case(seed=408, B=2, D=3, S=S, T=T)
    geo = tuple(t.cuda() for t in (dhw, ray, eye, zd))
    lay = values(408, (2, 3, T, T, 4), dtype).cuda()
    ups = upstream(409, 2, S, S)
    within_bar(texel_grad(lay, geo, ups, uses_T=True), planar_grad(lay, geo, ups, uses_T=True), f"{dtype} S={S} T={T}")


# 5. the one-pixel kernel: by choice (variant "gather") against the planar one-pixel backward, and as the fallback for layers one texel wide
@pytest.mark.parametrize("out_pm1", [False, True], ids=["01", "pm1"])
@pytest.mark.parametrize("shared", ["vpm2", "v2m"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_one_pixel_kernel_by_choice(entries, dtype, shared, out_pm1):
    from ml_gmpi_amd import _lib as L
    lay, geo, ups, kw = _many_tiles(dtype, 3, shared)
    got = texel_grad(lay, geo, ups, variant="gather", uses_T=True, out_pm1=out_pm1, **kw)
    assert entries["supports"] == [] and [c["variant"] for c in entries["launch"]] == [L.VARIANT_GATHER]
    within_bar(got, planar_grad(lay, geo, ups, variant="gather", uses_T=True, out_pm1=out_pm1, **kw), f"gather {dtype} {shared} pm1={out_pm1}")


def test_one_texel_wide_layers_fall_back_and_say_so(entries, monkeypatch):
    from ml_gmpi_amd import MPI, hip_mpi
    monkeypatch.setattr(hip_mpi, "_LAYERS_BACKWARD_WARNED", False)
    H, W = 19, 130
    dhw, ray, eye, zd = cameras(403, 4, 3, H, W)
    geo = tuple(t.cuda() for t in (dhw[:2].contiguous(), ray, eye, zd))
    lay = values(410, (2, 3, 36, 1, 4), torch.float32).cuda()
    ups = upstream(411, 4, H, W)
    mpi = MPI(on_out_of_plane="raise")
    with pytest.warns(RuntimeWarning, match="layers_backward_fallbacks") as rec:
        got = texel_grad(lay, geo, ups, mpi=mpi, uses_T=True, views_per_mpi=2)
    assert mpi.layers_backward_fallbacks == 1 and entries["supports"] == [0]
    assert len([w for w in rec if "layers_backward_fallbacks" in str(w.message)]) == 1
    with warnings.catch_warnings(record=True) as again:                              # once per process: the second launch counts and stays silent
        warnings.simplefilter("always")
        texel_grad(lay, geo, ups, mpi=mpi, uses_T=True, views_per_mpi=2)
    assert mpi.layers_backward_fallbacks == 2 and not [w for w in again if "layers_backward_fallbacks" in str(w.message)]
    within_bar(got, planar_grad(lay, geo, ups, uses_T=True, views_per_mpi=2), "Wt=1")


# 6. storage: texels at odd elements, an odd width, a slice along D, an expanded batch with a leaf behind it
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_strided_storage(entries, dtype):
    H, W = 19, 130
    M, D, Ht, Wt = 2, 3, 36, 44
    dhw, ray, eye, zd = cameras(403, 4, D, H, W)
    geo = tuple(t.cuda() for t in (dhw[:2].contiguous(), ray, eye, zd))
    ups = upstream(412, 4, H, W)
    kw = dict(uses_T=True, views_per_mpi=2)
    n = M * D * Ht * 48 * 4
    flat = values(413, (n + 8,), dtype)
    odd = flat[1:1 + n].view(M, D, Ht, 48, 4)[:, :, :, 2:2 + Wt]                     # a column slice whose first texel starts at element 9
    assert odd.storage_offset() % 2 == 1 and odd.stride(2) == 4 * 48
    dev = on_device(odd)
    assert dtype is torch.float32 or dev.data_ptr() % 4 == 2                         # 16-bit texels that are not dword aligned
    within_bar(texel_grad(dev, geo, ups, **kw), planar_grad(dev, geo, ups, **kw), f"{dtype} odd element base")
    narrow = values(414, (M, D, Ht, 23, 4), dtype).cuda()
    within_bar(texel_grad(narrow, geo, ups, **kw), planar_grad(narrow, geo, ups, **kw), f"{dtype} Wt=23")
    deep = values(415, (M, 2 * D, Ht, Wt, 4), dtype).cuda()[:, ::2]
    assert deep.stride(1) == 2 * Ht * Wt * 4
    within_bar(texel_grad(deep, geo, ups, **kw), planar_grad(deep, geo, ups, **kw), f"{dtype} every other plane")
    assert entries["supports"] == [1, 1, 1]
    # One MPI expanded to three (stride 0 on M), a leaf behind it: the leaf's gradient is the sum over the three.  The node returns the gradient of the
    # EXPANDED stack in the layers' type, autograd sums the three copies in that type: for 16-bit layers each copy is held to the bar on its own
    # (retain_grad) and the leaf to being their 16-bit sum (a relative 2^-8, one bf16 step; 1.2e-7: two fp16 subnormal steps); fp32: the leaf itself
    # against the planar path's leaf.
    from ml_gmpi_amd import MPI
    dhw3 = dhw[:1].expand(3, -1, -1).contiguous().cuda()
    geo3 = (dhw3,) + tuple(t[:3].contiguous().cuda() for t in (ray, eye, zd))
    ups3 = tuple(u[:3].contiguous() for u in ups)
    leaf = values(416, (1, D, Ht, Wt, 4), dtype).cuda().requires_grad_(True)
    lay = leaf.expand(3, -1, -1, -1, -1)
    lay.retain_grad()
    assert lay.stride(0) == 0
    _loss(MPI(on_out_of_plane="raise").render_views_layers(lay, *geo3, layers_backward="texel", **_kw()), ups3, True).backward()
    assert entries["launch"][-1]["rgba_stride"][0] == 0                              # read in place, stride 0 and all
    pleaf = leaf.detach().permute(0, 1, 4, 2, 3).contiguous().float().requires_grad_(True)
    pvol = pleaf.expand(3, -1, -1, -1, -1)
    pvol.retain_grad()
    _loss(MPI(on_out_of_plane="raise").render_views(pvol, *geo3, **_kw()), ups3, True).backward()
    torch.cuda.synchronize()
    assert tuple(leaf.grad.shape) == tuple(leaf.shape) and tuple(lay.grad.shape) == (3,) + tuple(leaf.shape[1:])
    within_bar(lay.grad, pvol.grad.permute(0, 1, 3, 4, 2).contiguous(), f"{dtype} expanded batch, per copy")
    if dtype is torch.float32:
        within_bar(leaf.grad, pleaf.grad.permute(0, 1, 3, 4, 2).contiguous(), f"{dtype} expanded batch, the leaf")
    else:
        total = lay.grad.float().sum(0, keepdim=True)
        off = (leaf.grad.float() - total).abs() - (2.0 ** -8 * total.abs() + 1.2e-7)
        print(f"{dtype} expanded batch, the leaf against the sum of its copies: largest excess over one 16-bit step {float(off.max()):.3e}")
        assert float(off.max()) <= 0


# 7. a ray field that is no pinhole camera's: footprints straddle and leave their tile's box (tests/_ray_field_cases.py); the planar one-pixel kernel
#    makes no pinhole assumption
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_a_ray_field_that_is_no_pinhole_cameras(entries, dtype):
    import _ray_field_cases as F
    case = F.scene("twin", "bulge")
    geo = tuple(torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in ("dhw", "ray", "eye", "zd"))
    M, D = case["dhw"].shape[:2]
    N, _, H, W = case["ray"].shape
    lay = values(417, (M, D, case["Ht"], case["Wt"], 4), dtype).cuda()
    ups = upstream(418, N, H, W)
    kw = dict(uses_T=True, view_to_mpi=[int(m) for m in case["v2m"]])
    got = texel_grad(lay, geo, ups, **kw)
    assert entries["supports"] == [1]
    within_bar(got, planar_grad(lay, geo, ups, variant="gather", **kw), f"{dtype} twin bulge")


# 8. what reaches the C entry: the layers themselves, a gradient in their order -- and no planar backward
@pytest.mark.parametrize("dtype,code", list(zip(DTYPES, (0, 1, 2))), ids=DTYPE_IDS)
def test_the_c_entry_sees_the_layers_and_a_gradient_in_their_order(entries, dtype, code):
    from ml_gmpi_amd.layers import layer_strides
    D, Ht, Wt, H, W = 3, 36, 44, 19, 130
    dhw, ray, eye, zd = cameras(403, 4, D, H, W)
    geo = tuple(t.cuda() for t in (dhw[:2].contiguous(), ray, eye, zd))
    lay = values(419, (2, D, Ht, 48, 4), dtype).cuda()[:, :, :, 3:3 + Wt]
    got = texel_grad(lay, geo, upstream(420, 4, H, W), views_per_mpi=2)
    assert entries["planar"] == [] and len(entries["launch"]) == 1
    call = entries["launch"][0]
    assert call["rgba"] == lay.data_ptr() and call["rgba_stride"] == list(layer_strides(lay)) == [D * Ht * 192, Ht * 192, 1, 192, 4] and call["dtype"] == code
    assert call["gst"] == [D * Ht * Wt * 4, Ht * Wt * 4, 1, 4 * Wt, 4]
    if dtype is torch.float32:
        assert call["grad"] == got.data_ptr()                                        # the filled tensor itself comes back


# 9. the allocator: one gradient volume at the peak, not two
def test_backward_holds_one_volume():
    from ml_gmpi_amd import MPI
    dev = torch.device("cuda:0")
    D, T, S = 8, 256, 64
    lay = torch.rand((1, D, T, T, 4), device=dev, generator=torch.Generator(device=dev).manual_seed(421)).requires_grad_(True)
    vol_bytes = lay.numel() * lay.element_size()
    assert vol_bytes == 8 * 2 ** 20
    _, dhw, ray, eye, zd = _random_case(seed=421, B=1, D=D, S=S, T=T)
    geo = tuple(t.cuda() for t in (dhw, ray, eye, zd))
    ups = upstream(422, 1, S, S)
    mpi = MPI(on_out_of_plane="raise")

    def peak(mode):
        _loss(mpi.render_views_layers(lay, *geo, want_transmittance=True, layers_backward=mode), ups, True).backward()   # anything cached exists
        lay.grad = None
        loss = _loss(mpi.render_views_layers(lay, *geo, want_transmittance=True, layers_backward=mode), ups, True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        loss.backward()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated(dev) - base
        assert torch.isfinite(lay.grad).all()
        lay.grad = None
        return rise
    texel, planar = peak("texel"), peak("planar")
    print(f"peak during backward above what was allocated before it: texel {texel} bytes, planar {planar} bytes (one volume: {vol_bytes})")
    assert texel <= 1.25 * vol_bytes, texel
    assert planar >= 2 * vol_bytes, planar                                           # what the keyword is for


# 10. the default is the planar path, untouched
def test_default_is_the_planar_path(entries):
    from ml_gmpi_amd import MPI
    H, W = 19, 130
    dhw, ray, eye, zd = cameras(403, 4, 3, H, W)
    geo = tuple(t.cuda() for t in (dhw[:2].contiguous(), ray, eye, zd))
    ups = upstream(423, 4, H, W)
    for uses_T, name in ((False, PLANAR_ENTRIES[0]), (True, PLANAR_ENTRIES[1])):
        del entries["planar"][:]
        lay = values(424, (2, 3, 36, 44, 4), torch.float32).cuda().requires_grad_(True)
        _loss(MPI(on_out_of_plane="raise").render_views_layers(lay, *geo, **_kw(views_per_mpi=2)), ups, uses_T).backward()
        assert name in entries["planar"] and entries["launch"] == [] and entries["supports"] == []
        explicit = values(424, (2, 3, 36, 44, 4), torch.float32).cuda().requires_grad_(True)
        _loss(MPI(on_out_of_plane="raise").render_views_layers(explicit, *geo, layers_backward="planar", **_kw(views_per_mpi=2)), ups, uses_T).backward()
        torch.cuda.synchronize()
        assert entries["launch"] == [] and float(lay.grad.abs().max()) > 0
        assert float((explicit.grad - lay.grad).abs().max()) <= BAR * float(lay.grad.abs().max())
