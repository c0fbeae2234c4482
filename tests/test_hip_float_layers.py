"""Channels-last FLOAT layers on the device: `[M, D, Ht, Wt, 4]` fp32 / bf16 / fp16, read in place by the texel instances of the gather kernel and by
the staged kernel of render_layers.hip (`MPI.render_views_layers`, gmpi_mpi_render_layers_launch).

Every case is held against two references: `render_views(layers.permute(0, 1, 4, 2, 3).contiguous(), variant="gather")` -- the planar copy of the same
values through the planar gather kernel -- and the CPU oracle on that volume.  Strict-order mode: `array_equal` with both, for "gather", "lds" and
"auto".  Default mode: the gather instance `array_equal` with the planar gather kernel; the staged kernel within 1e-5 of the strict result (the
project's default-mode bar; the largest difference is printed).  The tests that look at the launch struct and at the allocator are the ones a build
that copies the layers into a planar volume first fails.
Run on the MI355X box:  python -m pytest tests/test_hip_float_layers.py -m gpu"""
import numpy as np
import pytest
import torch

import oracle
from test_hip_parity import TOL, _random_case

pytestmark = pytest.mark.gpu
KEYS = ("color", "depth", "T")
VARIANTS = ("gather", "lds", "auto")
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DTYPE_IDS = ["f32", "bf16", "f16"]
assert TOL == 1e-5


def values(seed, shape, dtype):
    """Seeded CPU layers in [0, 1) of the storage type (the cast is part of the data: every reference reads the stored values)."""
    return torch.rand(tuple(shape), generator=torch.Generator().manual_seed(seed)).to(dtype)


def on_device(view):
    """A CPU tensor on the device with ITS strides and storage offset (a plain .cuda() would compact a strided view)."""
    base = view._base if view._base is not None else view
    assert base.is_contiguous()
    return base.cuda().as_strided(tuple(view.shape), view.stride(), view.storage_offset())


def _kw(check_last, out_pm1, view_to_mpi, views_per_mpi):
    v2m = None if view_to_mpi is None else torch.tensor(view_to_mpi, dtype=torch.int32).cuda()
    return dict(views_per_mpi=views_per_mpi, view_to_mpi=v2m, check_last_plane=check_last, want_transmittance=True, out_pm1=out_pm1)


def _host(out):
    torch.cuda.synchronize()
    assert int(out["status"][0].item()) == 0
    return {k: out[k].cpu().numpy() for k in KEYS}


def render_layers(lay_dev, geo, *, variant, strict, ac=True, mpi=None, **kw):
    from ml_gmpi_amd import MPI
    mpi = mpi or MPI(align_corners=ac, strict_order=strict, on_out_of_plane="raise")
    with torch.no_grad():
        return _host(mpi.render_views_layers(lay_dev, *geo, variant=variant, **kw))


def render_planar(planar_dev, geo, *, strict, ac=True, **kw):
    from ml_gmpi_amd import MPI
    with torch.no_grad():
        return _host(MPI(align_corners=ac, variant="gather", strict_order=strict, on_out_of_plane="raise").render_views(planar_dev, *geo, **kw))


def check_layers(lay, dhw, ray, eye, zd, *, variants=VARIANTS, ac=True, out_pm1=False, check_last=True, view_to_mpi=None, views_per_mpi=1, label=""):
    """lay: CPU layers [M,D,Ht,Wt,4] (any strides the layout allows).  Returns (oracle dict, {variant: strict result})."""
    from ml_gmpi_amd import is_float_layers
    assert is_float_layers(lay), (label, lay.stride())
    lay_dev = on_device(lay)
    assert lay_dev.stride() == lay.stride() and lay_dev.dtype is lay.dtype
    planar = lay.permute(0, 1, 4, 2, 3).contiguous()
    geo = tuple(t.cuda() for t in (dhw, ray, eye, zd))
    kw = _kw(check_last, out_pm1, view_to_mpi, views_per_mpi)
    v2m = view_to_mpi if view_to_mpi is not None else (None if views_per_mpi == 1 else [n // views_per_mpi for n in range(ray.shape[0])])
    orc = oracle.render(planar.float(), dhw, ray, eye, zd, view_to_mpi=None if v2m is None else np.asarray(v2m, dtype=np.int32), align_corners=ac, threads=True)
    want = dict(color=2 * orc["color"] - 1 if out_pm1 else orc["color"], depth=orc["depth"], T=orc["T"])    # (2 c - 1 is exact in fp32 for c in [0, 1])
    ref = {s: render_planar(planar.cuda(), geo, strict=s, ac=ac, **kw) for s in (True, False)}
    res = {}
    for variant in variants:
        strict = render_layers(lay_dev, geo, variant=variant, strict=True, ac=ac, **kw)
        fast = render_layers(lay_dev, geo, variant=variant, strict=False, ac=ac, **kw)
        diff = {k: float(np.abs(fast[k] - strict[k]).max()) for k in KEYS}
        print(f"{label} {lay.dtype} {variant}: default vs strict max|diff| {diff}")
        for k in KEYS:
            assert np.array_equal(strict[k], ref[True][k]), (label, variant, "strict vs planar gather", k, float(np.abs(strict[k] - ref[True][k]).max()))
            assert np.array_equal(strict[k], want[k]), (label, variant, "strict vs oracle", k, float(np.abs(strict[k] - want[k]).max()))
            if variant == "gather":
                assert np.array_equal(fast[k], ref[False][k]), (label, "default gather vs planar gather", k, float(np.abs(fast[k] - ref[False][k]).max()))
            else:
                assert diff[k] <= TOL, (label, variant, "default vs strict", k, diff[k])
        res[variant] = strict
    return orc, res


def camera_case(seed, B, D, H, W, extreme=False):
    """dhw, ray, eye, zd of B seeded poses seen by an H x W pinhole camera (test_hip_u8_storage.py::test_non_square_image's construction)."""
    from ml_gmpi_amd.pinhole import gen_cam
    from ml_gmpi_amd.renderer import MPIRenderer, PRESETS
    kw = dict(PRESETS["FFHQ"])
    kw.update(n_mpi_planes=D, plan_spatial_enlarge_factor=1.001, plane_distances_sample_method="inverse", cam_sample_method="truncated_gaussian",
              mpi_align_corners=True, use_confined_volume=True, device=torch.device("cpu"))
    r = MPIRenderer(**kw)
    r.cam = gen_cam(h=H, w=W, f=W / (2 * np.tan(np.pi * r.cam_fov / 360)), ray_from_pix_center=True)
    r.render_h, r.render_w = H, W
    torch.manual_seed(seed)
    cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    dhw = r.static_mpi_plane_dhws.reshape(1, -1, 3).expand(B, -1, -1).contiguous()
    ray = torch.cat(cam[3])
    assert tuple(ray.shape) == (B, 3, H, W)
    return dhw, ray, torch.cat(cam[4]), torch.cat(cam[5])


# 1. tiles ragged against 32 x 16: 33 x 17 pixels (a second tile column and row of one pixel each) from a 24 x 20 texture, both conventions
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_ragged_tiles_both_conventions(dtype, ac):
    dhw, ray, eye, zd = camera_case(301, 2, 4, 17, 33)
    check_layers(values(301, (2, 4, 20, 24, 4), dtype), dhw, ray, eye, zd, ac=ac, out_pm1=ac, label=f"33x17 ac={ac}")


# 2. a non-square image over a non-square texture
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_non_square_image(dtype):
    dhw, ray, eye, zd = camera_case(302, 2, 3, 24, 40)
    check_layers(values(302, (2, 3, 40, 48, 4), dtype), dhw, ray, eye, zd, label="24x40")


# 3. the plane table: one plane, a few, and 65 -- a refill and the prefetch that must not cross it -- with thin alphas, so that every plane counts
@pytest.mark.parametrize("D", [1, 3, 65])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_plane_table_chunks(dtype, D):
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ml-gmpi_amd", "csrc", "render_layers.hip")).read()
    assert int(re.search(r"constexpr int kLChunk = (\d+);", src).group(1)) == 64
    rgba, dhw, ray, eye, zd = _random_case(seed=303, B=1, D=D, S=32, alpha="thin")
    lay = rgba.permute(0, 1, 3, 4, 2).contiguous().to(dtype)
    orc, _ = check_layers(lay, dhw, ray, eye, zd, label=f"D={D}")
    if D > 3:
        assert float(orc["T"].min()) > 1e-6 and float(np.median(orc["T"])) > 1e-3     # the stack never goes opaque: plane 64 moves the result


# 4. box paths: a texture much finer than the image (no box fits: every plane takes gather_plane over whole texels), one much coarser
@pytest.mark.parametrize("S,T", [(16, 256), (64, 16)])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_texture_scale(dtype, S, T):
    _, dhw, ray, eye, zd = _random_case(seed=304, B=2, D=3, S=S, T=T)
    check_layers(values(304, (2, 3, T, T, 4), dtype), dhw, ray, eye, zd, label=f"S={S} T={T}")


# 5. extreme poses, and rays past the edge: zeros padding on all four sides
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_extreme_poses_and_rays_past_every_edge(dtype):
    _, dhw, ray, eye, zd = _random_case(seed=305, B=4, D=4, S=48, extreme=True)
    check_layers(values(305, (4, 4, 48, 48, 4), dtype), dhw, ray, eye, zd, check_last=False, label="extreme")
    _, dhw, ray, eye, zd = _random_case(seed=115, B=4, D=4, S=48)
    eye = eye.clone()
    half_w, half_h = 0.5 * dhw[0, 0, 2], 0.5 * dhw[0, 0, 1]
    eye[0, 0] += half_w; eye[1, 0] -= half_w; eye[2, 1] += half_h; eye[3, 1] -= half_h       # noqa: E702  one view per side
    ix, iy = oracle.coords(dhw, ray, eye, 48, 48)
    ix, iy = np.asarray(ix), np.asarray(iy)
    for n, out in enumerate(((ix[0] > 48), (ix[1] < -1), (iy[2] > 48), (iy[3] < -1))):
        assert 0.1 < float(out.mean()) < 0.9, (n, float(out.mean()))
    orc, _ = check_layers(values(306, (4, 4, 48, 48, 4), dtype), dhw, ray, eye, zd, check_last=False, label="past the edge")
    assert float((orc["T"] == 1.0).mean()) > 0.01                                    # those pixels see no plane at all


# 6. views that share MPIs
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_shared_and_ragged_views(dtype):
    _, dhw, ray, eye, zd = _random_case(seed=307, B=5, D=3, S=40)
    lay = values(307, (3, 3, 40, 40, 4), dtype)
    check_layers(lay[:2], dhw[:2], ray[:4], eye[:4], zd[:4], views_per_mpi=2, label="2 views per MPI")
    check_layers(lay, dhw[:3], ray, eye, zd, view_to_mpi=[0, 0, 1, 2, 2], label="ragged view_to_mpi")


# 7. strided storage, all of it on the staged path (explicit "lds" is in every check)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_strided_storage(dtype):
    _, dhw, ray, eye, zd = _random_case(seed=308, B=2, D=4, S=40)
    M, D, T = 2, 4, 40
    wide = values(308, (M, D, T, 2 * T, 4), dtype)
    rows = wide[:, :, :, :T]
    assert rows.stride(2) == 8 * T
    check_layers(rows, dhw, ray, eye, zd, label="rows padded")
    one = wide[:, :, :, 1:1 + T]                                                     # the pointer moves by ONE texel: 16 / 8 bytes
    assert one.storage_offset() == 4
    check_layers(one, dhw, ray, eye, zd, label="columns from texel 1")
    deep = values(309, (M, 2 * D, T, T, 4), dtype)
    check_layers(deep[:, ::2], dhw, ray, eye, zd, label="every other plane")
    both = values(310, (1, D, T, T, 4), dtype).expand(M, -1, -1, -1, -1)
    assert both.stride(0) == 0
    check_layers(both, dhw, ray, eye, zd, label="MPI stride 0")


# 8. 16-bit layers the staged kernel cannot take (an odd width): AUTO is the gather kernel, "lds" falls back, counts and warns; fp32 stages them
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_odd_width(dtype, monkeypatch):
    from ml_gmpi_amd import MPI, hip_mpi, _lib as L
    monkeypatch.setattr(hip_mpi, "_LAYERS_LDS_WARNED", False)
    lib = L.load_library()
    seen = []
    real = lib.gmpi_mpi_render_layers_launch
    monkeypatch.setattr(lib, "gmpi_mpi_render_layers_launch", lambda params, *rest: (seen.append(int(params._obj.variant)), real(params, *rest))[1])
    dhw, ray, eye, zd = camera_case(311, 2, 3, 24, 40)
    lay = values(311, (2, 3, 30, 23, 4), dtype)
    _, res = check_layers(lay, dhw, ray, eye, zd, variants=("gather", "auto"), label="Wt=23")
    for k in KEYS:
        assert np.array_equal(res["auto"][k], res["gather"][k]), k
    geo = tuple(t.cuda() for t in (dhw, ray, eye, zd))
    mpi = MPI(variant="lds", strict_order=True, on_out_of_plane="raise")
    del seen[:]
    if dtype is torch.float32:                                                       # one texel per item: any width
        out = render_layers(on_device(lay), geo, variant=None, strict=True, mpi=mpi, want_transmittance=True)
        assert mpi.layers_lds_fallbacks == 0 and seen == [L.VARIANT_LDS]
    else:
        with pytest.warns(RuntimeWarning, match="layers_lds_fallbacks"):
            out = render_layers(on_device(lay), geo, variant=None, strict=True, mpi=mpi, want_transmittance=True)
        assert mpi.layers_lds_fallbacks == 1 and seen == [L.VARIANT_GATHER]
    for k in KEYS:
        assert np.array_equal(out[k], res["gather"][k]), k


# 9. ray fields that are no pinhole camera's: footprints leave their tile's box and take the per-lane gather (tests/_ray_field_cases.py)
@pytest.mark.parametrize("field", ["permuted", "bulge"])
@pytest.mark.parametrize("tex", ["twin", "coarse"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_ray_fields_that_are_no_pinhole_cameras(dtype, tex, field):
    import _ray_field_cases as F
    assert field in F.MOVED
    case = F.scene(tex, field)
    geo = tuple(torch.from_numpy(case[k]) for k in ("dhw", "ray", "eye", "zd"))
    M, D = case["dhw"].shape[:2]
    lay = values(312, (M, D, case["Ht"], case["Wt"], 4), dtype)
    check_layers(lay, *geo, check_last=False, label=f"{tex} {field}")


# 10. the range check
@pytest.mark.parametrize("bad", [1.5, float("nan")])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_range_check(dtype, bad):
    """A texel inside a sampled region sets STATUS_RGBA_RANGE in both kernels, whatever channel holds it; one outside every footprint (and outside every
    staged box: a frontal camera that sees the middle of a large texture) is caught by range_check="full" alone."""
    from ml_gmpi_amd import MPI, _lib as L
    S, T, D = 32, 128, 2
    _, dhw, ray, eye, zd = _random_case(seed=313, B=1, D=D, S=T, T=T)
    ray = ray[:, :, 48:80, 48:80].contiguous()                                       # the middle 32 x 32 pixels of a 128 x 128 camera: still a pinhole field
    ix, iy = oracle.coords(dhw, ray, eye, T, T)
    ix, iy = np.asarray(ix), np.asarray(iy)
    assert ix.min() > 24 and ix.max() < T - 24 and iy.min() > 24 and iy.max() < T - 24           # far from the corner texel below: no box reaches it
    geo = tuple(t.cuda() for t in (dhw, ray, eye, zd))
    cx, cy = int(ix[0, 1, S // 2, S // 2]), int(iy[0, 1, S // 2, S // 2])                     # plane 1, the centre pixel's north-west tap
    for variant in ("gather", "lds"):
        for chan in (0, 3):
            lay = values(313, (1, D, T, T, 4), dtype)
            lay[0, 1, cy, cx, chan] = bad
            mpi = MPI(variant=variant, on_out_of_plane="raise")
            with torch.no_grad():
                out = mpi.render_views_layers(lay.cuda(), *geo, defer_status=True)
            torch.cuda.synchronize()
            assert int(out["status"][0].item()) & L.STATUS_RGBA_RANGE, (variant, chan)
            out["status"].zero_()
            with torch.no_grad(), pytest.raises(AssertionError, match="range"):
                mpi.render_views_layers(lay.cuda(), *geo)
        lay = values(313, (1, D, T, T, 4), dtype)
        lay[0, 0, 1, 2, 1] = bad                                                     # a corner texel nobody samples or stages
        for check, caught in (("touched", False), ("off", False), ("full", True)):
            mpi = MPI(variant=variant, range_check=check, on_out_of_plane="raise")
            with torch.no_grad():
                out = mpi.render_views_layers(lay.cuda(), *geo, defer_status=True)
            torch.cuda.synchronize()
            assert bool(int(out["status"][0].item()) & L.STATUS_RGBA_RANGE) == caught, (variant, check)
            out["status"].zero_()


# 11. gradients: layers.grad against the gradient of render_views on the planar copy, to test_hip_backward.py's bar between two of the project's kernels
@pytest.mark.parametrize("uses_T", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_gradients_come_back_as_layers(dtype, uses_T):
    from ml_gmpi_amd import MPI
    _, dhw, ray, eye, zd = _random_case(seed=314, B=2, D=4, S=40)
    geo = tuple(t.cuda() for t in (dhw, ray, eye, zd))
    wide = values(314, (2, 4, 40, 48, 4), dtype).cuda()
    g = torch.Generator().manual_seed(315)
    gc, gd, gT = (torch.randn(s, generator=g).cuda() for s in ((2, 3, 40, 40), (2, 1, 40, 40), (2, 1, 40, 40)))

    def loss(res):
        return (res["color"] * gc).sum() + (res["depth"] * gd).sum() + ((res["T"] * gT).sum() if uses_T else 0.0)
    lay = wide[:, :, :, 4:44].detach().requires_grad_(True)                          # a view with padded rows: rendered in place
    res = MPI(on_out_of_plane="raise").render_views_layers(lay, *geo, want_transmittance=True)
    saved = [t for t in res["color"].grad_fn.saved_tensors if t.dim() == 5]
    assert len(saved) == 1 and saved[0].data_ptr() == lay.data_ptr() and saved[0].stride() == lay.stride()   # the layers, not a planar copy
    loss(res).backward()
    planar = lay.detach().permute(0, 1, 4, 2, 3).contiguous().requires_grad_(True)
    loss(MPI(on_out_of_plane="raise").render_views(planar, *geo, want_transmittance=True)).backward()
    assert tuple(lay.grad.shape) == tuple(lay.shape) and lay.grad.dtype is dtype
    a, b = lay.grad.float(), planar.grad.float().permute(0, 1, 3, 4, 2)
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    print(f"{dtype} uses_T={uses_T}: max|grad diff| {err:.3e} of {scale:.3e}")
    assert scale > 0 and err <= 1e-5 * scale, (err, scale)
    with pytest.raises(NotImplementedError):
        MPI(geometry_grad=True).render_views_layers(lay, geo[0].clone().requires_grad_(True), *geo[1:])


# 12. the launch struct, seen at the C entry, and the renderer / driver methods against the planar copy under the same seed
@pytest.fixture
def launches(monkeypatch):
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    real = lib.gmpi_mpi_render_layers_launch
    seen = []

    def spy(params, *rest):
        p = params._obj                                                              # (ctypes.byref(struct))
        seen.append((int(p.rgba), list(p.rgba_stride), int(p.rgba_dtype), int(p.M)))
        return real(params, *rest)
    monkeypatch.setattr(lib, "gmpi_mpi_render_layers_launch", spy)
    return seen


@pytest.mark.parametrize("dtype,code", list(zip(DTYPES, (0, 1, 2))), ids=DTYPE_IDS)
def test_renderer_and_drivers_hand_over_the_tensor_itself(launches, dtype, code):
    from ml_gmpi_amd import ViewBatchDriver, flush_status, make_renderer
    dev = torch.device("cuda:0")
    D, S = 6, 48
    r = make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise", strict_order=True)
    lay = values(316, (3, D, S, S, 4), dtype).to(dev)
    planar = lay.permute(0, 1, 4, 2, 3).contiguous()
    strides = [D * S * S * 4, S * S * 4, 1, 4 * S, 4]
    es = lay.element_size()
    outs = []
    for vol in (lay[:1], planar[:1]):
        del launches[:]
        torch.manual_seed(3)
        outs.append(r.render_layers(vol, S, S, want_transmittance=True) if vol.shape[-1] == 4 else r.render(vol, S, S, want_transmittance=True))
        if vol.shape[-1] == 4:
            assert launches == [(lay.data_ptr(), strides, code, 1)], launches
    for i in range(5):
        assert torch.equal(outs[0][i], outs[1][i]), i                                # colour, depth, c2w, angles, T: equal bits (strict order)
    yaws, pitches = np.linspace(0.3, -0.3, 5), np.linspace(-0.1, 0.1, 5)
    drv = ViewBatchDriver(r, batch=2)
    del launches[:]
    a = drv.render_path_layers(lay[1:2], S, yaws, pitches, want_transmittance=True)
    assert launches == [(lay.data_ptr() + es * lay.stride(0), strides, code, 1)] * 3, launches
    b = drv.render_path(planar[1:2], S, yaws, pitches, want_transmittance=True)
    for k in ("rgb", "depth", "T"):
        assert torch.equal(a[k], b[k]), k
    seeds = []
    for vol in (lay, planar):
        del launches[:]
        torch.manual_seed(4)
        d = ViewBatchDriver(r, batch=2)
        seeds.append(d.render_seeds_layers(vol, S, views_per_mpi=2) if vol is lay else d.render_seeds(vol, S, views_per_mpi=2))
        if vol is lay:
            assert launches == [(lay.data_ptr(), strides, code, 2), (lay.data_ptr() + 2 * es * lay.stride(0), strides, code, 1)], launches
    flush_status()
    assert seeds[0][0].shape == (6, 3, S, S)
    for i in range(4):
        assert torch.equal(seeds[0][i], seeds[1][i]), i


# 13. the allocator: a render of an 8 MiB stack of layers allocates its outputs and nothing like the volume
def test_a_render_allocates_no_copy_of_the_layers():
    from ml_gmpi_amd import MPI
    dev = torch.device("cuda:0")
    D, T, S = 8, 256, 64
    lay = torch.rand((1, D, T, T, 4), device=dev, generator=torch.Generator(device=dev).manual_seed(317))
    assert lay.numel() * lay.element_size() == 8 * 2 ** 20
    _, dhw, ray, eye, zd = _random_case(seed=317, B=1, D=D, S=S, T=T)
    geo = tuple(t.cuda() for t in (dhw, ray, eye, zd))
    mpi = MPI(on_out_of_plane="raise")

    def peak(call):
        with torch.no_grad():
            call()                                                                   # status words and anything cached exist
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        with torch.no_grad():
            out = call()
        torch.cuda.synchronize()
        assert torch.isfinite(out["color"]).all()
        return torch.cuda.max_memory_allocated(dev) - base
    rise = peak(lambda: mpi.render_views_layers(lay, *geo))
    copied = peak(lambda: mpi.render_views(lay.permute(0, 1, 4, 2, 3), *geo))
    print(f"peak above the inputs: in place {rise} bytes, render_views of the permuted view {copied} bytes")
    assert rise < 2 ** 20, rise
    assert copied >= 8 * 2 ** 20, copied                                             # what the layout's own entry is for
