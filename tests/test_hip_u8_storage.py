"""uint8 RGBA volumes on the device (GMPI_DTYPE_U8: code c = c / 255): the gather kernel's instance for the type, the staged kernel of
render_u8.hip and AUTO, against the CPU oracle on `q.float() / 255`.

Bars (tests/test_hip_kernel_paths.py): strict-order mode BIT-EXACT in colour, depth and T; default mode colour <= 0.5e-5 on the [0, 1] scale
(1e-5 where the colour is written as 2 c - 1: the same error, doubled), depth and T <= 1e-5.  An explicit "lds" is never caught here: a case in
which the staged kernel is expected to run fails when the library refuses it."""
import os
import re

import numpy as np
import pytest
import torch

import oracle
from test_hip_parity import TOL, _random_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("gather", "lds", "auto")
KEYS = ("color", "depth", "T")


def _chunk():
    """Planes per table refill of the staged kernel (kUChunk, render_u8.hip)."""
    src = open(os.path.join(ROOT, "ml-gmpi_amd", "csrc", "render_u8.hip")).read()
    return int(re.search(r"constexpr int kUChunk = (\d+);", src).group(1))


def codes(seed, shape, every_code=True):
    """Seeded CPU codes; every code occurs in every channel (asserted: the dequantisation of all 256 is in every comparison)."""
    q = torch.randint(0, 256, tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    if every_code:
        for c in range(4):
            assert len(torch.unique(q[:, :, c])) == 256, c
    return q


def on_device(view):
    """A CPU tensor on the device with ITS strides and storage offset (a plain .cuda() would compact a strided view)."""
    base = view._base if view._base is not None else view
    assert base.is_contiguous()
    return base.cuda().as_strided(tuple(view.shape), view.stride(), view.storage_offset())


def hip(q, dhw, ray, eye, zd, *, variant, strict=False, ac=True, out_pm1=False, check_last=True, view_to_mpi=None, views_per_mpi=1):
    from ml_gmpi_amd import MPI
    mpi = MPI(align_corners=ac, variant=variant, strict_order=strict, on_out_of_plane="raise")
    qd = on_device(q)
    assert qd.dtype is torch.uint8 and qd.stride() == q.stride()
    v2m = None if view_to_mpi is None else torch.tensor(view_to_mpi, dtype=torch.int32).cuda()
    with torch.no_grad():
        out = mpi.render_views(qd, dhw.cuda(), ray.cuda(), eye.cuda(), zd.cuda(), views_per_mpi=views_per_mpi, view_to_mpi=v2m, check_last_plane=check_last,
                               want_transmittance=True, out_pm1=out_pm1)
    torch.cuda.synchronize()
    assert int(out["status"][0].item()) == 0
    return {k: out[k].cpu().numpy() for k in KEYS}


def reference(q, dhw, ray, eye, zd, ac=True, view_to_mpi=None):
    vol = q.float() / 255                                         # the contract: the correctly rounded fp32 quotient
    return oracle.render(vol, dhw, ray, eye, zd, view_to_mpi=None if view_to_mpi is None else np.asarray(view_to_mpi, dtype=np.int32), align_corners=ac, threads=True)


def check(q, dhw, ray, eye, zd, *, variants=VARIANTS, ac=True, out_pm1=False, check_last=True, view_to_mpi=None, views_per_mpi=1, label=""):
    """Strict mode == oracle bit for bit, default mode within the bars, for every variant (status word 0: asserted in hip())."""
    v2m = view_to_mpi if view_to_mpi is not None else (None if views_per_mpi == 1 else [n // views_per_mpi for n in range(ray.shape[0])])
    orc = reference(q, dhw, ray, eye, zd, ac=ac, view_to_mpi=v2m)
    want_c = 2 * orc["color"] - 1 if out_pm1 else orc["color"]    # (2 c - 1 is exact in fp32 for c in [0, 1])
    want = dict(color=want_c, depth=orc["depth"], T=orc["T"])
    kw = dict(ac=ac, out_pm1=out_pm1, check_last=check_last, view_to_mpi=view_to_mpi, views_per_mpi=views_per_mpi)
    res = {}
    for variant in variants:
        strict = hip(q, dhw, ray, eye, zd, variant=variant, strict=True, **kw)
        fast = hip(q, dhw, ray, eye, zd, variant=variant, **kw)
        errs = {k: float(np.abs(fast[k] - want[k]).max()) for k in KEYS}
        print(f"{label} {variant}: strict equal {[bool(np.array_equal(strict[k], want[k])) for k in KEYS]}, default max|err| {errs}")
        for k in KEYS:
            assert np.array_equal(strict[k], want[k]), (label, variant, k, float(np.abs(strict[k] - want[k]).max()))
        assert errs["color"] <= (TOL if out_pm1 else 0.5 * TOL) and errs["depth"] <= TOL and errs["T"] <= TOL, (label, variant, errs)
        res[variant] = strict
    return orc, res


# 1. tiles ragged against 32 x 16, both sampling conventions; the colour written both ways
@pytest.mark.parametrize("ac", [True, False])
def test_ragged_tiles_both_conventions(ac):
    _, dhw, ray, eye, zd = _random_case(seed=101, B=2, D=5, S=48)
    q = codes(101, (2, 5, 4, 48, 48))
    check(q, dhw, ray, eye, zd, ac=ac, out_pm1=ac, label=f"ac={ac}")


# 2. a non-square image
def test_non_square_image():
    """H = 24, W = 40.  `MPIRenderer.set_cam` asserts a square image (as the reference's does), so the camera it would build for 24 x 40 -- the same
    focal length formula, focal = w / (2 tan(fov / 2)) -- is set here directly; poses and rays then come from the renderer as in `_random_case`."""
    from ml_gmpi_amd.pinhole import gen_cam
    from ml_gmpi_amd.renderer import MPIRenderer, PRESETS
    B, D, H, W, T = 2, 4, 24, 40, 48
    kw = dict(PRESETS["FFHQ"])
    kw.update(n_mpi_planes=D, plan_spatial_enlarge_factor=1.001, plane_distances_sample_method="inverse", cam_sample_method="truncated_gaussian",
              mpi_align_corners=True, use_confined_volume=True, device=torch.device("cpu"))          # (_random_case's renderer)
    r = MPIRenderer(**kw)
    r.cam = gen_cam(h=H, w=W, f=W / (2 * np.tan(np.pi * r.cam_fov / 360)), ray_from_pix_center=True)   # set_cam(r.cam_fov, H, W) without the assertion
    r.render_h, r.render_w = H, W
    torch.manual_seed(102)
    cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    dhw = r.static_mpi_plane_dhws.reshape(1, -1, 3).expand(B, -1, -1).contiguous()
    ray = torch.cat(cam[3])
    assert tuple(ray.shape) == (B, 3, H, W)
    check(codes(102, (B, D, 4, T, T)), dhw, ray, torch.cat(cam[4]), torch.cat(cam[5]), label="24x40")


# 3. chunk boundaries of the plane table, with an alpha under which every plane counts
@pytest.mark.parametrize("D", ["1", "2", "chunk-1", "chunk", "chunk+2"])
def test_plane_table_chunks(D):
    from _visible import make_alpha
    from ml_gmpi_amd import quantize_volume
    chunk = _chunk()
    D = {"1": 1, "2": 2, "chunk-1": chunk - 1, "chunk": chunk, "chunk+2": chunk + 2}[D]
    rgba, dhw, ray, eye, zd = _random_case(seed=103, B=1, D=D, S=64, alpha="thin")
    q = codes(103 + D, (1, D, 4, 64, 64), every_code=False)
    # the thin law's alpha (codes 0 .. 255 * 3 / D: the lowest dozen at D = 64), plus any code at all in one texel out of D: the alpha channel covers
    # the code range and the stack still never goes opaque, so the planes behind a chunk boundary move the result
    thin_a = make_alpha(rgba, "thin")[:, :, 3]
    q[:, :, 3] = quantize_volume(thin_a)
    g = torch.Generator().manual_seed(7)
    spread = torch.rand(q[:, :, 3].shape, generator=g) < 1.0 / max(D, 4)          # a few texels per ray path take any code
    q[:, :, 3][spread] = torch.randint(0, 256, (int(spread.sum()),), generator=g, dtype=torch.uint8)
    if D >= 2:
        assert len(torch.unique(q[:, :, 3])) > 200
    orc, _ = check(q, dhw, ray, eye, zd, label=f"D={D}")
    if D > 2:
        assert float(orc["T"].min()) > 1e-6 and float(np.median(orc["T"])) > 1e-3       # every plane counts: the stack never goes opaque


# 4. exactly opaque and exactly empty planes
def test_alpha_codes_zero_and_255():
    _, dhw, ray, eye, zd = _random_case(seed=104, B=2, D=6, S=32)
    q = codes(104, (2, 6, 4, 32, 32), every_code=False)
    q[:, :, 3] = torch.where(q[:, :, 3] > 127, 255, 0).to(torch.uint8)
    orc, _ = check(q, dhw, ray, eye, zd, label="alpha 0/255")
    assert float(orc["T"].min()) <= 1e-10 * 1.0001                                   # the 1e-10 floor is reached


# 5. the 2-sigma pose corner: sheared boxes
def test_extreme_poses():
    _, dhw, ray, eye, zd = _random_case(seed=105, B=4, D=12, S=128, extreme=True)
    check(codes(105, (4, 12, 4, 128, 128)), dhw, ray, eye, zd, check_last=False, label="extreme")


# 6. texture much finer than the image: no box fits, whole chunks go through gather_plane;  7. texture much coarser: boxes of a few texels
@pytest.mark.parametrize("S,T", [(32, 256), (128, 32)])
def test_texture_scale(S, T):
    _, dhw, ray, eye, zd = _random_case(seed=106, B=2, D=4, S=S, T=T)
    check(codes(106, (2, 4, 4, T, T)), dhw, ray, eye, zd, label=f"S={S} T={T}")


# 8. views that share MPIs
def test_shared_and_ragged_views():
    _, dhw, ray, eye, zd = _random_case(seed=108, B=5, D=4, S=48)
    q = codes(108, (3, 4, 4, 48, 48))
    check(q[:1], dhw[:1], ray[:3], eye[:3], zd[:3], views_per_mpi=3, label="3 views of one MPI")
    check(q, dhw[:3], ray, eye, zd, view_to_mpi=[0, 0, 1, 2, 2], label="ragged view_to_mpi")
    check(q, dhw[:3], ray, eye, zd, view_to_mpi=[2, 0, 1, 0, 2], label="unordered view_to_mpi")


# 9. strided storage, all of it on the staged path
def test_strided_storage():
    _, dhw, ray, eye, zd = _random_case(seed=109, B=2, D=4, S=48)
    one = codes(109, (1, 4, 4, 48, 48))
    check(one.expand(2, -1, -1, -1, -1), dhw, ray, eye, zd, label="batch stride 0")
    five = codes(110, (2, 4, 5, 48, 48), every_code=False)
    check(five[:, :, :4], dhw, ray, eye, zd, label="4 of 5 channels")
    wide = codes(111, (2, 4, 4, 48, 96), every_code=False)
    check(wide[..., :48], dhw, ray, eye, zd, label="row pitch 96")
    check(wide[..., 48:], dhw, ray, eye, zd, label="row pitch 96, offset 48")


# 10. volumes the staged kernel cannot take: refused by name, rendered by AUTO through the gather kernel
@pytest.mark.parametrize("kind", ["Wt=50", "base+1"])
def test_unstageable_volumes(kind):
    from ml_gmpi_amd import GmpiError
    if kind == "Wt=50":
        _, dhw, ray, eye, zd = _random_case(seed=112, B=2, D=4, S=48, T=50)
        q = codes(112, (2, 4, 4, 50, 50))
    else:
        _, dhw, ray, eye, zd = _random_case(seed=113, B=2, D=4, S=48)
        store = codes(113, (2, 4, 4, 48, 52), every_code=False)
        q = store[..., 1:49]                                                  # every stride a multiple of 4, the base pointer is not
        assert q.storage_offset() == 1 and q.stride(3) % 4 == 0
    with pytest.raises(GmpiError, match="GMPI_E_VARIANT"):
        hip(q, dhw, ray, eye, zd, variant="lds")
    with pytest.raises(GmpiError, match="GMPI_E_VARIANT"):
        hip(q, dhw, ray, eye, zd, variant="lds", strict=True)
    _, res = check(q, dhw, ray, eye, zd, variants=("gather", "auto"), label=kind)
    for k in KEYS:
        assert np.array_equal(res["auto"][k], res["gather"][k]), k


@pytest.mark.parametrize("variant", ["wave", "band"])
def test_variants_that_are_not_built_for_the_type_are_refused(variant):
    from ml_gmpi_amd import GmpiError
    _, dhw, ray, eye, zd = _random_case(seed=114, B=1, D=2, S=32)
    with pytest.raises(GmpiError, match="GMPI_E_VARIANT"):
        hip(codes(114, (1, 2, 4, 32, 32), every_code=False), dhw, ray, eye, zd, variant=variant)


# 11. a camera that looks past the planes' edge: part of the image takes the zeros padding
def test_rays_past_the_edge_take_zeros_padding():
    _, dhw, ray, eye, zd = _random_case(seed=115, B=2, D=5, S=48)
    eye = eye.clone()
    eye[:, 0] += 0.5 * dhw[0, 0, 2]                                           # half a plane width to the side
    ix, iy = oracle.coords(dhw, ray, eye, 48, 48)
    out = (ix < -1) | (ix > 48)
    assert 0.1 < float(out.mean()) < 0.9                                      # part of the image samples nothing but padding, part does not
    orc, _ = check(codes(115, (2, 5, 4, 48, 48)), dhw, ray, eye, zd, check_last=False, label="past the edge")
    assert float((orc["T"] == 1.0).mean()) > 0.01                             # those pixels see no plane at all


# 12. plumbing: renderer and drivers take the codes and give what they give for the dequantised volume
def _close(a, b, bar, what):
    err = float((a.float() - b.float()).abs().max())
    print(f"{what}: max|u8 - f32| {err:.3e}")
    assert err <= bar, (what, err)


def test_renderer_and_drivers_take_uint8():
    from ml_gmpi_amd import ViewBatchDriver, dequantize_volume, flush_status, make_renderer
    dev = torch.device("cuda:0")
    D, S = 8, 64
    q = codes(116, (1, D, 4, S, S)).to(dev)
    f = dequantize_volume(q)
    r = make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise")
    outs = []
    for vol in (q, f):
        torch.manual_seed(3)
        outs.append(r.render(vol, S, S, want_transmittance=True))
    _close(outs[0][0], outs[1][0], TOL, "render colour [-1, 1]"), _close(outs[0][1], outs[1][1], TOL, "render depth"), _close(outs[0][4], outs[1][4], TOL, "render T")
    assert torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][3], outs[1][3])          # the same poses
    yaws, pitches = np.linspace(0.3, -0.3, 8), np.linspace(-0.1, 0.1, 8)
    drv = ViewBatchDriver(r, batch=3)
    a, b = (drv.render_path(vol, S, yaws, pitches, to_uint8=True, want_transmittance=True) for vol in (q, f))
    _close(a["rgb"], b["rgb"], TOL, "path colour [-1, 1]"), _close(a["depth"], b["depth"], TOL, "path depth"), _close(a["T"], b["T"], TOL, "path T")
    for k in ("img8", "dep8"):
        d = int((a[k].to(torch.int16) - b[k].to(torch.int16)).abs().max())
        print(f"path {k}: max code difference {d}")
        assert d <= 1, k
    q3 = codes(117, (3, D, 4, S, S)).to(dev)
    seeds = []
    for vol in (q3, dequantize_volume(q3)):
        torch.manual_seed(4)
        seeds.append(ViewBatchDriver(r, batch=2).render_seeds(vol, S, views_per_mpi=2))
    flush_status()
    assert seeds[0][0].shape == (6, 3, S, S)
    _close(seeds[0][0], seeds[1][0], TOL, "seeds colour [-1, 1]"), _close(seeds[0][1], seeds[1][1], TOL, "seeds depth")
    assert torch.equal(seeds[0][2], seeds[1][2])


# 13. errors
def test_errors():
    from ml_gmpi_amd import MPI, LightRenderer, compute_depth, make_renderer, rays_from_c2w
    dev = torch.device("cuda:0")
    D, S = 3, 32
    r = make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise", geometry_grad=True)
    q = codes(118, (1, D, 4, S, S), every_code=False).to(dev)
    with torch.no_grad():
        c2w0 = r.render(q, S, S, given_yaws=torch.zeros(1, 1), given_pitches=torch.zeros(1, 1))[2]      # (with grad off the codes render)
    c2w = c2w0.to(dev).float().clone().requires_grad_()
    ray, eye, zd = rays_from_c2w(r, c2w)
    assert ray.requires_grad
    info = dict(batch_yaws=torch.zeros(1, 1), batch_pitches=torch.zeros(1, 1), batch_tf_c2w=c2w.detach(), batch_ray_dir=ray, batch_eye_pos=eye, batch_z_dir=zd)
    with pytest.raises(NotImplementedError, match="dequantize_volume"):
        r.render(q, S, S, given_cam_infos=info)
    dhw = r.static_mpi_plane_dhws.reshape(1, -1, 3).to(dev)
    ray, eye, zd = ray.detach(), eye.detach(), zd.detach()
    mpi = MPI(on_out_of_plane="raise")
    with pytest.raises(TypeError, match="uint8"):
        mpi.render_views_shared(q[:, 0, :3], q[:, :, 3:], dhw, ray, eye, zd)
    with pytest.raises(TypeError, match="uint8"):
        compute_depth(q[:, :, 3:], dhw[0, :, :1])
    lr = LightRenderer.__new__(LightRenderer)
    with pytest.raises(TypeError, match="uint8"):
        lr.render(q, dhw[0], torch.zeros((D, S, S, 3), device=dev))
    out = MPI(geometry_grad=True, on_out_of_plane="raise").render_views(q, dhw, ray, eye, zd)           # nothing requires grad: renders
    assert torch.isfinite(out["color"]).all()
