"""Sparse uint8 MPIs on the device: the occupancy map (`build_occupancy`) against its definition, and the sparse instances of the staged uint8 kernel
(`occupancy=`, gmpi_mpi_render_u8_sparse_launch) against the dense launch of the same build.

"Equal" is `torch.equal` on colour, depth, T (as int32 views: NaNs compare by their bits) and the status words, between a render with `occupancy=` and
the same render without it, for the planar and the channels-last layout, in strict-order mode and in default mode -- skipping a box of alpha code 0
moves no bit.  The dense kernels' own accuracy is tests/test_hip_u8_storage.py's and tests/test_hip_u8_interleaved.py's."""
import functools
import warnings

import numpy as np
import pytest
import torch

import _u8_occupancy_cases as C

pytestmark = pytest.mark.gpu
KEYS = ("color", "depth", "T")
TILE_H = 16   # rows of the staged kernel's pixel tile (kUH, render_u8.hip); its width is gmpi_query(16)
LAYOUTS = ("planar", "channels_last")


def _dev(t):
    return t.cuda() if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t)).cuda()


def on_device(view):
    """A CPU tensor on the device with ITS strides and storage offset."""
    base = view._base if view._base is not None else view
    if not base.is_contiguous():   # (a permuted view of a contiguous tensor: rebuild over its own storage)
        base = torch.empty(0, dtype=view.dtype).set_(view.untyped_storage())
    return base.cuda().as_strided(tuple(view.shape), view.stride(), view.storage_offset())


def _store(q, layout):
    from ml_gmpi_amd import layers_as_volume
    return q.cuda() if layout == "planar" else layers_as_volume(q.cuda().permute(0, 1, 3, 4, 2).contiguous())


@functools.lru_cache(maxsize=None)
def camera(D, H, W, poses):
    """dhw [1,D,3], rays [N,3,H,W], eyes, z axes of the FFHQ renderer's camera for an H x W image at the (yaw, pitch) of `poses`; CPU, left unchanged."""
    from ml_gmpi_amd.pinhole import gen_cam
    from ml_gmpi_amd.renderer import MPIRenderer, PRESETS
    kw = dict(PRESETS["FFHQ"])
    kw.update(n_mpi_planes=D, plan_spatial_enlarge_factor=1.001, plane_distances_sample_method="inverse", cam_sample_method="truncated_gaussian",
              mpi_align_corners=True, use_confined_volume=True, device=torch.device("cpu"))
    r = MPIRenderer(**kw)
    r.cam = gen_cam(h=H, w=W, f=W / (2 * np.tan(np.pi * r.cam_fov / 360)), ray_from_pix_center=True)   # (set_cam asserts a square image)
    r.render_h, r.render_w = H, W
    n = len(poses)
    cam = r.sample_cam_poses(n, 0, 0, 0, 0, False, given_yaws=torch.tensor([[float(y)] for y, _ in poses]), given_pitches=torch.tensor([[float(p)] for _, p in poses]))
    dhw = r.static_mpi_plane_dhws.reshape(1, -1, 3).float().contiguous()
    return dhw, torch.cat(cam[3]).contiguous(), torch.cat(cam[4]).contiguous(), torch.cat(cam[5]).contiguous()


def render(q, dhw, ray, eye, zd, *, occupancy=None, strict=False, variant="auto", mpi=None, **kw):
    from ml_gmpi_amd import MPI
    mpi = mpi or MPI(align_corners=True, variant=variant, strict_order=strict)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    occ = {} if occupancy is None else {"occupancy": occupancy}
    with torch.no_grad():
        out = mpi.render_views(q, _dev(dhw), _dev(ray), _dev(eye), _dev(zd), check_last_plane=True, want_transmittance=True, status=status, defer_status=True,
                               **occ, **kw)
    assert mpi.occupancy_fallbacks == 0
    return out


def assert_equal(a, b, label=""):
    for k in KEYS:
        assert a[k].dtype is torch.float32 and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (label, k, int((a[k].view(torch.int32) != b[k].view(torch.int32)).sum()))
    assert torch.equal(a["status"], b["status"]), (label, a["status"].tolist(), b["status"].tolist())


def stats_of(occ):
    torch.cuda.synchronize()
    return [int(v) for v in occ.stats.cpu().to(torch.int64).tolist()]


def n_tiles(H, W, N=1):
    from ml_gmpi_amd import load_library
    tw = load_library().gmpi_query(16)
    return N * (-(-W // tw)) * (-(-H // TILE_H))


def compare(q_cpu, dhw, ray, eye, zd, label, layouts=LAYOUTS, modes=(False, True), **kw):
    """Sparse == dense for every layout and mode; returns [(skipped, staged)] of the runs."""
    from ml_gmpi_amd import build_occupancy
    counts = []
    for layout in layouts:
        q = _store(q_cpu, layout)
        occ = build_occupancy(q, stats=True)
        for strict in modes:
            dense = render(q, dhw, ray, eye, zd, strict=strict, **kw)
            occ.stats.zero_()
            sparse = render(q, dhw, ray, eye, zd, strict=strict, occupancy=occ, **kw)
            assert_equal(sparse, dense, (label, layout, strict))
            counts.append(tuple(stats_of(occ)))
    return counts


# 1. the map
@pytest.mark.parametrize("shape", [(16, 16), (20, 36), (33, 68), (1, 4)])
def test_map_is_the_reference(shape):
    from ml_gmpi_amd import build_occupancy, occupancy_reference
    Ht, Wt = shape
    for i, q in enumerate([C.sparse_codes(11 + Ht, (2, 3, 4, Ht, Wt))] + C.corner_volumes(2, 3, Ht, Wt)):
        for name, v in C.stridings(q).items():
            vd = on_device(v)
            assert vd.stride() == v.stride() and torch.equal(vd.cpu(), v)
            occ = build_occupancy(vd)
            want = C.brute_force_map(v)
            assert occ.block == 16 and occ.stats is None and occ.map.dtype is torch.uint8 and occ.map.is_contiguous()
            assert torch.equal(occ.map.cpu(), want), (shape, i, name)
            assert torch.equal(occupancy_reference(vd).cpu(), want), (shape, i, name)
    st = build_occupancy(on_device(q), stats=True).stats
    assert st.dtype is torch.uint32 and tuple(st.shape) == (2,) and stats_of(build_occupancy(on_device(q), stats=True)) == [0, 0]


# 2. a lone texel at every position of the texture: every box edge and every block edge is crossed somewhere in the sweep
@pytest.mark.parametrize("yaw", [0.0, 0.5])
def test_lone_texel_at_every_position(yaw):
    Ht, Wt, H, W = 24, 40, 32, 64
    M = Ht * Wt
    g = torch.Generator().manual_seed(21)
    q = torch.randint(0, 256, (M, 2, 4, Ht, Wt), generator=g, dtype=torch.uint8)
    q[:, 0, 3] = 0
    q[:, 0, 3].reshape(M, Ht * Wt)[torch.arange(M), torch.arange(M)] = 255
    q[:, 1, 3] = 255
    assert int((q[:, 0, 3] != 0).sum()) == M and int(q[37, 0, 3, 0, 37]) == 255
    dhw, ray, eye, zd = camera(2, H, W, ((yaw, 0.0),))
    dhw, ray, eye, zd = dhw.expand(M, -1, -1).contiguous(), ray.expand(M, -1, -1, -1).contiguous(), eye.expand(M, -1).contiguous(), zd.expand(M, -1).contiguous()
    counts = compare(q, dhw, ray, eye, zd, f"lone texel, yaw {yaw}")
    total = n_tiles(H, W, M) * 2
    for skipped, staged in counts:   # plane 1 is never empty; plane 0 is empty for the tiles whose box misses the texel
        assert 0 < skipped < total // 2 and skipped + staged == total, (skipped, staged, total)


# 3. counts at the extremes
def test_counts_at_the_extremes():
    from ml_gmpi_amd import build_occupancy
    H, W, D = 48, 64, 5
    dhw, ray, eye, zd = camera(D, H, W, ((0.0, 0.0),))
    tiles = n_tiles(H, W)
    assert tiles == 6
    g = torch.Generator().manual_seed(31)
    base = torch.randint(0, 256, (1, D, 4, H, W), generator=g, dtype=torch.uint8)
    empty_front = base.clone()
    empty_front[:, :4, 3] = 0
    empty_front[:, 4, 3] = 255
    full = base.clone()
    full[:, :, 3] = torch.randint(1, 256, (1, D, H, W), generator=g, dtype=torch.uint8)
    for q_cpu, want in ((empty_front, [tiles * 4, tiles]), (full, [0, tiles * 5])):
        for layout in LAYOUTS:
            q = _store(q_cpu, layout)
            occ = build_occupancy(q, stats=True)
            for strict in (False, True):
                occ.stats.zero_()
                sparse = render(q, dhw, ray, eye, zd, strict=strict, occupancy=occ)
                assert_equal(sparse, render(q, dhw, ray, eye, zd, strict=strict), (layout, strict))
                assert stats_of(occ) == want and sum(want) == tiles * D, (layout, strict, stats_of(occ), want)
    # the counters accumulate over launches
    render(q, dhw, ray, eye, zd, occupancy=occ)
    assert stats_of(occ) == [0, 2 * tiles * 5]


# 4. shell and ramp volumes: a plane table that is refilled (D = 96), three poses, and a texture whose boxes do not fit
POSES = ((0.0, 0.0), (0.5, 0.0), (0.0, 0.3))


@pytest.mark.parametrize("kind", ["shell", "ramp"])
@pytest.mark.parametrize("D", [8, 96])
def test_shell_and_ramp_volumes(kind, D):
    S = 64
    dhw, ray, eye, zd = camera(D, S, S, POSES)
    counts = compare(C.volume(kind, S, D), dhw, ray, eye, zd, f"{kind} {S}^2 x {D}", views_per_mpi=len(POSES))
    total = n_tiles(S, S, len(POSES)) * D
    for skipped, staged in counts:
        print(f"{kind} {S}^2 x {D}: skipped {skipped} staged {staged} of {total}")
        assert 0 < skipped < total and skipped + staged == total, (skipped, staged, total)


@pytest.mark.parametrize("kind", ["shell", "ramp"])
def test_texture_finer_than_the_image_mixes_the_gather_path_in(kind):
    D, S, T = 8, 64, 128
    dhw, ray, eye, zd = camera(D, S, S, POSES)
    counts = compare(C.volume(kind, T, D), dhw, ray, eye, zd, f"{kind} {T}^2 at {S}^2", views_per_mpi=len(POSES))
    total = n_tiles(S, S, len(POSES)) * D
    for skipped, staged in counts:
        print(f"{kind} {T}^2 at {S}^2: skipped {skipped} staged {staged} of {total}")
        assert skipped + staged <= total


# 5. ray fields that are no pinhole camera's
@pytest.mark.parametrize("field", ["permuted", "bulge"])
def test_ray_fields_that_are_no_pinhole_cameras(field):
    import _ray_field_cases as R
    D, S = 8, 64
    dhw, ray, eye, zd = camera(D, S, S, POSES)
    moved = torch.from_numpy(R.apply(field, ray.numpy()))
    assert not torch.equal(moved, ray)
    compare(C.volume("shell", S, D), dhw, moved, eye, zd, field, views_per_mpi=len(POSES))


# 6. non-finite rays
@pytest.mark.parametrize("what", ["rz0_row", "inf", "nan"])
def test_non_finite_rays(what):
    D, S = 8, 64
    dhw, ray, eye, zd = camera(D, S, S, POSES)
    ray = ray.clone()
    if what == "rz0_row":
        ray[:, 2, 21, :] = 0.0
    elif what == "inf":
        ray[0, 0, 9, 13] = float("inf")
        ray[1, 2, 40, 50] = float("-inf")
    else:
        ray[0, 1, 9, 13] = float("nan")
        ray[2, 2, 33, 2] = float("nan")
    counts = compare(C.volume("shell", S, D), dhw, ray, eye, zd, what, views_per_mpi=len(POSES))
    assert all(skipped > 0 for skipped, _ in counts)
    out = render(C.volume("shell", S, D).cuda(), dhw, ray, eye, zd, views_per_mpi=len(POSES))
    assert not bool(torch.isfinite(out["depth"]).all()) or what == "inf"   # (the poison reaches an output: the comparison is not vacuous)


# 7. views and strides
def test_shuffled_views():
    D, S, M = 8, 64, 3
    q_cpu = torch.cat([C.volume("shell", S, D, seed=s) for s in range(M)])
    q_cpu[1] = C.volume("ramp", S, D, seed=5)[0]
    poses = POSES + ((-0.4, 0.1), (0.2, -0.2))
    dhw, ray, eye, zd = camera(D, S, S, poses)
    v2m = torch.tensor([2, 0, 1, 1, 0], dtype=torch.int32).cuda()
    compare(q_cpu, dhw.expand(M, -1, -1).contiguous(), ray, eye, zd, "shuffled", view_to_mpi=v2m)


def test_slice_of_a_larger_batch_with_padded_rows():
    from ml_gmpi_amd import build_occupancy
    D, S = 8, 64
    big = torch.full((4, D, 4, S, S + 8), 255, dtype=torch.uint8)   # (whatever lies in the padding is never read: codes 255)
    for m in range(4):
        big[m, :, :, :, 4:4 + S] = C.volume("shell", S, D, seed=10 + m)[0]
    big = big.cuda()
    q = big[1::2, :, :, :, 4:4 + S]
    assert not q.is_contiguous() and q.stride(3) == S + 8 and q.data_ptr() % 4 == 0
    dhw, ray, eye, zd = camera(D, S, S, POSES[:2])
    occ = build_occupancy(q, stats=True)
    assert torch.equal(occ.map.cpu(), C.brute_force_map(q.cpu()))
    for strict in (False, True):
        assert_equal(render(q, dhw.expand(2, -1, -1).contiguous(), ray, eye, zd, strict=strict, occupancy=occ),
                     render(q, dhw.expand(2, -1, -1).contiguous(), ray, eye, zd, strict=strict), strict)
    assert stats_of(occ)[0] > 0


# 8. host contract
def test_host_contract_on_the_device():
    from ml_gmpi_amd import build_occupancy
    D, S = 8, 64
    dhw, ray, eye, zd = camera(D, S, S, POSES[:1])
    q = C.volume("shell", S, D).clone().cuda()
    occ = build_occupancy(q)
    render(q, dhw, ray, eye, zd, occupancy=occ)
    with pytest.raises(ValueError, match="another volume"):
        render(q.clone(), dhw, ray, eye, zd, occupancy=occ)
    with pytest.raises(ValueError, match="another volume"):     # a map of another volume's shape
        render(q, dhw, ray, eye, zd, occupancy=build_occupancy(C.volume("shell", 128, D).cuda()))
    with pytest.raises(TypeError):
        render(q.float() / 255, dhw, ray, eye, zd, occupancy=occ)
    q[0, 0, 3, 0, 0] += 1
    with pytest.raises(ValueError, match="stale"):
        render(q, dhw, ray, eye, zd, occupancy=occ)
    render(q, dhw, ray, eye, zd, occupancy=build_occupancy(q))
    with torch.inference_mode():
        qi = C.volume("shell", S, D).clone().cuda()
        occ_i = build_occupancy(qi, stats=True)
    assert occ_i.identity[4] is None
    assert_equal(render(qi, dhw, ray, eye, zd, occupancy=occ_i), render(qi, dhw, ray, eye, zd), "inference_mode")
    assert stats_of(occ_i)[0] > 0


def test_fallback_where_the_staged_kernel_would_not_run():
    import ml_gmpi_amd.hip_mpi as hm
    from ml_gmpi_amd import MPI, build_occupancy
    D, S = 8, 64
    dhw, ray, eye, zd = camera(D, S, S, POSES[:1])
    hm._OCCUPANCY_FALLBACK_WARNED = False
    q = C.volume("shell", S, D).cuda()
    narrow = C.volume("shell", S, D)[..., :6].contiguous().cuda()   # Wt = 6: no multiple of 4
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for vol, variant in ((q, "gather"), (narrow, "auto"), (narrow, "gather")):
            mpi = MPI(align_corners=True, variant=variant)
            occ = build_occupancy(vol, stats=True)
            status = torch.zeros(4, dtype=torch.int32, device="cuda")
            kw = dict(check_last_plane=True, want_transmittance=True, status=status, defer_status=True)
            with torch.no_grad():
                a = mpi.render_views(vol, _dev(dhw), _dev(ray), _dev(eye), _dev(zd), occupancy=occ, **kw)
                assert mpi.occupancy_fallbacks == 1
                b = mpi.render_views(vol, _dev(dhw), _dev(ray), _dev(eye), _dev(zd), **kw)
            assert mpi.occupancy_fallbacks == 1
            assert_equal(a, b, variant)
            assert stats_of(occ) == [0, 0]
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning) and "occupancy" in str(w.message)]) == 1


# 9. the driver
def test_driver_paths_and_seeds():
    from ml_gmpi_amd import ViewBatchDriver, build_occupancy, make_renderer
    D, S = 8, 64
    r = make_renderer("FFHQ", n_planes=D, device=torch.device("cuda"))
    drv = ViewBatchDriver(r, batch=3)
    q = C.volume("shell", S, D).cuda()
    yaws, pitches = [-0.3, -0.1, 0.0, 0.2, 0.3], [0.0, 0.1, 0.0, -0.1, 0.05]
    plain = drv.render_path(q, S, yaws, pitches, want_transmittance=True)
    occ = build_occupancy(q, stats=True)
    for o in (True, occ):
        got = drv.render_path(q, S, yaws, pitches, want_transmittance=True, occupancy=o)
        for k in ("rgb", "depth", "T"):
            assert torch.equal(got[k].view(torch.int32), plain[k].view(torch.int32)), (k, o is True)
    assert stats_of(occ)[0] > 0 and r.mpi.occupancy_fallbacks == 0
    stack = torch.cat([C.volume("shell", S, D, seed=s) for s in range(5)]).cuda()
    occ = build_occupancy(stack, stats=True)
    outs = []
    for o in (None, True, occ):
        torch.manual_seed(77)
        outs.append(drv.render_seeds(stack, S, occupancy=o))
    for got in outs[1:]:
        assert len(got) == len(outs[0]) == 4
        for a, b in zip(got, outs[0]):
            assert torch.equal(a, b)
    assert stats_of(occ)[0] > 0 and r.mpi.occupancy_fallbacks == 0
    for bad in (lambda: r.render_shaded(q, torch.ones((1, 1, S, S), device="cuda"), S, S, occupancy=occ),
                lambda: r.render_chunks([q[:, :4], q[:, 4:]], S, S, occupancy=occ),
                lambda: r.render_layers(q.permute(0, 1, 3, 4, 2).contiguous(), S, S, occupancy=occ)):
        with pytest.raises(TypeError):
            bad()


# 10. gradients: the forward of geometry_grad="all" may take the sparse launch; the uint8 geometry backward is the same
def test_geometry_gradients_have_the_same_bits():
    from ml_gmpi_amd import MPI, build_occupancy, make_renderer, rays_from_c2w
    D, S = 8, 64
    q = C.volume("shell", S, D).cuda()
    occ = build_occupancy(q, stats=True)
    g = torch.Generator().manual_seed(41)
    wc, wd = torch.randn((1, 3, S, S), generator=g).cuda(), torch.randn((1, 1, S, S), generator=g).cuda()
    r = make_renderer("FFHQ", n_planes=D, device=torch.device("cuda"), geometry_grad="all")
    with torch.no_grad():
        c2w0 = r.render(q, S, S, assert_not_out_of_last_plane=False, given_yaws=torch.tensor([[0.2]]), given_pitches=torch.tensor([[0.1]]))[2]

    def c2w_grad(o):
        c2w = c2w0.clone().requires_grad_(True)
        ray, eye, zd = rays_from_c2w(r, c2w)
        info = dict(batch_yaws=torch.zeros(1, 1), batch_pitches=torch.zeros(1, 1), batch_tf_c2w=c2w.detach(), batch_ray_dir=[ray], batch_eye_pos=[eye], batch_z_dir=[zd])
        rgb, depth = r.render(q, S, S, assert_not_out_of_last_plane=False, given_cam_infos=info, **({} if o is None else {"occupancy": o}))[:2]
        ((rgb * wc).sum() + (depth * wd).sum()).backward()
        return c2w.grad

    a, b = c2w_grad(None), c2w_grad(occ)
    assert float(a.abs().max()) > 0 and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert stats_of(occ)[0] > 0

    dhw0, ray, eye, zd = (_dev(t) for t in camera(D, S, S, POSES[1:2]))

    def dhw_grad(o):
        dhw = dhw0.clone().requires_grad_(True)
        out = MPI(align_corners=True, geometry_grad="all").render_views(q, dhw, ray, eye, zd, check_last_plane=False, **({} if o is None else {"occupancy": o}))
        ((out["color"] * wc).sum() + (out["depth"] * wd).sum()).backward()
        return dhw.grad

    a, b = dhw_grad(None), dhw_grad(occ)
    assert float(a.abs().max()) > 0 and torch.equal(a.view(torch.int32), b.view(torch.int32))
