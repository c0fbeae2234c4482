"""The plane-chunked render on the device (gmpi_mpi_render_chunk_launch / _chunk_backward_launch through MPI.render_views_chunks, MPI.chunked_render
and MPIRenderer.render_chunks): the forward against the one-shot render of the concatenation BIT FOR BIT (and, strict order, against the CPU
oracle), the status word, the backward against the committed autograd fixtures and against the one-shot backward, the renderer's wrapper, and the
peak memory of a generator of chunks.

Forward shape: texture 36 x 40 (Wt a multiple of the 8-texel loader item), image 40 x 72 -- ragged against the 32 x 16 tiles and the 64 x 4 gather
blocks --, D = 7, M = 2; three views as [2, 1] and four as 2 + 2; poses from the renderer's own sampler, one of them at the edge of the preset's range."""
import functools

import numpy as np
import pytest
import torch

import oracle
from _util import load_npz

pytestmark = pytest.mark.gpu

M, D, HT, WT, H, W = 2, 7, 36, 40, 40, 72
SPLITS = ((7,), (1, 6), (3, 1, 3), (1,) * 7)
STORAGE = ("f32", "bf16", "f16", "u8", "u8cl")
KEYS = ("color", "depth", "T")
VIEWS = {"2+1": dict(views_per_mpi=[2, 1], v2m=[0, 0, 1]), "2+2": dict(views_per_mpi=2, v2m=[0, 0, 1, 1])}


@functools.lru_cache(maxsize=None)
def _cameras():
    """dhw [M, D, 3] and four views (rays 40 x 72) from the renderer's sampler; view 2 sits at the edge of the FFHQ pose range."""
    from ml_gmpi_amd.pinhole import gen_cam
    from ml_gmpi_amd.renderer import MPIRenderer, PRESETS
    kw = dict(PRESETS["FFHQ"])
    kw.update(n_mpi_planes=D, plan_spatial_enlarge_factor=1.001, plane_distances_sample_method="inverse", cam_sample_method="truncated_gaussian",
              mpi_align_corners=True, use_confined_volume=True, device=torch.device("cpu"))
    r = MPIRenderer(**kw)
    r.cam = gen_cam(h=H, w=W, f=W / (2 * np.tan(np.pi * r.cam_fov / 360)), ray_from_pix_center=True)   # (set_cam asserts a square image)
    r.render_h, r.render_w = H, W
    torch.manual_seed(301)
    cam = r.sample_cam_poses(4, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    n = r.cam_pose_n_truncated_stds
    edge = r.sample_cam_poses(1, 0, 0, 0, 0, False, given_yaws=torch.tensor([[n * r.horizontal_std]], dtype=torch.float32),
                              given_pitches=torch.tensor([[-n * r.vertical_std]], dtype=torch.float32))
    ray, eye, zd = (torch.cat(cam[i]).clone() for i in (3, 4, 5))
    ray[2], eye[2], zd[2] = edge[3][0][0], edge[4][0][0], edge[5][0][0]
    dhw = r.static_mpi_plane_dhws.reshape(1, -1, 3).expand(M, -1, -1).contiguous()
    assert tuple(ray.shape) == (4, 3, H, W) and tuple(dhw.shape) == (M, D, 3)
    return dhw, ray, eye, zd


@functools.lru_cache(maxsize=None)
def _volume(storage):
    """(the stack as the kernels store it, on the CPU; the fp32 values it stands for)."""
    g = torch.Generator().manual_seed(302)
    v = torch.rand((M, D, 4, HT, WT), generator=g)
    v[:, :, 3] *= 0.6   # (the stack stays translucent to its last plane: every chunk moves the result)
    if storage in ("u8", "u8cl"):
        q = (v * 255).round().to(torch.uint8)
        vals = q.float() / 255
        if storage == "u8cl":
            q = q.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)   # channels-last memory seen as [M, D, 4, Ht, Wt]
            assert q.stride(2) == 1 and q.stride(4) == 4
        return q, vals
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[storage]
    return v.to(dt), v.to(dt).float()


def _chunks_on_device(storage, split):
    """The stack cut into `split`, every chunk a tensor of its own on the device (channels-last chunks keep that layout)."""
    q, _ = _volume(storage)
    out, k = [], 0
    for d in split:
        c = q[:, k:k + d]
        if storage == "u8cl":
            c = c.permute(0, 1, 3, 4, 2).contiguous().cuda().permute(0, 1, 4, 2, 3)
            assert c.stride(2) == 1 and c.stride(4) == 4
        else:
            c = c.contiguous().cuda()
        out.append(c)
        k += d
    return out


@functools.lru_cache(maxsize=None)
def _oracle(values_of, ac, views):
    dhw, ray, eye, zd = _cameras()
    v2m = VIEWS[views]["v2m"]
    n = len(v2m)
    return oracle.render(_volume(values_of)[1], dhw, ray[:n], eye[:n], zd[:n], view_to_mpi=np.asarray(v2m, np.int32), align_corners=ac, threads=True)


def _geo(views):
    dhw, ray, eye, zd = _cameras()
    n = len(VIEWS[views]["v2m"])
    return dhw.cuda(), ray[:n].cuda(), eye[:n].cuda(), zd[:n].cuda()


def _run(mpi, storage, split, views, *, one_shot=False, out_pm1=False, check_last=True, chunks=None, **kw):
    chunks = _chunks_on_device(storage, split) if chunks is None else chunks
    kw = dict(views_per_mpi=VIEWS[views]["views_per_mpi"], check_last_plane=check_last, out_pm1=out_pm1, want_transmittance=True, defer_status=True, **kw)
    with torch.no_grad():
        if one_shot:
            assert len(chunks) == 1
            res = mpi.render_views(chunks[0], *_geo(views), **kw)
        else:
            res = mpi.render_views_chunks(chunks, *_geo(views), **kw)
    torch.cuda.synchronize()
    out = {k: res[k].cpu().numpy() for k in KEYS}
    out["status"] = int(res["status"][0].item())
    res["status"].zero_()
    return out


# ---- forward: the bits of the one-shot render ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("storage", STORAGE)
def test_chunked_forward_has_the_bits_of_the_one_shot_render(storage, ac):
    from ml_gmpi_amd import MPI
    values_of = "u8" if storage == "u8cl" else storage
    for views in VIEWS:
        orc = _oracle(values_of, ac, views)
        for variant in ("gather", "lds"):
            for strict in (True, False):
                mpi = MPI(align_corners=ac, variant=variant, strict_order=strict, on_out_of_plane="raise")
                for pm1 in (False, True):
                    one = _run(mpi, storage, (D,), views, one_shot=True, out_pm1=pm1)
                    if strict:   # the oracle, bit for bit (2 c - 1 is exact for c in [0, 1])
                        want = dict(color=2 * orc["color"] - 1 if pm1 else orc["color"], depth=orc["depth"], T=orc["T"])
                        for k in KEYS:
                            assert np.array_equal(one[k], want[k]), (storage, ac, views, variant, pm1, k)
                        assert one["status"] == orc["status"]
                    else:        # the project's default-mode bar against the oracle
                        assert np.abs(one["depth"] - orc["depth"]).max() <= 1e-5 and np.abs(one["T"] - orc["T"]).max() <= 1e-5
                    for split in SPLITS:
                        got = _run(mpi, storage, split, views, out_pm1=pm1)
                        for k in KEYS:   # default mode too: the per-plane arithmetic does not know the chunk
                            assert np.array_equal(got[k], one[k]), (storage, ac, views, variant, strict, pm1, split, k, float(np.abs(got[k] - one[k]).max()))
                        assert got["status"] == one["status"], (storage, ac, views, variant, strict, pm1, split)
                    assert mpi.chunk_variant_fallbacks == 0


@pytest.mark.parametrize("storage", ["f32", "bf16", "u8cl"])
def test_in_place_state_and_two_state_buffers_give_the_same_bits(storage):
    """`ChunkedRender` reads and writes one state; here the C entry is driven with two buffers that alternate."""
    import ctypes
    from ml_gmpi_amd import MPI, _lib
    from ml_gmpi_amd.hip_mpi import _DTYPES
    views, split = "2+1", (3, 1, 3)
    for variant in ("gather", "lds"):
        mpi = MPI(variant=variant, strict_order=True, on_out_of_plane="raise")
        want = _run(mpi, storage, split, views)
        chunks = _chunks_on_device(storage, split)
        dhw, ray, eye, zd = _geo(views)
        v2m = torch.tensor(VIEWS[views]["v2m"], dtype=torch.int32).cuda()
        N = ray.shape[0]
        states = [torch.full((N, 5, H, W), float("nan"), device="cuda") for _ in range(2)]
        color, depth, T = (torch.empty((N, c, H, W), device="cuda") for c in (3, 1, 1))
        status = torch.zeros(4, dtype=torch.int32, device="cuda")
        lib, k0 = _lib.load_library(), 0
        for i, c in enumerate(chunks):
            last = i == len(chunks) - 1
            rows = dhw[:, k0:k0 + c.shape[1]].contiguous()
            p = _lib.GmpiRenderParams()
            p.struct_size = ctypes.sizeof(p)
            p.flags = _lib.FLAG_ALIGN_CORNERS | _lib.FLAG_CHECK_RANGE | _lib.FLAG_STRICT_ORDER | (_lib.FLAG_CHECK_LAST_PLANE if last else 0)
            p.variant, p.rgba_dtype = _lib.VARIANTS[variant], _DTYPES[c.dtype]
            p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = N, M, c.shape[1], HT, WT, H, W, 1
            p.rgba = c.data_ptr()
            p.rgba_stride[:] = c.stride()
            p.view_to_mpi, p.dhw, p.ray_dir, p.eye_pos, p.z_dir = v2m.data_ptr(), rows.data_ptr(), ray.data_ptr(), eye.data_ptr(), zd.data_ptr()
            p.status = status.data_ptr()
            if last:
                p.rgb_out, p.depth_out, p.transmittance_out = color.data_ptr(), depth.data_ptr(), T.data_ptr()
            carry = _lib.GmpiCarry()
            carry.struct_size = ctypes.sizeof(carry)
            carry.state_in = None if i == 0 else states[(i - 1) % 2].data_ptr()
            carry.state_out = None if last else states[i % 2].data_ptr()
            _lib.check(lib.gmpi_mpi_render_chunk_launch(ctypes.byref(p), ctypes.byref(carry), torch.cuda.current_stream().cuda_stream), "chunk launch")
            k0 += c.shape[1]
            torch.cuda.synchronize()   # (rows, p: alive until the launch has run)
        got = dict(color=color.cpu().numpy(), depth=depth.cpu().numpy(), T=T.cpu().numpy())
        for k in KEYS:
            assert np.array_equal(got[k], want[k]), (storage, variant, k)
        assert int(status[0].item()) == want["status"]
        assert torch.isfinite(states[0]).all() and torch.isfinite(states[1]).all()   # every pixel of both states was written


# ---- status --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["gather", "lds"])
def test_status_bits_of_a_chunked_stack(variant):
    from ml_gmpi_amd import MPI, _lib
    mpi = MPI(variant=variant, strict_order=True, on_out_of_plane="raise")
    views, split = "2+1", (3, 1, 3)
    clean = _run(mpi, "f32", split, views)
    # a texel of 1.5 in the MIDDLE chunk: GMPI_STATUS_RGBA_RANGE, by status word and by assertion
    chunks = _chunks_on_device("f32", split)
    chunks[1][:, 0, 1, HT // 2 - 2:HT // 2 + 2, WT // 2 - 2:WT // 2 + 2] = 1.5
    bad = _run(mpi, "f32", split, views, chunks=chunks)
    assert bad["status"] == clean["status"] | _lib.STATUS_RGBA_RANGE and not clean["status"] & _lib.STATUS_RGBA_RANGE
    with torch.no_grad(), pytest.raises(AssertionError, match="alpha to be within"):
        mpi.render_views_chunks(chunks, *_geo(views), views_per_mpi=VIEWS[views]["views_per_mpi"])
    # the last-plane bit comes from the FINAL chunk only: a ray that leaves every plane sets it once, with check_last_plane, and never without
    dhw, ray, eye, zd = _geo(views)
    bent = ray.clone()
    bent[1, :, H - 1, W - 1] = torch.tensor([0.8, 0.0, 0.6], device="cuda")
    cr = mpi.chunked_render(dhw, bent, eye, zd, views_per_mpi=VIEWS[views]["views_per_mpi"], check_last_plane=True, defer_status=True)
    words = []
    with torch.no_grad():
        for c in _chunks_on_device("f32", split):
            cr.add(c)
            words.append(int(cr.status[0].item()))
    assert [w & _lib.STATUS_OUT_OF_LAST_PLANE for w in words] == [0, 0, _lib.STATUS_OUT_OF_LAST_PLANE]
    cr.finish()
    with torch.no_grad():
        res = mpi.render_views_chunks(_chunks_on_device("f32", split), dhw, bent, eye, zd, views_per_mpi=VIEWS[views]["views_per_mpi"],
                                      check_last_plane=False, defer_status=True)
        assert not int(res["status"][0].item()) & _lib.STATUS_OUT_OF_LAST_PLANE
        with pytest.raises(RuntimeError, match="goes out of plane"):
            mpi.render_views_chunks(_chunks_on_device("f32", split), dhw, bent, eye, zd, views_per_mpi=VIEWS[views]["views_per_mpi"], check_last_plane=True)


# ---- backward: the committed fixtures of the reference's own autograd ----------------------------------------------------------------------------
FIXTURES = ("backward_ffhq_d8_32", "backward_ffhq_d8_32_opaque", "backward_ffhq_d6_tex40_img24_ac0", "backward_forward_ragged_views")


def _cut(vol, split):
    out, k = [], 0
    for d in split:
        out.append(vol[:, k:k + d].contiguous())
        k += d
    assert k == vol.shape[1]
    return out


def _fixture_run(fx, variant, split, uses_T=False, dtype=torch.float32, needs=None):
    """Forward + backward of the fixture's stack cut into `split` (None: the one-shot render_views); the gradient as one [M, D, 4, Ht, Wt] array."""
    from ml_gmpi_amd import MPI
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    N = fx["ray_dir"].shape[0]
    v2m = fx["view_to_mpi"] if "view_to_mpi" in fx else np.arange(N, dtype=np.int32)
    pm1 = "ref_rgb_pm1" in fx
    mpi = MPI(align_corners=fx["meta"]["ac"], variant=variant, on_out_of_plane="raise")
    geo = (t(fx["dhw"]), t(fx["ray_dir"]), t(fx["eye"]), t(fx["zdir"]))
    kw = dict(view_to_mpi=t(v2m.astype(np.int32)), check_last_plane=False, out_pm1=pm1, want_transmittance=uses_T)
    vol = t(fx["rgba"]).to(dtype)
    if split is None:
        leaves = [vol.requires_grad_(True)]
        out = mpi.render_views(vol, *geo, **kw)
    else:
        leaves = _cut(vol, split)
        for i, c in enumerate(leaves):
            c.requires_grad_(needs is None or i in needs)
        out = mpi.render_views_chunks(leaves, *geo, **kw)
    loss = (out["color"] * t(fx["g_rgb"])).sum() + (out["depth"] * t(fx["g_depth"])).sum()
    if uses_T:
        loss = loss + (out["T"] * 2.0).sum()   # (the T term of the marshal tests' loss_of)
    loss.backward()
    torch.cuda.synchronize()
    return out, leaves


def _grad_of(leaves):
    return torch.cat([c.grad.float() for c in leaves], 1).cpu().numpy()


@pytest.mark.parametrize("name", FIXTURES)
def test_chunked_backward_matches_the_reference_autograd_fixtures(name):
    fx = load_npz(name + ".npz")
    ref_g = fx["ref_grad_rgba"]
    scale, Dp = np.abs(ref_g).max(), fx["rgba"].shape[1]
    for variant in ("auto", "gather"):   # the 64 x 8 tile kernel | the one-pixel all-atomic kernel
        one = _grad_of(_fixture_run(fx, variant, None)[1])
        one_T = _grad_of(_fixture_run(fx, variant, None, uses_T=True)[1])
        for split in ((3, Dp - 3), (1, Dp - 1), (1,) * Dp):
            out, leaves = _fixture_run(fx, variant, split)
            got = _grad_of(leaves)
            err_ref, err_one = np.abs(got - ref_g).max(), np.abs(got - one).max()
            print(f"{name} {variant} {split}: |chunked - fixture| {err_ref / scale:.2e}, |chunked - one-shot| {err_one / scale:.2e} of the largest gradient")
            assert np.isfinite(got).all()
            assert err_ref <= 1e-4 * scale, (name, variant, split, err_ref, scale)     # the reference's own autograd
            assert err_one <= 1e-5 * scale, (name, variant, split, err_one, scale)     # the one-shot backward of the same kernel
            # a loss that also uses T: the one-shot backward_ex path
            got_T = _grad_of(_fixture_run(fx, variant, split, uses_T=True)[1])
            err_T = np.abs(got_T - one_T).max()
            assert err_T <= 1e-5 * np.abs(one_T).max(), (name, variant, split, err_T)


def test_the_opaque_fixture_puts_dead_pixels_in_front_of_the_chunks_behind():
    """What makes the case above mean something: behind the opaque planes T_in of a chunk is below 1e-30 for some pixels, and not for all."""
    from ml_gmpi_amd import MPI
    fx = load_npz("backward_ffhq_d8_32_opaque.npz")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    with torch.no_grad():
        T = MPI(align_corners=fx["meta"]["ac"]).render_views(t(fx["rgba"])[:, :7], t(fx["dhw"])[:, :7].contiguous(), t(fx["ray_dir"]), t(fx["eye"]), t(fx["zdir"]),
                                                               want_transmittance=True)["T"]
    dead = float((T < 1e-30).float().mean())
    assert 0.0 < dead < 1.0, dead


def test_only_some_chunks_require_grad_and_bf16_chunks_get_bf16_gradients():
    fx = load_npz("backward_ffhq_d8_32.npz")
    split = (3, 1, 4)   # the fixture holds 8 planes: (3, 1, 3) and one more behind
    full = _fixture_run(fx, "auto", split)[1]
    out, part = _fixture_run(fx, "auto", split, needs=(0, 2))
    assert part[1].grad is None and out["color"].requires_grad
    scale = max(float(c.grad.abs().max()) for c in full)
    for i in (0, 2):   # unchanged, up to the order of the atomic adds (this file's bar between two runs of one kernel)
        assert float((part[i].grad - full[i].grad).abs().max()) <= 1e-5 * scale, i
    _, low = _fixture_run(fx, "auto", split, dtype=torch.bfloat16)
    ref = _grad_of(_fixture_run(fx, "auto", None, dtype=torch.bfloat16)[1])
    for c in low:
        assert c.grad.dtype is torch.bfloat16 and c.grad.shape == c.shape
    assert np.abs(_grad_of(low) - ref).max() <= 2.0 ** -7 * np.abs(ref).max()   # two bf16 roundings of gradients that agree to 1e-5


# ---- MPIRenderer.render_chunks -------------------------------------------------------------------------------------------------------------------
def test_renderer_render_chunks_is_render():
    from ml_gmpi_amd import make_renderer
    dev = torch.device("cuda:0")
    r = make_renderer("FFHQ", n_planes=D, device=dev, kernel_variant="lds", strict_order=True, on_out_of_plane="raise")
    S = 40
    g = torch.Generator().manual_seed(303)
    vol = torch.rand((2, D, 4, S, S), generator=g).to(dev)
    chunks = _cut(vol, (3, 1, 3))
    with torch.no_grad():
        # without given_cam_infos, the same seed: the same RNG use -- c2w and angles are identical (and so is everything else)
        torch.manual_seed(5)
        a = r.render(vol, S, S, want_transmittance=True)
        ra = torch.rand(1)
        torch.manual_seed(5)
        b = r.render_chunks(iter(chunks), S, S, want_transmittance=True)
        rb = torch.rand(1)
        assert len(a) == len(b) == 5 and torch.equal(ra, rb)
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
        # with given_cam_infos: the tuple is bit-identical
        torch.manual_seed(6)
        cam = r.sample_cam_poses(2, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
        info = dict(batch_yaws=cam[0], batch_pitches=cam[1], batch_tf_c2w=cam[2], batch_ray_dir=torch.cat(cam[3]).clone(), batch_eye_pos=torch.cat(cam[4]).clone(),
                    batch_z_dir=torch.cat(cam[5]).clone())
        a = r.render(vol, S, S, given_cam_infos=info, want_transmittance=True)
        b = r.render_chunks(chunks, S, S, given_cam_infos=info, want_transmittance=True)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        c = r.render_chunks(chunks, S, S, given_cam_infos=info)
        assert len(c) == 4 and torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])


# ---- memory --------------------------------------------------------------------------------------------------------------------------------------
def test_a_generator_of_chunks_never_holds_the_stack():
    """M = 1, D = 32, 128^2 fp32: 8 MiB of stack in chunks of 4 planes (1 MiB) from a generator, without grad.  Above what is allocated before the
    call: at most two chunks (the one being rendered; the allocator may not have reused its block when the next is made), the state, the outputs."""
    from ml_gmpi_amd import make_renderer
    dev = torch.device("cuda:0")
    Dm, S, Dc = 32, 128, 4
    r = make_renderer("FFHQ", n_planes=Dm, device=dev, on_out_of_plane="raise")
    r.set_cam(r.cam_fov, S, S)
    torch.manual_seed(7)
    cam = r.sample_cam_poses(1, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    dhw = r.static_mpi_plane_dhws.reshape(1, -1, 3).to(dev).contiguous()
    ray, eye, zd = (torch.cat(cam[i]).to(dev).clone() for i in (3, 4, 5))
    made = []

    def chunks():
        g = torch.Generator(device=dev).manual_seed(8)
        for _ in range(Dm // Dc):
            made.append(1)
            yield torch.rand((1, Dc, 4, S, S), generator=g, device=dev)

    with torch.no_grad():
        r.mpi.render_views_chunks(chunks(), dhw, ray, eye, zd)   # (warm-up: the library is loaded, the status words exist)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        res = r.mpi.render_views_chunks(chunks(), dhw, ray, eye, zd, want_transmittance=True)
        torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    chunk, image = Dc * 4 * S * S * 4, S * S * 4
    state, outputs = 5 * image, (3 + 1 + 1) * image
    print(f"peak above the inputs {peak} B; a chunk {chunk} B, the state {state} B, the outputs {outputs} B; the stack {Dm // Dc * chunk} B")
    assert len(made) == 2 * (Dm // Dc) and res["color"].shape == (1, 3, S, S)
    assert peak <= 2 * chunk + state + outputs + (1 << 20), peak
    assert peak < Dm // Dc * chunk // 2   # nowhere near the 8 MiB the concatenation alone takes
