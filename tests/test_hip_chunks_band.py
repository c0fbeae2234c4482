"""The plane-chunked render through the band kernel's carry instances on the device (gmpi_mpi_render_chunk_band_launch through `chunk_kernel="band"` /
"band+tile" of MPI.render_views_chunks, MPI.chunked_render): strict order against the CPU oracle and the one-shot band render BIT FOR BIT however the
stack is cut, default mode within test_hip_band.py's bars (and, where every texel box fits the band kernel, the bits of the one-shot band render), the
state in place and in two buffers, a dirty workspace, stacks handed between the tile and the band kernel, views that share MPIs, the status word, the
autograd forward, and the fallback of chunks the band entry cannot take.

Shapes: the smallest of test_hip_band.py at which a band can go wrong -- an image smaller than one band with rays that leave the texture, a ragged band
over a texture that is not the image, two band columns, tilted cameras whose boxes do not fit (the in-kernel direct gather; with "band+tile" the tile
kernel's carry instances behind the view gate)."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import oracle
from _util import load_npz
from test_hip_parity import TOL, _random_case

pytestmark = pytest.mark.gpu

KEYS = ("color", "depth", "T")
KERNELS = ("band", "band+tile")
CASES16 = {
    "small": dict(seed=24, B=3, D=5, S=72, T=64),                      # image smaller than one band; rays leave the texture (zeros padding)
    "ragged": dict(seed=23, B=2, D=9, S=200, T=208),                   # ragged band, texture != image
    "columns": dict(seed=22, B=1, D=12, S=512),                        # two band columns
    "extreme": dict(seed=25, B=2, D=16, S=320, T=256, extreme=True),   # boxes that do not fit
}
CASES32 = {
    "columns": dict(seed=26, B=2, D=12, S=256),
    "ragged": dict(seed=27, B=2, D=7, S=200, T=204),
    "extreme": dict(seed=28, B=2, D=9, S=320, T=256, extreme=True),
}
CASES = [("bf16", n) for n in CASES16] + [("f16", n) for n in CASES16] + [("f32", n) for n in CASES32]
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def _splits(D):
    """whole; (1, D - 1); three uneven pieces; all single planes"""
    a = max(D // 4, 1)
    return ((D,), (1, D - 1), (a, 1, D - a - 1), (1,) * D)


@functools.lru_cache(maxsize=None)
def _case(storage, name):
    """(the volume as stored, on the CPU; dhw, rays, eyes, axes) -- never written to."""
    rgba, dhw, ray, eye, zd = _random_case(**(CASES32 if storage == "f32" else CASES16)[name])
    return rgba.to(DTYPES[storage]), dhw, ray, eye, zd


@functools.lru_cache(maxsize=None)
def _oracle(storage, name, ac):
    vol, dhw, ray, eye, zd = _case(storage, name)
    return oracle.render(vol.float(), dhw, ray, eye, zd, align_corners=ac, threads=True)


def _cut(vol, split):
    out, k = [], 0
    for d in split:
        out.append(vol[:, k:k + d].contiguous())
        k += d
    assert k == vol.shape[1]
    return out


def _result(res):
    torch.cuda.synchronize()
    out = {k: res[k].cpu().numpy() for k in KEYS}
    out["status"] = int(res["status"][0].item())
    res["status"].zero_()
    return out


def _chunked(mpi, vol, geo, split, kernel, **kw):
    kw = dict(dict(check_last_plane=True, want_transmittance=True, defer_status=True), **kw)
    with torch.no_grad():
        return _result(mpi.render_views_chunks(_cut(vol, split), *geo, chunk_kernel=kernel, **kw))


def _one_shot(mpi, vol, geo, **kw):
    kw = dict(dict(check_last_plane=True, want_transmittance=True, defer_status=True), **kw)
    with torch.no_grad():
        return _result(mpi.render_views(vol, *geo, **kw))


def _on_device(storage, name):
    vol, *geo = _case(storage, name)
    return vol.cuda(), tuple(t.cuda() for t in geo)


# ---- strict order: the oracle's bits, however the stack is cut --------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,name", CASES)
def test_strict_order_has_the_bits_of_the_oracle_and_of_the_one_shot_band_render(storage, name):
    from ml_gmpi_amd import MPI
    vol, geo = _on_device(storage, name)
    for ac in (True, False):
        orc = _oracle(storage, name, ac)
        mpi = MPI(align_corners=ac, variant="band", strict_order=True, on_out_of_plane="raise")
        for pm1 in (False, True):
            want = dict(color=2 * orc["color"] - 1 if pm1 else orc["color"], depth=orc["depth"], T=orc["T"])   # (2 c - 1 is exact for c in [0, 1])
            one = _one_shot(mpi, vol, geo, out_pm1=pm1)
            for k in KEYS:
                assert np.array_equal(one[k], want[k]), (storage, name, ac, pm1, k)
            for kernel in KERNELS:
                for split in _splits(vol.shape[1]):
                    got = _chunked(mpi, vol, geo, split, kernel, out_pm1=pm1)
                    for k in KEYS:
                        assert np.array_equal(got[k], want[k]), (storage, name, ac, pm1, kernel, split, k, float(np.abs(got[k] - want[k]).max()))
                        assert np.array_equal(got[k], one[k]), (storage, name, ac, pm1, kernel, split, k)
                    assert got["status"] == orc["status"] == one["status"], (storage, name, ac, pm1, kernel, split, got["status"])
        assert mpi.chunk_band_fallbacks == 0 and mpi.chunk_variant_fallbacks == 0


# ---- default mode ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,name", CASES)
def test_default_mode_is_within_the_bars_and_where_every_box_fits_has_the_bits_of_the_one_shot_band_render(storage, name):
    """Bars: test_hip_band.py's -- colour 0.5e-5, depth and T 1e-5 against the oracle.  Where every box fits the band kernel (the cases that are not
    `extreme`) the per-plane arithmetic does not know the chunk: the bits of the one-shot band render.  Under the extreme poses some bands take the
    direct gather, which forms its bilinear weights as the strict order does, not as the staged default-mode taps do -- and WHICH bands do depends on
    the planes of the launch (a band gathers when any box of its chunk does not fit): only the bars hold there, as DESIGN.md 3.3f says of the tile kernel."""
    from ml_gmpi_amd import MPI
    vol, geo = _on_device(storage, name)
    for ac in (True, False):
        orc = _oracle(storage, name, ac)
        mpi = MPI(align_corners=ac, variant="band", on_out_of_plane="raise")
        one = _one_shot(mpi, vol, geo)
        for kernel in KERNELS:
            for split in _splits(vol.shape[1]):
                got = _chunked(mpi, vol, geo, split, kernel)
                err = {k: float(np.abs(got[k] - orc[k]).max()) for k in KEYS}
                print(storage, name, ac, kernel, split, err)
                assert err["color"] <= 0.5 * TOL and err["depth"] <= TOL and err["T"] <= TOL, (storage, name, ac, kernel, split, err)
                assert got["status"] == orc["status"]
                if name != "extreme":
                    for k in KEYS:
                        assert np.array_equal(got[k], one[k]), (storage, name, ac, kernel, split, k, float(np.abs(got[k] - one[k]).max()))
        assert mpi.chunk_band_fallbacks == 0


# ---- the state: in place, two buffers, a dirty workspace --------------------------------------------------------------------------------------------
def _drive(vol, geo, split, variant, strict, two_states, dirty):
    """The C entry itself over `split`: the state in one buffer or in two that alternate; `dirty`: the workspace filled with 0xFF between the chunks."""
    from ml_gmpi_amd import _lib
    from ml_gmpi_amd.hip_mpi import _DTYPES
    dhw, ray, eye, zd = geo
    lib, stream = _lib.load_library(), torch.cuda.current_stream().cuda_stream
    N, _, H, W = ray.shape
    states = [torch.full((N, 5, H, W), float("nan"), device="cuda") for _ in range(2 if two_states else 1)]
    color, depth, T = (torch.empty((N, c, H, W), device="cuda") for c in (3, 1, 1))
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws, k0 = None, 0
    chunks = _cut(vol, split)
    for i, c in enumerate(chunks):
        last = i == len(chunks) - 1
        rows = dhw[:, k0:k0 + c.shape[1]].contiguous()
        p = _lib.GmpiRenderParams()
        p.struct_size = ctypes.sizeof(p)
        p.flags = _lib.FLAG_ALIGN_CORNERS | _lib.FLAG_CHECK_RANGE | (_lib.FLAG_STRICT_ORDER if strict else 0) | (_lib.FLAG_CHECK_LAST_PLANE if last else 0)
        p.variant, p.rgba_dtype = variant, _DTYPES[c.dtype]
        p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = N, c.shape[0], c.shape[1], c.shape[3], c.shape[4], H, W, 1
        p.rgba = c.data_ptr()
        p.rgba_stride[:] = c.stride()
        p.dhw, p.ray_dir, p.eye_pos, p.z_dir, p.status = rows.data_ptr(), ray.data_ptr(), eye.data_ptr(), zd.data_ptr(), status.data_ptr()
        if last:
            p.rgb_out, p.depth_out, p.transmittance_out = color.data_ptr(), depth.data_ptr(), T.data_ptr()
        assert lib.gmpi_render_chunk_band_supports(ctypes.byref(p)) == 1
        need = int(lib.gmpi_render_chunk_band_workspace_bytes(ctypes.byref(p)))
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        if dirty:
            ws.fill_(0xFF)
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
        carry = _lib.GmpiCarry()
        carry.struct_size = ctypes.sizeof(carry)
        carry.state_in = None if i == 0 else states[(i - 1) % len(states)].data_ptr()
        carry.state_out = None if last else states[i % len(states)].data_ptr()
        _lib.check(lib.gmpi_mpi_render_chunk_band_launch(ctypes.byref(p), ctypes.byref(carry), stream), "band chunk launch")
        k0 += c.shape[1]
        torch.cuda.synchronize()   # (rows, p: alive until the launch has run)
    assert all(torch.isfinite(s).all() for s in states)   # every pixel of every state was written
    return dict(color=color.cpu().numpy(), depth=depth.cpu().numpy(), T=T.cpu().numpy(), status=int(status[0].item()))


@pytest.mark.parametrize("storage,name", [("bf16", "ragged"), ("bf16", "extreme"), ("f32", "ragged"), ("f32", "extreme")])
def test_state_in_place_two_state_buffers_and_a_dirty_workspace_give_the_same_bits(storage, name):
    from ml_gmpi_amd import _lib
    vol, geo = _on_device(storage, name)
    D = vol.shape[1]
    split = (D // 4, 1, D - D // 4 - 1)
    orc = _oracle(storage, name, True)
    for variant in (_lib.VARIANT_BAND, _lib.VARIANT_AUTO):
        for strict in (True, False):
            runs = [_drive(vol, geo, split, variant, strict, two, dirty) for two, dirty in ((False, False), (True, False), (False, True), (True, True))]
            for other in runs[1:]:
                for k in KEYS + ("status",):
                    assert np.array_equal(other[k], runs[0][k]), (storage, name, variant, strict, k)
            if strict:
                for k in KEYS:
                    assert np.array_equal(runs[0][k], orc[k]), (storage, name, variant, k)
                assert runs[0]["status"] == orc["status"]


# ---- one stack, two kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,name", [("bf16", "ragged"), ("f16", "extreme"), ("f32", "ragged"), ("f32", "extreme")])
def test_a_stack_passes_between_the_tile_kernel_and_the_band_kernel(storage, name):
    """The state is one format: chunks through gmpi_mpi_render_chunk_launch's tile kernel (chunk_kernel = None) and through the band kernel, alternating
    either way.  Strict order: the oracle's bits."""
    from ml_gmpi_amd import MPI
    vol, geo = _on_device(storage, name)
    D = vol.shape[1]
    orc = _oracle(storage, name, True)
    mpi = MPI(variant="lds", strict_order=True, on_out_of_plane="raise")
    for kernel in KERNELS:
        for order in ((None, kernel, None, kernel), (kernel, None, kernel, None)):
            chunks = _cut(vol, (2, 1, D - 5, 2))
            with torch.no_grad():
                cr = mpi.chunked_render(*geo, check_last_plane=True, want_transmittance=True, defer_status=True)
                for c, kk in zip(chunks, order):
                    cr.chunk_kernel = kk
                    cr.add(c)
                got = _result(cr.finish())
            for k in KEYS:
                assert np.array_equal(got[k], orc[k]), (storage, name, kernel, order, k)
            assert got["status"] == orc["status"]
    assert mpi.chunk_band_fallbacks == 0 and mpi.chunk_variant_fallbacks == 0


def test_band_and_tile_kernel_share_the_views_of_one_chunk_launch():
    """"band+tile" with one view the band kernel stages and one it cannot (the extreme pose): the table kernel of every chunk launch stamps the gate word
    of the second view alone, the band carry kernel renders the first, the tile carry kernel the second -- each state passes through one kernel."""
    from ml_gmpi_amd import MPI, hip_mpi
    cfg = dict(CASES16["extreme"])
    vol, dhw, ray, eye, zd = _case("bf16", "extreme")
    _, _, ray_m, eye_m, zd_m = _random_case(**dict(cfg, extreme=False))
    ray, eye, zd = ray.clone(), eye.clone(), zd.clone()
    ray[0], eye[0], zd[0] = ray_m[0], eye_m[0], zd_m[0]
    orc = oracle.render(vol.float(), dhw, ray, eye, zd, threads=True)
    geo = (dhw.cuda(), ray.cuda(), eye.cuda(), zd.cuda())
    mpi = MPI(variant="band", strict_order=True, on_out_of_plane="raise")
    split = (5, 1, 10)
    _chunked(mpi, vol.cuda(), geo, split, "band+tile")   # (the stream's workspace exists now)
    ws = hip_mpi.workspace_of(torch.device("cuda:0"))
    ws.zero_()
    got = _chunked(mpi, vol.cuda(), geo, split, "band+tile")
    for k in KEYS:
        assert np.array_equal(got[k], orc[k]), k
    assert got["status"] == orc["status"]
    n_bands = 2 * ((cfg["S"] + 255) // 256) * ((cfg["S"] + 7) // 8)
    gate = ws[4 * n_bands:4 * (n_bands + 2)].view(torch.int32).cpu().tolist()   # the gate words behind the band headers, as the last chunk launch left them
    assert gate[0] == 0 and gate[1] != 0, gate


# ---- views that share MPIs ----------------------------------------------------------------------------------------------------------------------------
def test_views_sharing_one_mpi_cut_in_two():
    """test_hip_band.py::test_band_views_sharing_one_mpi's case (bf16, four views of two MPIs, D = 8, 256^2), the stack cut in two."""
    from ml_gmpi_amd import MPI
    rgba, dhw, ray, eye, zd = _random_case(seed=41, B=4, D=8, S=256)
    one, dhw1 = rgba[:2].to(torch.bfloat16), dhw[:2].contiguous()
    orc = oracle.render(one.float(), dhw1, ray, eye, zd, view_to_mpi=np.array([0, 0, 1, 1], dtype=np.int32), threads=True)
    vol, geo = one.cuda(), (dhw1.cuda(), ray.cuda(), eye.cuda(), zd.cuda())
    mpi = MPI(variant="band", strict_order=True, on_out_of_plane="raise")
    for kernel in KERNELS:
        for split in ((4, 4), (3, 5)):
            out = _chunked(mpi, vol, geo, split, kernel, views_per_mpi=2)
            out2 = _chunked(mpi, vol, geo, split, kernel, view_to_mpi=torch.tensor([0, 0, 1, 1], dtype=torch.int32).cuda())
            for k in KEYS:
                assert np.array_equal(out[k], orc[k]) and np.array_equal(out2[k], orc[k]), (kernel, split, k)
            geo3 = (geo[0], geo[1][:3], geo[2][:3], geo[3][:3])
            out3 = _chunked(mpi, vol, geo3, split, kernel, views_per_mpi=[2, 1])   # ragged groups
            for k in KEYS:
                assert np.array_equal(out3[k], orc[k][:3]), (kernel, split, k)
            assert out["status"] == out2["status"] == out3["status"] == 0


# ---- status -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_status_bits_of_a_chunked_stack(storage, kernel):
    from ml_gmpi_amd import MPI, _lib
    vol, geo = _on_device(storage, "ragged")
    D, Ht, Wt = vol.shape[1], vol.shape[3], vol.shape[4]
    split = (3, 1, D - 4)
    dhw, ray, eye, zd = geo
    for strict in (True, False):
        mpi = MPI(variant="band", strict_order=strict, on_out_of_plane="raise")
        clean = _chunked(mpi, vol, geo, split, kernel)
        assert clean["status"] == 0
        # a texel of 1.5 in the MIDDLE chunk with the range check on: GMPI_STATUS_RGBA_RANGE, by status word and by assertion; off: nothing
        bad = vol.clone()
        bad[:, 3, 1, Ht // 2 - 2:Ht // 2 + 2, Wt // 2 - 2:Wt // 2 + 2] = 1.5
        assert _chunked(mpi, bad, geo, split, kernel)["status"] == _lib.STATUS_RGBA_RANGE
        with torch.no_grad(), pytest.raises(AssertionError, match="alpha to be within"):
            mpi.render_views_chunks(_cut(bad, split), *geo, chunk_kernel=kernel)
        off = MPI(variant="band", strict_order=strict, range_check="off", on_out_of_plane="raise")
        assert _chunked(off, bad, geo, split, kernel)["status"] == 0
    # a ray that leaves the last plane is reported from the LAST chunk only, with check_last_plane, and never without
    mpi = MPI(variant="band", strict_order=True, on_out_of_plane="raise")
    bent = ray.clone()
    bent[1, :, -1, -1] = torch.tensor([0.8, 0.0, 0.6], device="cuda")
    words = []
    with torch.no_grad():
        cr = mpi.chunked_render(dhw, bent, eye, zd, check_last_plane=True, defer_status=True, chunk_kernel=kernel)
        for c in _cut(vol, split):
            cr.add(c)
            words.append(int(cr.status[0].item()))
        cr.finish()
        assert [w & _lib.STATUS_OUT_OF_LAST_PLANE for w in words] == [0, 0, _lib.STATUS_OUT_OF_LAST_PLANE]
        res = mpi.render_views_chunks(_cut(vol, split), dhw, bent, eye, zd, check_last_plane=False, defer_status=True, chunk_kernel=kernel)
        assert not int(res["status"][0].item()) & _lib.STATUS_OUT_OF_LAST_PLANE
        with pytest.raises(RuntimeError, match="goes out of plane"):
            mpi.render_views_chunks(_cut(vol, split), dhw, bent, eye, zd, check_last_plane=True, chunk_kernel=kernel)
    # the camera behind a plane of the MIDDLE chunk: GMPI_STATUS_CAMERA_BEHIND_PLANE appears with that chunk's launch
    behind = dhw.clone()
    behind[:, 3, 0] = float(eye[0, 2].item()) - 0.5
    words = []
    with torch.no_grad():
        cr = mpi.chunked_render(behind, ray, eye, zd, defer_status=True, chunk_kernel=kernel)
        for c in _cut(vol, split):
            cr.add(c)
            words.append(int(cr.status[0].item()) & _lib.STATUS_CAMERA_BEHIND_PLANE)
    assert words == [0, _lib.STATUS_CAMERA_BEHIND_PLANE, _lib.STATUS_CAMERA_BEHIND_PLANE]


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["backward_ffhq_d8_32", "backward_ffhq_d8_32_opaque"])
def test_autograd_through_band_chunks_matches_the_fixtures(name):
    """The forward of `_ChunkedRenderFunction` through the band kernel, the chunk backward unchanged: test_hip_chunks.py's bars -- 1e-4 of the largest
    gradient against the reference's own autograd, 1e-5 against the one-shot backward (default mode; the backward reads the T images the forward kept)."""
    from ml_gmpi_amd import MPI
    fx = load_npz(name + ".npz")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    N, Dp = fx["ray_dir"].shape[0], fx["rgba"].shape[1]
    v2m = fx["view_to_mpi"] if "view_to_mpi" in fx else np.arange(N, dtype=np.int32)
    geo = (t(fx["dhw"]), t(fx["ray_dir"]), t(fx["eye"]), t(fx["zdir"]))
    kw = dict(view_to_mpi=t(v2m.astype(np.int32)), check_last_plane=False, out_pm1="ref_rgb_pm1" in fx)
    ref_g = fx["ref_grad_rgba"]
    scale = np.abs(ref_g).max()

    def run(split, kernel):
        mpi = MPI(align_corners=fx["meta"]["ac"], on_out_of_plane="raise")
        vol = t(fx["rgba"])
        if split is None:
            leaves = [vol.requires_grad_(True)]
            out = mpi.render_views(vol, *geo, **kw)
        else:
            leaves = [c.requires_grad_(True) for c in _cut(vol, split)]
            out = mpi.render_views_chunks(leaves, *geo, chunk_kernel=kernel, **kw)
        ((out["color"] * t(fx["g_rgb"])).sum() + (out["depth"] * t(fx["g_depth"])).sum()).backward()
        torch.cuda.synchronize()
        assert mpi.chunk_band_fallbacks == 0
        return torch.cat([c.grad.float() for c in leaves], 1).cpu().numpy()

    one = run(None, None)
    for kernel in KERNELS:
        for split in ((3, Dp - 3), (1,) * Dp):
            got = run(split, kernel)
            err_ref, err_one = np.abs(got - ref_g).max(), np.abs(got - one).max()
            print(f"{name} {kernel} {split}: |chunked - fixture| {err_ref / scale:.2e}, |chunked - one-shot| {err_one / scale:.2e} of the largest gradient")
            assert np.isfinite(got).all()
            assert err_ref <= 1e-4 * scale, (name, kernel, split, err_ref, scale)
            assert err_one <= 1e-5 * scale, (name, kernel, split, err_one, scale)
    # the T images the forward keeps per chunk (what the backward starts from), strict order: the tile path's, bit for bit
    strict = MPI(align_corners=fx["meta"]["ac"], variant="lds", strict_order=True, on_out_of_plane="raise")
    Ts = {}
    with torch.no_grad():
        for kernel in (None,) + KERNELS:
            cr = strict.chunked_render(*geo, view_to_mpi=kw["view_to_mpi"], defer_status=True, chunk_kernel=kernel)
            Ts[kernel] = []
            for c in _cut(t(fx["rgba"]), (3, 1, Dp - 4)):
                T = torch.full((N, 1) + tuple(geo[1].shape[2:]), float("nan"), device="cuda")
                cr.add(c, _T=T)
                Ts[kernel].append(T)
            cr.finish()
    for kernel in KERNELS:
        for a, b in zip(Ts[kernel], Ts[None]):
            assert torch.equal(a, b), kernel


# ---- fallback ---------------------------------------------------------------------------------------------------------------------------------------
def test_uint8_chunks_fall_back_to_todays_path_and_are_counted():
    from ml_gmpi_amd import MPI
    vol, geo = _on_device("f32", "ragged")
    codes = (vol * 255).round().to(torch.uint8)
    split = (3, 1, vol.shape[1] - 4)
    for strict in (True, False):
        mpi = MPI(strict_order=strict, on_out_of_plane="raise")
        want = _chunked(mpi, codes, geo, split, None)
        for n, kernel in enumerate(KERNELS, 1):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)   # (the fallback's warning, given once per process)
                got = _chunked(mpi, codes, geo, split, kernel)
            for k in KEYS + ("status",):
                assert np.array_equal(got[k], want[k]), (strict, kernel, k)
            assert mpi.chunk_band_fallbacks == 3 * n and mpi.chunk_variant_fallbacks == 0

