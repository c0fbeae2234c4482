"""GPU tests of the shaded render of an RGBA volume (MPI.render_views_shaded, gmpi_mpi_render_shaded_launch / _backward_launch, render_shaded.hip):
by definition the render of apply_shading(rgba, shading), which the kernels never build.

Bars: strict-order mode == oracle.render on the shaded volume, bit for bit; default mode colour <= 0.5 TOL on the [0, 1] scale, depth and T <= TOL
(TOL of tests/test_hip_parity.py); gradients: max(5e-5, 4 e_ref) max|g_ref| + 1e-6 per gradient tensor (+ the format's half ulp for 16-bit
inputs), the rule of tests/test_hip_shared_color.py.  The shading is random per texel in [0.4, 1.6]: the clip bites for 10-60 % of the colour
texels of every case, and no product lies within 1e-3 of the kink at 1 (the shading is nudged where one does), so that the fp32 and float64
references agree on the mask."""
import itertools
import warnings

import numpy as np
import pytest
import torch

import oracle
import _transmittance_ref
from _util import load_npz
from test_hip_parity import TOL, _random_case
from test_hip_shared_color import _half_ulp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def make_shading(seed, vol):
    """vol: CPU float32 tensor holding the STORED values [M,D,4,Ht,Wt] -> shading [M,1,Ht,Wt] fp32 in [0.4, 1.6] (a little above where nudged)."""
    M, _, _, Ht, Wt = vol.shape
    s = 0.4 + 1.2 * torch.rand((M, 1, Ht, Wt), generator=torch.Generator().manual_seed(1000 + seed))
    rgb = vol[:, :, :3].float()
    for _ in range(40):
        near = ((rgb * s[:, None] - 1).abs() < 1e-3).flatten(1, 2).any(1, keepdim=True)
        if not bool(near.any()):
            break
        s = torch.where(near, s * 1.004, s)
    p32, p64 = rgb * s[:, None], rgb.double() * s.double()[:, None]
    assert not bool(((p32 - 1).abs() < 1e-3).any())
    assert bool(((p32 > 1) == (p64 > 1)).all()) and bool(((p32 >= 0) == (p64 >= 0)).all())
    frac = float((p32 > 1).float().mean())
    assert 0.10 <= frac <= 0.60, frac
    return s


def stored(rgba, dtype):
    """The values a volume of `dtype` holds, as CPU float32."""
    return rgba.to(dtype).float()


def shaded_volume(vol, s, dtype=torch.float32):
    """apply_shading in `dtype` (float64: the reference chain; float32: the definition itself)."""
    from ml_gmpi_amd import apply_shading
    if dtype == torch.float32:
        return apply_shading(vol, s)
    return torch.cat((torch.clip(vol[:, :, :3].to(dtype) * s.to(dtype)[:, None], 0.0, 1.0), vol[:, :, 3:].to(dtype)), 2)


_CASES = {}


def case(name, dtype=torch.float32, ac=True, v2m=None, **cfg):
    """Inputs, shading and the oracle's render of the shaded volume, computed once per (name, dtype, ac) and left unchanged."""
    key = (name, dtype, ac)
    if key not in _CASES:
        M = cfg.pop("M", None)
        rgba, dhw, ray, eye, zd = _random_case(**cfg)
        if M is not None:
            rgba, dhw = rgba[:M], dhw[:M]
        vol = stored(rgba, dtype)
        s = make_shading(cfg["seed"], vol)
        orc = oracle.render(shaded_volume(vol, s).numpy(), dhw, ray, eye, zd, view_to_mpi=v2m, align_corners=ac, threads=True)
        _CASES[key] = (vol, s, dhw, ray, eye, zd, orc)
    return _CASES[key]


def shaded_render(vol, s, dhw, ray, eye, zd, *, dtype=torch.float32, ac=True, variant="auto", strict=False, views_per_mpi=1, view_to_mpi=None,
                  check_last=True, range_check="touched", out_pm1=False, prep=None, two_step=False):
    """MPI.render_views_shaded on the device -> numpy dict.  prep(vol_t, s_t) -> (vol_t, s_t): the tensors as the case wants them laid out.
    two_step: render_views of apply_shading on the device instead."""
    from ml_gmpi_amd import MPI, apply_shading
    dev = torch.device(DEV)
    t = lambda a: torch.as_tensor(a).to(dev)
    vol_t, s_t = t(vol).to(dtype), t(s)
    if prep is not None:
        vol_t, s_t = prep(vol_t, s_t)
    mpi = MPI(align_corners=ac, variant=variant, strict_order=strict, range_check=range_check, on_out_of_plane="raise")
    v2m = None if view_to_mpi is None else t(np.asarray(view_to_mpi, dtype=np.int32))
    kw = dict(views_per_mpi=views_per_mpi, view_to_mpi=v2m, check_last_plane=check_last, want_transmittance=True, out_pm1=out_pm1)
    with torch.no_grad():
        if two_step:
            out = mpi.render_views(apply_shading(vol_t, s_t), t(dhw), t(ray), t(eye), t(zd), **kw)
        else:
            out = mpi.render_views_shaded(vol_t, s_t, t(dhw), t(ray), t(eye), t(zd), **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


# ---- spies on the C ABI: which variant reached the launch, what the support query said -------------------------------------------------------
@pytest.fixture
def abi(monkeypatch):
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    real_launch, real_supports = lib.gmpi_mpi_render_shaded_launch, lib.gmpi_render_shaded_supports
    seen = dict(launched=[], supports=[])

    def launch(p, sh, stream):
        seen["launched"].append(int(p._obj.variant))
        return real_launch(p, sh, stream)

    def supports(p, sh):
        rc = real_supports(p, sh)
        seen["supports"].append(rc)
        return rc
    monkeypatch.setattr(lib, "gmpi_mpi_render_shaded_launch", launch)
    monkeypatch.setattr(lib, "gmpi_render_shaded_supports", supports)
    return seen


def check_forward(abi, c, *, dtype=torch.float32, ac=True, must_stage=True, variants=("gather", "lds", "auto"), **kw):
    from ml_gmpi_amd import _lib as L
    vol, s, dhw, ray, eye, zd, orc = c
    for variant in variants:
        abi["launched"].clear(), abi["supports"].clear()
        strict = shaded_render(vol, s, dhw, ray, eye, zd, dtype=dtype, ac=ac, variant=variant, strict=True, **kw)
        fast = shaded_render(vol, s, dhw, ray, eye, zd, dtype=dtype, ac=ac, variant=variant, **kw)
        if variant == "gather":
            assert abi["launched"] == [L.VARIANT_GATHER] * 2 and abi["supports"] == [], abi
        elif must_stage:   # an explicit "lds" (and "auto") reaches the staged kernel: no silent fall-back
            assert abi["supports"] == [1, 1] and abi["launched"] == [L.VARIANT_LDS] * 2, (variant, abi)
        else:
            assert all(q in (0, 1) for q in abi["supports"]) and len(abi["supports"]) == 2, abi
            assert abi["launched"] == [L.VARIANT_LDS if q == 1 else L.VARIANT_GATHER for q in abi["supports"]], abi
        for k in ("color", "depth", "T"):
            assert np.array_equal(strict[k], orc[k]), (variant, k, np.abs(strict[k] - orc[k]).max())
        errs = {k: float(np.abs(fast[k] - orc[k]).max()) for k in ("color", "depth", "T")}
        print(variant, "default mode", errs)
        assert errs["color"] <= 0.5 * TOL and errs["depth"] <= TOL and errs["T"] <= TOL, (variant, errs)
        assert int(strict["status"][0]) == 0 and int(fast["status"][0]) == 0


# ---- 1. forward against the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ac", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_matches_the_oracle_on_the_shaded_volume(abi, dtype, ac):
    check_forward(abi, case("fwd", dtype, ac, seed=1, B=2, D=8, S=96), dtype=dtype, ac=ac)


# ---- 2. ragged and strided inputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,must", [(80, True), (77, False)])
def test_ragged_image_and_texture_widths(abi, T, must):
    """100 x 100 pixels: the last tile row and column are ragged.  Wt = 80 must be staged; Wt = 77: rows are not 16-byte aligned, the query may refuse."""
    check_forward(abi, case(("ragged", T), seed=4, B=3, D=7, S=100, T=T), must_stage=must)


def test_views_per_mpi_and_view_to_mpi(abi):
    c = case("vpm", seed=6, B=4, D=6, S=64, M=2, v2m=[0, 0, 1, 1])
    check_forward(abi, c, views_per_mpi=2)
    c = case("v2m", seed=6, B=4, D=6, S=64, M=2, v2m=[1, 0, 0, 1])
    check_forward(abi, c, view_to_mpi=[1, 0, 0, 1])


def test_expanded_and_row_padded_shading(abi):
    """One MPI, three views, the shading an `expand`ed image (MPI stride 0); then a shading whose rows are padded to 72 elements; then both tensors
    with a ragged width inside aligned rows (Wt = 62 in rows of 64: the staged kernel zeroes the texels past the row's end)."""
    c = case("expanded", seed=7, B=3, D=5, S=64, M=1, v2m=[0, 0, 0])
    seen = []

    def expanded(vol_t, s_t):
        e = torch.as_strided(s_t, (1, 1) + tuple(s_t.shape[2:]), (0, 0, s_t.stride(2), 1))   # (what `expand` of one image over a batch leaves)
        assert e.stride(0) == 0
        seen.append(e.data_ptr())
        return vol_t, e
    check_forward(abi, c, views_per_mpi=3, prep=expanded)

    def padded(vol_t, s_t):
        buf = torch.full((s_t.shape[0], 1, s_t.shape[2], s_t.shape[3] + 8), float("nan"), device=s_t.device)
        buf[..., :s_t.shape[3]] = s_t
        v = buf[..., :s_t.shape[3]]
        assert v.stride(2) == s_t.shape[3] + 8
        return vol_t, v
    check_forward(abi, c, views_per_mpi=3, prep=padded)

    c = case("ragged-in-rows", seed=8, B=2, D=5, S=64, T=62)

    def both_padded(vol_t, s_t):
        vb = torch.full(vol_t.shape[:-1] + (64,), 7.0, device=vol_t.device, dtype=vol_t.dtype)
        vb[..., :62] = vol_t
        sb = torch.full(s_t.shape[:-1] + (64,), float("nan"), device=s_t.device)
        sb[..., :62] = s_t
        return vb[..., :62], sb[..., :62]
    check_forward(abi, c, prep=both_padded)


@pytest.mark.parametrize("D", [1, 63, 64, 66])
def test_plane_counts_around_the_box_table_refill(abi, D):
    """Thin alphas (tests/_visible.py): every plane counts across the 64-plane refill of the box table."""
    c = case(("planes", D), seed=9, B=1, D=D, S=64, alpha="thin")
    check_forward(abi, c, variants=("gather", "lds"))


def test_texture_four_times_finer_than_the_image_gathers_in_the_kernel(abi):
    """32 x 32 pixels over 128 x 128 texels: a tile's box is ~128 texels wide, none fits the 56 x 27 buffer -- the staged kernel samples every plane
    directly, and strict order gives the one-pixel kernel's bits (both are compared with the oracle's)."""
    c = case("fine", seed=10, B=2, D=4, S=32, T=128)
    check_forward(abi, c, variants=("gather", "lds"))


# ---- 2b. the paths the staged kernel shares with the shared-colour one (its namesakes: tests/test_hip_shared_forward_staged.py, the same shapes) -----------
def _strict_pair(abi, vol, s, dhw, ray, eye, zd):
    """(staged kernel, one-pixel kernel) in strict order; the staged kernel was reached."""
    from ml_gmpi_amd import _lib as L
    abi["launched"].clear(), abi["supports"].clear()
    a = shaded_render(vol, s, dhw, ray, eye, zd, variant="lds", strict=True, check_last=False)
    assert abi["supports"] == [1] and abi["launched"] == [L.VARIANT_LDS], abi
    b = shaded_render(vol, s, dhw, ray, eye, zd, variant="gather", strict=True, check_last=False)
    return a, b


def test_nan_ray_component_gives_the_one_pixel_kernels_pixels(abi):
    """The per-lane direct path of the staged kernel (shaded_gather_sample) and a tile none of whose boxes fits."""
    vol, s, dhw, ray, eye, zd, _ = case("fwd", torch.float32, True, seed=1, B=2, D=8, S=96)
    ray = torch.as_tensor(ray).clone()
    ray[0, 0, 50, 41] = float("nan")      # inside a tile: that pixel alone
    ray[1, 2, 0, 0] = float("nan")        # a tile corner: the tile's boxes do not fit
    a, b = _strict_pair(abi, vol, s, dhw, ray, eye, zd)
    for k in ("color", "depth", "T"):
        assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert np.isnan(a["depth"][0, 0, 50, 41]) and int(np.isnan(a["depth"]).sum()) == 2
    assert int(a["status"][0]) == 0 and int(b["status"][0]) == 0


def test_staged_and_gathered_planes_in_one_launch(abi):
    from test_hip_shared_forward_staged import _boxes, _fit_counts
    vol, s, dhw, ray, eye, zd, _ = case("mixed", seed=2, B=2, D=12, S=112, T=128, extreme=True)
    spare, never, n = _fit_counts(_boxes(dhw, ray, eye, 128, 128, True))
    print("mixed case: boxes that fit with spare", spare, "never", never, "of", n)
    assert spare > 0 and never > 0, (spare, never, n)
    a, b = _strict_pair(abi, vol, s, dhw, ray, eye, zd)
    for k in ("color", "depth", "T"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def _lds_status(vol, s, dhw, ray, eye, zd):
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    t = lambda a: torch.as_tensor(a).to(dev)
    mpi = MPI(variant="lds", on_out_of_plane="raise")
    with torch.no_grad():
        out = mpi.render_views_shaded(t(vol), t(s), t(dhw), t(ray), t(eye), t(zd), defer_status=True)
    word = int(out["status"][0].item())
    out["status"].zero_()
    return word


@pytest.mark.parametrize("path", ["staged", "in-kernel gather"])
def test_alpha_above_one_sets_the_range_bit_and_a_colour_above_one_before_the_clip_does_not(abi, path):
    """staged: every box fits, the poked texel is the image centre, which every frontal view samples.  in-kernel gather: no box fits (256^2 texels under
    32^2 pixels), pixels are 8 texels apart, so a block of 17 x 17 texels around the centre is poked: some footprint lies in it."""
    from ml_gmpi_amd import _lib as L
    from test_hip_shared_forward_staged import _boxes, _fit_counts
    if path == "staged":
        vol, s, dhw, ray, eye, zd, _ = case("range", seed=3, B=1, D=5, S=64)
        T, poke = 64, (slice(32, 33), slice(32, 33))
    else:
        vol, s, dhw, ray, eye, zd, _ = case("range-fine", seed=32, B=2, D=5, S=32, T=256)
        T, poke = 256, (slice(120, 137), slice(120, 137))
        spare, never, n = _fit_counts(_boxes(dhw, ray, eye, T, T, True))
        assert never == n, (spare, never, n)
    assert float((vol[:, :, :3] * s[:, None] > 1).float().mean()) >= 0.10   # colours above one before the clip, all over the volume
    assert _lds_status(vol, s, dhw, ray, eye, zd) == 0
    bad = vol.clone()
    bad[0, 0, 3, poke[0], poke[1]] = 1.5
    assert _lds_status(bad, s, dhw, ray, eye, zd) == 2, path
    assert abi["launched"] == [L.VARIANT_LDS] * 2 and abi["supports"] == [1, 1], abi


# ---- 3. equal to the two-step path on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_strict_bits_equal_the_render_of_apply_shading_on_the_device(dtype):
    vol, s, dhw, ray, eye, zd, _ = case("fwd", dtype, True, seed=1, B=2, D=8, S=96)
    for variant in ("gather", "auto"):
        a = shaded_render(vol, s, dhw, ray, eye, zd, dtype=dtype, variant=variant, strict=True)
        b = shaded_render(vol, s, dhw, ray, eye, zd, dtype=dtype, variant="gather", strict=True, two_step=True)
        for k in ("color", "depth", "T"):
            assert np.array_equal(a[k], b[k]), (variant, k)


def test_unit_shading_gives_the_plain_render():
    vol, _, dhw, ray, eye, zd, _ = case("fwd", torch.float32, True, seed=1, B=2, D=8, S=96)
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    t = lambda a: torch.as_tensor(a).to(dev)
    for variant in ("gather", "auto"):
        mpi = MPI(variant=variant, strict_order=True, on_out_of_plane="raise")
        with torch.no_grad():
            a = mpi.render_views_shaded(t(vol), torch.ones((2, 1, 96, 96), device=dev), t(dhw), t(ray), t(eye), t(zd), want_transmittance=True)
            b = mpi.render_views(t(vol), t(dhw), t(ray), t(eye), t(zd), want_transmittance=True)
        for k in ("color", "depth", "T"):
            assert torch.equal(a[k], b[k]), (variant, k)


def _light_pair(D, S, seed):
    import ml_gmpi_amd
    dev = torch.device(DEV)
    r = ml_gmpi_amd.make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise", strict_order=True)
    Ls = [ml_gmpi_amd.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, ka_max=0.9, kd_max=0.9, n_grow_iters=1) for _ in range(2)]
    for L in Ls:
        L.step = 10
    xyz, _ = r.get_xyz(S, S, ret_single_res=True)
    return r, Ls, xyz


def test_shading_image_then_render_views_shaded_equals_light_render_then_render_views():
    import ml_gmpi_amd
    from ml_gmpi_amd import MPI, apply_shading
    from _visible import make_alpha
    dev = torch.device(DEV)
    D, S = 8, 64
    rgba, dhw, ray, eye, zd = _random_case(seed=11, B=2, D=D, S=S)
    vol = make_alpha(rgba, "surface").to(dev)   # (a depth image with structure: the Lambert term varies)
    r, (L1, L2), xyz = _light_pair(D, S, 11)
    t = lambda a: torch.as_tensor(a).to(dev)
    with torch.no_grad():
        torch.manual_seed(3)
        shaded = L1.render(vol, r.static_mpi_plane_dhws, xyz)
        state = torch.get_rng_state()
        torch.manual_seed(3)
        s = L2.shading_image(vol, r.static_mpi_plane_dhws, xyz)
        assert torch.equal(state, torch.get_rng_state())
        assert (L1.step, L1.cur_ka, L1.cur_kd) == (L2.step, L2.cur_ka, L2.cur_kd)
        assert s.shape == (2, 1, S, S) and s.dtype == torch.float32 and float(s.std()) > 1e-3
        assert torch.equal(apply_shading(vol, s), shaded)
        for variant in ("gather", "auto"):
            mpi = MPI(variant=variant, strict_order=True, on_out_of_plane="raise")
            a = mpi.render_views_shaded(vol, s, t(dhw), t(ray), t(eye), t(zd), want_transmittance=True)
            b = mpi.render_views(shaded, t(dhw), t(ray), t(eye), t(zd), want_transmittance=True)
            for k in ("color", "depth", "T"):
                assert torch.equal(a[k], b[k]), (variant, k)


def test_nan_colour_texel_and_alpha_above_one_give_the_two_step_paths_outputs_and_status():
    """A NaN colour texel is shaded to 0, as gmpi_light_apply_launch shades it; an alpha of 1.5 sets the range bit.  Compared on the device with
    gmpi_light_apply_launch followed by render_views (torch.clip would keep the NaN)."""
    import ctypes
    from ml_gmpi_amd import MPI
    from ml_gmpi_amd.hip_mpi import _call
    vol, s, dhw, ray, eye, zd, _ = case("fwd", torch.float32, True, seed=1, B=2, D=8, S=96)
    dev = torch.device(DEV)
    t = lambda a: torch.as_tensor(a).to(dev)
    bad = t(vol).clone()
    bad[0, 0, 1, 40:44, 40:44] = float("nan")
    bad[1, 1, 3, 50, 50] = 1.5
    s_t = t(s)
    two = torch.empty_like(bad)
    _call("gmpi_light_apply_launch", dev, bad.data_ptr(), 0, (ctypes.c_int64 * 5)(*bad.stride()), s_t.data_ptr(), two.data_ptr(), 2, 8, 96, 96)
    assert not bool(torch.isnan(two[:, :, :3]).any())
    for variant in ("gather", "auto"):
        mpi = MPI(variant=variant, strict_order=True, on_out_of_plane="raise")
        with torch.no_grad():
            a = mpi.render_views_shaded(bad, s_t, t(dhw), t(ray), t(eye), t(zd), want_transmittance=True, defer_status=True)
            b = mpi.render_views(two, t(dhw), t(ray), t(eye), t(zd), want_transmittance=True, defer_status=True)
        for k in ("color", "depth", "T"):
            assert torch.equal(a[k], b[k]), (variant, k)
        assert int(a["status"][0].item()) == int(b["status"][0].item()) == 2, (variant, a["status"], b["status"])
        a["status"].zero_(), b["status"].zero_()


# ---- 4. gradients ---------------------------------------------------------------------------------------------------------------------------------
def _reference_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, out_pm1, dtype, align_corners=True):
    """d(sum gC colour + sum gZ depth + sum gT T) / d(vol, s) of tests/_transmittance_ref.render(apply_shading(vol, s)) in `dtype` on the CPU."""
    ins = [vol.to(dtype).clone().requires_grad_(True), s.to(dtype).clone().requires_grad_(True)]
    c = lambda a: torch.as_tensor(a).to(dtype)
    color, depth, T = _transmittance_ref.render(shaded_volume(ins[0], ins[1], dtype), c(dhw), c(ray), c(eye), c(zd), v2m, align_corners=align_corners)
    if out_pm1:
        color = 2 * color - 1
    loss = torch.zeros((), dtype=dtype)
    for out, g in ((color, gc), (depth, gd), (T, gT)):
        if g is not None:
            loss = loss + (out * c(g)).sum()
    loss.backward()
    return [(i.grad if i.grad is not None else torch.zeros_like(i)).double().numpy() for i in ins]


def _hip_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, out_pm1, variant, dtype, needs=(True, True), backward="atomic", align_corners=True,
               range_check=None, views_per_mpi=None, prep=None):
    """-> (the two leaves, the module).  views_per_mpi: uniform views instead of the index v2m.  prep(vol_t, s_t) -> (vol_t, s_t): the tensors the
    render is given, as views (or functions) of the leaves; ins stays the leaves."""
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    t = lambda a: torch.as_tensor(a).to(dev)
    ins = [t(vol).to(dtype).requires_grad_(needs[0]), t(s).clone().requires_grad_(needs[1])]
    mpi = MPI(align_corners=align_corners, variant=variant, on_out_of_plane="raise", backward=backward, range_check=range_check)
    views = dict(view_to_mpi=t(np.asarray(v2m, dtype=np.int32))) if views_per_mpi is None else dict(views_per_mpi=views_per_mpi)
    vol_t, s_t = (ins[0], ins[1]) if prep is None else prep(ins[0], ins[1])
    out = mpi.render_views_shaded(vol_t, s_t, t(dhw), t(ray), t(eye), t(zd), check_last_plane=False, out_pm1=out_pm1, want_transmittance=True, **views)
    loss = 0
    for key, g in (("color", gc), ("depth", gd), ("T", gT)):
        if g is not None:
            loss = loss + (out[key] * t(g)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return ins, mpi


def _compare(got, ref64, ref32, dtypes, label):
    failures = []
    for name, g, r64, r32, dt in zip(("vol", "shading"), got, ref64, ref32, dtypes):
        scale = float(np.abs(r64).max())
        e_ref = float(np.abs(r32 - r64).max()) / scale if scale > 0 else 0.0
        bound = max(5e-5, 4 * e_ref) * scale + 1e-6 + _half_ulp(np.maximum(np.abs(g), np.abs(r64)), dt)
        err = np.abs(g - r64)
        worst = float((err - bound).max())
        print(f"{label} {name}: max|g_ref| {scale:.3e} e_ref {e_ref:.2e} max err {float(err.max()):.3e} margin {worst:.2e}")
        if worst > 0:
            failures.append((name, float(err.max()), scale, e_ref))
    assert not failures, (label, failures)


def _bwd_case(name, D, S, dtype, seed=5, extreme=False):
    key = ("bwd", name, dtype)
    if key not in _CASES:
        rgba, dhw, ray, eye, zd = _random_case(seed=seed, B=3, D=D, S=S, extreme=extreme)
        vol = stored(rgba[:2], dtype)
        s = make_shading(seed, vol)
        g = np.random.default_rng(7)
        gc, gd, gT = (g.standard_normal((3, ch, S, S)).astype(np.float32) for ch in (3, 1, 1))
        _CASES[key] = (vol, s, dhw[:2], ray, eye, zd, [0, 0, 1], gc, gd, gT)
    return _CASES[key]


COMBOS = [c for c in itertools.product([True, False], repeat=3) if any(c)]   # (g_color, g_depth, g_T): every combination that reaches an output


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "".join(n for n, on in zip("CZT", c) if on))
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_matches_float64_autograd_through_apply_shading(dtype, combo):
    vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT = _bwd_case("d8", 8, 64, dtype)
    gc, gd, gT = (g if on else None for g, on in zip((gc, gd, gT), combo))
    for out_pm1 in ((False, True) if combo[0] else (False,)):
        ref64 = _reference_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, out_pm1, torch.float64)
        ref32 = _reference_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, out_pm1, torch.float32)
        for variant in ("auto", "gather"):   # the 64 x 8 tile backward | the one-pixel backward
            ins, _ = _hip_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, out_pm1, variant, dtype)
            assert ins[0].grad.dtype == dtype and ins[0].grad.shape == ins[0].shape and ins[1].grad.dtype == torch.float32 and ins[1].grad.shape == ins[1].shape
            got = [i.grad.double().cpu().numpy() for i in ins]
            _compare(got, ref64, ref32, (dtype, torch.float32), f"{variant} pm1={out_pm1}")


def test_backward_partial_needs():
    """Only the volume requires grad, then only the shading: the other gets no gradient (and no buffer: the memory test below measures it; the
    shading-only backward runs the chain rule per tap in the one-pixel kernel, whatever the variant)."""
    vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT = _bwd_case("d8", 8, 64, torch.float32)
    ref64 = _reference_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, False, torch.float64)
    ref32 = _reference_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, False, torch.float32)
    for needs in ((True, False), (False, True)):
        for variant in ("auto", "gather"):
            ins, _ = _hip_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, False, variant, torch.float32, needs=needs)
            for i, (inp, need) in enumerate(zip(ins, needs)):
                assert (inp.grad is not None) == need
                if need:
                    got = inp.grad.double().cpu().numpy()
                    _compare([got], [ref64[i]], [ref32[i]], (torch.float32,), f"{variant} needs={needs}")


def test_backward_extreme_poses_tiles_straddle_the_texture_border():
    vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT = _bwd_case("extreme", 16, 256, torch.float32, seed=6, extreme=True)
    ref64 = _reference_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, True, torch.float64)
    ref32 = _reference_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, True, torch.float32)
    for variant in ("auto", "gather"):
        ins, _ = _hip_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, True, variant, torch.float32)
        _compare([i.grad.double().cpu().numpy() for i in ins], ref64, ref32, (torch.float32, torch.float32), f"extreme {variant}")


# ---- 5. the G-step chain ---------------------------------------------------------------------------------------------------------------------------
def test_g_step_chain_shading_image_render_shaded_against_light_render_render():
    from _visible import make_alpha
    dev = torch.device(DEV)
    D, S = 8, 64
    rgba, _, _, _, _ = _random_case(seed=12, B=2, D=D, S=S)
    base = make_alpha(rgba, "surface")
    base[:, D - 1, 3] = 1.0
    r, (L1, L2), xyz = _light_pair(D, S, 12)
    g = np.random.default_rng(5)
    gc, gd = (torch.from_numpy(g.standard_normal((2, ch, S, S)).astype(np.float32)).to(dev) for ch in (3, 1))
    outs, grads = [], []
    for fused in (False, True):
        vol = base.to(dev).requires_grad_(True)
        torch.manual_seed(4)
        if fused:
            s = L2.shading_image(vol, r.static_mpi_plane_dhws, xyz)
            rgb, depth, c2w, ang = r.render_shaded(vol, s, S, S)
        else:
            rgb, depth, c2w, ang = r.render(L1.render(vol, r.static_mpi_plane_dhws, xyz), S, S)
        ((rgb * gc).sum() + (depth * gd).sum()).backward()
        torch.cuda.synchronize()
        outs.append((rgb.detach(), depth.detach(), c2w, ang, torch.get_rng_state()))
        grads.append(vol.grad.double().cpu().numpy())
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))
    # both chains run the same fp32 op chain up to the order of the atomic adds: the two-step chain stands for the fp32 reference, and the bound is the
    # project's 5e-5 of the largest gradient (+ 1e-6)
    scale = float(np.abs(grads[0]).max())
    err = float(np.abs(grads[0] - grads[1]).max())
    print(f"G-step chain: max|g| {scale:.3e} max difference {err:.3e}")
    assert err <= 5e-5 * scale + 1e-6, (err, scale)
    assert float(np.abs(grads[1][:, :, 3]).max()) > 0 and float(np.abs(grads[1][:, :, :3]).max()) > 0


def test_g_step_gradient_against_a_float64_torch_chain():
    """An independent reference for the gradient that reaches the volume through BOTH the render and the shading image: tests/_torch_ref.py's
    torch_light_render (the reference's LightRenderer.render in plain torch) followed by tests/_transmittance_ref.render, in float64, against the same
    chain in fp32 on the CPU -- the rule of (4).  The colours are moved off the clip's kink (no product within 1e-3 of 1), as everywhere in this file."""
    from _torch_ref import torch_light_render
    from _visible import make_alpha
    from ml_gmpi_amd import MPI, poses
    dev = torch.device(DEV)
    D, S = 8, 64
    rgba, dhw, ray, eye, zd = _random_case(seed=14, B=2, D=D, S=S)
    base = make_alpha(rgba, "surface")
    r, (L, _), xyz = _light_pair(D, S, 14)
    plane_ds, xyz_last = r.static_mpi_plane_dhws[:, 0].cpu(), xyz[-1, :, :, :3].cpu()
    torch.manual_seed(4)   # the light the seeded shading_image call below draws
    c2w, _, _ = poses.gen_sphere_path(n_cams=2, sphere_center=L.sphere_center, sphere_r=1.0, yaw_mean=L.l_h_mean, yaw_std=L.l_h_std,
                                      pitch_mean=L.l_v_mean, pitch_std=L.l_v_std, n_truncated_stds=2, flag_rnd=True, sample_method="truncated_gaussian")
    ld = poses._unit(L.sphere_center.reshape(1, 3) - torch.FloatTensor(c2w[:, :3, 3]))
    ka = kd = 0.9   # (_light_pair: step 10 -> 11 of a one-step ramp)
    chain = lambda v, dt: torch_light_render(v, plane_ds.to(dt), xyz_last.to(dt), ld.to(dt), ka, kd, L._k1d.to(dt))
    half = base.clone()
    half[:, :, :3] = 0.5
    s64 = chain(half.double(), torch.float64)[:, 0, :1] / 0.5                    # the shading itself: 0.5 s < 1 is never clipped
    assert float(s64.max()) < 2.0 and float(s64.std()) > 1e-3
    for _ in range(40):
        near = (base[:, :, :3].double() * s64[:, None] - 1).abs() < 1e-3
        if not bool(near.any()):
            break
        base[:, :, :3] = torch.where(near, base[:, :, :3] * 0.99, base[:, :, :3])
    assert not bool(((base[:, :, :3].double() * s64[:, None] - 1).abs() < 1e-3).any())
    g = np.random.default_rng(9)
    gc, gd = (g.standard_normal((2, ch, S, S)).astype(np.float32) for ch in (3, 1))
    refs = []
    for dt in (torch.float64, torch.float32):
        vin = base.to(dt).clone().requires_grad_(True)
        c = lambda a: torch.as_tensor(a).to(dt)
        color, depth, _ = _transmittance_ref.render(chain(vin, dt), c(dhw), c(ray), c(eye), c(zd), [0, 1])
        ((color * c(gc)).sum() + (depth * c(gd)).sum()).backward()
        refs.append(vin.grad.double().numpy())
    t = lambda a: torch.as_tensor(a).to(dev)
    for variant in ("auto", "gather"):
        L2 = _light_pair(D, S, 14)[1][0]
        vol = base.to(dev).requires_grad_(True)
        torch.manual_seed(4)
        s = L2.shading_image(vol, r.static_mpi_plane_dhws, xyz)
        assert (L2.cur_ka, L2.cur_kd) == (ka, kd)
        # the reference's light is the one this call drew: another draw of the light moves the shading by 1e-2 and more, the fp32 kernels' own noise
        # (normals from differences of neighbouring points) is 1e-5 .. 1e-4 here -- the accuracy of the shading itself is tests/test_light_render.py's
        assert float((s.detach().cpu().double() - s64).abs().max()) <= 1e-3
        out = MPI(variant=variant, on_out_of_plane="raise").render_views_shaded(vol, s, t(dhw), t(ray), t(eye), t(zd), check_last_plane=False)
        ((out["color"] * t(gc)).sum() + (out["depth"] * t(gd)).sum()).backward()
        torch.cuda.synchronize()
        got = vol.grad.double().cpu().numpy()
        _compare([got], [refs[0]], [refs[1]], (torch.float32,), f"G-step against float64, {variant}")
        _compare([got[:, :, 3:]], [refs[0][:, :, 3:]], [refs[1][:, :, 3:]], (torch.float32,), f"G-step against float64, alpha channel, {variant}")


def test_lds_module_falls_back_counted_and_warned_once():
    """variant="lds" by name over tensors the staged loader cannot take (a volume whose base is 4 bytes off a 16-byte boundary): the one-pixel kernel
    runs, the same strict bits, counted in MPI.shaded_lds_fallbacks, one RuntimeWarning."""
    from ml_gmpi_amd import MPI, hip_mpi, _lib as L
    vol, s, dhw, ray, eye, zd, orc = case("fwd", torch.float32, True, seed=1, B=2, D=8, S=96)
    dev = torch.device(DEV)
    t = lambda a: torch.as_tensor(a).to(dev)
    buf = torch.empty(vol.numel() + 1, device=dev)
    odd = buf[1:].view(vol.shape)
    odd.copy_(t(vol))
    assert odd.data_ptr() % 16 == 4
    hip_mpi._SHADED_LDS_WARNED = False
    mpi = MPI(variant="lds", strict_order=True, on_out_of_plane="raise")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.no_grad():
            for _ in range(2):
                out = mpi.render_views_shaded(odd, t(s), t(dhw), t(ray), t(eye), t(zd), want_transmittance=True)
    assert mpi.shaded_lds_fallbacks == 2
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning) and 'variant="lds"' in str(w.message)]) == 1
    for k in ("color", "depth", "T"):
        assert np.array_equal(out[k].cpu().numpy(), orc[k]), k
    auto = MPI(variant="auto", strict_order=True, on_out_of_plane="raise")
    with torch.no_grad():
        auto.render_views_shaded(odd, t(s), t(dhw), t(ray), t(eye), t(zd))
    assert auto.shaded_lds_fallbacks == 0   # (only a request by name is counted)


# ---- 6. memory ------------------------------------------------------------------------------------------------------------------------------------
def test_nothing_volume_sized_is_allocated_but_the_one_gradient():
    import ml_gmpi_amd
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    M, D, S = 2, 8, 128
    rgba, dhw, ray, eye, zd = _random_case(seed=13, B=M, D=D, S=S)
    t = lambda a: torch.as_tensor(a).to(dev)
    dhw, ray, eye, zd = t(dhw), t(ray), t(eye), t(zd)
    s0 = t(make_shading(13, rgba))
    V = rgba.numel() * 4
    assert V == 4 << 20
    mpi = MPI(on_out_of_plane="raise")

    def run(fused, backward, needs=(True, True)):
        vol = t(rgba).requires_grad_(backward and needs[0])
        s = s0.clone().requires_grad_(backward and needs[1])
        g = torch.ones((M, 3, S, S), device=dev)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        with torch.enable_grad() if backward else torch.no_grad():
            if fused:
                out = mpi.render_views_shaded(vol, s, dhw, ray, eye, zd, want_transmittance=True)
            else:
                out = mpi.render_views(ml_gmpi_amd.apply_shading(vol, s), dhw, ray, eye, zd, want_transmittance=True)
            if backward:
                torch.autograd.backward([out["color"]], [g])   # (no loss tensors of the test's own in the measure)
        torch.cuda.synchronize()
        outputs = sum(out[k].numel() * out[k].element_size() for k in ("color", "depth", "T", "status"))
        return torch.cuda.max_memory_allocated(dev) - base - outputs   # above the inputs and the outputs
    run(True, True)   # (warm-up: lazily created buffers -- status words, pinned rings -- are not this call's)
    fwd, both = run(True, False), run(True, True)
    two = run(False, True)
    only_s = run(True, True, needs=(False, True))   # only the shading requires grad: no volume buffer at all
    print(f"peak above the inputs and outputs, in volumes of {V >> 20} MiB: fused forward {fwd / V:.3f}, fused forward + backward {both / V:.3f}, "
          f"render_views(apply_shading) forward + backward {two / V:.3f}")
    assert fwd < 0.25 * V, fwd / V
    assert both <= 1.25 * V, both / V
    print(f"only the shading requires grad: fused forward + backward {only_s / V:.3f}")
    assert only_s < 0.25 * V, only_s / V   # (the forward's margin: images and the allocator's rounding)


# ---- 7. the backward="gather" module -----------------------------------------------------------------------------------------------------------------
def test_backward_gather_module_takes_the_default_backward_and_says_so():
    from ml_gmpi_amd import hip_mpi
    vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT = _bwd_case("d8", 8, 64, torch.float32)
    ref64 = _reference_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, False, torch.float64)
    ref32 = _reference_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, False, torch.float32)
    hip_mpi._SHADED_BACKWARD_WARNED = False
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        ins, mpi = _hip_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, False, "auto", torch.float32, backward="gather")
        assert mpi.shaded_backward_fallbacks == 1
        ins2, mpi2 = _hip_grads(vol, s, dhw, ray, eye, zd, v2m, gc, gd, gT, False, "auto", torch.float32, backward="gather")
        assert mpi2.shaded_backward_fallbacks == 1
    mine = [w for w in caught if issubclass(w.category, RuntimeWarning) and "shaded render" in str(w.message)]
    assert len(mine) == 1, [str(w.message) for w in caught]
    _compare([i.grad.double().cpu().numpy() for i in ins], ref64, ref32, (torch.float32, torch.float32), "backward=gather module")
