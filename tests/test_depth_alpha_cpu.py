"""Depth-alpha layout without a GPU: the executable definition (`expand_depth_alpha`) against the generator's expression bit for bit, the
autograd mask of the clamp, what `hip_mpi` hands the two C entries (through test_marshal_cpu's recorder), the entries' argument errors on the
host, and the register budget of the new kernels."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_marshal_cpu import (BACKWARD_ENTRIES, FORWARD_ENTRIES, Recorder, check_backward_struct, check_shared_color, check_struct, loss_of,
                              make_inputs, M, D, Ht, Wt)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PAIRS = [(zr, n) for zr in (1, 2) for n in (3, 7, 10, 100, 256)]
DEPTH_ENTRIES = ("gmpi_mpi_render_depth_launch", "gmpi_mpi_render_depth_backward_launch")


def _images(M_=2, Ht_=9, Wt_=11, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((M_, 3, Ht_, Wt_), generator=g).to(dtype), torch.rand((M_, 1, Ht_, Wt_), generator=g).to(dtype),
            torch.rand((M_, 3, Ht_, Wt_), generator=g).to(dtype))


def _generator_alpha(depth, tex_z, z_range, n_z_bins):
    """networks_vanilla_depth2alpha.py:650-663 with Python-float scalars; tex_z [D,1,1,1] is constant per plane."""
    z_lo, z_hi = -1.0 * z_range / n_z_bins, 1.0 * z_range / n_z_bins
    z_diff = torch.clamp(tex_z.unsqueeze(0) - depth.unsqueeze(1), z_lo, z_hi)
    return (z_diff - z_lo) / (z_hi - z_lo + 1e-8)


# ---- the definition ----------------------------------------------------------------------------------------------------------------------------
def test_bounds_are_python_floats():
    from ml_gmpi_amd import depth_alpha_bounds
    for zr, n in PAIRS:
        lo, hi = depth_alpha_bounds(zr, n)
        assert type(lo) is float and type(hi) is float and lo == -zr / n and hi == zr / n


@pytest.mark.parametrize("z_range,n_z_bins", PAIRS)
def test_expand_is_bit_identical_to_the_generators_expression(z_range, n_z_bins):
    from ml_gmpi_amd import depth_alpha_bounds, expand_depth_alpha
    rgb, depth, bg = _images(seed=n_z_bins)
    Dn = 13
    plane_z = torch.linspace(0, 1, Dn)
    # depths on, next to and far from the planes: both clamps, the ramp, and its two ends
    depth.view(-1)[:Dn] = plane_z
    depth.view(-1)[Dn:2 * Dn] = plane_z + z_range / n_z_bins
    depth.view(-1)[2 * Dn:3 * Dn] = plane_z - z_range / n_z_bins
    lo, hi = depth_alpha_bounds(z_range, n_z_bins)
    vol = expand_depth_alpha(rgb, depth, plane_z, lo, hi, bg)
    assert vol.shape == (2, Dn, 4, 9, 11) and vol.dtype == torch.float32
    want = _generator_alpha(depth, plane_z.reshape(Dn, 1, 1, 1), z_range, n_z_bins)
    assert torch.equal(vol[:, :, 3:].view(torch.int32), want.view(torch.int32))
    alpha = vol[:, :, 3]
    assert float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0
    assert float(alpha.min()) == 0.0 and float(alpha.max()) > 1.0 - 2e-6     # both clamps occur
    assert bool(((alpha > 0) & (alpha < 1 - 2e-6)).any())                    # and the ramp between them
    for k in range(Dn):
        assert torch.equal(vol[:, k, :3], bg if k == Dn - 1 else rgb), k
    assert torch.equal(expand_depth_alpha(rgb, depth, plane_z, lo, hi)[:, -1, :3], rgb)


def test_expand_follows_the_stated_fp32_chain_step_by_step():
    """numpy, one fp32 rounding per step, the constants rounded first (den from the double sum)."""
    from ml_gmpi_amd import expand_depth_alpha
    from ml_gmpi_amd.depth_alpha import ramp_constants
    rgb, depth, _ = _images(seed=5)
    plane_z = torch.linspace(0, 1, 6)
    for z_lo, z_hi in ((-1 / 3, 1 / 3), (-2 / 256, 2 / 256), (-0.1, 0.3)):
        lo, hi, den = ramp_constants(z_lo, z_hi)
        assert (np.float32(lo), np.float32(hi)) == (np.float32(z_lo), np.float32(z_hi)) and np.float32(den) == np.float32(z_hi - z_lo + 1e-8)
        assert lo == float(np.float32(lo)) and den == float(np.float32(den))
        t = plane_z.numpy().reshape(1, 6, 1, 1, 1) - depth.numpy()[:, None]
        t = np.minimum(np.maximum(t, np.float32(lo)), np.float32(hi))
        want = (t - np.float32(lo)) / np.float32(den)
        assert want.dtype == np.float32
        got = expand_depth_alpha(rgb, depth, plane_z, z_lo, z_hi)[:, :, 3:].numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_plane_tables_per_mpi_and_shared():
    from ml_gmpi_amd import expand_depth_alpha
    rgb, depth, bg = _images(seed=2)
    pz = torch.stack([torch.linspace(0, 1, 5), torch.linspace(0.1, 0.8, 5)])
    both = expand_depth_alpha(rgb, depth, pz, -0.2, 0.2, bg)
    for m in range(2):
        one = expand_depth_alpha(rgb[m:m + 1], depth[m:m + 1], pz[m], -0.2, 0.2, bg[m:m + 1])
        assert torch.equal(both[m:m + 1], one)
    assert torch.equal(expand_depth_alpha(rgb, depth, pz[0], -0.2, 0.2), expand_depth_alpha(rgb, depth, pz[:1].expand(2, -1), -0.2, 0.2))
    assert not torch.equal(both[1], expand_depth_alpha(rgb, depth, pz[0], -0.2, 0.2, bg)[1])


def test_computes_in_at_least_fp32_and_in_float64_when_given():
    from ml_gmpi_amd import expand_depth_alpha
    rgb, depth, bg = _images(seed=3, dtype=torch.bfloat16)
    pz = torch.linspace(0, 1, 4)
    vol = expand_depth_alpha(rgb, depth, pz, -0.25, 0.25, bg)
    assert vol.dtype == torch.float32 and torch.equal(vol, expand_depth_alpha(rgb.float(), depth.float(), pz, -0.25, 0.25, bg.float()))
    assert expand_depth_alpha(rgb.double(), depth.double(), pz, -0.25, 0.25).dtype == torch.float64


def test_autograd_mask_is_inclusive_at_both_bounds():
    from ml_gmpi_amd import expand_depth_alpha
    from ml_gmpi_amd.depth_alpha import ramp_constants
    lo, hi, den = ramp_constants(-0.25, 0.25)   # exact in fp32
    pz = torch.tensor([0.0])
    # plane_z - depth = lo, hi (on the bounds), just outside either, the middle (a plane at 0: the negation is exact)
    diffs = torch.tensor([lo, hi, float(np.nextafter(np.float32(lo), np.float32(-1))), float(np.nextafter(np.float32(hi), np.float32(1))), 0.0])
    depth = (-diffs).reshape(1, 1, 1, 5).requires_grad_(True)
    assert torch.equal(pz - depth.detach().reshape(-1), diffs) and diffs[2] < lo and diffs[3] > hi
    rgb = torch.zeros((1, 3, 1, 5), requires_grad=True)
    vol = expand_depth_alpha(rgb, depth, pz, -0.25, 0.25)
    vol[:, :, 3].sum().backward()
    g = depth.grad.reshape(-1)
    inside = torch.tensor(-1.0 / den)
    assert torch.equal(g, torch.stack([inside, inside, torch.tensor(0.0), torch.tensor(0.0), inside]))
    assert torch.equal(vol[0, 0, 3, 0].detach(), torch.tensor([0.0, 1.0, 0.0, 1.0, 0.5]))


def test_gradients_through_expand_sum_the_alpha_planes():
    """float64: d depth = -1/den times the sum over the planes whose difference lies on the ramp of d rgba[:, k, 3]; the colours as in the
    shared-colour layout."""
    from ml_gmpi_amd import expand_depth_alpha
    from ml_gmpi_amd.depth_alpha import ramp_constants
    rgb, depth, bg = (t.double() for t in _images(seed=4))
    pz = torch.linspace(0, 1, 6)
    ins = [t.clone().requires_grad_(True) for t in (rgb, depth, bg)]
    vol = expand_depth_alpha(ins[0], ins[1], pz, -0.15, 0.15, ins[2])
    g = torch.randn(vol.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    (vol * g).sum().backward()
    lo, hi, den = ramp_constants(-0.15, 0.15)
    t = pz.double().reshape(1, 6, 1, 1, 1) - depth.unsqueeze(1)
    on = ((t >= lo) & (t <= hi)).double()
    assert 0 < float(on.mean()) < 1
    assert torch.allclose(ins[1].grad, -(g[:, :, 3:] * on).sum(1) / den, rtol=1e-13, atol=0)
    assert torch.allclose(ins[0].grad, g[:, :5, :3].sum(1), rtol=1e-13, atol=0) and torch.equal(ins[2].grad, g[:, 5, :3])


# ---- marshalling -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    from ml_gmpi_amd import _lib
    r = Recorder(FORWARD_ENTRIES + BACKWARD_ENTRIES + DEPTH_ENTRIES)
    monkeypatch.setattr(_lib, "load_library", lambda: r)
    return r


def depth_inputs(dtype=torch.float32, background=True, per_mpi_table=False):
    _, dhw, ray, eye, zd = make_inputs(2, dtype)
    g = torch.Generator().manual_seed(1)
    depth = torch.rand((M, 1, Ht, Wt), generator=g).to(dtype)
    rgb = torch.rand((M, 3, Ht, Wt), generator=g).to(dtype)
    bg = torch.rand((M, 3, Ht, Wt), generator=g).to(dtype) if background else None
    pz = torch.rand((M, D), generator=g) if per_mpi_table else torch.linspace(0, 1, D)
    return rgb, depth, pz, bg, (dhw, ray, eye, zd)


def check_depth_alpha(da, pz, z_lo, z_hi):
    from ml_gmpi_amd import _lib
    assert ctypes.sizeof(_lib.GmpiDepthAlpha) == 40 and da.struct_size == 40
    assert da.plane_z == pz.data_ptr() and da.plane_z_stride == (pz.stride(0) if pz.ndim == 2 else 0)
    want = (np.float32(z_lo), np.float32(z_hi), np.float32(z_hi - z_lo + 1e-8))   # (the sum in double, then one rounding)
    assert (np.float32(da.z_lo), np.float32(da.z_hi), np.float32(da.z_den)) == want
    assert (da.z_lo, da.z_hi, da.z_den) == tuple(float(v) for v in want)


@pytest.mark.parametrize("per_mpi_table", [False, True])
@pytest.mark.parametrize("dtype,code", [(torch.float32, 0), (torch.bfloat16, 1), (torch.float16, 2)])
def test_forward_structs(rec, dtype, code, per_mpi_table):
    from ml_gmpi_amd.hip_mpi import MPI
    rgb, depth, pz, bg, geo = depth_inputs(dtype, per_mpi_table=per_mpi_table)
    with torch.no_grad():
        res = MPI().render_views_depth(rgb, depth, pz, (-1 / 7, 1 / 7), *geo, background=bg)
    (c,) = rec.calls
    assert c.name == "gmpi_mpi_render_depth_launch" and c.args[3] == 0
    # the depth image seen as [M,1,1,Ht,Wt]; D is the number of planes of dhw
    check_struct(c.args[0], res, (depth,) + geo, variant=0, rgba_dtype=code, D=D, rgba_stride=[48, 48, 48, 8, 1])
    check_shared_color(c.args[1], rgb, bg)
    check_depth_alpha(c.args[2], pz, -1 / 7, 1 / 7)


def test_forward_without_background_gather_variant_and_a_strided_depth_view(rec):
    from ml_gmpi_amd.hip_mpi import MPI
    rgb, depth, pz, _, geo = depth_inputs(background=False)
    rgbd = torch.cat((rgb, depth), 1)
    view = rgbd[:, 3:]
    assert not view.is_contiguous()
    with torch.no_grad():
        res = MPI(variant="gather", range_check="full").render_views_depth(rgb, view, pz, (-0.5, 0.5), *geo)
    # range_check="full" passes over the colour image only
    assert [c.name for c in rec.calls] == ["gmpi_rgba_range_check_launch", "gmpi_mpi_render_depth_launch"]
    assert rec.calls[0].args == (rgb.data_ptr(), 0, rgb.numel(), res["status"].data_ptr(), 0)
    c = rec.calls[1]
    check_struct(c.args[0], res, (view,) + geo, variant=1, rgba_stride=[192, 48, 48, 8, 1])
    assert c.args[0].rgba == view.data_ptr() != depth.data_ptr()
    check_shared_color(c.args[1], rgb, None)


@pytest.mark.parametrize("uses_T", [False, True])
@pytest.mark.parametrize("background", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_backward_rebuilds_the_forward_structs(rec, dtype, background, uses_T):
    from ml_gmpi_amd.hip_mpi import MPI
    rgb, depth, pz, bg, geo = depth_inputs(dtype, background, per_mpi_table=True)
    for t in (rgb, depth, bg):
        if t is not None:
            t.requires_grad_(True)
    res = MPI().render_views_depth(rgb, depth, pz, (-2 / 10, 2 / 10), *geo, background=bg, want_transmittance=True)
    loss_of(res, uses_T).backward()
    fwd, bwd = rec.calls
    assert (fwd.name, bwd.name) == DEPTH_ENTRIES
    b, f = bwd.args[0], fwd.args[0]
    assert bwd.name.endswith("depth_backward_launch")
    check_backward_struct(bwd._replace(name="gmpi_mpi_render_shared_backward_launch"), fwd, uses_T)   # (same rules as the shared entry: one launch name for both T cases)
    assert bytes(bwd.args[1]) == bytes(fwd.args[1]) and bytes(bwd.args[2]) == bytes(fwd.args[2])
    check_shared_color(bwd.args[1], rgb, bg)
    check_depth_alpha(bwd.args[2], pz, -2 / 10, 2 / 10)
    assert bwd.args[3] is not None and bwd.args[4] is not None and (bwd.args[5] is not None) == uses_T and bwd.args[-1] == 0
    # gradient tensors: rgb, depth image, background -- pointer and (MPI, channel, row) strides; NULL without a background
    assert bwd.args[6] is not None and bwd.args[7] == [144, 48, 8]
    assert bwd.args[8] is not None and bwd.args[9] == [48, 48, 8]
    assert (bwd.args[10] is not None) == background and (bwd.args[11] == [144, 48, 8] if background else bwd.args[11] is None)
    for t in (rgb, depth, bg):
        assert t is None or (t.grad.shape == t.shape and t.grad.dtype == dtype)


def test_partial_requires_grad_passes_null_for_the_others(rec):
    from ml_gmpi_amd.hip_mpi import MPI
    rgb, depth, pz, bg, geo = depth_inputs()
    depth.requires_grad_(True)
    res = MPI().render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg)
    res["color"].sum().backward()
    bwd = rec.calls[1]
    assert bwd.args[6] is None and bwd.args[8] is not None and bwd.args[10] is None and bwd.args[4] is None and bwd.args[5] is None
    assert depth.grad is not None and rgb.grad is None and bg.grad is None


def test_refusals_on_the_host(rec):
    from ml_gmpi_amd.hip_mpi import MPI
    rgb, depth, pz, bg, geo = depth_inputs()
    call = lambda mpi=None, **kw: (mpi or MPI()).render_views_depth(kw.get("rgb", rgb), kw.get("depth", depth), pz, (-0.2, 0.2), *kw.get("geo", geo),
                                                                    background=kw.get("bg", bg))
    with pytest.raises(TypeError, match="one storage dtype"):
        call(rgb=rgb.bfloat16())
    with pytest.raises(TypeError, match="one storage dtype"):
        call(bg=bg.half())
    with pytest.raises(TypeError, match="uint8"):
        call(rgb=(rgb * 255).to(torch.uint8), depth=(depth * 255).to(torch.uint8), bg=None)
    dhw, ray, eye, zd = geo
    with pytest.raises(NotImplementedError, match="depth-alpha"):
        call(MPI(geometry_grad=True), geo=(dhw, ray.clone().requires_grad_(True), eye, zd))
    with pytest.raises(NotImplementedError):
        call(MPI(geometry_grad=True), geo=(dhw.clone().requires_grad_(True), ray, eye, zd))
    with pytest.raises(AssertionError):
        MPI().render_views_depth(rgb, depth, torch.linspace(0, 1, D + 1), (-0.2, 0.2), *geo)
    for name in ("lds", "wave", "band", "dma"):   # a kernel the layout does not have is refused by name
        with pytest.raises(ValueError, match="not built"):
            MPI().render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, variant=name)
    assert rec.calls == []
    # geometry_grad=True with camera tensors that do not require grad renders
    with torch.no_grad():
        call(MPI(geometry_grad=True))
    assert [c.name for c in rec.calls] == ["gmpi_mpi_render_depth_launch"]


def test_renderer_render_depth_takes_the_normalised_plane_depths(rec):
    from ml_gmpi_amd import depth_alpha_bounds, make_renderer
    r = make_renderer("FFHQ", n_planes=4, device=torch.device("cpu"), ray_backend="torch")
    S = 8
    g = torch.Generator().manual_seed(0)
    rgb, depth = torch.rand((1, 3, S, S), generator=g), torch.rand((1, 1, S, S), generator=g)
    seen, render_views = {}, r.mpi.render_views
    r.mpi.render_views = lambda *a, **kw: seen.update(kw) or render_views(*a, **kw)   # (the table is a temporary: looked at while it lives)
    torch.manual_seed(0)
    with torch.no_grad():
        out = r.render_depth(rgb, depth, S, S, z_range=1, n_z_bins=4, want_transmittance=True)
    assert len(out) == 5 and out[0].shape == (1, 3, S, S) and out[4].shape == (1, 1, S, S)
    c = rec.named("gmpi_mpi_render_depth_launch")[0]
    da = c.args[2]
    want = r.get_xyz_single_res(S, S, only_z=True)[1].reshape(-1)
    assert want.shape == (4,) and torch.equal(seen["_layout"].plane_z, want.float())
    assert da.plane_z == seen["_layout"].plane_z.data_ptr() and da.plane_z_stride == 0
    lo, hi = depth_alpha_bounds(1, 4)
    assert (da.z_lo, da.z_hi) == (lo, hi) and c.args[0].D == 4 and c.args[0].flags & 2   # (OUT_PM1: render()'s colour range)


# ---- the C entries on the host -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_depth_entries_as_plain_c(tmp_path):
    src = tmp_path / "d.c"
    src.write_text(
        '#include "gmpi_render.h"\n'
        "int main(void) {\n"
        "    GmpiDepthAlpha da;\n"
        "    int (*fwd)(const GmpiRenderParams *, const GmpiSharedColor *, const GmpiDepthAlpha *, void *) = gmpi_mpi_render_depth_launch;\n"
        "    int (*bwd)(const GmpiRenderParams *, const GmpiSharedColor *, const GmpiDepthAlpha *, const float *, const float *, const float *, float *,\n"
        "               const int64_t *, float *, const int64_t *, float *, const int64_t *, void *) = gmpi_mpi_render_depth_backward_launch;\n"
        "    da.struct_size = (uint32_t)sizeof(GmpiDepthAlpha); da.plane_z = 0; da.plane_z_stride = 0; da.z_lo = -1.0f; da.z_hi = 1.0f; da.z_den = 2.0f;\n"
        "    return (fwd == 0) + (bwd == 0) + (da.struct_size != 40) + (GMPI_ABI_VERSION != 2) + (sizeof(GmpiRenderParams) != 184) + (sizeof(GmpiSharedColor) != 72);\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "d.o")], check=True)


def test_argument_error_codes_and_the_query_on_the_host():
    """Every call below is refused (or has no views) before anything is launched: no device is needed, the pointers are never followed."""
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    assert lib.gmpi_query(22) == 1 and lib.gmpi_query(21) == -1 and lib.gmpi_query(0) == 2
    host = np.zeros(64, dtype=np.float32)
    fake = host.ctypes.data   # (a non-NULL address)

    def params(N=1):
        p = L.GmpiRenderParams()
        p.struct_size = ctypes.sizeof(L.GmpiRenderParams)
        p.flags, p.variant, p.rgba_dtype = L.FLAG_ALIGN_CORNERS, L.VARIANT_AUTO, L.DTYPE_F32
        p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = N, 1, 3, 4, 4, 4, 4, 1
        p.rgba = fake
        p.rgba_stride[:] = [16, 0, 0, 4, 1]   # [1], [2]: ignored
        p.dhw = p.ray_dir = p.eye_pos = p.z_dir = p.rgb_out = p.depth_out = fake
        return p

    def shared(with_bg=True):
        s = L.GmpiSharedColor()
        s.struct_size = ctypes.sizeof(L.GmpiSharedColor)
        s.rgb, s.background = fake, (fake if with_bg else None)
        s.rgb_stride[:] = [48, 16, 4]
        s.background_stride[:] = [48, 16, 4]
        return s

    def ramp(lo=-0.25, hi=0.25, den=0.5):
        d = L.GmpiDepthAlpha()
        d.struct_size = ctypes.sizeof(L.GmpiDepthAlpha)
        d.plane_z, d.plane_z_stride, d.z_lo, d.z_hi, d.z_den = fake, 0, lo, hi, den
        return d

    ref = lambda x: None if x is None else ctypes.byref(x)
    fwd = lambda p, s, d: lib.gmpi_mpi_render_depth_launch(ref(p), ref(s), ref(d), None)
    s3 = (ctypes.c_int64 * 3)(48, 16, 4)

    def bwd(p, s, d, go=fake, gr=fake, gd=fake, gb=fake, gds=s3):
        return lib.gmpi_mpi_render_depth_backward_launch(ref(p), ref(s), ref(d), go, None, None, gr, s3, gd, gds, gb, s3, None)

    for call in (fwd, bwd):
        assert call(params(N=0), shared(), ramp()) == 0                                              # no views: nothing to launch
        assert call(None, shared(), ramp()) == -1 and call(params(), None, ramp()) == -1 and call(params(), shared(), None) == -1   # GMPI_E_NULL
        d = ramp(); d.plane_z = None
        assert call(params(), shared(), d) == -1
        s = shared(); s.rgb = None
        assert call(params(), s, ramp()) == -1
        p = params(); p.rgba = None
        assert call(p, shared(), ramp()) == -1
        p = params(); p.rgba_dtype = L.DTYPE_U8
        assert call(p, shared(), ramp()) == -3                                                       # GMPI_E_DTYPE
        for lo, hi, den in ((0.25, 0.25, 0.5), (0.3, 0.25, 0.5), (-0.25, 0.25, 0.0), (-0.25, 0.25, -0.5), (float("nan"), 0.25, 0.5)):
            assert call(params(), shared(), ramp(lo, hi, den)) == -2, (lo, hi, den)                  # bad bounds: GMPI_E_SHAPE
        d = ramp(); d.plane_z_stride = -3
        assert call(params(), shared(), d) == -4                                                     # GMPI_E_STRIDE
        p = params(); p.rgba_stride[4] = 2
        assert call(p, shared(), ramp()) == -4
        d = ramp(); d.struct_size += 8
        assert call(params(), shared(), d) == -5                                                     # GMPI_E_ABI
        p = params(); p.struct_size -= 8
        assert call(p, shared(), ramp()) == -5
        for v in (L.VARIANT_LDS, L.VARIANT_WAVE, L.VARIANT_DMA, L.VARIANT_BAND, 9):
            p = params(); p.variant = v
            assert call(p, shared(), ramp()) == -6, v                                                # GMPI_E_VARIANT
        p = params(); p.flags |= 1 << 30
        assert call(p, shared(), ramp()) == -7                                                       # GMPI_E_FLAGS
        p = params(N=0); p.variant = L.VARIANT_GATHER
        assert call(p, shared(), ramp()) == 0
    p = params(); p.rgb_out = None
    assert fwd(p, shared(), ramp()) == -1                                                            # the forward needs its outputs
    p.depth_out = None
    assert bwd(p, shared(), ramp(), go=None) == -1                                                   # the backward does not, but the upstream gradient
    assert bwd(p, shared(), ramp(), gr=None, gd=None, gb=None) == -1                                 # all three NULL
    assert bwd(p, shared(with_bg=False), ramp()) == -1                                               # a background gradient without a background
    assert bwd(p, shared(), ramp(), gds=None) == -1                                                  # a gradient without its strides
    assert bwd(p, shared(), ramp(), gds=(ctypes.c_int64 * 3)(16, 0, 3)) == -4                        # rows overlap
    p0 = params(N=0); p0.rgb_out = p0.depth_out = None
    assert bwd(p0, shared(), ramp(), gr=None, gb=None) == 0 and bwd(p0, shared(with_bg=False), ramp(), gb=None) == 0


def test_library_exports_the_depth_entries_and_keeps_the_abi():
    from ml_gmpi_amd import _lib
    for name in DEPTH_ENTRIES + ("gmpi_mpi_render_shared_launch", "gmpi_mpi_render_shared_backward_launch", "gmpi_mpi_render_launch"):
        assert name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 2 and ctypes.sizeof(_lib.GmpiRenderParams) == 184 and ctypes.sizeof(_lib.GmpiSharedColor) == 72


@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_depth_kernels_have_no_scratch(tmp_path):
    csrc = os.path.join(ROOT, "ml-gmpi_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
             "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]   # = ml-gmpi_amd/csrc/Makefile
    mk = open(os.path.join(csrc, "Makefile")).read()
    for f in ("-ffp-contract=off", "-fno-slp-vectorize", "-O3", "render_depth.hip"):
        assert f in mk, f"the Makefile no longer has {f}: keep this test in step with it"
    res = subprocess.run([HIPCC, *flags, "-save-temps", "-c", os.path.join(csrc, "render_depth.hip"), "-o", "render_depth.o"], cwd=tmp_path,
                         capture_output=True, timeout=900)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    asm = open(os.path.join(tmp_path, "render_depth-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    seen = set()
    for name in sorted(set(re.findall(r"^(_Z\w*render_depth\w*):", asm, flags=re.M))):
        a = asm.index(name + ":")
        body = asm[a:asm.index(".Lfunc_end", a)]
        assert "scratch_" not in body, f"{name}: scratch (spill) operations in the kernel"
        meta = asm[asm.index(".amdhsa_kernel " + name):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1)) == 0, name
        seen.add(name)
    assert sum("render_depth_kernel" in n for n in seen) == 12, sorted(seen)            # 3 storage types x align_corners x strict order
    assert sum("render_depth_backward_kernel" in n for n in seen) == 6, sorted(seen)    # 3 storage types x align_corners
    shutil.rmtree(tmp_path, ignore_errors=True)
