"""CPU-side checks of LightRenderer(middle=...) and of the index math of the middle's adjoint kernels (csrc/light_kernels.hip): the gather forms the
kernels implement -- replica sums over the replicate-padded border, the gather over the cells that use a point, the three preimages of a texel under
reflect padding -- are restated in numpy float64 (tests/_light_middle_ref.py) and held against torch autograd of `torch_light_render`'s own middle.
No GPU: tests/test_hip_light_middle.py runs the kernels."""
import os
import subprocess

import numpy as np
import pytest
import torch

import _light_cases as lc
import _light_middle_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL64 = 1e-11   # float64 against float64, another order of the same few hundred operations: relative to max|g_ref|


def test_middle_keyword_is_checked():
    import ml_gmpi_amd
    kw = dict(sphere_center_z=1.0, sphere_r=1.0)
    assert ml_gmpi_amd.LightRenderer(**kw).middle == "torch"
    assert ml_gmpi_amd.LightRenderer(middle="torch", **kw).middle == "torch"
    assert ml_gmpi_amd.LightRenderer(middle="hip", **kw).middle == "hip"
    for bad in ("bogus", "HIP", None, ""):
        with pytest.raises(ValueError, match="middle"):
            ml_gmpi_amd.LightRenderer(middle=bad, **kw)


def test_library_declares_exports_and_reports_the_new_entries():
    from ml_gmpi_amd import _lib
    lib = _lib.load_library()
    for name in ("gmpi_light_shading_backward_launch", "gmpi_light_blur_backward_launch", "gmpi_light_shade_images_launch",
                 "gmpi_light_shade_images_backward_launch"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.gmpi_query(46) == 1 and lib.gmpi_query(45) == -1 and lib.gmpi_query(47) == -1
    assert lib.gmpi_query(0) == _lib.ABI_VERSION == 2


def test_header_with_the_new_prototypes_compiles_as_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gmpi_render.h"\n'
                   "int main(void){int (*f)(const float *, float *, int32_t, int32_t, int32_t, const float *, int32_t, void *) = gmpi_light_blur_backward_launch;\n"
                   "GmpiRenderParams p; p.struct_size=sizeof p; return f == 0 || (int)p.struct_size==0;}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


def _case(H, W, seed):
    rng = np.random.default_rng(seed)
    return mr.surface(seed, H, W), lc.texel_grid(H, W), lc.LIGHT_DIRS, rng.standard_normal((mr.B, H, W))


@pytest.mark.parametrize("shape", [(3, 3), (3, 8), (8, 3), (5, 7)])
def test_shading_adjoint_in_gather_form_equals_autograd(shape):
    """(3, 3): one interior cell takes the whole image; (3, 8) / (8, 3): every cell takes a whole column / row, the end cells two."""
    H, W = shape
    blurred, xyz, light, g_s = _case(H, W, 40 + H * W)
    s, want = mr.middle_autograd(blurred, xyz, light, lc.KA, lc.KD, [1.0], g_s)
    got, roles = mr.shading_backward_gather(blurred[:, 0], xyz, light, lc.KD, g_s, parts=True)
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want[:, 0]).max())
    print(f"shading adjoint {H}x{W}: max|g_ref| {scale:.3e} err {err:.3e} lit {float((s > lc.KA).mean()):.2f}")
    assert scale > 0 and (s > lc.KA).any()
    assert err <= TOL64 * scale
    # the four cross products add up to (up - down) x (left - right): the centre's own gradient is rounding residue, which is why the kernel
    # gathers from four cells, not five
    assert float(np.abs(roles["c"]).max()) <= 1e-12 * float(np.abs(roles["u"]).max())
    # the replica sums matter: a gradient on the border ring alone reaches the depth
    ring = np.zeros_like(g_s)
    ring[:, 0], ring[:, -1], ring[:, :, 0], ring[:, :, -1] = g_s[:, 0], g_s[:, -1], g_s[:, :, 0], g_s[:, :, -1]
    _, want_ring = mr.middle_autograd(blurred, xyz, light, lc.KA, lc.KD, [1.0], ring)
    got_ring = mr.shading_backward_gather(blurred[:, 0], xyz, light, lc.KD, ring)
    assert float(np.abs(want_ring).max()) > 0 and float(np.abs(got_ring - want_ring[:, 0]).max()) <= TOL64 * float(np.abs(want_ring).max())


@pytest.mark.parametrize("shape", [(5, 7), (9, 6), (21, 37)])
def test_blur_adjoint_and_whole_middle_in_gather_form_equal_autograd(shape):
    """(5, 7): n = r + 1 along H, both reflected preimages of a row are live at once."""
    H, W = shape
    depth, xyz, light, g_s = _case(H, W, 70 + H * W)
    k1d = lc.k1d()
    k = k1d.double().numpy()
    # the blur alone: autograd of the padded convolution, the transposed dense operator, and the three-preimage gather
    leaf = torch.from_numpy(depth).double().requires_grad_(True)
    (want_blur,) = torch.autograd.grad(mr.blur64(leaf, k1d.double()), leaf, torch.from_numpy(g_s)[:, None])
    got_blur = mr.blur_backward_gather(g_s, k)
    dense = np.einsum("jy,bjx->byx", mr.blur_matrix(H, k), np.einsum("bjk,kx->bjx", g_s, mr.blur_matrix(W, k)))   # My^T g Mx
    scale = float(want_blur.abs().max())
    assert float(np.abs(got_blur - want_blur[:, 0].numpy()).max()) <= TOL64 * scale
    assert float(np.abs(dense - want_blur[:, 0].numpy()).max()) <= TOL64 * scale
    # the whole middle
    with torch.no_grad():
        blurred = mr.blur64(torch.from_numpy(depth).double(), k1d.double())[:, 0].numpy()
    s, want = mr.middle_autograd(depth, xyz, light, lc.KA, lc.KD, k, g_s)
    got = mr.blur_backward_gather(mr.shading_backward_gather(blurred, xyz, light, lc.KD, g_s), k)
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want[:, 0]).max())
    print(f"whole middle {H}x{W}: max|g_ref| {scale:.3e} err {err:.3e} lit {float((s > lc.KA).mean()):.2f}")
    assert scale > 0 and (s > lc.KA).any()
    assert err <= TOL64 * scale
