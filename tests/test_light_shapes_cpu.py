"""The CPU side of the shading-augmentation shape tests (no GPU):

* `oracle.light_shade`, `tests/_torch_ref.torch_light_render` and the host halves of the product's backward (`light._blur_torch` with the two
  `_blur_matrix` operators, `light._shading_torch`) are pinned to the reference's own `LightRenderer` at two shapes with H != W
  (tests/golden/light_render_nonsquare.npz): an H / W transposition in any of them is invisible on the square fixture.
* Every case of tests/_light_cases.py is shown to have a bar that means something before a GPU is involved: the fp32 noise floor n0 recorded in
  the table is the one measured here (and at most 1e-5 for shapes up to 64 texels), a transposed texel grid and a depth shifted by one texel each
  move the float64 reference by at least 50 bars, the gradient reaches colours and alphas, and a real share of the alpha gradient comes through
  the shading."""
import numpy as np
import pytest
import torch

import oracle
import _light_cases as lc
from _torch_ref import torch_light_render
from _util import load_npz
from test_light_render import _scipy_blur

NONSQUARE = ("21x37", "50x18")


@pytest.fixture(scope="module")
def fx():
    return load_npz("light_render_nonsquare.npz")


@pytest.mark.parametrize("name", NONSQUARE)
def test_cpu_references_match_the_reference_at_nonsquare_shapes(fx, name):
    """Bars: the fixture is the reference's own fp32 chain.  float64 against it: 1e-5, the project's bar for this path (test_light_render.py).
    An fp32 restatement against it: two fp32 chains, each within that bar of float64 -> 2e-5."""
    rgba, xyz, ld = fx[f"rgba_{name}"], fx[f"xyz_last_{name}"], fx[f"light_dir_{name}"]
    ka, kd = fx[f"ka_kd_{name}"]
    ref = fx[f"ref_{name}"]
    assert (ref[:, :, :3] == 1).mean() > 0.05 and ka + kd > 1          # the clip at 1 is in play
    out, _ = oracle.light_shade(rgba, fx["dhw"][:, 0], xyz, ld, ka, kd)
    errs = {"oracle": float(np.abs(out - ref).max())}
    assert np.array_equal(out[:, :, 3], rgba[:, :, 3])
    for dt in (torch.float32, torch.float64):
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
        got = torch_light_render(t(rgba), t(fx["dhw"][:, 0]), t(xyz), t(ld), float(ka), float(kd), lc.k1d().to(dt)).double().numpy()
        errs[str(dt)] = float(np.abs(got - ref).max())
    print(name, errs)
    assert errs["oracle"] <= 2e-5 and errs["torch.float32"] <= 2e-5 and errs["torch.float64"] <= 1e-5, errs


@pytest.mark.parametrize("name", NONSQUARE)
def test_host_halves_of_the_backward_match_the_reference_intermediates(fx, name):
    """`_blur_torch(_blur_matrix(H), _blur_matrix(W))` against the reference's blurred depth (its stand-in blur, fp32: today's blur bar 1.5e-6) and
    scipy's float64 blur; `_shading_torch` in float64 against ka + kd * max(-n.l, 0) from the reference's normals (fp32 normals: 1e-5) and against
    the numpy restatement of the kernel that the GPU test compares with (same formula in float64: 1e-12)."""
    from ml_gmpi_amd.light import _blur_matrix, _blur_torch, _shading_torch
    depth, blurred, normal = fx[f"ref_depth_{name}"], fx[f"ref_blurred_{name}"], fx[f"ref_normal_{name}"]
    xyz, ld = fx[f"xyz_last_{name}"], fx[f"light_dir_{name}"]
    ka, kd = (float(v) for v in fx[f"ka_kd_{name}"])
    H, W = depth.shape[-2:]
    assert H != W
    k1, cpu = lc.k1d(), torch.device("cpu")
    my, mx = _blur_matrix(H, k1, cpu), _blur_matrix(W, k1, cpu)
    assert tuple(my.shape) == (H, H) and tuple(mx.shape) == (W, W)
    got = _blur_torch(torch.from_numpy(depth), my, mx).numpy()
    e_ref, e_scipy = float(np.abs(got - blurred).max()), float(np.abs(got - _scipy_blur(depth)).max())
    print(name, "blur vs reference", e_ref, "vs scipy", e_scipy)
    assert e_ref <= 1.5e-6 and e_scipy <= 1.5e-6
    want = ka + kd * np.maximum(-(normal.astype(np.float64) * ld.astype(np.float64).reshape(-1, 1, 1, 3)).sum(3), 0.0)
    s = _shading_torch(torch.from_numpy(blurred).double(), torch.from_numpy(xyz), torch.from_numpy(ld), ka, kd).numpy()
    s_np = lc.shading_numpy(blurred[:, 0], xyz, ld, ka, kd, np.float64)
    e_n, e_np = float(np.abs(s - want).max()), float(np.abs(s - s_np).max())
    print(name, "shading vs reference normals", e_n, "vs numpy float64", e_np, "range", float(want.min()), float(want.max()))
    assert tuple(s.shape) == (depth.shape[0], H, W) and e_n <= 1e-5 and e_np <= 1e-12
    assert want.max() - want.min() > 0.1                                # the diffuse term varies over the image


def test_case_table_covers_the_matrix():
    shapes = {(c["H"], c["W"]) for c in lc.CASES.values()}
    assert shapes == set(lc.SHAPES) and all(h != w for h, w in shapes)
    for dt in lc.DTYPES:
        assert {(c["H"], c["W"]) for c in lc.CASES.values() if c["dtype"] == dt} == set(lc.SHAPES), dt
        assert {c["layout"] for c in lc.CASES.values() if c["dtype"] == dt} == set(lc.LAYOUTS), dt
    assert set(lc.N0) == set(lc.CASES)


@pytest.mark.parametrize("name", list(lc.CASES))
def test_layout_of_case_is_the_one_its_name_says(name):
    inp = lc.inputs(name)
    view = lc.lay_out(inp["stored"], inp["layout"])
    H, W, lay = inp["H"], inp["W"], inp["layout"]
    assert torch.equal(view.double(), inp["values"]) and view.stride(4) == 1
    want_vec = W % 4 == 0 and lay in ("contiguous", "rowpad4", "expand", "chanslice")
    assert lc.takes_vector_instance(view) == want_vec, (view.stride(), view.storage_offset())
    if lay == "rowpad4":
        assert view.stride(3) == W + 4
    if lay == "rowpad1":
        assert view.stride(3) == W + 1
    if lay == "expand":
        assert view.stride(0) == 0
    if lay == "offset1":
        assert view.storage_offset() == 1 and view.is_contiguous()
    if lay == "chanslice":
        assert view.stride(1) == 6 * H * W and view.storage_offset() == H * W
    v = inp["values"].numpy()
    assert (v[:, :, :3] == 0).any() and (v[:, :, :3] == 1).any() and (v[:, -1, 3] == 1).all()
    assert 0 < inp["nudged"] < 0.05


@pytest.mark.parametrize("name", list(lc.CASES))
def test_bar_of_case_is_above_the_noise_and_far_below_a_wrong_kernel(name):
    inp = lc.inputs(name)
    H, W = inp["H"], inp["W"]
    n0, bar = lc.noise_floor(inp), lc.bar(name)
    ref = lc.reference(inp)
    rgb = (slice(None), slice(None), slice(0, 3))
    transposed = float(np.abs(lc.reference(inp, xyz=lc.transposed_grid(inp)) - ref)[rgb].max())
    shifted = float(np.abs(lc.reference(inp, values=lc.shifted_alpha(inp)) - ref)[rgb].max())
    clipped = float((ref[rgb] == 1).mean())
    print(f"{name}: n0 {n0:.3e} recorded {lc.N0[name]:.1e} bar {bar:.1e} transposed grid {transposed / bar:.0f} bars, shifted depth {shifted / bar:.0f} bars, "
          f"{clipped:.2f} of rgb*s clip at 1")
    assert 0.85 * lc.N0[name] <= n0 <= lc.N0[name], (n0, lc.N0[name])       # the table holds what is measured here, rounded up
    if max(H, W) <= lc.WIDE:
        assert lc.N0[name] <= lc.NOISE_CAP and bar <= 4 * lc.NOISE_CAP
    assert transposed >= 50 * bar and shifted >= 50 * bar
    assert clipped > 0.05
    # the shading kernel's comparison (float64 numpy from a given fp32 blurred depth): its own floor and the transposed grid
    blurred = _scipy_blur(oracle.alpha_depth(inp["values"][:, :, 3:].float().numpy(), inp["plane_ds"])[0]).astype(np.float32)[:, 0]
    args = (inp["light_dir"], inp["ka"], inp["kd"])
    s64 = lc.shading_numpy(blurred, inp["xyz"], *args, np.float64)
    n0_s = float(np.abs(lc.shading_numpy(blurred, inp["xyz"], *args, np.float32) - s64).max())
    bar_s = max(1e-5, 4 * n0_s)
    t_s = float(np.abs(lc.shading_numpy(blurred, lc.transposed_grid(inp), *args, np.float64) - s64).max())
    print(f"{name}: shading kernel floor {n0_s:.3e} bar {bar_s:.1e} transposed grid {t_s / bar_s:.0f} bars")
    if max(H, W) <= lc.WIDE:
        assert n0_s <= lc.NOISE_CAP
    assert t_s >= 50 * bar_s


@pytest.mark.parametrize("name", list(lc.CASES))
def test_gradient_of_case_reaches_every_tensor(name):
    inp = lc.inputs(name)
    _, g64 = lc.reference(inp, grad=True)
    _, g32 = lc.reference(inp, dtype=torch.float32, grad=True)
    scale = float(np.abs(g64).max())
    e_ref = float(np.abs(g32 - g64).max()) / scale
    upstream = inp["g"][:, :, 3].sum(0, keepdims=True) if inp["layout"] == "expand" else inp["g"][:, :, 3]
    share = float(np.abs(g64[:, :, 3] - upstream).max()) / scale
    print(f"{name}: max|g_ref| {scale:.3e} rgb {np.abs(g64[:, :, :3]).max():.3e} alpha {np.abs(g64[:, :, 3]).max():.3e} e_ref {e_ref:.2e} "
          f"shading share of the alpha gradient {share:.2e}")
    assert g64.shape[0] == (1 if inp["layout"] == "expand" else lc.B)
    assert np.abs(g64[:, :, :3]).max() > 0 and np.abs(g64[:, :, 3]).max() > 0
    assert share > 1e-3
    assert e_ref <= 2.5e-4          # the fp32 chain itself is within the order of the backward's 2e-4 bar: 4 * e_ref stays a tight bar
    assert (g64[:, :, :3] == 0).any()   # clipped texels pass no gradient


def test_territory_formula_places_both_loops():
    """The indexing model by which tests/test_hip_aux_kernels.py places a bad value in the unrolled body or in the remainder loop of
    range_check_vec_kernel, against a walk through the kernel's two loops."""
    import test_hip_aux_kernels as aux
    for nvec in (1, 255, 1024, 3 * aux.FULL_GRID, 3 * aux.FULL_GRID + 1, 4 * aux.FULL_GRID + 5, 10 * aux.FULL_GRID + 777):
        G = min((nvec + aux.THREADS - 1) // aux.THREADS, aux.BLOCKS_MAX) * aux.THREADS
        for g in (0, 1, 4, 5, 776, 777, G - 1):
            if g >= G:
                continue
            i, owned = g, {}
            while i + 3 * G < nvec:
                for u in range(4):
                    owned[i + u * G] = "unrolled"
                i += 4 * G
            while i < nvec:
                owned[i] = "remainder"
                i += G
            assert all(aux._territory(j, nvec) == kind for j, kind in owned.items()), (nvec, g)
            assert sorted(owned) == list(range(g, nvec, G))
