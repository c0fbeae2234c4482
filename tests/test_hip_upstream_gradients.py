"""Every backward kernel on upstream gradients other than dense N(0,1) (tests/_upstream_cases.py: scaled by 2^-40 and 2^40, same-sign, sparse,
two scales side by side, one infinite / NaN pixel), each held to float64 autograd by the project's per-slab rule (tests/_visible.py
`slab_compare`: max(5e-5, 4 e_ref) of the slab's own maximum, nothing left out).  The staged backwards pick their fixed-point scale, their
headroom and whether they stage at all from exactly this input; tests/test_upstream_cases_cpu.py holds the inputs to the conditions that make
the comparisons below mean something (which path a texture takes, no denormals, the masks).

One table (`paths`) drives the same cases through the volume entry (tile kernel, fp32 and bf16; variant="gather"; backward="gather"), the chunked
render cut 2 + 3, the shaded render, the shared-colour and depth-alpha layouts with each of their backwards, and the geometry pass.  Per path and
texture:
  (a) finite families: every slab within the rule, everything finite, a slab whose reference is 0 exactly 0;
  (b) `two_scale`: the same rule with everything outside the right-hand region R set to 0 -- the dim half is held to its own maximum;
  (c) grads(2^k g) == ldexp(grads(g), k), k = +-40, bit for bit on the paths without atomics (the three gather pairs, the geometry pass);
  (d) `sparse`: exactly 0 on `far` and on the whole MPI of the all-zero view;
  (e) one infinite / NaN pixel: finite on `far` and equal to the clean run there (bit for bit without atomics, within (a)'s bar with them), and
      non-finite where the pixel's largest bilinear weight lands -- what a loss scaler's overflow check depends on;
      -- on every texture: `far` is smaller on the coarse ones, never empty; the geometry pass keeps the poison to its ray and view;
  (f) upstream gradients that are not contiguous, handed to the bridge as they are, give the bits of the contiguous ones.
Run on the MI355X box:  python -m pytest tests/test_hip_upstream_gradients.py -m gpu"""
import functools

import numpy as np
import pytest
import torch

import _upstream_cases as U
from _visible import SLAB_REF_FACTOR, SLAB_REL, half_ulp, slab_compare, slab_stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TEX = list(U.TEXTURES)


class Path:
    def __init__(self, name, kind, exact=False, dtype="f32", vpm=None, textures=None, **kw):
        self.name, self.kind, self.exact, self.dtype, self.vpm, self.kw = name, kind, exact, dtype, vpm, kw
        self.textures = TEX if textures is None else list(textures)

    @property
    def torch_dtype(self):
        return {"f32": torch.float32, "bf16": torch.bfloat16}[self.dtype]


def paths():
    """exact: neither atomics nor a data-dependent order -- (c) and (e) hold bit for bit."""
    return [
        Path("tile-f32", "volume"),
        Path("tile-bf16", "volume", dtype="bf16"),
        Path("tile-vpm2", "volume", vpm=2, textures=["twin"]),
        Path("variant-gather", "volume", variant="gather"),
        Path("backward-gather", "volume", exact=True, backward="gather"),
        Path("chunks-2+3", "chunks"),
        Path("shaded", "shaded"),
        Path("shared-tile", "shared", mode="tile"),
        Path("shared-gather", "shared", exact=True, mode="gather"),
        Path("depth-pixel", "depth", mode="pixel"),
        Path("depth-tile", "depth", mode="tile"),
        Path("depth-gather", "depth", exact=True, mode="gather"),
    ]


PATHS = paths()
RUNS = [(p, t) for p in PATHS for t in p.textures]
IDS = [f"{p.name}-{t}" for p, t in RUNS]
EXACT = [(p, t) for p, t in RUNS if p.exact]
POISONED = [(p, t, f) for p, t in RUNS for f in ("inf_pixel", "nan_pixel")]   # (every texture: `far` is smaller on the coarse ones, never empty)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).to(DEV)


def _dot(out, gc, gd, gT):
    ((out["color"] * gc).sum() + (out["depth"] * gd).sum() + (out["T"] * gT).sum()).backward()


def run(path, tex, ups, backward=_dot, field=None):
    """Forward + backward of `path` on the scene of `tex` under the upstream gradients `ups` = (gc, gd, gT) -> the gradients as CPU tensors in
    the order of the path's references.  backward(out, gc, gd, gT) back-propagates (default: through the sum of the three products).  field: a
    ray field of tests/_ray_field_cases.py in place of the camera's rays (tests/test_hip_ray_fields.py)."""
    from ml_gmpi_amd import MPI
    case = U.scene(tex, path.vpm, path.dtype, path.kind == "shaded", field)
    geo = tuple(_t(case[k]) for k in ("dhw", "ray", "eye", "zd"))
    kw = dict(views_per_mpi=path.vpm or 1, check_last_plane=False, want_transmittance=True)
    if path.kind in ("volume", "chunks", "shaded"):
        vol = _t(case["rgba"]).to(path.torch_dtype)
        assert torch.equal(vol.float().cpu(), torch.from_numpy(case["rgba"]))   # the references were fed the stored values
        mpi = MPI(align_corners=True, on_out_of_plane="raise", range_check="off" if path.kind == "shaded" else None, **path.kw)
        if path.kind == "volume":
            leaves = [vol.requires_grad_(True)]
            out = mpi.render_views(vol, *geo, **kw)
        elif path.kind == "chunks":
            leaves = [c.contiguous().requires_grad_(True) for c in torch.split(vol, [2, 3], 1)]
            out = mpi.render_views_chunks(leaves, *geo, **kw)
        else:
            leaves = [vol.requires_grad_(True), _t(case["shading"]).requires_grad_(True)]
            out = mpi.render_views_shaded(leaves[0], leaves[1], *geo, **kw)
    else:
        parts, extra = U.layout_parts(path.kind, tex)
        leaves = [_t(p).clone().requires_grad_(True) for p in parts]
        mpi = MPI(align_corners=True, on_out_of_plane="raise")
        if path.kind == "shared":
            out = mpi.render_views_shared(leaves[0], leaves[1], *geo, background=leaves[2], shared_backward=path.kw["mode"], **kw)
        else:
            out = mpi.render_views_depth(leaves[0], leaves[1], _t(extra[0]), extra[1], *geo, background=leaves[2], depth_backward=path.kw["mode"], **kw)
    backward(out, *(_t(g) for g in ups))
    torch.cuda.synchronize()
    if path.kind in ("shared", "depth"):
        assert mpi.layout_gather_fallbacks == 0
    for leaf in leaves:
        assert leaf.grad is not None and leaf.grad.dtype == leaf.dtype and leaf.grad.shape == leaf.shape
    grads = [leaf.grad.detach().cpu() for leaf in leaves]
    return [torch.cat(grads, 1)] if path.kind == "chunks" else grads


@functools.lru_cache(maxsize=None)
def grads(path, tex, family):
    """The path's gradients under a family, computed once (the clean run serves (c) and (e) too); never written to."""
    case = U.scene(tex, path.vpm)
    return run(path, tex, U.upstream(family, case["N"], U.H, U.W, 5))


def refs(path, tex, family):
    if path.kind in ("shared", "depth"):
        return U.layout_refs(path.kind, tex, family)
    r64, r32 = U.volume_refs(tex, family, path.vpm, path.dtype, path.kind == "shaded")
    return (list(r64), list(r32)) if path.kind == "shaded" else ([r64], [r32])


def _allowed(r64, r32):
    """(a)'s bar per slab, broadcast to the tensor: max(5e-5, 4 e_ref) of the slab's own maximum."""
    scale, e_ref = slab_stats(r64, r32)
    return (np.maximum(SLAB_REL, SLAB_REF_FACTOR * e_ref) * scale)[..., None, None]


# ---- (a), (b), (d) --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,tex", RUNS, ids=IDS)
def test_finite_families_against_float64(path, tex):
    failures = {}
    for family in U.FINITE:
        r64, r32 = refs(path, tex, family)
        got = [g.double().numpy() for g in grads(path, tex, family)]
        for i, (g, a, b) in enumerate(zip(got, r64, r32)):
            label = f"RATIO {path.name} {tex} {family} [{i}]"
            dt = path.torch_dtype if path.kind != "shaded" or i == 0 else torch.float32
            if not np.isfinite(g).all():
                failures[family, i, "finite"] = int((~np.isfinite(g)).sum())
                continue
            res = slab_compare(g, a, b, dt, min_rel_scale=0, label=label)   # (a slab whose reference is exactly 0 must be exactly 0)
            assert res["skipped"] == 0
            if res["failures"]:
                failures[family, i] = (len(res["failures"]), res["worst"], res["where"], res["failures"][:3])
            if family == "two_scale":                                       # (b)
                R = U.mask_for(U.right_region(tex, path.vpm), g)
                res = slab_compare(np.where(R, g, 0.0), np.where(R, a, 0.0), np.where(R, b, 0.0), dt, min_rel_scale=0, label=label + " right half")
                assert res["skipped"] == 0
                if res["failures"]:
                    failures[family, i, "right half"] = (len(res["failures"]), res["worst"], res["where"], res["failures"][:3])
            if family == "sparse":                                          # (d)
                if path.vpm is None and np.any(g[U.SPARSE_ZERO_VIEW]):
                    failures[family, i, "the MPI of the all-zero view"] = int(np.count_nonzero(g[U.SPARSE_ZERO_VIEW]))
                stray = np.count_nonzero(g[U.mask_for(U.far_mask(tex, "sparse", path.vpm), g)])
                if stray:
                    failures[family, i, "far"] = int(stray)
    assert not failures, failures


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,tex", EXACT, ids=[f"{p.name}-{t}" for p, t in EXACT])
def test_a_power_of_two_factor_commutes_with_the_backward(path, tex):
    base = grads(path, tex, "normal")
    for family, k in (("up40", 40), ("down40", -40)):
        for i, (g, g0) in enumerate(zip(grads(path, tex, family), base)):
            want = torch.ldexp(g0, torch.tensor(k))
            assert bool(torch.isfinite(want).all()) and float(g0.abs().max()) > 0
            assert torch.equal(g, want), (family, i, int((g != want).sum()), float((g - want).abs().max() / want.abs().max()))


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layout_alpha(kind, tex):
    """[M,D,Ht,Wt]: the alpha planes of the layout's expanded volume (CPU)."""
    from ml_gmpi_amd import expand_depth_alpha, expand_shared_color
    parts, extra = U.layout_parts(kind, tex)
    vol = expand_shared_color(*parts) if kind == "shared" else expand_depth_alpha(parts[0], parts[1], extra[0], extra[1][0], extra[1][1], parts[2])
    return vol[:, :, 3]


@pytest.mark.parametrize("path,tex,family", POISONED, ids=[f"{p.name}-{t}-{f}" for p, t, f in POISONED])
def test_one_poisoned_pixel_stays_in_its_footprint_and_arrives(path, tex, family):
    clean, dirty = grads(path, tex, "normal"), grads(path, tex, family)
    r64, r32 = refs(path, tex, "normal")
    far = U.far_mask(tex, family, path.vpm)
    for i, (c, d) in enumerate(zip(clean, dirty)):
        c, d = c.double().numpy(), d.double().numpy()
        mask = U.mask_for(far, d)
        assert np.isfinite(d[mask]).all(), (i, int((~np.isfinite(d[mask])).sum()))
        if path.exact:
            assert np.array_equal(d[mask], c[mask]), (i, int((d[mask] != c[mask]).sum()))
        else:
            dt = path.torch_dtype if path.kind != "shaded" or i == 0 else torch.float32
            bar = np.broadcast_to(_allowed(r64[i], r32[i]), d.shape) + half_ulp(np.maximum(np.abs(c), np.abs(d)), dt) * 2
            over = (np.abs(d - c) > bar) & mask
            assert not over.any(), (i, int(over.sum()), float(np.abs(np.where(mask, d - c, 0)).max()))
    # arrival: per plane, the texel under the pixel's largest bilinear weight
    inf = family == "inf_pixel"
    for m, k, y, x, inside in U.peak_texels(tex, path.vpm):
        assert inside
        if path.kind in ("volume", "chunks", "shaded"):
            cell = dirty[0][m, k, :, y, x].float()
            assert not bool(torch.isfinite(cell[3])), (k, cell)
            if inf and path.kind != "shaded":   # (shaded: a colour whose clip is closed passes nothing)
                assert not bool(torch.isfinite(cell[:3]).any()), (k, cell)
        elif path.kind == "shared":
            assert not bool(torch.isfinite(dirty[1][m, k, 0, y, x])), k
    if path.kind in ("shared", "depth"):
        # the images shared by the planes: a colour gradient w_k gC reaches the taps of every plane whose sampled alpha is not 0 (rgb; the last
        # plane's go to the background), a depth gradient the alphas alone
        alpha = _layout_alpha(path.kind, tex)
        fed = [(k, y, x) for m, k, y, x, _ in U.peak_texels(tex, path.vpm) if float(alpha[m, k, y, x]) > 0]
        if path.kind == "depth":   # behind the surface the planes are opaque (T = 0: nothing arrives): the front-most plane that has alpha only
            fed = fed[:1]
        assert fed and fed[0][0] < U.D - 1 and (path.kind == "depth" or fed[-1][0] == U.D - 1), fed
        m = U.peak_texels(tex, path.vpm)[0][0]
        if inf:
            for k, y, x in fed:
                assert not bool(torch.isfinite(dirty[2 if k == U.D - 1 else 0][m, :, y, x]).any()), k
        if path.kind == "depth":   # the depth image: somewhere in the footprint (a texel off every plane's ramp passes nothing)
            assert not bool(torch.isfinite(dirty[1][m]).all())
    if path.kind == "shaded" and inf:   # (the shading gradient is a sum of colour gradients: a depth gradient does not reach it)
        assert not bool(torch.isfinite(dirty[1]).all())


# ---- the geometry pass ------------------------------------------------------------------------------------------------------------------------------
def _geometry(tex, family):
    from test_hip_geometry_grad import _run
    case = U.scene(tex)
    gc, gd, _ = U.upstream(family, case["N"], U.H, U.W, 5)
    got, stored = _run(case["rgba"], case["dhw"], case["ray"], case["eye"], case["zd"], None, gc, gd, True, True, views_per_mpi=1)
    assert np.array_equal(stored, case["rgba"])
    return got


@pytest.mark.parametrize("tex", TEX)
def test_geometry_pass_under_every_finite_family(tex):
    """d/d(dhw, ray_dir, eye_pos, z_dir) in strict-order mode against tests/_geometry_ref.py under the bar of tests/test_hip_geometry_grad.py (1e-4,
    relative: the scaled families need no other number); (c) bit for bit -- the pass has no atomics; `sparse`: a ray without an upstream gradient gets none."""
    from test_hip_geometry_grad import _check
    got = {f: _geometry(tex, f) for f in U.FINITE}
    for k, family in ((40, "up40"), (-40, "down40")):
        for name, g, g0 in zip(("dhw", "ray", "eye", "z_dir"), got[family], got["normal"]):
            want = np.ldexp(g0, k)
            assert np.isfinite(want).all() and np.array_equal(g, want), (family, name, int((g != want).sum()))
    gc, gd, _ = U.upstream("sparse", U.M, U.H, U.W, 5)
    quiet = ~(np.abs(gc).sum(1) + np.abs(gd).sum(1)).astype(bool)
    assert not np.any(np.abs(got["sparse"][1]).sum(1)[quiet])
    failures = {}
    for family in U.FINITE:
        assert all(np.isfinite(g).all() for g in got[family]), family
        try:
            _check(got[family], U.geometry_refs(tex, family))
        except AssertionError as e:
            failures[family] = str(e)[:200]
    assert not failures, failures


@pytest.mark.parametrize("family", ["inf_pixel", "nan_pixel"])
@pytest.mark.parametrize("tex", TEX)
def test_geometry_pass_keeps_a_poisoned_pixel_to_its_own_ray_and_view(tex, family):
    """(e) for the geometry pass: the ray gradient of every other pixel, and the eye and z_dir gradients of the other view, are finite and have the
    bits of the clean run (no atomics); the poisoned ray's gradient is not finite, nor are the sums it enters (its view's eye, its MPI's dhw)."""
    clean, dirty = _geometry(tex, "normal"), _geometry(tex, family)
    n0, py, px = U.POISON
    others = np.ones(clean[1].shape, dtype=bool)
    others[n0, :, py, px] = False
    assert np.isfinite(dirty[1][others]).all() and np.array_equal(dirty[1][others], clean[1][others])
    assert not np.isfinite(dirty[1][n0, :, py, px]).all()
    for c, d in zip(clean[2:], dirty[2:]):   # eye, z_dir per view
        assert np.array_equal(d[1 - n0], c[1 - n0]) and np.isfinite(d[1 - n0]).all()
    assert np.array_equal(dirty[0][1 - n0], clean[0][1 - n0]) and np.isfinite(dirty[0][1 - n0]).all()   # dhw of the other MPI (views_per_mpi = 1)
    assert not np.isfinite(dirty[2][n0]).all() and not np.isfinite(dirty[0][n0]).all()


# ---- (f) --------------------------------------------------------------------------------------------------------------------------------------------
def test_strided_upstream_gradients_give_the_contiguous_bits():
    """Gradients that are NOT contiguous handed straight to the bridge (`torch.autograd.backward(outputs, grad_tensors)`: the engine passes a
    strided tensor of the right shape and dtype on as it is; a loss on `color.permute(...)` or `depth[..., ::2]` does not -- the backward of those
    ops returns a dense tensor): colour as a transposed buffer viewed back to [N,3,H,W], depth as every second column of a buffer twice as wide
    (a launch that read either as if it were dense would stay inside the buffer).  `_upstream` (hip_mpi.py) must make them contiguous: the
    gradients are those of the same values handed over dense, bit for bit (backward="gather": no atomics).  A float64 gradient cannot reach the
    bridge through autograd -- the engine casts grad_tensors to the output's dtype --: tests/test_upstream_cases_cpu.py calls `_upstream` with one."""
    path = next(p for p in PATHS if p.name == "backward-gather")
    ups = U.upstream("normal", U.M, U.H, U.W, 5)
    want = run(path, "twin", ups)[0]
    seen = []

    def strided(out, c, d, t):
        gc = c.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
        wide = torch.zeros((*d.shape[:-1], 2 * d.shape[-1]), dtype=d.dtype, device=d.device)
        wide[..., ::2] = d
        gd = wide[..., ::2]
        assert not gc.is_contiguous() and not gd.is_contiguous() and torch.equal(gc, c) and torch.equal(gd, d)
        seen.append((gc.stride(), gd.stride()))
        torch.autograd.backward([out["color"], out["depth"], out["T"]], [gc, gd, t])

    got = run(path, "twin", ups, backward=strided)[0]
    assert seen and float(want.abs().max()) > 0
    assert torch.equal(got, want), int((got != want).sum())
