"""The LDS-staged kernels on ray fields that are NOT a pinhole camera's (tests/_ray_field_cases.py: `permuted`, `bulge`), and the texel gather's
escape for a (view, plane) without a usable homography.

Every staged kernel sizes a tile's texel box from the tile's four corner pixels.  The kernels under test promise more than the pinhole case
(include/gmpi_render.h; the heads of render_shared_forward.hip, render_shaded.hip, render_u8.hip, render_depth_window.hip, render_backward.hip,
render_shared.hip, render_depth_tile.hip): a pixel whose taps fall outside its tile's box takes a per-lane path, so any ray field gives correct
pixels / gradients.  The two fields keep every corner pixel's bits, so the boxes are the pinhole field's, and move a quarter of the other
pixels far out of their boxes (`permuted`) or by up to five texels across the box edges (`bulge`); tests/test_ray_field_cases_cpu.py counts, with
the kernels' own constants, how many footprints land where (at least 500 far, at least 100 straddling a box edge, tiles with all classes).

Forward (`twin` 36 x 52 and `coarse` 14 x 28 texels, strict-order and default mode): the staged shared-colour forward with a background, the
staged shaded forward, the uint8 staged kernel planar and channels-last plus a chunked uint8 stack cut 2 + 3, the depth window forward --
strict mode bit-equal to the one-pixel kernel of the same entry and to `oracle.render` on the expanded volume, default mode within the bars of
each kernel's own test file, status word 0, and a spy on the C ABI that proves the staged kernel took the launch.

Backward (`twin`, `broad` 42 x 170, `coarse`; upstream families `normal` and `same_sign`): `test_hip_upstream_gradients.run` with the scene's
rays replaced, every (MPI, plane, channel) slab held by `slab_compare` to float64 autograd through the same rays -- max(5e-5, 4 e_ref) of the
slab's own maximum, nothing left out.  For `permuted` the run under equally permuted upstream gradients is also compared with the PINHOLE run
of the same path: the same sum in another order, under the same bar -- a cold path that agreed with a wrong reference would not.  The
volume entry's FORWARD is staged under the module's default variant and takes a pinhole field as a precondition (below), and its backward
starts from the transmittance that forward left: in these tests the forward launches of the volume and chunk entries reach the library as
GMPI_VARIANT_GATHER (`bwd_abi`), the backward's as the module's own -- recorded, so a path that ran another backward fails.

The texel gather without a usable homography: images of 1 x 40 and 40 x 1 pixels fail `p.W >= 2 && p.H >= 2` in `homography_kernel`
(render_backward_gather.hip), "a (view, plane) without a usable homography looks at every pixel: slow, still exact" -- the three gather pairs
under the slab rule, twice for equal bits, with the proof that the pair ran.

Out of scope, by the header's own words (include/gmpi_render.h), which make a pinhole field a PRECONDITION there:
  * the volume forward's LDS, WAVE and BAND variants and so AUTO -- `ray_dir`: "The LDS-staged variants (LDS, WAVE, BAND and therefore AUTO) stage,
    per pixel tile and plane, the texel box spanned by the tile's four corner pixels: that contains every tap of the tile iff the field is a pinhole
    camera's [...]; an arbitrary smooth field needs GMPI_VARIANT_GATHER";
  * the three gather pairs on `permuted` and `bulge` -- "`ray_dir` must be a pinhole ray field [...] for the tile kernels' texel boxes and for the
    gather's candidate windows", "The candidate windows assume a pinhole ray field (see ray_dir above)";
  * rays that are not finite: no finite-ray cases; the NaN-ray tests of each kernel's own file keep covering them.
Run on the MI355X box:  python -m pytest tests/test_hip_ray_fields.py -m gpu"""
import functools

import numpy as np
import pytest
import torch

import oracle
import _ray_field_cases as F
import _upstream_cases as U
import test_hip_depth_alpha_window as DW
import test_hip_shaded_render as SR
import test_hip_shared_forward_staged as SF
import test_hip_u8_interleaved as U8I
import test_hip_u8_storage as U8
import test_hip_upstream_gradients as T
from _visible import half_ulp, slab_compare
from test_hip_depth_alpha_window import abi as window_abi          # noqa: F401  (fixtures, under names of their own)
from test_hip_parity import TOL
from test_hip_shaded_render import abi as shaded_abi               # noqa: F401
from test_hip_shared_forward_staged import abi as shared_abi       # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("color", "depth", "T")
FWD_TEX = ("twin", "coarse")
BWD_TEX = ("twin", "broad", "coarse")
FAMILIES = ("normal", "same_sign")
BWD_PATHS = ("tile-f32", "tile-bf16", "tile-vpm2", "chunks-2+3", "shaded", "shared-tile", "depth-tile", "variant-gather", "depth-pixel")
BWD_RUNS = [(p, t) for p in T.PATHS if p.name in BWD_PATHS for t in p.textures if t in BWD_TEX]
BWD_IDS = [f"{p.name}-{t}" for p, t in BWD_RUNS]
assert {p.name for p, _ in BWD_RUNS} == set(BWD_PATHS) and len(BWD_RUNS) == 8 * 3 + 1


def _geo(tex, field):
    case = F.scene(tex, field)
    return tuple(torch.from_numpy(case[k]) for k in ("dhw", "ray", "eye", "zd"))


# ---- forward ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", F.MOVED)
@pytest.mark.parametrize("tex", FWD_TEX)
def test_staged_shared_colour_forward(shared_abi, tex, field):
    """`variant="lds"` with a background: strict == `variant="gather"` == the oracle, default within the bars, both launches staged (SF._check)."""
    (rgb, alpha, bg), _ = U.layout_parts("shared", tex)
    SF._check(shared_abi, ("ray field", tex, field), rgb, alpha, bg, *_geo(tex, field), True)


@functools.lru_cache(maxsize=None)
def _shaded_case(tex, field):
    case = F.scene(tex, field, shaded=True)
    vol, s = torch.from_numpy(case["rgba"]), torch.from_numpy(case["shading"])
    geo = _geo(tex, field)
    orc = oracle.render(SR.shaded_volume(vol, s).numpy(), *geo, align_corners=True, threads=True)
    return (vol, s, *geo, orc)


@pytest.mark.parametrize("field", F.MOVED)
@pytest.mark.parametrize("tex", FWD_TEX)
def test_staged_shaded_forward(shaded_abi, tex, field):
    """`variant="gather"` and `variant="lds"`: each strict == the oracle on the shaded volume (so equal to each other), default within the bars,
    the "lds" launches staged (SR.check_forward)."""
    SR.check_forward(shaded_abi, _shaded_case(tex, field), variants=("gather", "lds"), check_last=False)


@pytest.fixture
def volume_abi(monkeypatch):
    """(variant, dtype, planes) of every launch of the volume entry and of the chunk entry."""
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    seen = dict(render=[], chunk=[])
    for key, name in (("render", "gmpi_mpi_render_launch"), ("chunk", "gmpi_mpi_render_chunk_launch")):
        def spy(params, *rest, _real=getattr(lib, name), _key=key):
            p = params._obj
            seen[_key].append((int(p.variant), int(p.rgba_dtype), int(p.D)))
            return _real(params, *rest)
        monkeypatch.setattr(lib, name, spy)
    return seen


@functools.lru_cache(maxsize=None)
def _codes(tex):
    Ht, Wt = U.TEXTURES[tex]
    return U8.codes(300 + Ht, (U.M, U.D, 4, Ht, Wt))


@pytest.mark.parametrize("layout", ["planar", "channels-last"])
@pytest.mark.parametrize("field", F.MOVED)
@pytest.mark.parametrize("tex", FWD_TEX)
def test_staged_uint8_forward(volume_abi, tex, field, layout):
    """Strict == the oracle on q / 255 for "gather" and "lds", default mode within the uint8 files' bars (U8.check: colour 0.5e-5 on the [0, 1]
    scale, depth and T 1e-5) and, for the staged kernel's colour, within 5e-7 -- four ulps of 1, what a blend of five planes in another order of
    roundings can move; channels-last also bit-equal to the planar volume of the same codes (U8I.check_both).  An explicit "lds" the library
    cannot stage is refused, never re-routed: the spy sees every "lds" launch reach the entry as LDS on the uint8 type."""
    from ml_gmpi_amd import _lib as L
    q = _codes(tex)
    if layout == "planar":
        orc, _ = U8.check(q, *_geo(tex, field), variants=("gather", "lds"), check_last=False, label=f"{tex} {field}")
    else:
        q = U8I.as_volume(U8I.as_layers(q))
        orc, _ = U8I.check_both(q, *_geo(tex, field), variants=("gather", "lds"), check_last=False, label=f"{tex} {field} cl")
    fast = U8.hip(q, *_geo(tex, field), variant="lds", check_last=False)
    assert float(np.abs(fast["color"] - orc["color"]).max()) <= 5e-7
    staged = [s for s in volume_abi["render"] if s[0] == L.VARIANT_LDS]
    assert len(staged) >= 2 and all(s == (L.VARIANT_LDS, L.DTYPE_U8, U.D) for s in staged), volume_abi
    assert {s[0] for s in volume_abi["render"]} == {L.VARIANT_LDS, L.VARIANT_GATHER}


@pytest.mark.parametrize("field", F.MOVED)
def test_chunked_uint8_stack_cut_2_plus_3(volume_abi, field):
    """The carry instance of the staged uint8 kernel: two launches, the pixel's state handed from one to the next; the bits of the oracle (strict)
    and of the one-shot staged render (both modes)."""
    from ml_gmpi_amd import MPI, _lib as L
    tex = "twin"
    q = _codes(tex)
    geo = _geo(tex, field)
    orc = U8.reference(q, *geo)
    dgeo = tuple(t.cuda() for t in geo)
    for strict in (True, False):
        mpi = MPI(align_corners=True, variant="lds", strict_order=strict, on_out_of_plane="raise")
        volume_abi["chunk"].clear()
        with torch.no_grad():
            res = mpi.render_views_chunks([q[:, :2].contiguous().cuda(), q[:, 2:].contiguous().cuda()], *dgeo, check_last_plane=False,
                                          want_transmittance=True, defer_status=True)
        torch.cuda.synchronize()
        assert volume_abi["chunk"] == [(L.VARIANT_LDS, L.DTYPE_U8, 2), (L.VARIANT_LDS, L.DTYPE_U8, 3)] and mpi.chunk_variant_fallbacks == 0, volume_abi
        assert int(res["status"][0].item()) == 0
        got = {k: res[k].cpu().numpy() for k in KEYS}
        one = U8.hip(q, *geo, variant="lds", strict=strict, check_last=False)
        for k in KEYS:
            assert np.array_equal(got[k], one[k]), (strict, k)
            if strict:
                assert np.array_equal(got[k], orc[k]), k
        errs = {k: float(np.abs(got[k] - orc[k]).max()) for k in KEYS}
        assert errs["color"] <= 0.5 * TOL and errs["depth"] <= TOL and errs["T"] <= TOL, (strict, errs)


@pytest.mark.parametrize("field", F.MOVED)
@pytest.mark.parametrize("tex", FWD_TEX)
def test_depth_window_forward(window_abi, tex, field):
    """`depth_forward="window"`: both modes bit-equal to the one-pixel kernel, strict == the oracle on the expanded volume, default within the
    bars, the window kernel launched (DW._check).  (The row swap of tests/test_hip_depth_alpha_window.py stays where it is.)"""
    (rgb, depth, bg), (plane_z, zb) = U.layout_parts("depth", tex)
    DW._check(window_abi, ("ray field", tex, field), (rgb, depth, plane_z, bg, *_geo(tex, field), zb))


# ---- backward ---------------------------------------------------------------------------------------------------------------------------------------
# the C entry every path's backward must reach, and the variant in its launch struct (AUTO: the tile kernel; GATHER: one pixel per lane)
BWD_ENTRY = {"volume": "gmpi_mpi_render_backward_ex_launch", "chunks": "gmpi_mpi_render_chunk_backward_launch", "shaded": "gmpi_mpi_render_shaded_backward_launch",
             "shared": "gmpi_mpi_render_shared_backward_launch", "depth-tile": "gmpi_mpi_render_depth_backward_tile_launch",
             "depth-pixel": "gmpi_mpi_render_depth_backward_launch"}


@pytest.fixture
def bwd_abi(monkeypatch):
    """The volume entry's FORWARD takes a pinhole field as a precondition in every variant but GATHER (include/gmpi_render.h, `ray_dir`), and the
    Python layer picks the tile backward only for a module whose forward is one of those.  What is under test here is the backward, which makes
    no such assumption and starts from the transmittance the forward left: the forward launches of the volume and chunk entries are handed to the
    library as GMPI_VARIANT_GATHER (the launch struct is put back before the bridge reads it), so that T is defined; the backward's struct is
    rebuilt from the module's own variant.  Every backward launch is recorded as (entry, variant)."""
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    seen = dict(forward=[], backward=[])
    for name in ("gmpi_mpi_render_launch", "gmpi_mpi_render_chunk_launch"):
        def forward(params, *rest, _real=getattr(lib, name)):
            p = params._obj
            asked = int(p.variant)
            seen["forward"].append(asked)
            p.variant = L.VARIANT_GATHER
            try:
                return _real(params, *rest)
            finally:
                p.variant = asked
        monkeypatch.setattr(lib, name, forward)
    for name in BWD_ENTRY.values():
        def backward(params, *rest, _real=getattr(lib, name), _name=name):
            seen["backward"].append((_name, int(params._obj.variant)))
            return _real(params, *rest)
        monkeypatch.setattr(lib, name, backward)
    return seen


def _launched(path):
    """What `bwd_abi` must have seen of one run of `path`."""
    from ml_gmpi_amd import _lib as L
    key = path.kind if path.kind != "depth" else f"depth-{path.kw['mode']}"
    variant = L.VARIANT_GATHER if path.kw.get("variant") == "gather" else L.VARIANT_AUTO
    return [(BWD_ENTRY[key], variant)] * (2 if path.kind == "chunks" else 1)


def _refs(path, tex, field, family):
    if path.kind in ("shared", "depth"):
        return F.layout_refs(path.kind, tex, field, family)
    r64, r32 = F.volume_refs(tex, field, family, path.vpm, path.dtype, path.kind == "shaded")
    return (list(r64), list(r32)) if path.kind == "shaded" else ([r64], [r32])


def _dtype(path, i):
    return path.torch_dtype if path.kind != "shaded" or i == 0 else torch.float32


@pytest.mark.parametrize("field", F.MOVED)
@pytest.mark.parametrize("path,tex", BWD_RUNS, ids=BWD_IDS)
def test_backward_against_float64_through_the_same_rays(bwd_abi, path, tex, field):
    failures = {}
    for family in FAMILIES:
        case = F.scene(tex, field, path.vpm)
        bwd_abi["backward"].clear()
        got = [g.double().numpy() for g in T.run(path, tex, U.upstream(family, case["N"], U.H, U.W, 5), field=field)]
        assert bwd_abi["backward"] == _launched(path), bwd_abi
        r64, r32 = _refs(path, tex, field, family)
        for i, (g, a, b) in enumerate(zip(got, r64, r32)):
            if not np.isfinite(g).all():
                failures[family, i, "finite"] = int((~np.isfinite(g)).sum())
                continue
            res = slab_compare(g, a, b, _dtype(path, i), min_rel_scale=0, label=f"RATIO {path.name} {tex} {field} {family} [{i}]")
            assert res["skipped"] == 0
            if res["failures"]:
                failures[family, i] = (len(res["failures"]), res["worst"], res["where"], res["failures"][:3])
    assert not failures, failures


@functools.lru_cache(maxsize=None)
def _pinhole_run(path, tex, family):
    """The path's gradients on the camera's own rays (computed once, under the same fixture; never written to)."""
    case = U.scene(tex, path.vpm)
    return T.run(path, tex, U.upstream(family, case["N"], U.H, U.W, 5))


@pytest.mark.parametrize("path,tex", BWD_RUNS, ids=BWD_IDS)
def test_permuted_rays_under_permuted_gradients_give_the_pinhole_runs_gradients(bwd_abi, path, tex):
    """ray'[q] = ray[pi q] and g'[q] = g[pi q]: pixel q does what pixel pi(q) does in the pinhole run, so every texel receives the same terms in
    another order.  Held to (a)'s bar per slab, max(5e-5, 4 e_ref) of the slab's own maximum (+ an ulp of a gradient returned in 16 bits: each run
    rounds once), against the kernel's OWN pinhole run -- no reference of the moved field enters."""
    failures = {}
    for family in FAMILIES:
        case = F.scene(tex, "permuted", path.vpm)
        ups = tuple(F.permute_pixels(g) for g in U.upstream(family, case["N"], U.H, U.W, 5))
        moved = T.run(path, tex, ups, field="permuted")
        still = _pinhole_run(path, tex, family)
        assert bwd_abi["backward"][-len(_launched(path)):] == _launched(path), bwd_abi
        r64, r32 = T.refs(path, tex, family)   # the pinhole references: the scale and e_ref of every slab
        for i, (m, s) in enumerate(zip(moved, still)):
            m, s = m.double().numpy(), s.double().numpy()
            assert np.isfinite(m).all() and np.isfinite(s).all() and float(np.abs(s).max()) > 0
            bar = np.broadcast_to(T._allowed(r64[i], r32[i]), m.shape) + 2 * half_ulp(np.maximum(np.abs(m), np.abs(s)), _dtype(path, i))
            ratio = np.abs(m - s) / np.where(bar > 0, bar, 1.0)
            ratio = np.where(bar > 0, ratio, np.where(m == s, 0.0, np.inf))
            print(f"RATIO-PINHOLE {path.name} {tex} {family} [{i}] worst {ratio.max():.3f}")
            if ratio.max() > 1.0:
                failures[family, i] = (int((ratio > 1).sum()), float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    assert not failures, failures


# ---- the texel gather without a usable homography -------------------------------------------------------------------------------------------------
@pytest.fixture
def gather_abi(monkeypatch):
    """The volume pair's workspace query (what it answered) and whether the backward launch was lent a workspace."""
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    seen = dict(query=[], lent=[])
    real_query, real_launch = lib.gmpi_render_backward_workspace_bytes, lib.gmpi_mpi_render_backward_ex_launch

    def query(params):
        need = int(real_query(params))
        seen["query"].append(need)
        return need

    def launch(params, *rest):
        p = params._obj
        seen["lent"].append((int(p.workspace or 0) != 0, int(p.workspace_bytes), bool(int(p.flags) & L.FLAG_GRAD_OVERWRITE)))
        return real_launch(params, *rest)
    monkeypatch.setattr(lib, "gmpi_render_backward_workspace_bytes", query)
    monkeypatch.setattr(lib, "gmpi_mpi_render_backward_ex_launch", launch)
    return seen


def _line_run(kind, H, W):
    """Forward + backward of one gather pair on `line_scene(H, W)` -> (gradients as CPU tensors, module)."""
    from ml_gmpi_amd import MPI
    case = F.line_scene(H, W)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).to(DEV)
    geo = tuple(t(case[k]) for k in ("dhw", "ray", "eye", "zd"))
    kw = dict(views_per_mpi=1, check_last_plane=False, want_transmittance=True)
    if kind == "volume":
        mpi = MPI(align_corners=True, on_out_of_plane="raise", backward="gather")
        leaves = [t(case["rgba"]).requires_grad_(True)]
        out = mpi.render_views(leaves[0], *geo, **kw)
    else:
        parts, extra = U.layout_parts(kind, F.LINE_TEX)
        leaves = [t(p).clone().requires_grad_(True) for p in parts]
        mpi = MPI(align_corners=True, on_out_of_plane="raise")
        if kind == "shared":
            out = mpi.render_views_shared(leaves[0], leaves[1], *geo, background=leaves[2], shared_backward="gather", **kw)
        else:
            out = mpi.render_views_depth(leaves[0], leaves[1], t(extra[0]), extra[1], *geo, background=leaves[2], depth_backward="gather", **kw)
    assert tuple(out["color"].shape) == (case["N"], 3, H, W)
    ((out["color"] * t(case["gc"])).sum() + (out["depth"] * t(case["gd"])).sum() + (out["T"] * t(case["gT"])).sum()).backward()
    torch.cuda.synchronize()
    return [leaf.grad.detach().cpu() for leaf in leaves], mpi


@pytest.mark.parametrize("shape", F.LINES, ids=[f"{h}x{w}" for h, w in F.LINES])
@pytest.mark.parametrize("kind", ["volume", "shared", "depth"])
def test_gather_pairs_without_a_usable_homography(gather_abi, kind, shape):
    """One pixel row / one pixel column: no (view, plane) gets a usable homography, every texel looks at every pixel.  The slab rule against
    float64, two runs with equal bits, and the pair -- not the atomic kernels -- took the launch."""
    H, W = shape
    first, mpi = _line_run(kind, H, W)
    again, _ = _line_run(kind, H, W)
    if kind == "volume":
        assert len(gather_abi["query"]) == 2 and min(gather_abi["query"]) > 0, gather_abi
        assert gather_abi["lent"] == [(True, gather_abi["query"][0], True)] * 2, gather_abi
    else:
        assert mpi.layout_gather_fallbacks == 0
    r64, r32 = F.line_refs(kind, H, W)
    failures = {}
    for i, (g, g2, a, b) in enumerate(zip(first, again, r64, r32)):
        assert torch.equal(g, g2), (i, int((g != g2).sum()))
        assert bool(torch.isfinite(g).all())
        res = slab_compare(g.double().numpy(), a, b, min_rel_scale=0, label=f"RATIO line {kind} {H}x{W} [{i}]")
        assert res["skipped"] == 0
        if res["failures"]:
            failures[i] = (len(res["failures"]), res["worst"], res["where"], res["failures"][:3])
    assert not failures, failures
