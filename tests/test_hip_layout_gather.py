"""The atomics-free backward of the shared-colour and depth-alpha layouts on the GPU (render_backward_gather.hip: layout_pixel_pass_kernel,
layout_texel_gather_kernel, layout_reduce_kernel; `shared_backward="gather"` / `depth_backward="gather"`): bit-reproducible, equal to the layouts'
atomic backwards up to the order of the adds, equal to float64 autograd through `expand_shared_color` / `expand_depth_alpha` under the project's
rule, under every number of plane runs; every cell written once and nothing else touched; non-finite records contained; fallbacks; refusals.

Three checks recur (fp32 inputs):
  (a) two gather runs are `torch.equal` for every gradient tensor;
  (b) gather against the layout's atomic default within 1e-5 max|g| per tensor (the bar tests/test_hip_backward.py uses for the volume pair);
  (c) gather against float64 autograd under tests/test_hip_shared_color._compare's rule, max(5e-5, 4 e_ref) max|g_ref| + 1e-6, with e_ref <= 2e-4
      asserted (tests/test_hip_depth_alpha._compare_capped).
The cameras are test_hip_backward._rot_cam's (yaw, pitch, roll), the textures oracle.synth_rgba's white noise cut up by test_hip_shared_color._parts,
the depth surfaces test_hip_depth_alpha._depth_image's (smooth, no texel within 1e-4 of a bound of a ramp), cropped to the texture.  For every case
below the fp32 torch chain alone was checked on the CPU against float64 first: e_ref is 1.6e-6 to 6.4e-5 per tensor for all of them (largest where the texture is
finer than the image), below the 2e-4 cap, and max|g_ref background| is at least 1.6e-2 max|g_ref rgb| (the 130-plane shared-colour stack; 0.3 to 1.8
elsewhere).
The float64 and fp32 references of a case are computed once and shared by the tests that use it."""
import ctypes
import functools
import itertools
import warnings

import numpy as np
import pytest
import torch

import oracle
import test_hip_depth_alpha as DA
import test_hip_shared_color as SC
from test_hip_backward import _rot_cam
from test_hip_edge_cases import _dhw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("shared", "depth")
ARG = {"shared": "shared_backward", "depth": "depth_backward"}

# the seven shapes of test_hip_backward.test_gather_backward_matches_autograd_and_is_bit_reproducible
SHAPES = [
    dict(H=160, W=160, Ht=128, Wt=128, yaw=0.0, pitch=0.0, roll=0.0, vpm=1),
    dict(H=160, W=192, Ht=192, Wt=160, yaw=0.35, pitch=0.12, roll=0.0, vpm=1),     # tilted: the pixel boxes of the texel tiles shear
    dict(H=144, W=160, Ht=128, Wt=128, yaw=0.25, pitch=-0.1, roll=0.5, vpm=1),     # in-plane rotation: a texel's candidates are a rotated window
    dict(H=144, W=160, Ht=128, Wt=128, yaw=0.1, pitch=0.1, roll=1.3, vpm=2),       # nearly a quarter turn; two views of every MPI summed in registers
    dict(H=96, W=224, Ht=40, Wt=56, yaw=0.3, pitch=0.0, roll=0.2, vpm=1),          # texture coarser than the image: many pixels per texel
    dict(H=100, W=130, Ht=300, Wt=260, yaw=0.3, pitch=0.1, roll=-0.3, vpm=1),      # texture finer than the image: most texels get nothing
    dict(H=40, W=1800, Ht=32, Wt=64, yaw=0.2, pitch=0.0, roll=0.0, vpm=1),         # a pixel box wider than a chunk (column blocks)
]
SMALL = dict(H=64, W=80, Ht=37, Wt=83, yaw=0.2, pitch=0.1, roll=0.3, vpm=1)        # Wt, Ht no multiples of 64 / 16; two tile columns, three rows


class Case:
    """One scene: parts = (rgb, alpha planes | depth image, background or None) in the storage dtype, the geometry, the upstream gradients."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def v2m(self):
        return [n // self.vpm for n in range(self.N)]


@functools.lru_cache(maxsize=None)
def _case(kind, with_bg, H, W, Ht, Wt, yaw, pitch, roll, vpm, M=2, D=5, nzb=4, dtype=torch.float32, alpha_scale=None, reach=None, n_views=None):
    """Cached: shared by the tests, never written to.  alpha_scale: the white-noise alphas are thinned (with a background: by 0.5, so that the
    last plane keeps a gradient worth comparing; deep stacks say their own).  reach: the depth surface scaled to this maximum (holes)."""
    N = n_views or M * vpm
    rgba = torch.from_numpy(oracle.synth_rgba(63, (M, D, 4, Ht, Wt)))
    ray, eye, zd = _rot_cam(N, H, W, yaw, pitch, roll)
    dhw = _dhw(M, D, ext=0.30, last=0.6)
    g = np.random.default_rng(19)
    gc, gd, gT = (g.standard_normal((N, c, H, W)).astype(np.float32) for c in (3, 1, 1))
    if kind == "shared":
        rgb, mid, bg = SC._parts(rgba, dtype)
        mid = (mid.float() * (alpha_scale or (0.5 if with_bg else 1.0))).to(dtype)
        plane_z = zb = None
    else:
        q = lambda t: t.contiguous().to(dtype)
        rgb, bg = q(rgba[:, 0, :3]), q(rgba[:, -1, :3])
        depth, plane_z = DA._depth_image(M, max(Ht, Wt), D, nzb, dtype, reach)
        mid, zb = depth[:, :, :Ht, :Wt].contiguous(), DA._bounds(nzb)
    return Case(kind=kind, with_bg=with_bg, parts=(rgb, mid, bg if with_bg else None), plane_z=plane_z, zb=zb, dhw=dhw, ray=ray, eye=eye, zd=zd,
                vpm=vpm, N=N, M=M, D=D, H=H, W=W, Ht=Ht, Wt=Wt, dtype=dtype, gc=gc, gd=gd, gT=gT)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(float64, fp32) gradients of the torch reference through the layout's expand function (CPU), computed once per case."""
    out = []
    for dtype in (torch.float64, torch.float32):
        if case.kind == "shared":
            out.append(SC._reference_grads(case.parts, case.dhw, case.ray, case.eye, case.zd, case.v2m, case.gc, case.gd, case.gT, False, dtype))
        else:
            rgb, depth, bg = case.parts
            tup = (rgb, depth, case.plane_z, bg, torch.as_tensor(case.dhw), case.ray, case.eye, case.zd, case.zb)
            out.append(DA._reference_grads(tup, case.with_bg, case.v2m, case.gc, case.gd, case.gT, False, dtype))
    return tuple(out)


def _run(case, mode=None, needs=(True, True, True), runs=None, ac=True, view_to_mpi=None, gc=None):
    """One forward + backward through `MPI`; mode None: the layout's default (atomic) backward.  Returns (gradients, outputs, module)."""
    from ml_gmpi_amd import MPI
    dev = torch.device(DEV)
    ins = [None if p is None else p.to(dev).clone().requires_grad_(n) for p, n in zip(case.parts, needs)]
    mpi = MPI(align_corners=ac, on_out_of_plane="raise")
    t = lambda a: torch.as_tensor(a).to(dev)
    kw = dict(background=ins[2], check_last_plane=False, want_transmittance=True)
    if view_to_mpi is None:
        kw["views_per_mpi"] = case.vpm
    else:
        kw["view_to_mpi"] = torch.as_tensor(np.asarray(view_to_mpi, dtype=np.int32)).to(dev)
    if mode is not None:
        kw[ARG[case.kind]] = mode
    if runs is not None:
        kw["_gather_runs"] = runs
    geo = (t(case.dhw), t(case.ray), t(case.eye), t(case.zd))
    if case.kind == "shared":
        out = mpi.render_views_shared(ins[0], ins[1], *geo, **kw)
    else:
        out = mpi.render_views_depth(ins[0], ins[1], t(case.plane_z), case.zb, *geo, **kw)
    loss = 0
    for key, g in (("color", case.gc if gc is None else gc), ("depth", case.gd), ("T", case.gT)):
        loss = loss + (out[key] * t(g)).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = [None if i is None or i.grad is None else i.grad.detach().clone() for i in ins]
    return grads, {k: v.detach() for k, v in out.items() if isinstance(v, torch.Tensor)}, mpi


def _equal(a, b, label):   # check (a)
    for x, y in zip(a, b):
        assert (x is None) == (y is None), label
        assert x is None or torch.equal(x, y), label


def _close(a, b, label):   # check (b): 1e-5 max|g| per tensor
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), label
        if x is not None:
            scale = float(y.abs().max())
            err = float((x - y).abs().max())
            print(f"{label} tensor {i}: max|g| {scale:.3e} max diff {err:.3e} ({err / max(scale, 1e-30):.2e} rel)")
            assert bool(torch.isfinite(x).all()) and err <= 1e-5 * scale, (label, i, err, scale)


def _autograd(case, grads, label):   # check (c)
    ref64, ref32 = _reference(case)
    got = [None if g is None else g.double().cpu().numpy() for g in grads]
    DA._compare_capped(got, ref64, ref32, case.dtype, label, True, case.with_bg)


# ---- 1. parity and reproducibility ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg", SHAPES, ids=lambda c: f"{c['H']}x{c['W']}-{c['Ht']}x{c['Wt']}")
def test_gather_is_bit_reproducible_and_matches_the_atomic_backward_and_autograd(cfg, kind, with_bg):
    """Upstream gradients on colour, depth and T; M = 2, D = 5, depth-alpha with n_z_bins = 4; checks (a), (b), (c)."""
    case = _case(kind, with_bg, **cfg)
    first, out_g, mpi = _run(case, "gather")
    again, _, _ = _run(case, "gather")
    atomic, out_a, _ = _run(case)
    assert mpi.layout_gather_fallbacks == 0
    for g, p in zip(first, case.parts):
        assert (g is None) == (p is None) and (g is None or (g.shape == p.shape and g.dtype == p.dtype))
    _equal(first, again, "two gather runs")
    for k in ("color", "depth", "T"):
        assert torch.equal(out_g[k], out_a[k]), k   # (the forward does not depend on the name)
    _close(first, atomic, f"{kind} gather vs atomic")
    _autograd(case, first, f"{kind} gather")


# ---- 2. every run count -------------------------------------------------------------------------------------------------------------------------
def _actual_runs(case, runs):
    """The plane runs the library uses for this case when `runs` is forced (None: its rule), asked through the C ABI."""
    return _abi(case, launch=False, runs=runs)[2]["runs"]


@pytest.mark.parametrize("kind", KINDS)
def test_every_run_count_gives_the_same_gradients(kind):
    """D = 5 at test size: the rule picks one plane per run (five runs); forcing 1, 2, 3 gives every other count ceil(5 / ceil(5 / R)) the rule
    can pick (1, 2, 3; 4 is 3).  Each under check (c), each pair under check (b); the count is read back from the library."""
    case = _case(kind, True, **SHAPES[1])
    assert _actual_runs(case, None) == 5
    res = {}
    for runs in (1, 2, 3, 5):
        assert _actual_runs(case, runs) == runs
        res[runs], _, _ = _run(case, "gather", runs=runs)
        _autograd(case, res[runs], f"{kind} runs={runs}")
    by_rule, _, _ = _run(case, "gather")
    _equal(by_rule, res[5], "the rule's count, forced")
    for a, b in itertools.combinations(res, 2):
        _close(res[a], res[b], f"{kind} runs {a} vs {b}")


EXTRA = {
    "one_plane": dict(SMALL, D=1, nzb=1),                                   # D = 1 with a background: the only plane is the background's; rgb gets zeros
    "130_planes": dict(SMALL, H=48, W=72, D=130, alpha_scale=0.02, reach=1.35),   # more than one plane chunk of the volume pair; the tile kernels' table holds 128
    "ragged": dict(SMALL, vpm=2),                                           # Wt, Ht no multiples of the texel tile; two views per MPI
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(EXTRA))
def test_plane_counts_and_ragged_textures(name, kind):
    """With a background.  Check (c) for the rule's run count and, against it, another count under check (b).  130 planes: the alphas are thinned to
    0.02 (shared-colour) and the depth surface reaches 1.35 (holes: depth-alpha), so that the last plane keeps a gradient worth comparing."""
    case = _case(kind, True, **EXTRA[name])
    by_rule, _, mpi = _run(case, "gather")
    assert mpi.layout_gather_fallbacks == 0
    _autograd(case, by_rule, f"{kind} {name}")
    other = 1 if case.D > 1 else None
    if other is not None:
        assert _actual_runs(case, None) == case.D and _actual_runs(case, other) == 1
        one, _, _ = _run(case, "gather", runs=other)
        _close(one, by_rule, f"{kind} {name} one run vs {case.D}")
    atomic, _, _ = _run(case)
    _close(by_rule, atomic, f"{kind} {name} vs atomic")
    if name == "one_plane" and kind == "shared":
        assert int(torch.count_nonzero(by_rule[0])) == 0 and int(torch.count_nonzero(by_rule[2])) > 0


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------------
def _abi(case, *, launch=True, overwrite=True, bufs=None, needs=(True, True, True), ws_fill=None, ws="ok", tweak=None, runs=None, null_upstream=False):
    """The layout's gather entry through the C ABI, on the structs of a forward of `case` (its private transmittance buffer included).
    bufs: the three gradient views to write into (None: fresh, NaN-filled); ws: "ok", "small", "misaligned" or "none"; ws_fill: a byte the
    workspace is filled with first; tweak(p): changes to the parameter struct before the query.  Returns (code, views, info)."""
    from ml_gmpi_amd import MPI, _lib
    from ml_gmpi_amd.hip_mpi import _depth_alpha, _shared_color
    dev = torch.device(DEV)
    lib = _lib.load_library()
    t = lambda a: None if a is None else torch.as_tensor(a).to(dev)
    rgb, mid, bg = (t(p) for p in case.parts)
    geo = (t(case.dhw), t(case.ray), t(case.eye), t(case.zd))
    mpi = MPI(on_out_of_plane="raise")
    kw = dict(background=bg, views_per_mpi=case.vpm, check_last_plane=False, want_transmittance=True, _in_autograd_fn=True)
    with torch.no_grad():
        if case.kind == "shared":
            res = mpi.render_views_shared(rgb, mid, *geo, **kw)
        else:
            plane_z = t(case.plane_z)
            res = mpi.render_views_depth(rgb, mid, plane_z, case.zb, *geo, **kw)
    bwd = res.pop("_bwd")
    p = _lib.GmpiRenderParams.from_buffer_copy(bwd[0])
    p.rgb_out = p.depth_out = p.status = None
    p.variant, p.workspace, p.workspace_bytes = _lib.VARIANT_AUTO, None, 0
    rgb_k, bg_k = bwd[2]
    sc = _shared_color(rgb_k, bg_k)
    da = None if case.kind == "shared" else _depth_alpha(plane_z, *case.zb)
    structs = (ctypes.byref(sc),) + (() if da is None else (ctypes.byref(da),))
    if tweak is not None:
        tweak(p)
    if overwrite:
        p.flags |= _lib.FLAG_GRAD_OVERWRITE
    if runs is not None:
        lib.gmpi_render_layout_backward_gather_set_runs(runs)
    try:
        need = int(lib.gmpi_render_layout_backward_gather_workspace_bytes(ctypes.byref(p), ctypes.byref(sc), None if da is None else ctypes.byref(da)))
        info = dict(need=need, runs=int(lib.gmpi_render_layout_backward_gather_runs(ctypes.byref(p), ctypes.byref(sc), None if da is None else ctypes.byref(da))))
        if not launch:
            return 0, None, info
        pixels = case.N * case.D * case.H * case.W * 24
        size = need if need else pixels + 4096
        space = torch.empty(size + 256, dtype=torch.uint8, device=dev)
        if ws_fill is not None:
            space.fill_(ws_fill)
        assert space.data_ptr() % 256 == 0
        if ws == "ok":
            p.workspace, p.workspace_bytes = space.data_ptr(), size
        elif ws == "small":
            p.workspace, p.workspace_bytes = space.data_ptr(), size - 1
        elif ws == "misaligned":
            p.workspace, p.workspace_bytes = space.data_ptr() + 128, size
        shapes = [(case.M, 3, case.Ht, case.Wt), (case.M, case.D, 1, case.Ht, case.Wt) if case.kind == "shared" else (case.M, 1, case.Ht, case.Wt),
                  (case.M, 3, case.Ht, case.Wt)]
        if bufs is None:
            bufs = [torch.full(sh, float("nan"), device=dev) if n and (i < 2 or bg is not None) else None for i, (sh, n) in enumerate(zip(shapes, needs))]
        dims = [(0, 1, 2), (0, 1, 3) if case.kind == "shared" else (0, 1, 2), (0, 1, 2)]
        args = []
        for v, d in zip(bufs, dims):
            args += [None, None] if v is None else [v.data_ptr(), (ctypes.c_int64 * 3)(*[v.stride(i) for i in d])]
        up = [t(case.gc), t(case.gd), t(case.gT)]
        entry = lib.gmpi_mpi_render_shared_backward_gather_launch if case.kind == "shared" else lib.gmpi_mpi_render_depth_backward_gather_launch
        rc = entry(ctypes.byref(p), *structs, None if null_upstream else up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), *args,
                   torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
    finally:
        if runs is not None:
            lib.gmpi_render_layout_backward_gather_set_runs(0)
    return rc, bufs, info


# ---- 3. step-like ramp: most planes are skipped in the pixel pass --------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bg", [False, True])
def test_step_like_ramp_writes_zero_records_for_the_planes_it_skips(with_bg):
    """n_z_bins = 256, D = 32, 96^2: a texel lies on the ramp of at most one plane, in front of the surface every plane is skipped.  The workspace is
    filled with NaN bytes first: a record the pixel pass left out would reach the gradients.  They must be finite and pass check (c)."""
    case = _case("depth", with_bg, H=96, W=96, Ht=96, Wt=96, yaw=0.25, pitch=0.1, roll=0.2, vpm=2, M=1, D=32, nzb=256)
    rc, grads, info = _abi(case, ws_fill=0xFF)
    assert rc == 0 and info["need"] > 0
    for g in grads:
        assert g is None or bool(torch.isfinite(g).all())
    assert float(grads[1].abs().max()) > 0
    _autograd(case, grads, "steps")
    rc, shared_grads, _ = _abi(_case("shared", with_bg, **SMALL), ws_fill=0xFF)   # (the shared-colour pixel pass skips nothing: the same guard)
    assert rc == 0 and all(g is None or bool(torch.isfinite(g).all()) for g in shared_grads)


# ---- 4. written once, padding untouched ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("runs", [None, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_every_cell_is_written_once_and_the_padding_is_never_touched(kind, runs):
    """Gradient tensors whose MPI, channel / plane and row strides exceed the tensor.  With GMPI_FLAG_GRAD_OVERWRITE into NaN: no NaN inside [Ht, Wt],
    NaN everywhere else.  Without it into 1.0: 1 + g bit for bit (read, add, write back by the cell's one owner), the padding still 1.0."""
    case = _case(kind, True, **SMALL)
    dev = torch.device(DEV)
    M, D, Ht, Wt = case.M, case.D, case.Ht, case.Wt

    def padded(fill):
        full = [torch.full((M + 1, 4, Ht + 3, Wt + 5), fill, device=dev),
                torch.full((M + 1, D + 1, 1, Ht + 3, Wt + 5), fill, device=dev) if kind == "shared" else torch.full((M + 1, 2, Ht + 3, Wt + 5), fill, device=dev),
                torch.full((M + 1, 4, Ht + 3, Wt + 5), fill, device=dev)]
        views = [full[0][:M, :3, :Ht, :Wt], full[1][:M, :D, :, :Ht, :Wt] if kind == "shared" else full[1][:M, :1, :Ht, :Wt], full[2][:M, :3, :Ht, :Wt]]
        return full, views

    full, views = padded(float("nan"))
    rc, _, info = _abi(case, bufs=views, runs=runs)
    assert rc == 0 and info["runs"] == (1 if runs else case.D)
    g = []
    for f, v in zip(full, views):
        assert not bool(torch.isnan(v).any())
        assert int(torch.isnan(f).sum()) == f.numel() - v.numel()
        g.append(v.clone())
    dense = _abi(case, runs=runs)[1]
    _equal(g, dense, "strided vs dense gradient tensors")
    full, views = padded(1.0)
    rc, _, _ = _abi(case, bufs=views, overwrite=False, runs=runs)
    assert rc == 0
    for f, v, gi in zip(full, views, g):
        assert torch.equal(v, 1.0 + gi)
        assert int((f != 1.0).sum()) == int((v != 1.0).sum())


# ---- 5. partial outputs -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_each_subset_of_outputs_gives_the_full_runs_bits(kind):
    case = _case(kind, True, **dict(SMALL, vpm=2))
    full, _, _ = _run(case, "gather")
    for needs in itertools.product([True, False], repeat=3):
        if not any(needs) or all(needs):
            continue
        got, _, mpi = _run(case, "gather", needs=needs)
        assert mpi.layout_gather_fallbacks == 0
        for g, f, n in zip(got, full, needs):
            assert (g is None) == (not n)
            assert g is None or torch.equal(g, f), needs


# ---- 6. non-finite containment --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("runs", [None, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_an_infinite_upstream_gradient_stays_inside_its_pixels_footprints(kind, runs):
    """One pixel's upstream colour gradient is inf.  Its records are inf / NaN on every plane; a term is added only where its bilinear weight is not
    zero, so every gradient cell farther than 2 texels from all of that pixel's sample positions (the CPU oracle's coordinate chain) is finite and
    bit-identical to the run without the poison -- and the poison does arrive somewhere."""
    case = _case(kind, True, **SMALL)
    n0, py, px = 1, 29, 41
    gc = case.gc.copy()
    gc[n0, :, py, px] = np.inf
    clean, _, _ = _run(case, "gather", runs=runs)
    dirty, _, _ = _run(case, "gather", runs=runs, gc=gc)
    ix, iy = oracle.coords(case.dhw, case.ray, case.eye, case.Ht, case.Wt, view_to_mpi=np.asarray(case.v2m, dtype=np.int32))
    xs, ys = np.arange(case.Wt)[None, :], np.arange(case.Ht)[:, None]
    far = np.ones((case.M, case.Ht, case.Wt), dtype=bool)
    m0 = case.v2m[n0]
    for k in range(case.D):
        far[m0] &= (np.abs(xs - ix[n0, k, py, px]) > 2) | (np.abs(ys - iy[n0, k, py, px]) > 2)
    assert 0 < int((~far[m0]).sum()) < 200 and bool(far[1 - m0].all())
    far_t = torch.from_numpy(far).to(DEV)
    reached = 0
    for c, d in zip(clean, dirty):
        mask = far_t.reshape(case.M, *([1] * (c.ndim - 3)), case.Ht, case.Wt).expand_as(c)
        assert bool(torch.isfinite(d[mask]).all())
        assert torch.equal(d[mask], c[mask])
        reached += int((~torch.isfinite(d)).sum())
    assert reached > 0


# ---- 7. 16-bit storage ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16_bit_inputs_get_their_gradients_in_their_own_dtype(dtype, kind):
    """The kernels upcast the stored values (exact) and compute in fp32: the gradients are those of the fp32 run on the same values, rounded once to
    the inputs' dtype -- within half an ulp of that format (test_hip_shared_color._half_ulp; fp16: at least half its smallest subnormal step, 2^-25)."""
    case16 = _case(kind, True, dtype=dtype, **SMALL)
    case32 = Case(**dict(case16.__dict__, parts=tuple(None if p is None else p.float() for p in case16.parts), dtype=torch.float32))
    g16, _, mpi = _run(case16, "gather")
    g32, _, _ = _run(case32, "gather")
    assert mpi.layout_gather_fallbacks == 0
    floor = 2.0 ** -25 if dtype is torch.float16 else 0.0
    for a, b, p in zip(g16, g32, case16.parts):
        assert a.dtype == dtype and a.shape == p.shape and b.dtype == torch.float32
        a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
        assert np.isfinite(a).all() and np.abs(b).max() > 0
        bound = np.maximum(SC._half_ulp(np.maximum(np.abs(a), np.abs(b)), dtype), floor)
        assert (np.abs(a - b) <= bound).all(), float((np.abs(a - b) - bound).max())


# ---- 8. fallbacks -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_launches_the_pair_cannot_take_fall_back_to_the_atomic_path(kind, monkeypatch):
    """align_corners=False and a ragged view_to_mpi with "gather": the atomic path's gradients (check (b)), counted in MPI.layout_gather_fallbacks,
    one RuntimeWarning for all of them."""
    from ml_gmpi_amd import hip_mpi
    monkeypatch.setattr(hip_mpi, "_GATHER_FALLBACK_WARNED", False)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for case, kw in ((_case(kind, True, **SMALL), dict(ac=False)), (_case(kind, True, **dict(SMALL, n_views=3)), dict(view_to_mpi=[0, 1, 1]))):
            got, _, mpi = _run(case, "gather", **kw)
            assert mpi.layout_gather_fallbacks == 1, kw
            want, _, mpi0 = _run(case, **kw)
            assert mpi0.layout_gather_fallbacks == 0
            _close(got, want, f"{kind} fallback {kw}")
    hits = [w for w in seen if issubclass(w.category, RuntimeWarning) and "layout_gather_fallbacks" in str(w.message)]
    assert len(hits) == 1, [str(w.message) for w in seen]


# ---- 9. refusals of the C entries -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_entries_refuse_what_they_cannot_run_and_never_fall_back(kind):
    from ml_gmpi_amd import _lib as L
    case = _case(kind, True, **SMALL)
    rc, grads, info = _abi(case)
    assert rc == 0 and info["need"] > 0 and info["need"] % 256 == 0
    untouched = lambda bufs: all(b is None or bool(torch.isnan(b).all()) for b in bufs)
    for ws in ("small", "misaligned", "none"):
        rc, bufs, _ = _abi(case, ws=ws)
        assert rc == -8 and untouched(bufs), ws                                   # GMPI_E_WORKSPACE
    for variant in (L.VARIANT_GATHER, L.VARIANT_LDS, L.VARIANT_BAND):
        rc, bufs, info = _abi(case, tweak=lambda p: setattr(p, "variant", variant))
        assert rc == -6 and info["need"] == 0 and untouched(bufs), variant        # GMPI_E_VARIANT
    rc, bufs, info = _abi(case, tweak=lambda p: setattr(p, "rgba_dtype", L.DTYPE_U8))
    assert rc == -3 and info["need"] == 0 and untouched(bufs)                     # GMPI_E_DTYPE
    rc, bufs, _ = _abi(case, null_upstream=True)
    assert rc == -1 and untouched(bufs)                                           # GMPI_E_NULL
    rc, bufs, _ = _abi(case, needs=(False, False, False))
    assert rc == -1                                                               # all three NULL
    # support reasons: the query is 0 exactly where the launch is GMPI_E_VARIANT
    v2m = torch.zeros(case.N, dtype=torch.int32, device=DEV)
    for tweak in (lambda p: setattr(p, "flags", p.flags & ~L.FLAG_ALIGN_CORNERS), lambda p: setattr(p, "view_to_mpi", v2m.data_ptr())):
        rc, bufs, info = _abi(case, tweak=tweak)
        assert rc == -6 and info["need"] == 0 and info["runs"] == 0 and untouched(bufs)


# ---- 10. through MPIRenderer ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_renderer_passes_the_name_through_and_the_forward_is_untouched(kind):
    """render_shared(..., shared_backward="gather") / render_depth(..., depth_backward="gather"): the default call's outputs bit for bit, its
    gradients within check (b); twice the same bits."""
    from ml_gmpi_amd import make_renderer
    dev = torch.device(DEV)
    S, D, B = 96, 8, 2
    rgba, _, _, _, _ = SC._random_case(seed=12, B=B, D=D, S=S)
    rgb, alpha, bg = (t.to(dev) for t in SC._parts(rgba))
    depth = DA._depth_image(B, S, D, 4)[0].to(dev)
    res = {}
    for how in ("default", "gather", "gather again"):
        r = make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise")
        ins = [t.clone().requires_grad_(True) for t in ((rgb, alpha, bg) if kind == "shared" else (rgb, depth, bg))]
        kw = {} if how == "default" else {ARG[kind]: "gather"}
        torch.manual_seed(21)
        if kind == "shared":
            out = r.render_shared(ins[0], ins[1], S, S, background_rgb=ins[2], want_transmittance=True, **kw)
        else:
            out = r.render_depth(ins[0], ins[1], S, S, z_range=2, n_z_bins=4, background_rgb=ins[2], want_transmittance=True, **kw)
        g = torch.Generator(device="cpu").manual_seed(3)
        loss = sum((o * torch.randn(o.shape, generator=g).to(dev)).sum() for o in (out[0], out[1], out[4]))
        loss.backward()
        torch.cuda.synchronize()
        assert r.mpi.layout_gather_fallbacks == 0
        res[how] = ([o.detach() for o in (out[0], out[1], out[4])], [i.grad.clone() for i in ins])
    for a, b in zip(res["default"][0], res["gather"][0]):
        assert torch.equal(a, b)
    _equal(res["gather"][1], res["gather again"][1], "two gather runs through the renderer")
    _close(res["gather"][1], res["default"][1], f"{kind} renderer gather vs default")
