"""The replay harness and the cases of tests/test_hip_graph_families.py: forward launch families recorded into a HIP graph once and replayed over buffers
whose content changes.

`replay` is the pattern of tests/test_hip_graph.py::test_render_launch_replays_from_a_graph, once: every input lives on the device before anything is
launched; want[i] comes from uncaptured steps on the capture stream, each followed by a synchronise; the exact step is warmed up on that stream (its
workspace exists before the recording starts); ONE step is recorded with torch.cuda.graph on that one stream -- a chain, no parallel branches --; the
replays visit the content sets in an order that returns to the first (A, B, C, B, A), each set loaded with copy_ into the recorded buffers, every output
poisoned and the status words zeroed before the replay; after every replay: status word 0, nothing of the poison left, equality with want[i] as the case states.

Content sets change the volume AND the poses; set 1 has views from the edge of the pose distribution (`_random_case(extreme=True)`).  Shapes: the
smallest of each family's own GPU test file.  Nothing here is imported by the product."""
import functools

import numpy as np
import torch

import oracle
from test_hip_parity import TOL, _random_case

KEYS = ("color", "depth", "T")
ORDER = (0, 1, 2, 1, 0)   # A, B, C, B, A
DEV = "cuda:0"


# ---- comparisons -----------------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """torch.equal on the bits of two fp32 outputs (NaNs compare by theirs)."""
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def poison(t):
    """NaN: what a replay must overwrite.  Every output of a step is a float tensor (an integer has no value that cannot be a result)."""
    assert t.is_floating_point(), t.dtype
    t.fill_(float("nan"))


def poisoned(t):
    return bool(torch.isnan(t).any())


# ---- the harness -----------------------------------------------------------------------------------------------------------------------------------
def replay(build, compare, order=ORDER, n_sets=3):
    """build(dev) -> case, called on the capture stream: an object with `load(i)` (copy_ of content set i into the recorded buffers), `step()` -> {name:
    tensor} (the launches; every tensor an output of the step) and `status` (the words the step ORs into).  compare(i, got, want, last): the case's
    equality between a replay of set i and the uncaptured step; last: the final replay.  Returns the case."""
    dev = torch.device(DEV)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    assert len(set(order)) >= 3 and order[0] == order[-1], order
    with torch.cuda.stream(side):
        case = build(dev)
        want = []
        for i in range(n_sets):   # uncaptured, on the capture stream
            with torch.no_grad():
                case.load(i)
            res = case.step()
            torch.cuda.synchronize()
            assert int(case.status[0].item()) == 0, (i, case.status.tolist())
            want.append({k: v.detach().clone() for k, v in res.items()})
            del res
        with torch.no_grad():
            case.load(order[0])
        case.step()   # the warm-up of the exact step on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            outs = case.step()
        outs = {k: v.detach() for k, v in outs.items()}
    torch.cuda.synchronize()
    for n, i in enumerate(order):
        with torch.no_grad():
            case.load(i)
            for v in outs.values():
                poison(v)
            case.status.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert int(case.status[0].item()) == 0, (n, i, case.status.tolist())
        for k, v in outs.items():
            assert not poisoned(v), (n, i, k)
        compare(i, outs, want[i], n == len(order) - 1)
    return case


# ---- content sets ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scenes(seed, B, D, S, T=None, tilted=((), None, (0,))):
    """Three (rgba fp32 [B,D,4,T,T], dhw, ray, eye, zd) on the CPU, never written to: seeds seed, seed + 1, seed + 2.  tilted[i]: the views of set i that
    come from the edge of the pose distribution (None: all of them), as `_poses` of tests/test_hip_graph.py picks them."""
    out = []
    for i, tilt in enumerate(tilted):
        rgba, dhw, ray, eye, zd = _random_case(seed=seed + i, B=B, D=D, S=S, T=T)
        if tilt is None or len(tilt):
            _, _, ray_x, eye_x, zd_x = _random_case(seed=seed + i + 100, B=B, D=D, S=S, T=T, extreme=True)
            ray, eye, zd = ray.clone(), eye.clone(), zd.clone()
            for n in (range(B) if tilt is None else tilt):
                ray[n], eye[n], zd[n] = ray_x[n], eye_x[n], zd_x[n]
        out.append((rgba, dhw.contiguous(), ray.contiguous(), eye.contiguous(), zd.contiguous()))
    return tuple(out)


def oracle_of(volume, geo, view_to_mpi=None):
    """oracle.render of an expanded fp32 volume (CPU) -> {color, depth, T} as numpy."""
    v2m = None if view_to_mpi is None else np.asarray(view_to_mpi, dtype=np.int32)
    res = oracle.render(volume.float().numpy(), *geo, view_to_mpi=v2m, threads=True)
    return {k: res[k] for k in KEYS}


def within_the_bars(got, orc):
    """The default-mode bars every family's test file states against the oracle: colour 0.5e-5 on the [0, 1] scale, depth and T 1e-5."""
    errs = {k: float(np.abs(got[k].cpu().numpy() - orc[k]).max()) for k in KEYS}
    return errs["color"] <= 0.5 * TOL and errs["depth"] <= TOL and errs["T"] <= TOL, errs


# ---- forward families ------------------------------------------------------------------------------------------------------------------------------
class Family:
    """One forward family: parts(rgba, i) -> the CPU tensors of content set i as stored; store(parts, dev) -> the recorded buffers (default: clones on the
    device); launch(mpi, bufs, geo, kw) -> the render; expand(parts) -> the fp32 volume the oracle renders; module: MPI's keyword arguments."""

    def __init__(self, shape, parts, launch, expand, module=None, store=None):
        self.shape, self.parts, self.launch, self.expand, self.module, self.store = shape, parts, launch, expand, module or {}, store


def _u8_parts(rgba, i):
    from ml_gmpi_amd import quantize_volume
    return (quantize_volume(rgba),)


def _u8_channels_last(parts, dev):
    from ml_gmpi_amd import layers_as_volume
    return (layers_as_volume(parts[0].to(dev).permute(0, 1, 3, 4, 2).contiguous()),)


def _layers_parts(dtype):
    return lambda rgba, i: (rgba.permute(0, 1, 3, 4, 2).contiguous().to(dtype),)


def _shaded_parts(rgba, i):
    from test_hip_shaded_render import make_shading
    return rgba, make_shading(500 + i, rgba)


def _shared_parts(rgba, i):
    q = lambda t: t.contiguous()
    return q(rgba[:, 0, :3]), q(rgba[:, :, 3:]), q(rgba[:, -1, :3])


def _expand_shaded(parts):
    from ml_gmpi_amd import apply_shading
    return apply_shading(*parts)


def _expand_shared(parts):
    from ml_gmpi_amd import expand_shared_color
    return expand_shared_color(*parts)


_U8 = dict(seed=601, B=2, D=8, S=64)                    # 64^2 image, D = 8, texture 64^2
_LAYERS = dict(seed=611, B=2, D=4, S=48)                # tests/test_hip_float_layers.py
_STAGED = dict(seed=621, B=2, D=8, S=96)                # tests/test_hip_shaded_render.py, test_hip_shared_forward_staged.py
FAMILIES = {
    "u8-planar": Family(_U8, _u8_parts, lambda mpi, b, geo, kw: mpi.render_views(b[0], *geo, **kw), lambda p: p[0].float() / 255),
    "u8-channels-last": Family(_U8, _u8_parts, lambda mpi, b, geo, kw: mpi.render_views(b[0], *geo, **kw), lambda p: p[0].float() / 255, store=_u8_channels_last),
    "layers-f32-auto": Family(_LAYERS, _layers_parts(torch.float32), lambda mpi, b, geo, kw: mpi.render_views_layers(b[0], *geo, variant="auto", **kw),
                              lambda p: p[0].float().permute(0, 1, 4, 2, 3)),
    "layers-f32-gather": Family(_LAYERS, _layers_parts(torch.float32), lambda mpi, b, geo, kw: mpi.render_views_layers(b[0], *geo, variant="gather", **kw),
                                lambda p: p[0].float().permute(0, 1, 4, 2, 3)),
    "layers-bf16-auto": Family(_LAYERS, _layers_parts(torch.bfloat16), lambda mpi, b, geo, kw: mpi.render_views_layers(b[0], *geo, variant="auto", **kw),
                               lambda p: p[0].float().permute(0, 1, 4, 2, 3)),
    "layers-bf16-gather": Family(_LAYERS, _layers_parts(torch.bfloat16), lambda mpi, b, geo, kw: mpi.render_views_layers(b[0], *geo, variant="gather", **kw),
                                 lambda p: p[0].float().permute(0, 1, 4, 2, 3)),
    "shaded": Family(_STAGED, _shaded_parts, lambda mpi, b, geo, kw: mpi.render_views_shaded(b[0], b[1], *geo, **kw), _expand_shaded),
    "shared-lds": Family(_STAGED, _shared_parts, lambda mpi, b, geo, kw: mpi.render_views_shared(b[0], b[1], *geo, background=b[2], variant="lds", **kw), _expand_shared),
    "shared-auto": Family(_STAGED, _shared_parts, lambda mpi, b, geo, kw: mpi.render_views_shared(b[0], b[1], *geo, background=b[2], **kw), _expand_shared),
}


class ForwardCase:
    """A forward family on the device: three content sets, the recorded buffers (set 0's clones), caller-owned outputs and status words."""

    def __init__(self, family, strict, dev):
        from ml_gmpi_amd import MPI, _lib
        self.family, self._oracle = family, {}
        self.sets = []
        for i, (rgba, *geo) in enumerate(scenes(**family.shape)):
            self.sets.append((family.parts(rgba, i), tuple(geo)))
        store = family.store or (lambda parts, d: tuple(p.to(d).clone() for p in parts))
        self.dev_sets = [(tuple(p.to(dev) for p in parts), tuple(g.to(dev) for g in geo)) for parts, geo in self.sets]
        self.bufs = store(self.sets[0][0], dev)
        self.geo = tuple(g.to(dev).clone() for g in self.sets[0][1])
        N, _, H, W = self.geo[1].shape
        self.out = dict(color=torch.empty((N, 3, H, W), device=dev), depth=torch.empty((N, 1, H, W), device=dev), T=torch.empty((N, 1, H, W), device=dev))
        self.status = torch.zeros(_lib.STATUS_WORDS, dtype=torch.int32, device=dev)
        self.mpi = MPI(align_corners=True, strict_order=strict, on_out_of_plane="raise", **dict(dict(variant="auto"), **family.module))
        self.kw = dict(views_per_mpi=1, check_last_plane=True, want_transmittance=True, status=self.status, defer_status=True, out=self.out)

    def load(self, i):
        parts, geo = self.dev_sets[i]
        for dst, src in zip(self.bufs + self.geo, parts + geo):
            dst.copy_(src)

    def step(self):
        with torch.no_grad():
            self.family.launch(self.mpi, self.bufs, self.geo, self.kw)
        return dict(self.out)

    def oracle(self, i):
        if i not in self._oracle:
            parts, geo = self.sets[i]
            self._oracle[i] = oracle_of(self.family.expand(parts), geo)
        return self._oracle[i]

