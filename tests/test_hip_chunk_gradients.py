"""The chunk twins of the volume backward (render_backward_chunk_kernel, render_backward_tile2_chunk_kernel, render_backward_tile_chunk_kernel through
MPI.render_views_chunks) on stacks in which every plane counts, compared PER PLANE.  tests/test_hip_chunks.py runs them on the committed fixtures: at
most 8 planes, one column of tiles, white-noise alpha.  Here (tests/_deep_cases.py `twin_case`) the stacks are 97 to 200 planes deep with a healthy
T_out, the frame is 20 x 150 pixels (three ragged columns and rows of 64 x 8 tiles), and the splits put a launch boundary on, next to and far from
the kernels' 96-plane table chunk, make chunks of one plane and chunks deeper than the plane pipeline of the tile kernel needs to fill.

Bars: every (MPI, plane, channel) slab of the gradient against float64, max(5e-5, 4 e_ref) of the slab's own maximum (+ half an ulp for 16-bit
storage; tests/_visible.py `slab_compare`, no slab left out; tests/test_visible_stacks_cpu.py holds e_ref <= 1e-4 and every slab >= 1e-3 of the
largest for these inputs); and against the one-shot backward of the same variant, 1e-5 of the largest gradient (bf16: 2^-7), the bars of
tests/test_hip_chunks.py between two runs of one kernel."""
import functools

import numpy as np
import pytest
import torch

import _deep_cases as C
from _visible import slab_compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VARIANTS = ("auto", "gather")   # the tile twin | the one-pixel twin
SPLITS = {
    97: [(96, 1), (1, 96), (2, 95), (95, 2), (48, 49), (32, 32, 32, 1)],
    129: [(128, 1), (64, 65), (97, 32)],
    200: [(97, 96, 7), (100, 100), (4,) * 50],
    12: [(1,) * 12, (5, 7)],
}
DEEP = ["t97-thin", "t129-surface-ac0", "t200-thin", "t97-thin-bf16"]
RUNS = [(n, s) for n in DEEP for s in SPLITS[C.TWIN_CASES[n]["D"]]]
ONE_SHOT_REL = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -7}


def _split_id(split):
    return f"{split[0]}x{len(split)}" if len(set(split)) == 1 and len(split) > 2 else "+".join(map(str, split))


def _run(name, variant, split, needs=None):
    """Forward + backward of the case's stack cut into `split` (None: the one-shot render_views) -> (out, the leaves)."""
    from ml_gmpi_amd import MPI
    case = C.twin_case(name)
    dev = torch.device(DEV)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    vol = t(case["rgba"]).to(case["dtype"])
    assert torch.equal(vol.float().cpu(), torch.from_numpy(case["rgba"]))   # the references were fed the stored values
    mpi = MPI(align_corners=case["ac"], variant=variant, on_out_of_plane="raise")
    kw = dict(views_per_mpi=case["vpm"]) if case["vpm"] else dict(view_to_mpi=t(case["v2m"]))
    geo = (t(case["dhw"]), t(case["ray"]), t(case["eye"]), t(case["zd"]))
    if split is None:
        leaves = [vol.requires_grad_(True)]
        out = mpi.render_views(vol, *geo, check_last_plane=False, want_transmittance=True, **kw)
    else:
        assert sum(split) == case["D"]
        leaves = [c.contiguous().requires_grad_(needs is None or i in needs) for i, c in enumerate(torch.split(vol, list(split), 1))]
        out = mpi.render_views_chunks(leaves, *geo, check_last_plane=False, want_transmittance=True, **kw)
    assert float(out["T"].detach().max()) > 1e-3   # the sweep starts from the T the forward wrote, not from the walk that rebuilds an underflowed one
    ((out["color"] * t(case["gc"])).sum() + (out["depth"] * t(case["gd"])).sum() + (out["T"] * t(case["gT"])).sum()).backward()
    torch.cuda.synchronize()
    return out, leaves


@functools.lru_cache(maxsize=None)
def _one_shot(name, variant):
    leaf = _run(name, variant, None)[1][0]
    return leaf.grad.double().cpu().numpy()


def _check(name, split, variants=VARIANTS):
    case = C.twin_case(name)
    ref64, ref32 = C.twin_refs(name)
    failures = {}
    for variant in variants:
        _, leaves = _run(name, variant, split)
        for leaf in leaves:
            assert leaf.grad.dtype == case["dtype"] and leaf.grad.shape == leaf.shape
        got = torch.cat([leaf.grad.double() for leaf in leaves], 1).cpu().numpy()
        res = slab_compare(got, ref64, ref32, case["dtype"], min_rel_scale=0, label=f"{name} {variant} {_split_id(split)}:")
        assert res["skipped"] == 0
        if res["failures"]:
            failures[variant] = (len(res["failures"]), res["worst"], res["where"], res["failures"][:5])
        one = _one_shot(name, variant)
        err, scale = float(np.abs(got - one).max()), float(np.abs(one).max())
        print(f"{name} {variant} {_split_id(split)}: |chunked - one-shot| {err / scale:.2e} of the largest gradient")
        if not err <= ONE_SHOT_REL[case["dtype"]] * scale:
            failures[variant, "one-shot"] = (err, scale)
    assert not failures, failures


@pytest.mark.parametrize("name,split", RUNS, ids=[f"{n}-{_split_id(s)}" for n, s in RUNS])
def test_chunked_volume_gradient_per_slab(name, split):
    """D = 97, 129 and 200 on thin and surface stacks, both align_corners modes, fp32 and bf16; launch boundaries at, next to and away from the
    96-plane table boundary of both tile kernels, which count from the LAST plane of a launch -- a chunk of 97 planes holds a table boundary one
    plane behind its front, one of 96 none --; chunks of one plane up to 128."""
    _check(name, split)


def test_one_column_texture_reaches_the_32x16_tile_chunk_kernel():
    """Wt = 1 under variant "auto": `launch_backward_t<TexT, CHUNK = true>` (render_backward.hip) takes `tiles` for every variant but GATHER, and its
    guard `v1 = p.Wt < 2 || !plane_offsets_fit_32(...)` is true -- the 64 x 8 kernel loads its taps as (x, x + 1) pairs and needs two columns -- so
    the launch goes to render_backward_tile_chunk_kernel, the CHUNK instance of the 32 x 16 tile body with 64-bit sums, which no other test
    launches (the one-shot reference run here takes the same guard to render_backward_tile_kernel).  20 x 150 pixels are five columns and two rows
    of its tiles, both ragged.  Splits: twelve launches of one plane, and (5, 7).  Variant "gather" runs the same inputs through the one-pixel twin."""
    for name in ("t12-column", "t12-column-ac0"):
        assert C.twin_case(name)["rgba"].shape[-1] == 1
        for split in SPLITS[12]:
            _check(name, split)


@pytest.mark.parametrize("name", ["t12-views-v2m", "t12-views-vpm"])
def test_chunked_gradient_with_shared_mpis(name):
    """Three views over two MPIs by index ([0, 1, 1]) and four by views_per_mpi = 2: the views of one MPI add into the same gradient planes."""
    _check(name, (5, 7))


def test_only_the_outer_chunks_require_grad():
    """(32, 32, 33) with chunks 0 and 2 requiring grad: chunk 1 runs for the hand-over of the suffix sum alone and gets no gradient; the slabs of
    the other two meet the rule."""
    name, split = "t97-thin", (32, 32, 33)
    ref64, ref32 = C.twin_refs(name)
    failures = {}
    for variant in VARIANTS:
        out, leaves = _run(name, variant, split, needs=(0, 2))
        assert leaves[1].grad is None and out["color"].requires_grad
        for i, k0 in ((0, 0), (2, 64)):
            got = leaves[i].grad.double().cpu().numpy()
            sl = slice(k0, k0 + split[i])
            res = slab_compare(got, ref64[:, sl], ref32[:, sl], min_rel_scale=0, label=f"{name} {variant} chunk {i} of {split}, chunk 1 without grad:")
            assert res["skipped"] == 0
            if res["failures"]:
                failures[variant, i] = (len(res["failures"]), res["worst"], res["where"], res["failures"][:5])
    assert not failures, failures
