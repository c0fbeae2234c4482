"""GPU tests of the batch driver's shared-colour methods: `render_path_shared` / `render_seeds_shared` against `render_path` / `render_seeds` on
`expand_shared_color(rgb, alpha, background)`.  Strict-order mode: both sides are bit-identical to the oracle, hence to each other."""
import numpy as np
import pytest
import torch

from test_hip_parity import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, D = 64, 4
KEYS = ("rgb", "depth", "T")


def _renderer(strict=True, **kw):
    from ml_gmpi_amd import make_renderer
    return make_renderer("FFHQ", n_planes=D, device=torch.device(DEV), on_out_of_plane="raise", strict_order=strict, **kw)


def _mpi_parts(M, Ht=S, Wt=S, seed=0):
    g = torch.Generator().manual_seed(seed)
    dev = torch.device(DEV)
    return (torch.rand((M, 3, Ht, Wt), generator=g).to(dev), torch.rand((M, D, 1, Ht, Wt), generator=g).to(dev),
            torch.rand((M, 3, Ht, Wt), generator=g).to(dev))


@pytest.fixture
def launched(monkeypatch):
    """The variants that reach gmpi_mpi_render_shared_launch."""
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    real = lib.gmpi_mpi_render_shared_launch
    seen = []

    def spy(p, sc, stream):
        seen.append(int(p._obj.variant))
        return real(p, sc, stream)
    monkeypatch.setattr(lib, "gmpi_mpi_render_shared_launch", spy)
    return seen


YAWS, PITCHES = np.linspace(0.4, -0.4, 5), np.linspace(-0.1, 0.1, 5)   # 5 poses, batch 2: the last batch is ragged


@pytest.mark.parametrize("with_bg", [False, True])
def test_render_path_shared_equals_render_path_on_the_expanded_volume(launched, with_bg):
    from ml_gmpi_amd import ViewBatchDriver, expand_shared_color, _lib as L
    rgb, alpha, bg = _mpi_parts(1)
    bg = bg if with_bg else None
    vol = expand_shared_color(rgb, alpha, bg)
    drv = ViewBatchDriver(_renderer(), batch=2)
    ref = drv.render_path(vol, S, YAWS, PITCHES, to_uint8=True, want_transmittance=True)
    out = drv.render_path_shared(rgb, alpha, S, YAWS, PITCHES, background=bg, to_uint8=True, want_transmittance=True, variant="lds")
    assert launched == [L.VARIANT_LDS] * 3, launched   # three batches, all on the staged kernel
    assert set(out) == set(ref)
    for k in KEYS + ("img8", "dep8"):
        assert out[k].shape == ref[k].shape and torch.equal(out[k], ref[k]), k
    host_ref = {k: ref[k].cpu() for k in ("img8", "dep8")}
    piped = drv.render_path_shared(rgb, alpha, S, YAWS, PITCHES, background=bg, to_uint8=True, to_host=True, variant="lds")
    assert piped["img8_host"].is_pinned() and torch.equal(piped["img8_host"], host_ref["img8"]) and torch.equal(piped["dep8_host"], host_ref["dep8"])
    assert piped["T"] is None and torch.equal(piped["rgb"], ref["rgb"])
    sub = drv.render_path_shared(rgb, alpha, S, YAWS, PITCHES, background=bg, indices=[4, 1], to_uint8=True, to_host=True, want_transmittance=True, variant="lds")
    sub_ref = drv.render_path(vol, S, YAWS, PITCHES, indices=[4, 1], to_uint8=True, want_transmittance=True)
    for k in KEYS + ("img8", "dep8"):
        assert torch.equal(sub[k], sub_ref[k]) and torch.equal(sub[k], ref[k][[4, 1]]), k
    assert torch.equal(sub["img8_host"], host_ref["img8"][[4, 1]]) and torch.equal(sub["dep8_host"], host_ref["dep8"][[4, 1]])


@pytest.mark.parametrize("with_bg", [False, True])
def test_render_seeds_shared_equals_render_seeds_and_consumes_the_same_rng(launched, with_bg):
    from ml_gmpi_amd import ViewBatchDriver, expand_shared_color, _lib as L
    rgb, alpha, bg = _mpi_parts(3, seed=1)
    bg = bg if with_bg else None
    vol = expand_shared_color(rgb, alpha, bg)
    res, states = [], []
    for shared in (False, True):
        drv = ViewBatchDriver(_renderer(), batch=2)
        torch.manual_seed(17)
        if shared:
            res.append(drv.render_seeds_shared(rgb, alpha, S, background=bg, views_per_mpi=2, want_transmittance=True, variant="lds"))
        else:
            res.append(drv.render_seeds(vol, S, views_per_mpi=2, want_transmittance=True))
        torch.cuda.synchronize()
        states.append(torch.get_rng_state())
    assert launched == [L.VARIANT_LDS] * 2, launched   # 2 + 1 MPIs
    assert torch.equal(states[0], states[1])
    a, b = res
    assert len(a) == len(b) == 5 and a[0].shape == (6, 3, S, S)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])   # c2w, angles
    for i in (0, 1, 4):
        assert torch.equal(a[i], b[i]), i


def test_default_mode_other_variants_and_a_refused_layout(launched):
    from ml_gmpi_amd import ViewBatchDriver, expand_shared_color, _lib as L
    rgb, alpha, bg = _mpi_parts(1)
    strict = ViewBatchDriver(_renderer(), batch=2).render_path_shared(rgb, alpha, S, YAWS, PITCHES, background=bg, want_transmittance=True, variant="lds")
    drv = ViewBatchDriver(_renderer(strict=False), batch=2)
    launched.clear()
    for variant, want in (("lds", L.VARIANT_LDS), (None, L.VARIANT_AUTO), ("gather", L.VARIANT_GATHER)):
        out = drv.render_path_shared(rgb, alpha, S, YAWS, PITCHES, background=bg, want_transmittance=True, variant=variant)
        assert launched == [want] * 3, (variant, launched)
        launched.clear()
        for k in KEYS:
            assert float((out[k] - strict[k]).abs().max()) <= TOL, (variant, k)
    # seeds, default mode against strict mode under one seed
    rgb3, alpha3, bg3 = _mpi_parts(3, seed=1)
    outs = []
    for st in (True, False):
        torch.manual_seed(17)
        outs.append(ViewBatchDriver(_renderer(strict=st), batch=2).render_seeds_shared(rgb3, alpha3, S, background=bg3, views_per_mpi=2, variant="lds"))
    assert torch.equal(outs[0][2], outs[1][2])
    assert float((outs[0][0] - outs[1][0]).abs().max()) <= TOL and float((outs[0][1] - outs[1][1]).abs().max()) <= TOL
    # a texture whose rows are not 16-byte aligned (62 texels of fp32): the support query says no, the one-pixel kernel renders it
    launched.clear()
    rgb, alpha, bg = _mpi_parts(1, Ht=62, Wt=62, seed=2)
    sdrv = ViewBatchDriver(_renderer(), batch=2)
    out = sdrv.render_path_shared(rgb, alpha, S, YAWS, PITCHES, background=bg, want_transmittance=True, variant="lds")
    assert launched == [L.VARIANT_AUTO] * 3, launched
    ref = sdrv.render_path(expand_shared_color(rgb, alpha, bg), S, YAWS, PITCHES, want_transmittance=True)
    for k in KEYS:
        assert torch.equal(out[k], ref[k]), k
