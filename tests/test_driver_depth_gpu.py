"""GPU tests of the batch driver's depth-alpha methods: `render_path_depth` / `render_seeds_depth` against `render_path` / `render_seeds` on
`expand_depth_alpha(...)`, for both forwards.  Strict-order mode: both sides are bit-identical to the oracle, hence to each other."""
import numpy as np
import pytest
import torch

from test_hip_parity import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, D = 64, 8
KEYS = ("rgb", "depth", "T")
Z = dict(z_range=1, n_z_bins=4)
YAWS, PITCHES = np.linspace(0.4, -0.4, 5), np.linspace(-0.1, 0.1, 5)   # 5 poses, batch 2: the last batch is ragged


def _renderer(strict=True, **kw):
    from ml_gmpi_amd import make_renderer
    return make_renderer("FFHQ", n_planes=D, device=torch.device(DEV), on_out_of_plane="raise", strict_order=strict, **kw)


def _images(M, seed=0):
    """rgb, depth (a smooth surface between the planes' normalised depths, plus noise), background."""
    g = torch.Generator().manual_seed(seed)
    dev = torch.device(DEV)
    c = torch.rand((M, 1, 5, 5), generator=g)
    depth = 0.15 + 0.7 * torch.nn.functional.interpolate(c, size=(S, S), mode="bilinear", align_corners=True) + 0.02 * (torch.rand((M, 1, S, S), generator=g) - 0.5)
    return torch.rand((M, 3, S, S), generator=g).to(dev), depth.to(dev), torch.rand((M, 3, S, S), generator=g).to(dev)


def _volume(r, rgb, depth, bg):
    from ml_gmpi_amd import depth_alpha_bounds, expand_depth_alpha
    plane_z = r.get_xyz_single_res(S, S, only_z=True)[1].reshape(-1).to(rgb.device)
    return expand_depth_alpha(rgb, depth, plane_z, *depth_alpha_bounds(Z["z_range"], Z["n_z_bins"]), bg)


@pytest.fixture
def launched(monkeypatch):
    """The depth-alpha forward entries that are launched."""
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    seen = []
    for name, tag in (("gmpi_mpi_render_depth_window_launch", "window"), ("gmpi_mpi_render_depth_launch", "pixel")):
        def spy(p, sc, da, stream, real=getattr(lib, name), tag=tag):
            seen.append(tag)
            return real(p, sc, da, stream)
        monkeypatch.setattr(lib, name, spy)
    return seen


@pytest.mark.parametrize("how", ["pixel", "window"])
@pytest.mark.parametrize("with_bg", [False, True])
def test_render_path_depth_equals_render_path_on_the_expanded_volume(launched, with_bg, how):
    from ml_gmpi_amd import ViewBatchDriver
    rgb, depth, bg = _images(1)
    bg = bg if with_bg else None
    r = _renderer()
    vol = _volume(r, rgb, depth, bg)
    drv = ViewBatchDriver(r, batch=2)
    ref = drv.render_path(vol, S, YAWS, PITCHES, to_uint8=True, want_transmittance=True)
    out = drv.render_path_depth(rgb, depth, S, YAWS, PITCHES, background=bg, to_uint8=True, want_transmittance=True, depth_forward=how, **Z)
    assert launched == [how] * 3, launched   # three batches, all on the kernel asked for
    assert set(out) == set(ref)
    for k in KEYS:
        assert out[k].shape == ref[k].shape and torch.equal(out[k], ref[k]), k
    for k in ("img8", "dep8"):   # the same frames up to one code
        assert out[k].shape == ref[k].shape and int((out[k].int() - ref[k].int()).abs().max()) <= 1, k
    host_ref = {k: ref[k].cpu() for k in ("img8", "dep8")}
    piped = drv.render_path_depth(rgb, depth, S, YAWS, PITCHES, background=bg, to_uint8=True, to_host=True, depth_forward=how, **Z)
    assert piped["img8_host"].is_pinned() and piped["T"] is None and torch.equal(piped["rgb"], ref["rgb"])
    for k in ("img8", "dep8"):
        assert int((piped[k + "_host"].int() - host_ref[k].int()).abs().max()) <= 1, k
    sub = drv.render_path_depth(rgb, depth, S, YAWS, PITCHES, background=bg, indices=[4, 1], want_transmittance=True, depth_forward=how, **Z)
    for k in KEYS:
        assert torch.equal(sub[k], ref[k][[4, 1]]), k
    # default mode: within the parity bars of the strict frames
    fast = ViewBatchDriver(_renderer(strict=False), batch=2).render_path_depth(rgb, depth, S, YAWS, PITCHES, background=bg, want_transmittance=True,
                                                                                depth_forward=how, **Z)
    for k in KEYS:
        assert float((fast[k] - ref[k]).abs().max()) <= TOL, k


@pytest.mark.parametrize("how", ["pixel", "window"])
def test_render_seeds_depth_equals_render_seeds_and_consumes_the_same_rng(launched, how):
    from ml_gmpi_amd import ViewBatchDriver
    rgb, depth, bg = _images(3, seed=1)
    res, states = [], []
    for layout in ("volume", "depth"):
        r = _renderer()
        drv = ViewBatchDriver(r, batch=2)
        vol = _volume(r, rgb, depth, bg)
        torch.manual_seed(17)
        if layout == "depth":
            res.append(drv.render_seeds_depth(rgb, depth, S, background=bg, views_per_mpi=2, want_transmittance=True, depth_forward=how, **Z))
        else:
            res.append(drv.render_seeds(vol, S, views_per_mpi=2, want_transmittance=True))
        torch.cuda.synchronize()
        states.append(torch.get_rng_state())
    assert launched == [how] * 2, launched   # 2 + 1 MPIs
    assert torch.equal(states[0], states[1])
    a, b = res
    assert len(a) == len(b) == 5 and b[0].shape == (6, 3, S, S)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])   # c2w, angles
    for i in (0, 1, 4):
        assert float((a[i] - b[i]).abs().max()) <= TOL, i
        assert torch.equal(a[i], b[i]), i   # (strict order: the same bits)


def test_the_default_is_the_documented_one(launched):
    from ml_gmpi_amd import ViewBatchDriver, driver
    rgb, depth, bg = _images(1)
    ViewBatchDriver(_renderer(), batch=8).render_path_depth(rgb, depth, S, YAWS, PITCHES, background=bg, **Z)
    assert launched == [driver.DEPTH_FORWARD_DEFAULT], launched
