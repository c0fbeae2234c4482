"""The oracle of the geometry backward (tests/_geometry_ref.py) against F.grid_sample's own gradient w.r.t. the grid, in float64: the
hand-written bilinear sample (zero-padded taps, floors given, differentiable in the fractions) and grid_sampler's unnormalize are what
torch computes, value and grid gradient, for both align_corners settings."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _geometry_ref import bilinear, geometry_render, unnormalize


@pytest.mark.parametrize("ac", [True, False])
def test_oracle_sampling_matches_grid_sample_and_its_grid_gradient(ac):
    g = torch.Generator().manual_seed(7 + ac)
    P, C, Ht, Wt, H, W = 3, 4, 9, 13, 11, 17
    vol = torch.rand((P, C, Ht, Wt), generator=g, dtype=torch.float64)
    grid = torch.rand((P, H, W, 2), generator=g, dtype=torch.float64) * 2.4 - 1.2     # some taps outside: zeros padding
    ix, iy = unnormalize(grid[..., 0], Wt, ac), unnormalize(grid[..., 1], Ht, ac)
    keep = ((ix - ix.round()).abs() >= 1e-3) & ((iy - iy.round()).abs() >= 1e-3)       # away from texel edges (the kink of the bilinear map)
    assert keep.float().mean() > 0.9
    gout = torch.randn((P, C, H, W), generator=g, dtype=torch.float64)

    g1 = grid.clone().requires_grad_(True)
    ref = F.grid_sample(vol, g1, mode="bilinear", padding_mode="zeros", align_corners=ac)
    ((ref * gout) * keep[:, None]).sum().backward()

    g2 = grid.clone().requires_grad_(True)
    ix2, iy2 = unnormalize(g2[..., 0], Wt, ac), unnormalize(g2[..., 1], Ht, ac)
    got = bilinear(vol, ix2, iy2, torch.floor(ix2.detach()).long(), torch.floor(iy2.detach()).long()).permute(0, 3, 1, 2)
    ((got * gout) * keep[:, None]).sum().backward()

    k = keep[:, None].expand_as(ref)
    assert float((got.detach() - ref.detach())[k].abs().max()) <= 1e-10
    assert float((g2.grad - g1.grad).abs().max()) <= 1e-10


def test_oracle_render_matches_the_volume_reference():
    """With the geometry held fixed the oracle is the render of tests/_torch_ref.py (grid_sample + cumprod) to float64 rounding."""
    from _torch_ref import torch_render
    from test_hip_edge_cases import _cam, _dhw
    import oracle
    N, M, D, S = 2, 2, 4, 12
    rgba = oracle.synth_rgba(3, (M, D, 4, S, S))
    ray, eye, zd = _cam(N, S, S, seed=4, tilt=0.3)
    dhw = _dhw(M, D)
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    for ac in (True, False):
        c1, d1 = geometry_render(t(rgba), t(dhw), t(ray), t(eye), t(zd), [0, 1], align_corners=ac)
        c2, d2 = torch_render(t(rgba), t(dhw), t(ray), t(eye), t(zd), [0, 1], align_corners=ac)
        assert float((c1 - c2).abs().max()) <= 1e-6 and float((d1 - d2).abs().max()) <= 1e-6
