"""Inputs and the reference chain of the compute_depth_ramp tests (tests/test_light_depth_alpha_cpu.py, tests/test_hip_light_depth_alpha.py)."""
import functools

import torch

from test_hip_depth_alpha import _bounds, _knife_edges

B, D, H, W = 2, 12, 5, 300   # a ragged last block of 256 lanes and a second x-block


def plane_tables(D=D):
    """(plane_z, plane_ds): the normalised depths the ramp is taken of, and the metric distances that are composited -- two different tables."""
    return torch.linspace(0, 1, D), torch.linspace(0.95, 1.12, D)


@functools.lru_cache(maxsize=None)
def depth_image(n_z_bins, dtype=torch.float32, reach=None, B=B, H=H, W=W, D=D, seed=5):
    """depth = 0.25 + 0.25 (y + x) + 0.02 U with y, x in [0, 1] ([B,1,H,W]; `reach`: scaled so that its maximum is `reach` -- holes behind the last
    plane's ramp), then the knife-edge rule of tests/test_hip_depth_alpha.py::_depth_image: texels within 1e-4 of a ramp bound move by + 3.3e-4 until
    none is left; 16-bit storage: the stored values keep 1e-6.  Cached: shared by the tests, never written to."""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.linspace(0, 1, H).view(1, 1, H, 1), torch.linspace(0, 1, W).view(1, 1, 1, W)
    depth = 0.25 + 0.25 * (y + x) + 0.02 * torch.rand((B, 1, H, W), generator=g)
    if reach is not None:
        depth = depth * (reach / float(depth.max()))
    plane_z = plane_tables(D)[0]
    lo, hi = _bounds(n_z_bins)
    for _ in range(8):
        edge = _knife_edges(depth, plane_z, lo, hi, 1e-4)
        if not bool(edge.any()):
            break
        depth = depth + 3.3e-4 * edge
    assert not bool(_knife_edges(depth, plane_z, lo, hi, 1e-4).any())
    if dtype is not torch.float32:
        depth = depth.to(dtype)
        for _ in range(8):
            edge = _knife_edges(depth, plane_z, lo, hi, 1e-6)
            if not bool(edge.any()):
                break
            depth = torch.where(edge, (depth.float() * (1 + 2.0 ** -7)).to(dtype), depth)
        assert not bool(_knife_edges(depth, plane_z, lo, hi, 1e-6).any())
    return depth


def ramp_chain(depth, plane_z, lo, hi, plane_ds, dtype=torch.float64):
    """The definition as one torch chain in `dtype`, differentiable w.r.t. depth: the ramp on the stored values with the fp32-rounded constants,
    then LightRenderer.compute_depth's cumprod composite -> (depth [B,1,H,W], T [B,1,H,W])."""
    from ml_gmpi_amd.depth_alpha import ramp_constants
    lo32, hi32, den32 = ramp_constants(lo, hi)
    pz = plane_z.to(dtype).reshape((-1 if plane_z.ndim == 2 else 1, plane_z.shape[-1], 1, 1, 1))
    t = torch.clamp(pz - depth.to(dtype).unsqueeze(1), lo32, hi32)
    a = (t - lo32) / den32
    cp = torch.cumprod(torch.cat([torch.ones_like(a[:, :1]), 1 - a + 1e-10], 1), dim=1)
    z = torch.sum(a * cp[:, :-1] * plane_ds.to(dtype).reshape(1, -1, 1, 1, 1), dim=1)
    return z, cp[:, -1]


def oracle_reference(depth, plane_z, lo, hi, plane_ds):
    """(depth, T) numpy float32: oracle.alpha_depth on depth_alpha_planes computed on the CPU from the stored values."""
    import oracle
    from ml_gmpi_amd import depth_alpha_planes
    return oracle.alpha_depth(depth_alpha_planes(depth.cpu(), plane_z.cpu(), lo, hi).numpy(), plane_ds.numpy())
