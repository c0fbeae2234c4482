"""The depth-alpha layout of a multiplane image: ONE colour image and ONE depth image per MPI and, optionally, a separate colour image for the
last plane -- what GMPI's generator emits with `torgba_cond_on_pos_enc: "depth2alpha"` (networks_vanilla_depth2alpha.py:650-663, gmpi.yml:87,131).
The alpha of a texel on plane k is a ramp of the plane's (normalised) depth minus the texel's depth:

    z_diff = clamp(tex_z[k] - depth, z_lo, z_hi);  alpha[k] = (z_diff - z_lo) / (z_hi - z_lo + 1e-8);  z_lo, z_hi = -+ z_range / n_z_bins

`expand_depth_alpha` is the executable definition of what the depth-alpha render (`MPI.render_views_depth`, `gmpi_mpi_render_depth_launch`)
computes: the render of the volume it returns.  Plain torch, any device."""
from typing import Optional, Tuple

import numpy as np
import torch


def depth_alpha_bounds(z_range: float, n_z_bins: int) -> Tuple[float, float]:
    """(z_lo, z_hi) = (-z_range / n_z_bins, +z_range / n_z_bins) as Python floats (networks_vanilla_depth2alpha.py:650-652)."""
    return -1.0 * z_range / n_z_bins, 1.0 * z_range / n_z_bins


def ramp_constants(z_lo: float, z_hi: float) -> Tuple[float, float, float]:
    """The ramp's three constants rounded to fp32 once, as Python floats: f32(z_lo), f32(z_hi), f32(z_hi - z_lo + 1e-8) with the sum formed in
    double -- what the kernels are handed (GmpiDepthAlpha) and what `expand_depth_alpha` computes with."""
    return float(np.float32(z_lo)), float(np.float32(z_hi)), float(np.float32(float(z_hi) - float(z_lo) + 1e-8))


def _check_depth(depth: torch.Tensor, plane_z: torch.Tensor) -> None:
    assert depth.ndim == 4 and depth.shape[1] == 1, f"Expected depth of shape (#mpi, 1, h, w), got {tuple(depth.shape)}"
    M = depth.shape[0]
    assert plane_z.ndim == 1 or (plane_z.ndim == 2 and plane_z.shape[0] == M), f"Expected plane_z of shape (#planes,) or ({M}, #planes), got {tuple(plane_z.shape)}"


def _check(rgb: torch.Tensor, depth: torch.Tensor, plane_z: torch.Tensor, background: Optional[torch.Tensor]) -> None:
    _check_depth(depth, plane_z)
    M, _, Ht, Wt = depth.shape
    assert tuple(rgb.shape) == (M, 3, Ht, Wt), f"Expected rgb of shape {(M, 3, Ht, Wt)}, got {tuple(rgb.shape)}"
    if background is not None:
        assert tuple(background.shape) == (M, 3, Ht, Wt), f"Expected background of shape {(M, 3, Ht, Wt)}, got {tuple(background.shape)}"


def depth_alpha_planes(depth: torch.Tensor, plane_z: torch.Tensor, z_lo: float, z_hi: float) -> torch.Tensor:
    """depth [M,1,Ht,Wt], plane_z [D] or [M,D] -> the alpha planes [M,D,1,Ht,Wt] of the layout: the ramp of plane_z[k] - depth[m] between z_lo
    and z_hi.  Computed in depth's dtype promoted to at least fp32, one rounding per step, with the constants of `ramp_constants`; bit-identical
    to the generator's expression with Python-float scalars.  Differentiable: the clamp passes the gradient where lo <= plane_z[k] - depth <= hi,
    bounds included, and d alpha / d depth = -1 / den there."""
    lo, hi, den = ramp_constants(z_lo, z_hi)
    ct = torch.promote_types(depth.dtype, torch.float32)
    pz = plane_z.to(depth.device, ct).reshape((-1 if plane_z.ndim == 2 else 1, plane_z.shape[-1], 1, 1, 1))
    t = pz - depth.to(ct).unsqueeze(1)                                     # [M,D,1,Ht,Wt]
    t = torch.clamp(t, lo, hi)
    # (the divisor as a tensor on the device: a true division everywhere -- a host scalar is multiplied in as a reciprocal by some backends)
    return (t - lo) / torch.tensor(den, dtype=ct, device=depth.device)


def expand_depth_alpha(rgb: torch.Tensor, depth: torch.Tensor, plane_z: torch.Tensor, z_lo: float, z_hi: float,
                       background: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rgb [M,3,Ht,Wt], depth [M,1,Ht,Wt], plane_z [D] or [M,D], background [M,3,Ht,Wt] or None -> rgba [M,D,4,Ht,Wt]:
    rgba[m,k,:3] = rgb[m] (k = D-1: background[m] when one is given), rgba[m,k,3] = `depth_alpha_planes(depth, plane_z, z_lo, z_hi)[m,k,0]`, in
    depth's dtype promoted to at least fp32.  Differentiable."""
    from .shared_color import expand_shared_color
    _check(rgb, depth, plane_z, background)
    alpha = depth_alpha_planes(depth, plane_z, z_lo, z_hi)
    return expand_shared_color(rgb.to(alpha.dtype), alpha, None if background is None else background.to(alpha.dtype))
