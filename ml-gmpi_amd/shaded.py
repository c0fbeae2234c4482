"""The shaded render of an RGBA volume: the reference's shading augmentation (light_renderer.py:189-197) multiplies the colour of every plane
by ONE factor per texel and clips, `new_rgb = clip(rgb * shading[B,1,1,H,W], 0, 1)`, alpha passed through.  `apply_shading` is the executable
definition of what the shaded render (`MPI.render_views_shaded`, `gmpi_mpi_render_shaded_launch`) computes: the render of the volume it returns,
which the kernels never build.  Plain torch, any device."""
import torch


def _check(rgba: torch.Tensor, shading: torch.Tensor) -> None:
    if rgba.ndim != 5 or rgba.shape[2] != 4:
        raise ValueError(f"Expected rgba of shape (#mpi, #planes, 4, h, w), got {tuple(rgba.shape)}")
    M, _, _, Ht, Wt = rgba.shape
    if tuple(shading.shape) != (M, 1, Ht, Wt):
        raise ValueError(f"Expected shading of shape {(M, 1, Ht, Wt)}, got {tuple(shading.shape)}")


def apply_shading(rgba: torch.Tensor, shading: torch.Tensor) -> torch.Tensor:
    """rgba [M,D,4,Ht,Wt] (fp32, bf16 or fp16), shading [M,1,Ht,Wt] fp32 -> the shaded volume [M,D,4,Ht,Wt] fp32:
    colour = clip(rgba[:, :, :3] * shading[:, None], 0, 1), the product formed in fp32 with one rounding (what `gmpi_light_apply_launch`
    computes), alpha = rgba[:, :, 3:].  Differentiable.  One difference to the kernels: torch.clip keeps a NaN, the kernels' fminf(fmaxf(.))
    shades a NaN colour texel to 0."""
    _check(rgba, shading)
    return torch.cat((torch.clip(rgba[:, :, :3].float() * shading.float()[:, None], 0.0, 1.0), rgba[:, :, 3:].float()), 2)
