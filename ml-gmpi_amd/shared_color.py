"""The shared-colour layout of a multiplane image: ONE colour image per MPI, D alpha planes and, optionally, a separate colour image for
the last plane -- what GMPI's generator holds before it expands and concatenates (networks_cond_on_pos_enc.py:950-975 with
`torgba_sep_background: True`, gmpi.yml:137-145).  `expand_shared_color` is the executable definition of what the shared-colour render
(`MPI.render_views_shared`, `gmpi_mpi_render_shared_launch`) computes: the render of the volume it returns.  Plain torch, any device."""
from typing import Optional, Tuple

import torch


def _check(rgb: torch.Tensor, alpha: torch.Tensor, background: Optional[torch.Tensor]) -> None:
    assert alpha.ndim == 5 and alpha.shape[2] == 1, f"Expected alpha of shape (#mpi, #planes, 1, h, w), got {tuple(alpha.shape)}"
    M, D, _, Ht, Wt = alpha.shape
    assert tuple(rgb.shape) == (M, 3, Ht, Wt), f"Expected rgb of shape {(M, 3, Ht, Wt)}, got {tuple(rgb.shape)}"
    if background is not None:
        assert tuple(background.shape) == (M, 3, Ht, Wt), f"Expected background of shape {(M, 3, Ht, Wt)}, got {tuple(background.shape)}"


def expand_shared_color(rgb: torch.Tensor, alpha: torch.Tensor, background: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rgb [M,3,Ht,Wt], alpha [M,D,1,Ht,Wt], background [M,3,Ht,Wt] or None -> rgba [M,D,4,Ht,Wt]:
    rgba[m,k,:3] = rgb[m] (k = D-1: background[m] when one is given), rgba[m,k,3] = alpha[m,k,0].  Differentiable; the generator's own
    expand + two cats."""
    _check(rgb, alpha, background)
    D = alpha.shape[1]
    if background is None:
        colour = rgb.unsqueeze(1).expand(-1, D, -1, -1, -1)
    else:
        colour = torch.cat((rgb.unsqueeze(1).expand(-1, D - 1, -1, -1, -1), background.unsqueeze(1)), 1)
    return torch.cat((colour, alpha), 2)


def split_shared_color(rgba: torch.Tensor, background: bool = False) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """rgba [M,D,4,Ht,Wt] whose colour planes are all equal (with background=True: all but the last) -> (rgb, alpha, background or None).
    `alpha` is the view rgba[:, :, 3:] (no copy: the shared-colour render takes it as it is), rgb and background are views of planes 0 and
    D-1.  Raises ValueError when the colour planes differ (the volume is not a shared-colour MPI).  With background=True and D == 1 the one
    plane is the background and rgb is that plane as well (it colours no plane)."""
    assert rgba.ndim == 5 and rgba.shape[2] == 4, f"Expected rgba of shape (#mpi, #planes, 4, h, w), got {tuple(rgba.shape)}"
    D = rgba.shape[1]
    n_shared = D - 1 if background else D
    rgb = rgba[:, 0, :3]
    if n_shared > 1 and not bool((rgba[:, 1:n_shared, :3] == rgb.unsqueeze(1)).all()):
        raise ValueError("split_shared_color: the colour planes of this volume are not all equal")
    return rgb, rgba[:, :, 3:], (rgba[:, D - 1, :3] if background else None)
