"""8-bit storage of an RGBA volume: code c in 0..255 stands for the fp32 value c / 255 (GMPI_DTYPE_U8, include/gmpi_render.h).  The forward
render reads such a volume as it is (`MPI.render_views`, `MPIRenderer.render`, the `ViewBatchDriver` methods): by definition it renders
`dequantize_volume(q)`.  Plain torch, any device.

Two memory orders hold the same codes.  Planar: `[M, D, 4, Ht, Wt]` with innermost stride 1.  Interleaved (channels-last): what image files, numpy
and PIL hold, `[M, D, Ht, Wt, 4]` layers -- one 4-byte RGBA texel after the other -- seen as `[M, D, 4, Ht, Wt]` through `layers_as_volume`: channel
stride 1, texel stride 4.  The forward render reads either in place."""
import torch


def is_interleaved(q: torch.Tensor) -> bool:
    """q is an interleaved uint8 volume: shape [M, D, 4, Ht, Wt], channel stride 1, texel stride 4, rows that do not overlap, no negative stride.
    (`hip_mpi` hands exactly these to the kernels in place, as GMPI_DTYPE_U8 with these strides: include/gmpi_render.h.)"""
    return (q.dtype is torch.uint8 and q.ndim == 5 and q.shape[2] == 4 and q.stride(2) == 1 and q.stride(4) == 4 and q.stride(3) >= 4 * q.shape[4]
            and all(s >= 0 for s in q.stride()))


def layers_as_volume(layers: torch.Tensor) -> torch.Tensor:
    """uint8 layers `[M, D, Ht, Wt, 4]` with contiguous texels (channel stride 1, texel stride 4; rows, planes and MPIs may be strided) -> the
    interleaved volume `[M, D, 4, Ht, Wt]` over the same storage: a view, nothing is copied."""
    if layers.dtype is not torch.uint8:
        raise TypeError(f"layers_as_volume takes uint8 layers, got {layers.dtype}")
    if layers.ndim != 5 or layers.shape[4] != 4:
        raise ValueError(f"layers_as_volume takes layers of shape [M, D, Ht, Wt, 4], got {tuple(layers.shape)}")
    q = layers.permute(0, 1, 4, 2, 3)
    if not is_interleaved(q):
        raise ValueError(f"layers_as_volume: texels must be 4 contiguous bytes in rows that do not overlap, got strides {tuple(layers.stride())}")
    return q


def volume_as_layers(q: torch.Tensor) -> torch.Tensor:
    """The inverse of `layers_as_volume`: an interleaved uint8 volume `[M, D, 4, Ht, Wt]` -> its layers `[M, D, Ht, Wt, 4]`, a view.  A planar
    volume has no such view: ValueError (`q.permute(0, 1, 3, 4, 2).contiguous()` copies it into one)."""
    if q.dtype is not torch.uint8:
        raise TypeError(f"volume_as_layers takes a uint8 volume, got {q.dtype}")
    if q.ndim != 5 or q.shape[2] != 4:
        raise ValueError(f"volume_as_layers takes a volume of shape [M, D, 4, Ht, Wt], got {tuple(q.shape)}")
    if not is_interleaved(q):
        raise ValueError(f"volume_as_layers takes an interleaved volume (channel stride 1, texel stride 4), got strides {tuple(q.stride())}")
    return q.permute(0, 1, 3, 4, 2)


def quantize_volume(rgba: torch.Tensor, interleaved: bool = False) -> torch.Tensor:
    """Values in [0, 1] -> uint8 codes: 255 v rounded to the nearest integer, halves to even (formed in fp32).  A value outside [0, 1] or a
    NaN raises ValueError: a code cannot hold it, and clamping would hide what the float render reports as a range error.
    `interleaved=True` (a volume `[M, D, 4, Ht, Wt]`): the same codes in channels-last memory order, as an interleaved volume."""
    if not rgba.is_floating_point():
        raise TypeError(f"quantize_volume takes a floating-point volume, got {rgba.dtype}")
    v = rgba.detach().to(torch.float32)
    if v.numel() and not bool(((v >= 0) & (v <= 1)).all()):
        raise ValueError("quantize_volume: values must lie in [0, 1]")
    q = torch.round(v * 255.0).to(torch.uint8)   # (torch.round: half to even)
    if not interleaved:
        return q
    if q.ndim != 5 or q.shape[2] != 4:
        raise ValueError(f"quantize_volume(interleaved=True) takes a volume of shape [M, D, 4, Ht, Wt], got {tuple(q.shape)}")
    return layers_as_volume(q.permute(0, 1, 3, 4, 2).contiguous())


def dequantize_volume(q: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """uint8 codes -> `q.float() / 255` (the correctly rounded fp32 quotient: the volume a render of q renders), then cast to `dtype`."""
    if q.dtype is not torch.uint8:
        raise TypeError(f"dequantize_volume takes a uint8 volume, got {q.dtype}")
    return (q.float() / 255).to(dtype)
