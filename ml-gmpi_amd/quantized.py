"""8-bit storage of an RGBA volume: code c in 0..255 stands for the fp32 value c / 255 (GMPI_DTYPE_U8, include/gmpi_render.h).  The forward
render reads such a volume as it is (`MPI.render_views`, `MPIRenderer.render`, the `ViewBatchDriver` methods): by definition it renders
`dequantize_volume(q)`.  Plain torch, any device."""
import torch


def quantize_volume(rgba: torch.Tensor) -> torch.Tensor:
    """Values in [0, 1] -> uint8 codes: 255 v rounded to the nearest integer, halves to even (formed in fp32).  A value outside [0, 1] or a
    NaN raises ValueError: a code cannot hold it, and clamping would hide what the float render reports as a range error."""
    if not rgba.is_floating_point():
        raise TypeError(f"quantize_volume takes a floating-point volume, got {rgba.dtype}")
    v = rgba.detach().to(torch.float32)
    if v.numel() and not bool(((v >= 0) & (v <= 1)).all()):
        raise ValueError("quantize_volume: values must lie in [0, 1]")
    return torch.round(v * 255.0).to(torch.uint8)   # (torch.round: half to even)


def dequantize_volume(q: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """uint8 codes -> `q.float() / 255` (the correctly rounded fp32 quotient: the volume a render of q renders), then cast to `dtype`."""
    if q.dtype is not torch.uint8:
        raise TypeError(f"dequantize_volume takes a uint8 volume, got {q.dtype}")
    return (q.float() / 255).to(dtype)
