"""Channels-last float layers: `[M, D, Ht, Wt, 4]` fp32 / bf16 / fp16 -- one RGBA texel after the other, what image files, numpy, EXR readers and
channels-last networks hold.  `MPI.render_views_layers` (and `MPIRenderer.render_layers`, `ViewBatchDriver.render_path_layers` /
`render_seeds_layers`) render such a stack in place through gmpi_mpi_render_layers_launch (include/gmpi_render.h): nothing is copied into the planar
`[M, D, 4, Ht, Wt]` order first.  The uint8 twin of the layout is quantized.py's (`layers_as_volume`, `is_interleaved`).  Plain torch, any device."""
import torch

FLOAT_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def is_float_layers(t) -> bool:
    """t is a stack of float layers the kernels read in place: fp32 / bf16 / fp16, shape [M, D, Ht, Wt, 4], channel stride 1, texel stride 4, rows that do
    not overlap (row stride >= 4 Wt: padded rows are fine), no negative stride (a batch stride of 0 -- one MPI expanded -- is fine).  Slices along M, D,
    rows and columns of such a stack are such stacks."""
    return (t.dtype in FLOAT_DTYPES and t.ndim == 5 and t.shape[4] == 4 and t.stride(4) == 1 and t.stride(3) == 4 and t.stride(2) >= 4 * t.shape[3]
            and all(s >= 0 for s in t.stride()))


def layer_strides(layers: torch.Tensor):
    """GmpiRenderParams.rgba_stride of float layers (`is_float_layers`): the volume [M, D, 4, Ht, Wt] they are a view of, in elements."""
    s = layers.stride()
    return [s[0], s[1], 1, s[2], 4]
