"""The occupancy map of a uint8 RGBA volume, for the sparse render (`occupancy=` of `MPI.render_views`, `MPIRenderer.render`, `ViewBatchDriver.render_path`
and `render_seeds`; gmpi_mpi_render_u8_sparse_launch, include/gmpi_render.h).

Stored MPIs are mostly empty, and at 8 bits "empty" is the exact alpha code 0.  The map holds, per 16 x 16 texel block of every plane, the largest alpha
code of the block; the staged uint8 kernel then skips every (tile, plane) whose texel box lies in blocks of maximum 0 -- which moves no bit of the result.
A map describes the codes it was built from: it records the volume's identity (address, shape, strides, device, version counter), and a render with a map of
another volume, or of a volume written in place since, raises ValueError before anything is launched."""
import ctypes
from typing import Optional

import torch

from . import _lib
from .quantized import is_interleaved

BLOCK = 16   # texels per side of a block of the map (gmpi_query(53))


def _version(q: torch.Tensor) -> Optional[int]:
    """q's version counter; None for a tensor that has none (made under torch.inference_mode)."""
    try:
        return q._version
    except RuntimeError:
        return None


def _identity(q: torch.Tensor) -> tuple:
    return (q.data_ptr(), tuple(q.shape), tuple(q.stride()), q.device, _version(q))


def _check_volume(q, what: str) -> None:
    if not isinstance(q, torch.Tensor) or q.dtype is not torch.uint8:
        raise TypeError(f"{what} takes a uint8 volume [M, D, 4, Ht, Wt] (code 0 is the only exact zero the render can skip), got "
                        f"{q.dtype if isinstance(q, torch.Tensor) else type(q).__name__}")
    if q.ndim != 5 or q.shape[2] != 4:
        raise ValueError(f"{what} takes a volume of shape [M, D, 4, Ht, Wt], got {tuple(q.shape)}")


def occupancy_reference(q: torch.Tensor) -> torch.Tensor:
    """The executable definition of the map, plain torch on any device: uint8 [M, D, ceil(Ht / 16), ceil(Wt / 16)], each entry the largest alpha code among
    the texels of its 16 x 16 block that exist (border blocks are partial)."""
    _check_volume(q, "occupancy_reference")
    M, D, _, Ht, Wt = q.shape
    nby, nbx = -(-Ht // BLOCK), -(-Wt // BLOCK)
    a = torch.zeros((M, D, nby * BLOCK, nbx * BLOCK), dtype=torch.uint8, device=q.device)   # (padding 0: the smallest code)
    a[:, :, :Ht, :Wt] = q[:, :, 3]
    return a.view(M, D, nby, BLOCK, nbx, BLOCK).amax(dim=(3, 5))


class Occupancy:
    """What `build_occupancy` returns: `.map` (uint8 [M, D, ceil(Ht / 16), ceil(Wt / 16)]), `.block` (16), `.stats` (None, or a [2] uint32 device tensor to
    which every sparse launch adds the (tile, plane) pairs it skipped and those it staged: the caller zeroes and reads it) and the identity of the
    volume the map was built from."""

    def __init__(self, map: torch.Tensor, block: int, stats: Optional[torch.Tensor], identity: tuple):
        self.map, self.block, self.stats, self.identity = map, block, stats, identity

    def check(self, q: torch.Tensor) -> None:
        """Raises unless this map was built from q as it is now: TypeError for a volume that is not uint8, ValueError for another tensor (address,
        shape, strides or device differ) or one written in place since the build (its version counter moved).  A tensor without a version counter, on
        either side, is compared without it."""
        _check_volume(q, "occupancy=")
        have, want = _identity(q), self.identity
        if have[:4] != want[:4]:
            raise ValueError(f"occupancy= was built from another volume: data_ptr / shape / strides / device {want[:4]}, this render's {have[:4]}; "
                             "build_occupancy(q) of the volume that is rendered")
        if have[4] is not None and want[4] is not None and have[4] != want[4]:
            raise ValueError(f"occupancy= is stale: the volume was written in place since the map was built (version {want[4]} -> {have[4]}); "
                             "call build_occupancy(q) again")
        nby, nbx = -(-q.shape[3] // self.block), -(-q.shape[4] // self.block)
        if self.block != BLOCK or tuple(self.map.shape) != (q.shape[0], q.shape[1], nby, nbx) or self.map.dtype is not torch.uint8 or not self.map.is_contiguous():
            raise ValueError(f"occupancy=: the map must be contiguous uint8 {(q.shape[0], q.shape[1], nby, nbx)} with block {BLOCK}, got "
                             f"{self.map.dtype} {tuple(self.map.shape)} with block {self.block}")
        if self.map.device != q.device or (self.stats is not None and self.stats.device != q.device):
            raise ValueError(f"occupancy=: the map lies on {self.map.device}, the volume on {q.device}")

    def of_mpis(self, q: torch.Tensor, start: int, stop: int) -> "Occupancy":
        """This map of q, cut down to the MPIs q[start:stop] (a view of the map, the same counters): what a driver that renders a stack batch by batch passes on."""
        self.check(q)
        return Occupancy(self.map[start:stop], self.block, self.stats, _identity(q[start:stop]))

    def struct(self) -> _lib.GmpiOccupancy:
        occ = _lib.GmpiOccupancy()
        occ.map, occ.block = self.map.data_ptr(), self.block
        occ.stats = None if self.stats is None else self.stats.data_ptr()
        return occ


def build_occupancy(q: torch.Tensor, stats: bool = False) -> Occupancy:
    """The occupancy map of the uint8 volume q [M, D, 4, Ht, Wt] -- planar or channels-last (`layers_as_volume`), any outer strides -- built on q's device by one
    kernel that reads the alpha bytes alone (stream-ordered, no synchronisation).  `stats=True` adds a zeroed [2] uint32 counter tensor.  Build it again after
    every write to q: a render with a stale map raises ValueError."""
    from .hip_mpi import _call, _volume_operand
    _check_volume(q, "build_occupancy")
    src = _volume_operand(q)   # (the tensor the render reads: q itself unless its innermost stride is neither 1 nor the interleaved 4)
    M, D, _, Ht, Wt = src.shape
    p = _lib.GmpiRenderParams()
    p.struct_size = ctypes.sizeof(_lib.GmpiRenderParams)
    p.rgba_dtype, p.M, p.D, p.Ht, p.Wt = _lib.DTYPE_U8, M, D, Ht, Wt
    p.rgba = src.data_ptr()
    p.rgba_stride[:] = src.stride()
    assert is_interleaved(src) or src.stride(4) == 1
    omap = torch.empty((M, D, -(-Ht // BLOCK), -(-Wt // BLOCK)), dtype=torch.uint8, device=q.device)
    if omap.numel():
        _call("gmpi_u8_occupancy_launch", q.device, ctypes.byref(p), omap.data_ptr())
    counters = torch.zeros(2, dtype=torch.uint32, device=q.device) if stats else None
    return Occupancy(omap, BLOCK, counters, _identity(q))
