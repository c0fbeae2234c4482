"""Small textures as strided windows of one large device buffer: strides past 2^31 bytes, 2^32 bytes and 2^31 elements, on both sides of every
host-side guard that decides whether a kernel with 32-bit in-plane offsets may take a launch.

The stride arithmetic (`strides`, `image_strides`, `span`) is plain Python and is shared with the host-only test (tests/test_big_strides_cpu.py);
`Window` needs a device.

Texels: HT = 32 rows of 36 (fp32, uint8) or 32 (bf16 / fp16) texels in rows of PITCH = 40.  The staged loaders want the width to be a multiple of
their 16-byte item: 4 fp32 texels, but 8 sixteen-bit ones -- 36 texels of bf16 would be refused by every staged kernel whatever the strides, and the
tests could not say that the staged kernel ran.  All element strides (pitch, plane, MPI) are the same for the three float types.

Layouts (volume [M, D, 4, HT, WT]; `es` = bytes per element):
  outer    s_plane = 2^30 + 4096 elements (fp32: just past 2^32 bytes, 16-bit: just past 2^31), s_mpi = 2^31 + 8192 elements; the channel and row
           strides are the dense ones.  The same construction serves alpha [M, D, 1, ..], rgb / background [M, 3, ..] and depth [M, 1, ..]
           (`image_strides`: their MPI stride is the large one).
  chanA/B/C   [4, M, D, HT, PITCH] storage permuted to [M, D, 4, HT, WT]: 3 s_chan es = 2^31 - 2^24 (every staged kernel takes it), 2^31 + 2^24
           (offsets handled as signed 32-bit values go wrong here) and 2^32 + 2^24 (unsigned 32-bit offsets wrap), each rounded to whole 64-byte
           steps of s_chan -- down for A, up for B and C.
  rowB/C   [HT, M, D, 4, PITCH] storage permuted likewise: 31 s_row es = 2^31 + 2^24 and 2^32 + 2^24, rounded up.
  uint8    the outer layout with byte strides s_plane = 2^31 + 4096, s_mpi = 2^32 + 8192, planar and channels-last; chanA/B/C planar.

Margins: a wrong 32-bit byte offset reaches at most 2 GiB below a plane's first texel (signed) or 4 GiB above it (unsigned wrap).  Every buffer
starts LEAD = 2 GiB before its first window element and ends TAIL = 4 GiB behind its LAST window element, all of it NaN (uint8: 255, an opaque
white texel).  A truncated offset lands on the fill inside the allocation -- a failed assertion, never an access outside it.  Do not shrink them.
One buffer lives at a time (`Window` is a context manager; peak about 18 GiB for the fp32 outer layout), and a case skips when the device has
less than NEED_FREE = 24 GiB free -- which no MI355X does.

Channels-last float layers [M, D, HT, WT, 4] (texel stride 4, channel stride 1; `layer_strides`: (s_mpi, s_plane, s_row) in elements), for the
kernels that read whole texels in place (render_layers.hip, the texel instances of render_backward.hip and render_backward_geometry.hip):
  L-outer  s_row = 4 PITCH (dense rows), s_plane = S_PLANE, s_mpi = S_MPI: the large strides are the 64-bit ones.
  L-rowA/T/B/C   [HT, M, D, PITCH, 4] storage permuted to [M, D, HT, WT, 4]; the row stride in whole 64-byte steps.
           A: the largest the staged forward takes -- (32 + 1) s_row es + 16 * 64 + 128 < 2^31, the bound of layers_variant_supports --, which the
              tile backward takes too; T: the smallest with 33 s_row es >= 2^31: the staged forward refuses it, the tile backward, whose bound is
              (32 s_row + 4 WT) es < 2^31, takes it; B, C: 31 s_row es = 2^31 + 2^24 and 2^32 + 2^24, rounded up as rowB / rowC are: both refuse.
           The two bounds are restated here to FIND the strides; tests/test_big_strides_cpu.py asks the library on which side each one lies.
Their fp32 gradient [M, D, HT, WT, 4] (`grad_strides`), the same storage order, gs_row in dwords:
  G-byte   31 gs_row 4 bytes = 2^32 + 2^24 (rounded up): every dword offset of a plane is below 2^31, so the tile backward takes the launch -- and
           the bytes behind them are past 2^32: right only if nothing scales a dword offset by 4 in 32 bits.
  G-past   the first gs_row with HT gs_row + 4 WT >= 2^31, which layers_offsets_fit_32(gs_row, HT, WT, 1) refuses: the one-pixel kernel.
The shading image [M, 1, HT, WT] of the shaded render, fp32 (`shading_strides`: (s_mpi, s_row)):
  S-outer  s_mpi = S_MPI, rows of PITCH.
  S-rowA/B [HT, M, PITCH] storage permuted; s_row the largest / the smallest multiple of 16 elements with HT s_row + WT < / >= 2^31 / 4, the third
           guard of the shaded tile backward (plane_offsets_fit_32(0, s_row, HT, WT, 4)): the tile twin / the one-pixel twin.

Margins of the layouts above, by the unit the kernel counts an offset in.  Layers and the shading image are addressed at 32-bit BYTE offsets (l_off
and pass_off of the staged forward, s_row_b of the pair loads): a mistake reaches 2^31 bytes below or 2^32 bytes above -- LEAD and TAIL as they are.
The gradient of the texel tile backward is addressed at 32-bit DWORD offsets (row gs_row + column, counted in floats): a sign-extended offset
reaches 2^31 dwords = 8 GiB below the box origin, a wrapped one less than 2^32 dwords = 16 GiB above it; a dword offset scaled to bytes in 32 bits
loses multiples of 4 GiB and lands below the true cell, never below the origin.  So a gradient window has GRAD_LEAD = 4 LEAD in front of its first
element and GRAD_TAIL = 4 TAIL behind its last: 8 + 4 + 16 = 28 GiB for G-byte, 8 + 8 + 16 = 32 GiB for G-past.  Both are more than NEED_FREE:
`Window(need=...)` states the case's own need (the buffer, the contiguous copy and 2 GiB of room) and skips below it."""
import gc

HT, PITCH = 32, 40
S_PLANE, S_MPI = 2 ** 30 + 4096, 2 ** 31 + 8192          # elements (float types)
U8_S_PLANE, U8_S_MPI = 2 ** 31 + 4096, 2 ** 32 + 8192    # bytes
LEAD, TAIL = 2 ** 31, 2 ** 32                            # bytes
NEED_FREE = 24 * 2 ** 30
CHAN_BYTES = {"chanA": 2 ** 31 - 2 ** 24, "chanB": 2 ** 31 + 2 ** 24, "chanC": 2 ** 32 + 2 ** 24}   # 3 s_chan es
ROW_BYTES = {"rowB": 2 ** 31 + 2 ** 24, "rowC": 2 ** 32 + 2 ** 24}                                  # 31 s_row es
FLOAT_LAYOUTS = ("outer", "chanA", "chanB", "chanC", "rowB", "rowC")
FITS_32 = ("outer", "chanA")      # every in-plane byte offset is below 2^31: all staged kernels and the atomics-free backward pair take these
PLANES = {"outer": 2, "L-outer": 2}   # D; every other layout has 3
GRAD_LEAD, GRAD_TAIL = 4 * LEAD, 4 * TAIL                # bytes: offsets counted in dwords
LAYER_LAYOUTS = ("L-outer", "L-rowA", "L-rowT", "L-rowB", "L-rowC")
LAYERS_STAGED = ("L-outer", "L-rowA")                    # the staged forward takes these (gmpi_render_layers_supports) ...
LAYERS_TILE = ("L-outer", "L-rowA", "L-rowT")            # ... the tile backward these (gmpi_render_layers_backward_supports)
GRAD_LAYOUTS = ("G-byte", "G-past")
SHADING_LAYOUTS = ("S-outer", "S-rowA", "S-rowB")
SHADING_TILE = ("S-outer", "S-rowA")                     # inside the shaded tile backward's third guard


def wt_of(es):
    return 36 if es != 2 else 32


def planes_of(layout):
    return PLANES.get(layout, 3)


def _step(nbytes, es, up):
    """nbytes / es elements as a multiple of 64 bytes, rounded down or up."""
    q = 64 // es
    return nbytes // es // q * q if not up else -(-nbytes // (es * q)) * q


def chan_stride(layout, es):
    return _step(-(-CHAN_BYTES[layout] // 3) if layout != "chanA" else CHAN_BYTES[layout] // 3, es, up=layout != "chanA")


def row_stride(layout, es):
    return _step(-(-ROW_BYTES[layout] // (HT - 1)), es, up=True)


def strides(layout, es, D=None, C=4, u8=False):
    """(s_mpi, s_plane, s_chan, s_row) of a [M, D, C, HT, WT] tensor in `layout`, in elements (u8: es = 1, bytes)."""
    D = planes_of(layout) if D is None else D
    if layout == "outer":
        return (U8_S_MPI, U8_S_PLANE, HT * PITCH, PITCH) if u8 else (S_MPI, S_PLANE, HT * PITCH, PITCH)
    if layout in CHAN_BYTES:
        return (D * HT * PITCH, HT * PITCH, chan_stride(layout, es), PITCH)
    if layout in ROW_BYTES:
        return (D * C * PITCH, C * PITCH, PITCH, row_stride(layout, es))
    raise KeyError(layout)


def image_strides(layout, es, C=3):
    """(s_mpi, s_chan, s_row) of an image tensor [M, C, HT, WT] (rgb, background, depth): the outer layout puts the large stride between the
    MPIs, the channel-major ones between the channels."""
    if layout == "outer":
        return (S_MPI, HT * PITCH, PITCH)
    if layout in CHAN_BYTES:
        return (HT * PITCH, chan_stride(layout, es), PITCH)
    raise KeyError(layout)


def layer_row_stride(layout, es):
    """s_row of a row layout of float layers, in elements (the module docstring has the four bounds)."""
    if layout == "L-rowA":
        return _step((2 ** 31 - 16 * 64 - 128 - 1) // 33, es, up=False)
    if layout == "L-rowT":
        return _step(-(-2 ** 31 // 33), es, up=True)
    return row_stride({"L-rowB": "rowB", "L-rowC": "rowC"}[layout], es)


def layer_strides(layout, es, D=None):
    """(s_mpi, s_plane, s_row) of layers [M, D, HT, WT, 4] in `layout`, in elements; the texel stride is 4, the channel stride 1."""
    D = planes_of(layout) if D is None else D
    if layout == "L-outer":
        return (S_MPI, S_PLANE, 4 * PITCH)
    return (D * 4 * PITCH, 4 * PITCH, layer_row_stride(layout, es))


def grad_strides(layout, wt, D=3):
    """(gs_mpi, gs_plane, gs_row) of the fp32 gradient [M, D, HT, wt, 4] of float layers, in dwords."""
    gs_row = row_stride("rowC", 4) if layout == "G-byte" else -(-(2 ** 31 - 4 * wt) // HT)
    assert layout in GRAD_LAYOUTS
    return (D * 4 * PITCH, 4 * PITCH, gs_row)


def shading_strides(layout, wt):
    """(s_mpi, s_row) of the fp32 shading image [M, 1, HT, wt], in elements."""
    if layout == "S-outer":
        return (S_MPI, PITCH)
    lim = 2 ** 31 // 4
    s_row = (lim - wt - 1) // HT // 16 * 16 if layout == "S-rowA" else -(-(lim - wt) // (HT * 16)) * 16
    assert layout in SHADING_LAYOUTS
    return (PITCH, s_row)


def span(shape, stride):
    """Offset of the last element of a view, in elements."""
    return sum((n - 1) * s for n, s in zip(shape, stride))


def plane_bytes(layout, es, wt=None):
    """(3 s_chan + HT s_row + WT) es: what the 32-bit guards of the backward compare with 2^31."""
    _, _, s_chan, s_row = strides(layout, es)
    return (3 * s_chan + HT * s_row + (wt_of(es) if wt is None else wt)) * es


def release():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def need_memory(need=NEED_FREE):
    import pytest
    import torch
    release()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need / 2 ** 30:.0f} GiB of free device memory for the margins, {free >> 30} GiB are free")


class Window:
    """`values` (a host tensor) as a view with element strides `stride` inside a fresh buffer filled with `fill`:

        with Window(values, stride) as w:      # w.view: the strided view, w.copy: a contiguous copy on the device
            ...

    The buffer never leaves the device and is released on exit (keep no reference to `w.view`: let tensors made from it die with the block's
    helper functions).  lead, tail: the margins in bytes (the module docstring derives them from the unit the kernel counts offsets in); need: the
    free device memory below which the case skips -- NEED_FREE, or the case's own need where its buffer is larger than that allows."""

    def __init__(self, values, stride, fill=float("nan"), device="cuda:0", lead=LEAD, tail=TAIL, need=None):
        self.values, self.stride, self.fill, self.device = values, tuple(stride), fill, device
        self.lead_bytes, self.tail_bytes = lead, tail
        es = values.element_size()
        assert lead >= LEAD and tail >= TAIL and lead % es == 0 and len(self.stride) == values.dim()
        dims = sorted((s, n) for n, s in zip(values.shape, self.stride) if n > 1)
        assert all(s > 0 for s, _ in dims) and all(b[0] >= a[0] * a[1] for a, b in zip(dims, dims[1:])), "the window's elements must not overlap"
        self.lead = lead // es
        self.numel = self.lead + span(values.shape, self.stride) + 1 + tail // es
        self.need = max(NEED_FREE, self.numel * es + values.numel() * es + 2 ** 31) if need is None else need

    def __enter__(self):
        import torch
        need_memory(self.need)
        torch.cuda.reset_peak_memory_stats()   # (the tests print max_memory_allocated: each its own)
        buf = torch.empty((self.numel,), dtype=self.values.dtype, device=self.device)
        buf.fill_(self.fill)
        self.view = buf.as_strided(tuple(self.values.shape), self.stride, self.lead)
        self.view.copy_(self.values.to(self.device))
        self.copy = self.values.to(self.device).contiguous()
        assert self.view.data_ptr() % 64 == 0
        # the margins, from the addresses: 2 GiB of fill below the first element, 4 GiB behind the last one, inside the allocation
        es = buf.element_size()
        first, last = self.view.data_ptr(), self.view.data_ptr() + span(self.values.shape, self.stride) * es
        assert first - buf.data_ptr() >= self.lead_bytes and buf.data_ptr() + buf.numel() * es - last > self.tail_bytes
        del buf
        return self

    def __exit__(self, *exc):
        self.view = self.copy = None
        release()
        return False
