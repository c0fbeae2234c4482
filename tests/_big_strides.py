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
less than NEED_FREE = 24 GiB free -- which no MI355X does."""
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
PLANES = {"outer": 2}             # D; every other layout has 3


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


def need_memory():
    import pytest
    import torch
    release()
    free, _ = torch.cuda.mem_get_info()
    if free < NEED_FREE:
        pytest.skip(f"needs {NEED_FREE >> 30} GiB of free device memory for the NaN margins, {free >> 30} GiB are free")


class Window:
    """`values` (a host tensor) as a view with element strides `stride` inside a fresh buffer filled with `fill`:

        with Window(values, stride) as w:      # w.view: the strided view, w.copy: a contiguous copy on the device
            ...

    The buffer never leaves the device and is released on exit (keep no reference to `w.view`: let tensors made from it die with the block's
    helper functions)."""

    def __init__(self, values, stride, fill=float("nan"), device="cuda:0"):
        self.values, self.stride, self.fill, self.device = values, tuple(stride), fill, device
        es = values.element_size()
        assert LEAD % es == 0 and len(self.stride) == values.dim()
        dims = sorted((s, n) for n, s in zip(values.shape, self.stride) if n > 1)
        assert all(s > 0 for s, _ in dims) and all(b[0] >= a[0] * a[1] for a, b in zip(dims, dims[1:])), "the window's elements must not overlap"
        self.lead = LEAD // es
        self.numel = self.lead + span(values.shape, self.stride) + 1 + TAIL // es

    def __enter__(self):
        import torch
        need_memory()
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
        assert first - buf.data_ptr() >= LEAD and buf.data_ptr() + buf.numel() * es - last > TAIL
        del buf
        return self

    def __exit__(self, *exc):
        self.view = self.copy = None
        release()
        return False
