"""The plane-chunked render through the band kernel, without a GPU: the three C entries' exports, answers and refusals on the host (the real library: every
call returns before anything is launched, no pointer is followed), and what `hip_mpi` hands them for `chunk_kernel` None / "band" / "band+tile" (a
recorder that records the launches and lets the two host-side queries through to the real library)."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from test_chunks_cpu import FWD, stack_inputs, SIZES
from test_depth_alpha_cpu import ROOT
from test_marshal_cpu import Call, Recorder, H, W

from ml_gmpi_amd import _lib
from ml_gmpi_amd import hip_mpi
from ml_gmpi_amd.hip_mpi import MPI

BAND, BYTES, SUPPORTS = "gmpi_mpi_render_chunk_band_launch", "gmpi_render_chunk_band_workspace_bytes", "gmpi_render_chunk_band_supports"


# ---- exports and ABI ---------------------------------------------------------------------------------------------------------------------------
def test_exports_header_and_queries():
    header = open(os.path.join(ROOT, "include", "gmpi_render.h")).read()
    for name in (BAND, BYTES, SUPPORTS):
        assert name in _lib.EXPORTS and name + "(" in header, name
    lib = _lib.load_library()
    assert lib.gmpi_query(50) == 1 and lib.gmpi_query(49) == -1 and lib.gmpi_query(51) == -1
    assert lib.gmpi_query(0) == 2 and lib.gmpi_query(1) == 184
    assert _lib.ABI_VERSION == 2 and ctypes.sizeof(_lib.GmpiRenderParams) == 184 and ctypes.sizeof(_lib.GmpiCarry) == 24
    assert len(lib.gmpi_mpi_render_chunk_band_launch.argtypes) == 3 and lib.gmpi_render_chunk_band_workspace_bytes.restype is ctypes.c_uint64


class Host:
    """Fake tensors for calls that are refused before a launch: one host buffer, addresses 256-byte aligned inside it."""

    def __init__(self):
        self.buf = np.zeros(1 << 20, dtype=np.uint8)
        self.base = (self.buf.ctypes.data + 255) // 256 * 256
        self.room = self.buf.ctypes.data + self.buf.nbytes - self.base

    def params(self, N=1, variant=_lib.VARIANT_BAND, dtype=_lib.DTYPE_F32, outputs=False, D=3, S=16, T=16, ws=None):
        p = _lib.GmpiRenderParams()
        p.struct_size = ctypes.sizeof(_lib.GmpiRenderParams)
        p.flags, p.variant, p.rgba_dtype = _lib.FLAG_ALIGN_CORNERS, variant, dtype
        p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = N, 1, D, T, T, S, S, 1
        p.rgba = self.base
        p.rgba_stride[:] = [D * 4 * T * T, 4 * T * T, T * T, T, 1]
        p.dhw = p.ray_dir = p.eye_pos = p.z_dir = self.base
        if outputs:
            p.rgb_out = p.depth_out = self.base
        if ws is not None:
            p.workspace, p.workspace_bytes = self.base + ws[0], ws[1]
        return p

    def carry(self, size=None, state_out=True):
        c = _lib.GmpiCarry()
        c.struct_size = ctypes.sizeof(_lib.GmpiCarry) if size is None else size
        c.state_in, c.state_out = None, (self.base if state_out else None)
        return c


def test_refusals_on_the_host():
    lib, h = _lib.load_library(), Host()
    fwd = lambda p, c: lib.gmpi_mpi_render_chunk_band_launch(None if p is None else ctypes.byref(p), None if c is None else ctypes.byref(c), None)
    sup = lambda p: lib.gmpi_render_chunk_band_supports(None if p is None else ctypes.byref(p))
    need = lambda p: lib.gmpi_render_chunk_band_workspace_bytes(None if p is None else ctypes.byref(p))
    assert fwd(h.params(), None) == -1 and fwd(None, h.carry()) == -1                  # GMPI_E_NULL
    assert sup(None) == -1 and need(None) == 0
    assert fwd(h.params(), h.carry(size=16)) == -5                                     # GMPI_E_ABI
    p = h.params(); p.struct_size -= 8
    assert fwd(p, h.carry()) == -5 and sup(p) == -5 and need(p) == 0
    for v in (_lib.VARIANT_GATHER, _lib.VARIANT_LDS, _lib.VARIANT_WAVE, _lib.VARIANT_DMA, 9):
        assert fwd(h.params(variant=v), h.carry()) == -6, v                            # GMPI_E_VARIANT
        assert sup(h.params(variant=v)) == 0 and need(h.params(variant=v)) == 0, v
    # the workspace: missing, too small, misaligned -> GMPI_E_WORKSPACE; BAND and AUTO alike
    for v in (_lib.VARIANT_BAND, _lib.VARIANT_AUTO):
        p = h.params(variant=v)
        n = need(p)
        assert sup(p) == 1 and 0 < n <= h.room - 256
        assert fwd(p, h.carry()) == -8
        assert fwd(h.params(variant=v, ws=(0, n - 1)), h.carry()) == -8
        assert fwd(h.params(variant=v, ws=(128, n)), h.carry()) == -8
        assert fwd(h.params(variant=v, ws=(0, n)), h.carry(state_out=False)) == -1      # nothing to write: GMPI_E_NULL
        assert fwd(h.params(variant=v, ws=(0, n), N=0), h.carry()) == 0 and fwd(h.params(variant=v, N=0), None) == 0   # no views: GMPI_OK at once
        assert need(h.params(variant=v, N=0)) == 0
    # uint8: not built for the band kernel
    p = h.params(dtype=_lib.DTYPE_U8, ws=(0, 1 << 16))
    assert fwd(p, h.carry()) == -6 and sup(p) == 0 and need(p) == 0
    # a texture the band kernel cannot address, a volume its 16-byte items cannot take
    p = h.params(T=8200, ws=(0, 1 << 16))
    assert fwd(p, h.carry()) == -6 and sup(p) == 0 and need(p) == 0
    p = h.params(ws=(0, 1 << 16)); p.rgba += 4
    assert fwd(p, h.carry()) == -6 and sup(p) == 0 and need(p) == 0
    # every other error as at gmpi_mpi_render_chunk_launch
    p = h.params(); p.flags |= 1 << 30
    assert fwd(p, h.carry()) == -7 and sup(p) == -7
    p = h.params(); p.rgba_stride[4] = 2
    assert fwd(p, h.carry()) == -4
    assert fwd(h.params(dtype=7), h.carry()) == -3
    p = h.params(); p.D = 0
    assert fwd(p, h.carry()) == -2
    # the old entry is what it was: BAND and WAVE refused, no workspace read
    old = lambda p, c: lib.gmpi_mpi_render_chunk_launch(ctypes.byref(p), ctypes.byref(c), None)
    assert old(h.params(variant=_lib.VARIANT_BAND, ws=(0, 1 << 16)), h.carry()) == -6 and old(h.params(variant=_lib.VARIANT_WAVE), h.carry()) == -6


@pytest.mark.parametrize("shape", [dict(N=2, D=5, S=72, T=64), dict(N=3, D=9, S=200, T=208), dict(N=1, D=12, S=512, T=512)])
@pytest.mark.parametrize("dtype", [_lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16])
def test_the_bytes_are_the_band_table_of_the_chunk(shape, dtype):
    lib, h = _lib.load_library(), Host()
    for v in (_lib.VARIANT_BAND, _lib.VARIANT_AUTO):
        p = h.params(variant=v, dtype=dtype, **shape)
        p.M, p.views_per_mpi = shape["N"], 1
        q = _lib.GmpiRenderParams.from_buffer_copy(p)
        q.variant, q.rgb_out, q.depth_out = _lib.VARIANT_BAND, h.base, h.base   # (the one-shot query wants outputs)
        want = lib.gmpi_render_workspace_bytes(ctypes.byref(q))
        assert want > 0 and lib.gmpi_render_chunk_band_workspace_bytes(ctypes.byref(p)) == want, (v, want)
    # ... and it grows with the chunk's planes alone: a chunk of one plane asks for less than the stack
    one = h.params(dtype=dtype, **dict(shape, D=1))
    assert lib.gmpi_render_chunk_band_workspace_bytes(ctypes.byref(one)) < want


# ---- marshalling ---------------------------------------------------------------------------------------------------------------------------------
class BandRecorder(Recorder):
    """test_marshal_cpu's records-only recorder, except that the band entry's two host-side queries are answered by the real library (`takes`: or by
    a constant) and recorded too."""

    def __init__(self, takes=None):
        super().__init__((FWD, BAND, "gmpi_rgba_range_check_launch"))
        self.lib, self.takes = _lib.load_library(), takes

    def __getattr__(self, name):
        if name in (BYTES, SUPPORTS):
            def query(ref):
                value = self.takes if name == SUPPORTS and self.takes is not None else getattr(self.lib, name)(ref)
                self.calls.append(Call(name, (self._copy(ref), value), None))
                return value
            return query
        return super().__getattr__(name)


@pytest.fixture
def rec(monkeypatch):
    r = BandRecorder()
    monkeypatch.setattr(_lib, "load_library", lambda: r)
    return r


def aligned_chunks(dtype=torch.float32):
    """stack_inputs' stack with every chunk's storage on a 16-byte boundary (the CPU allocator's 64 bytes: asserted), as the band kernel asks."""
    chunks, geo = stack_inputs(dtype=dtype)
    assert all(c.data_ptr() % 16 == 0 for c in chunks)
    return chunks, geo


def launches(rec):
    return [c for c in rec.calls if c.name in (FWD, BAND)]


def test_none_records_the_old_entry_only(rec):
    chunks, geo = aligned_chunks()
    with torch.no_grad():
        MPI().render_views_chunks(chunks, *geo)
        MPI().render_views_chunks(chunks, *geo, chunk_kernel=None)
    assert [c.name for c in rec.calls] == [FWD] * 6
    assert all(c.args[0].workspace is None and c.args[0].variant == _lib.VARIANT_AUTO for c in rec.calls)


@pytest.mark.parametrize("kernel,variant", [("band", _lib.VARIANT_BAND), ("band+tile", _lib.VARIANT_AUTO)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_band_values_record_the_new_entry_with_a_lent_workspace(rec, kernel, variant, dtype):
    chunks, geo = aligned_chunks(dtype)
    kw = dict(check_last_plane=True, out_pm1=True, want_transmittance=True)
    mpi = MPI(variant="lds", strict_order=True)
    with torch.no_grad():
        res = mpi.render_views_chunks(chunks, *geo, chunk_kernel=kernel, **kw)
        new = list(rec.calls)
        del rec.calls[:]
        mpi.render_views_chunks(chunks, *geo, **kw)
        old = list(rec.calls)
    assert [c.name for c in new] == [SUPPORTS, BYTES, BAND] * 3 and [c.name for c in old] == [FWD] * 3
    for i, (d, t) in enumerate(zip(SIZES, chunks)):
        sup, need, call = new[3 * i:3 * i + 3]
        p, c = call.args[0], call.args[1]
        q, k = old[i].args[0], old[i].args[1]
        assert sup.args[1] == 1 and need.args[1] > 0 and sup.args[0].variant == need.args[0].variant == variant
        assert p.variant == variant and p.D == d and p.rgba == t.data_ptr()
        assert p.workspace is not None and p.workspace_bytes >= need.args[1]
        # the same flags, geometry and carry as the old path: the state in place, outputs and the two last-chunk flags on the last launch only
        assert p.flags == q.flags and (p.N, p.M, p.Ht, p.Wt, p.H, p.W, p.rgba_dtype, p.views_per_mpi) == (q.N, q.M, q.Ht, q.Wt, q.H, q.W, q.rgba_dtype, q.views_per_mpi)
        assert list(p.rgba_stride) == list(q.rgba_stride) and (p.ray_dir, p.eye_pos, p.z_dir) == (q.ray_dir, q.eye_pos, q.z_dir)
        assert (c.state_in is None, c.state_out is None) == (k.state_in is None, k.state_out is None) == (i == 0, i == 2)
        assert (p.rgb_out is None, p.depth_out is None, p.transmittance_out is None) == (i < 2,) * 3
        assert c.struct_size == 24 and (i == 0 or c.state_in == new[2].args[1].state_out)
    base = _lib.FLAG_ALIGN_CORNERS | _lib.FLAG_CHECK_RANGE | _lib.FLAG_STRICT_ORDER
    assert [c.args[0].flags for c in new[2::3]] == [base, base, base | _lib.FLAG_OUT_PM1 | _lib.FLAG_CHECK_LAST_PLANE]
    assert new[8].args[0].rgb_out == res["color"].data_ptr() and new[8].args[0].transmittance_out == res["T"].data_ptr()
    assert len({c.args[0].status for c in new[2::3]}) == 1
    assert mpi.chunk_band_fallbacks == 0 and mpi.chunk_variant_fallbacks == 0


def test_the_attribute_is_read_at_every_add(rec):
    chunks, geo = aligned_chunks()
    with torch.no_grad():
        cr = MPI().chunked_render(*geo, chunk_kernel="band")
        assert cr.chunk_kernel == "band"
        cr.add(chunks[0])
        cr.chunk_kernel = None
        cr.add(chunks[1])
        cr.chunk_kernel = "band+tile"
        cr.add(chunks[2])
        cr.finish()
    calls = launches(rec)
    assert [c.name for c in calls] == [BAND, FWD, BAND]
    assert [c.args[0].variant for c in calls] == [_lib.VARIANT_BAND, _lib.VARIANT_AUTO, _lib.VARIANT_AUTO]
    state = calls[0].args[1].state_out
    assert [(c.args[1].state_in, c.args[1].state_out) for c in calls] == [(None, state), (state, state), (state, None)]   # one state, whichever kernel
    assert calls[1].args[0].workspace is None
    with pytest.raises(AssertionError, match="chunk_kernel"):
        MPI().chunked_render(*geo, chunk_kernel="tile")


def test_autograd_forward_takes_the_keyword_and_the_backward_is_unchanged(rec, monkeypatch):
    bwd = "gmpi_mpi_render_chunk_backward_launch"
    monkeypatch.setattr(rec, "entries", rec.entries + (bwd,))
    chunks, geo = aligned_chunks()
    for c in chunks:
        c.requires_grad_(True)
    res = MPI(backward="gather").render_views_chunks(chunks, *geo, chunk_kernel="band")
    assert [c.name for c in launches(rec)] == [BAND] * 3
    kept = [c.args[0].transmittance_out for c in launches(rec)]
    assert None not in kept and len(set(kept)) == 3
    (res["color"].sum() + res["depth"].sum()).backward()
    back = rec.named(bwd)
    assert [c.args[0].D for c in back] == list(reversed(SIZES)) and all(c.args[0].workspace is None for c in back)
    assert all(c.args[0].variant == _lib.VARIANT_AUTO for c in back)   # the module's variant: the band value never reaches the backward
    assert all(t.grad is not None and t.grad.shape == t.shape for t in chunks)


def test_an_unsupported_chunk_falls_back_counted_and_warned_once(rec, monkeypatch):
    monkeypatch.setattr(hip_mpi, "_CHUNK_BAND_WARNED", False)
    chunks, geo = aligned_chunks()
    codes = [(c * 255).to(torch.uint8) for c in chunks]
    view = [torch.cat([c.new_zeros(c.shape[:4] + (1,)), c], 4)[..., 1:] for c in chunks]   # a column slice: rows start 4 bytes off a 16-byte boundary
    assert all(v.data_ptr() % 16 == 4 and v.stride(4) == 1 for v in view)
    mpi = MPI()
    with torch.no_grad(), warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        mpi.render_views_chunks(codes, *geo, chunk_kernel="band")
        mpi.render_views_chunks(view, *geo, chunk_kernel="band+tile")
    assert [c.name for c in launches(rec)] == [FWD] * 6 and BYTES not in [c.name for c in rec.calls]
    assert all(c.args[0].variant == _lib.VARIANT_AUTO and c.args[0].workspace is None for c in launches(rec))   # today's path, call for call
    assert mpi.chunk_band_fallbacks == 6 and mpi.chunk_variant_fallbacks == 0
    mine = [w for w in seen if issubclass(w.category, RuntimeWarning) and "chunk_band_fallbacks" in str(w.message)]
    assert len(mine) == 1 and 'chunk_kernel="band"' in str(mine[0].message)


@pytest.mark.parametrize("name", ["band", "wave"])
def test_band_module_without_the_keyword_still_counts_the_variant_fallback(rec, name, monkeypatch):
    monkeypatch.setattr(hip_mpi, "_CHUNK_VARIANT_WARNED", False)
    chunks, geo = aligned_chunks()
    mpi = MPI(variant=name)
    with torch.no_grad(), warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        mpi.render_views_chunks(chunks, *geo)
        assert mpi.chunk_variant_fallbacks == 3 and mpi.chunk_band_fallbacks == 0
        assert [c.name for c in rec.calls] == [FWD] * 3 and all(c.args[0].variant == _lib.VARIANT_AUTO for c in rec.calls)
        # ... and with the keyword the same module takes the band entry: nothing falls back, nothing more is counted
        mpi.render_views_chunks(chunks, *geo, chunk_kernel="band")
    assert mpi.chunk_variant_fallbacks == 3 and mpi.chunk_band_fallbacks == 0 and [c.name for c in launches(rec)] == [FWD] * 3 + [BAND] * 3
    assert len([w for w in seen if "chunk_variant_fallbacks" in str(w.message)]) == 1


def test_renderer_render_chunks_passes_the_keyword_through(rec, monkeypatch):
    monkeypatch.setattr(rec, "entries", rec.entries + ("gmpi_mpi_render_launch",))
    from ml_gmpi_amd.renderer import make_renderer
    D7 = sum(SIZES)
    r = make_renderer("FFHQ", n_planes=D7, device="cpu", ray_backend="torch")
    g = torch.Generator().manual_seed(3)
    chunks = [torch.rand((2, d, 4, 8, 8), generator=g) for d in SIZES]
    with torch.no_grad():
        out = r.render_chunks(iter(chunks), 8, 8, chunk_kernel="band+tile")
        with pytest.raises(AssertionError, match="render_chunks"):
            r.render(torch.cat(chunks, 1), 8, 8, chunk_kernel="band")
    assert [c.name for c in launches(rec)] == [BAND] * 3 and all(c.args[0].variant == _lib.VARIANT_AUTO for c in launches(rec))
    assert out[0].shape == (2, 3, 8, 8)
