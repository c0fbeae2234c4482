"""The occupancy map of a uint8 volume on the CPU: `occupancy_reference` (the executable definition of what `build_occupancy` builds on the device) against
a brute-force loop, and the part of the host contract of `occupancy=` that needs no device.  tests/test_hip_u8_occupancy.py has the kernels."""
import pytest
import torch

import _u8_occupancy_cases as C

SHAPES = [(16, 16), (20, 36), (33, 68), (1, 4)]   # (Ht, Wt): one block, partial border blocks, one texel past a block, a single row
M, D = 2, 3


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_is_the_block_maximum_of_the_alpha_codes(shape):
    from ml_gmpi_amd import occupancy_reference
    Ht, Wt = shape
    vols = [C.sparse_codes(11 + Ht, (M, D, 4, Ht, Wt))] + C.corner_volumes(M, D, Ht, Wt)
    for i, q in enumerate(vols):
        for name, v in C.stridings(q).items():
            want = C.brute_force_map(v)
            got = occupancy_reference(v)
            assert got.dtype is torch.uint8 and tuple(got.shape) == (v.shape[0], D, -(-Ht // 16), -(-Wt // 16)) and got.is_contiguous(), (i, name)
            assert torch.equal(got, want), (shape, i, name)
            if i > 0:   # a lone code at a corner of every block: no block is empty, and the block holds exactly that code
                assert int((got == 0).sum()) == 0, (shape, i, name)
    # only the alpha channel counts
    q = torch.zeros((1, 1, 4, Ht, Wt), dtype=torch.uint8)
    q[:, :, :3] = 255
    assert int(occupancy_reference(q).sum()) == 0


def test_synthetic_volumes_are_mostly_empty():
    """The shell's share of all-zero blocks grows with the resolution; the noise volume has none (the figures are printed: the tool's rows quote them)."""
    last = 0.0
    for S, Dp in ((64, 8), (256, 32)):
        blocks, hoods = C.empty_shares(C.volume("shell", S, Dp))
        print(f"shell {S}^2 x {Dp}: empty blocks {blocks:.3f}, empty 5 x 3 neighbourhoods {hoods:.3f}")
        assert 0.0 < hoods < blocks < 1.0 and blocks > last
        last = blocks
    assert C.empty_shares(C.volume("noise", 64, 8)) == (0.0, 0.0)
    blocks, hoods = C.empty_shares(C.volume("ramp", 64, 8))
    assert 0.0 < hoods < blocks < 1.0


def test_float_volumes_are_refused():
    from ml_gmpi_amd import build_occupancy, occupancy_reference, Occupancy
    f = torch.zeros((1, 2, 4, 16, 16))
    for fn in (build_occupancy, occupancy_reference):
        with pytest.raises(TypeError):
            fn(f)
        with pytest.raises(TypeError):
            fn(f.half())
    with pytest.raises(ValueError):
        occupancy_reference(torch.zeros((2, 3, 16, 16), dtype=torch.uint8))
    occ = Occupancy(torch.zeros((1, 2, 1, 1), dtype=torch.uint8), 16, None, (0, (1, 2, 4, 16, 16), (0, 0, 0, 0, 0), torch.device("cpu"), 0))
    with pytest.raises(TypeError):
        occ.check(f)


def _hand_made(q):
    from ml_gmpi_amd import Occupancy, occupancy_reference
    from ml_gmpi_amd.occupancy import _identity
    return Occupancy(occupancy_reference(q), 16, None, _identity(q))


def test_identity_mismatch_raises_before_any_launch():
    q = C.sparse_codes(5, (2, 3, 4, 20, 36))
    occ = _hand_made(q)
    occ.check(q)                                   # the volume itself
    occ.check(q.detach())                          # (what an autograd node hands on: same storage, same version counter)
    with pytest.raises(ValueError, match="another volume"):
        occ.check(q.clone())                       # another address
    with pytest.raises(ValueError, match="another volume"):
        occ.check(q[:1])                           # another shape
    with pytest.raises(ValueError, match="another volume"):
        occ.check(q.permute(0, 1, 2, 4, 3))        # other strides
    with pytest.raises(ValueError, match="another volume"):
        _hand_made(C.sparse_codes(6, (2, 3, 4, 40, 36))).check(q)   # a map of another volume's shape
    q[0, 0, 3, 0, 0] += 1                          # written in place since the build
    with pytest.raises(ValueError, match="stale"):
        occ.check(q)
    _hand_made(q).check(q)                         # rebuilt: accepted again
    # the MPIs of a batch: a view of the map under the identity of the slice
    part = _hand_made(q).of_mpis(q, 1, 2)
    part.check(q[1:2])
    assert torch.equal(part.map, _hand_made(q).map[1:2])
    with pytest.raises(ValueError):
        part.check(q)


def test_a_tensor_without_a_version_counter_is_accepted_unversioned():
    with torch.inference_mode():
        q = C.sparse_codes(7, (1, 2, 4, 16, 32)).clone()
    occ = _hand_made(q)
    assert occ.identity[4] is None
    occ.check(q)
    with pytest.raises(ValueError, match="another volume"):
        occ.check(q[:, :1])


def test_wrong_map_shape_or_block_is_refused():
    from ml_gmpi_amd import Occupancy
    from ml_gmpi_amd.occupancy import _identity
    q = C.sparse_codes(8, (1, 2, 4, 20, 36))
    with pytest.raises(ValueError, match="map must be"):
        Occupancy(torch.zeros((1, 2, 1, 3), dtype=torch.uint8), 16, None, _identity(q)).check(q)
    with pytest.raises(ValueError, match="map must be"):
        Occupancy(torch.zeros((1, 2, 3, 5), dtype=torch.uint8), 8, None, _identity(q)).check(q)


def test_entries_are_declared_and_refused_elsewhere():
    """The four C entries are exported and declared; the block size and the feature flag are gmpi_query values behind the ids in use; `MPI.forward` keeps
    the reference's signature, and the layout, layer, shaded and chunked entries have no such keyword."""
    import inspect
    import os
    from ml_gmpi_amd import MPI, ViewBatchDriver, _lib, load_library
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gmpi_render.h")).read()
    for name in ("gmpi_u8_occupancy_bytes", "gmpi_u8_occupancy_launch", "gmpi_mpi_render_u8_sparse_launch", "gmpi_render_u8_sparse_supports"):
        assert name in _lib.EXPORTS and name + "(" in header, name
    lib = load_library()
    assert lib.gmpi_query(52) == 1 and lib.gmpi_query(53) == 16 and lib.gmpi_query(54) == -1
    assert lib.gmpi_query(0) == _lib.ABI_VERSION
    assert "occupancy" in inspect.signature(MPI.render_views).parameters
    assert "occupancy" in inspect.signature(ViewBatchDriver.render_path).parameters and "occupancy" in inspect.signature(ViewBatchDriver.render_seeds).parameters
    for fn in (MPI.forward, MPI.render_views_layers, MPI.render_views_shaded, MPI.render_views_shared, MPI.render_views_depth):
        assert "occupancy" not in inspect.signature(fn).parameters, fn
    mpi = MPI()
    z = torch.zeros(1)
    with pytest.raises(TypeError):
        mpi.forward(batch_rgba=z, batch_dhw=z, batch_ray_dir=[z], batch_eye_pos=[z], batch_z_dir=[z], separate_background=None, occupancy=None)
    with pytest.raises(TypeError):
        mpi.chunked_render(z, z, z, z, occupancy=object())
    # the struct query without a device: a NULL map and a wrong block are refused by the existing codes, a float volume by its type
    p = _lib.GmpiRenderParams()
    import ctypes
    p.struct_size = ctypes.sizeof(_lib.GmpiRenderParams)
    assert lib.gmpi_u8_occupancy_bytes(ctypes.byref(p)) == 0
    p.M, p.D, p.Ht, p.Wt, p.rgba, p.rgba_dtype = 2, 3, 33, 68, 4096, _lib.DTYPE_U8
    p.rgba_stride[:] = (3 * 4 * 33 * 68, 4 * 33 * 68, 33 * 68, 68, 1)
    assert lib.gmpi_u8_occupancy_bytes(ctypes.byref(p)) == 2 * 3 * 3 * 5
    assert lib.gmpi_u8_occupancy_launch(ctypes.byref(p), None, None) == -1          # GMPI_E_NULL: no map
    p.rgba_dtype = _lib.DTYPE_F32
    assert lib.gmpi_u8_occupancy_bytes(ctypes.byref(p)) == 0 and lib.gmpi_u8_occupancy_launch(ctypes.byref(p), 4096, None) == -3   # GMPI_E_DTYPE
