"""The tile backward of the depth-alpha layout without a GPU: what `hip_mpi` hands the new C entry (the recorder of test_depth_alpha_cpu), the
entry's argument errors on the host, its declaration, and the resources of the new kernels read from their kernel descriptors."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_depth_alpha_cpu import DEPTH_ENTRIES, HIPCC, ROOT, depth_inputs, rec  # noqa: F401  (rec: the recorder fixture)
from test_marshal_cpu import loss_of

PIXEL, TILE = "gmpi_mpi_render_depth_backward_launch", "gmpi_mpi_render_depth_backward_tile_launch"


@pytest.fixture
def rec2(rec):
    """The recorder of test_depth_alpha_cpu, which also knows the new entry."""
    rec.entries = tuple(rec.entries) + (TILE,)
    return rec


def _record(rec, uses_T, background, dtype=torch.float32, **kw):
    from ml_gmpi_amd.hip_mpi import MPI
    rgb, depth, pz, bg, geo = depth_inputs(dtype, background, per_mpi_table=True)
    for t in (rgb, depth, bg):
        if t is not None:
            t.requires_grad_(True)
    del rec.calls[:]
    res = MPI().render_views_depth(rgb, depth, pz, (-2 / 10, 2 / 10), *geo, background=bg, want_transmittance=True, **kw)
    loss_of(res, uses_T).backward()
    fwd, bwd = rec.calls
    return fwd, bwd, (rgb, depth, bg)


@pytest.mark.parametrize("uses_T", [False, True])
@pytest.mark.parametrize("background", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tile_backward_records_the_new_entry_with_the_default_paths_structs(rec2, dtype, background, uses_T):
    fwd_p, bwd_p, ins_p = _record(rec2, uses_T, background, dtype)
    fwd_e, bwd_e, _ = _record(rec2, uses_T, background, dtype, depth_backward="pixel")
    fwd_t, bwd_t, ins_t = _record(rec2, uses_T, background, dtype, depth_backward="tile")
    assert (fwd_p.name, bwd_p.name) == DEPTH_ENTRIES == (fwd_e.name, bwd_e.name)       # the default path is today's
    assert (fwd_t.name, bwd_t.name) == (DEPTH_ENTRIES[0], TILE)
    assert len(bwd_t.args) == len(bwd_p.args) == 13

    def scalars(p):   # the struct without its addresses (every run has its own tensors)
        from test_marshal_cpu import scalars_of
        return scalars_of(p)
    assert scalars(bwd_t.args[0]) == scalars(bwd_p.args[0]) == scalars(bwd_e.args[0]) and scalars(fwd_t.args[0]) == scalars(fwd_p.args[0])
    # the three structs of the backward are byte-equal to those of the forward of the same run, as on the default path (addresses included)
    for fwd, bwd in ((fwd_p, bwd_p), (fwd_t, bwd_t)):
        assert bytes(bwd.args[1]) == bytes(fwd.args[1]) and bytes(bwd.args[2]) == bytes(fwd.args[2])
        f, b = fwd.args[0], bwd.args[0]
        for name in ("rgba", "view_to_mpi", "dhw", "ray_dir", "eye_pos", "z_dir", "transmittance_out"):
            assert getattr(b, name) == getattr(f, name), name
        assert (b.flags, b.variant, b.rgba_dtype, list(b.rgba_stride)) == (f.flags, f.variant, f.rgba_dtype, list(f.rgba_stride))
    # the same inputs (depth_inputs is seeded) give byte-equal ramp structs up to the table's address, and byte-equal stride fields
    for i in (1, 2):
        a, b = bwd_p.args[i], bwd_t.args[i]
        assert a.struct_size == b.struct_size and ctypes.sizeof(a) == ctypes.sizeof(b)
    assert (bwd_t.args[2].z_lo, bwd_t.args[2].z_hi, bwd_t.args[2].z_den, bwd_t.args[2].plane_z_stride) == \
           (bwd_p.args[2].z_lo, bwd_p.args[2].z_hi, bwd_p.args[2].z_den, bwd_p.args[2].plane_z_stride)
    assert list(bwd_t.args[1].rgb_stride) == list(bwd_p.args[1].rgb_stride) and list(bwd_t.args[1].background_stride) == list(bwd_p.args[1].background_stride)
    # gradient pointers and strides: the same pattern
    for i in (3, 4, 5, 6, 8, 10):
        assert (bwd_t.args[i] is None) == (bwd_p.args[i] is None), i
    assert (bwd_t.args[5] is not None) == uses_T and bwd_t.args[-1] == 0
    for i in (7, 9, 11):
        assert bwd_t.args[i] == bwd_p.args[i], i
    assert bwd_t.args[7] == [144, 48, 8] and bwd_t.args[9] == [48, 48, 8] and (bwd_t.args[11] == [144, 48, 8] if background else bwd_t.args[11] is None)
    for t in ins_t:
        assert t is None or (t.grad.shape == t.shape and t.grad.dtype == dtype)


def test_one_run_hands_both_entries_byte_equal_structs(rec2):
    """Two backward passes over ONE graph cannot be recorded (the entry is fixed at the forward), so: the same tensors rendered twice."""
    from ml_gmpi_amd.hip_mpi import MPI
    rgb, depth, pz, bg, geo = depth_inputs(torch.float32, True)
    depth.requires_grad_(True)
    recs = []
    for how in ("pixel", "tile"):
        del rec2.calls[:]
        res = MPI().render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg, depth_backward=how)
        res["color"].sum().backward()
        recs.append(rec2.calls[1])
    a, b = recs
    assert (a.name, b.name) == (PIXEL, TILE)
    for i in (1, 2):   # GmpiSharedColor, GmpiDepthAlpha: the same tensors, byte for byte
        assert bytes(a.args[i]) == bytes(b.args[i]), i
    pa, pb = a.args[0], b.args[0]
    for name, _ in pa._fields_:   # GmpiRenderParams: every field but the node's private transmittance buffer
        if name != "transmittance_out":
            va, vb = getattr(pa, name), getattr(pb, name)
            assert (list(va) if isinstance(va, ctypes.Array) else va) == (list(vb) if isinstance(vb, ctypes.Array) else vb), name
    assert a.args[6] is None and a.args[10] is None and b.args[6] is None and b.args[10] is None and b.args[8] is not None and a.args[9] == b.args[9]


def test_unknown_name_is_refused_before_any_call(rec2):
    from ml_gmpi_amd import make_renderer
    from ml_gmpi_amd.hip_mpi import MPI
    rgb, depth, pz, bg, geo = depth_inputs()
    depth.requires_grad_(True)
    for name in ("tiles", "lds", "", None, 1):
        with pytest.raises(ValueError, match="depth_backward"):
            MPI().render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, background=bg, depth_backward=name)
    # variant= keeps its refusals next to the new argument
    with pytest.raises(ValueError, match="not built"):
        MPI().render_views_depth(rgb, depth, pz, (-0.2, 0.2), *geo, variant="lds", depth_backward="tile")
    r = make_renderer("FFHQ", n_planes=4, device=torch.device("cpu"), ray_backend="torch")
    g = torch.Generator().manual_seed(0)
    with pytest.raises(ValueError, match="depth_backward"):
        r.render_depth(torch.rand((1, 3, 8, 8), generator=g), torch.rand((1, 1, 8, 8), generator=g), 8, 8, z_range=1, n_z_bins=4, depth_backward="box")
    assert rec2.calls == []


def test_renderer_passes_the_argument_through(rec2):
    from ml_gmpi_amd import make_renderer
    r = make_renderer("FFHQ", n_planes=4, device=torch.device("cpu"), ray_backend="torch")
    g = torch.Generator().manual_seed(0)
    rgb, depth = torch.rand((1, 3, 8, 8), generator=g), torch.rand((1, 1, 8, 8), generator=g).requires_grad_(True)
    for how, want in ((None, PIXEL), ("pixel", PIXEL), ("tile", TILE)):
        del rec2.calls[:]
        torch.manual_seed(0)
        out = r.render_depth(rgb, depth, 8, 8, z_range=1, n_z_bins=4, **({} if how is None else {"depth_backward": how}))
        out[0].sum().backward()
        assert [c.name for c in rec2.calls if "backward" in c.name] == [want], how


# ---- the C entry on the host -------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_tile_entry_as_plain_c(tmp_path):
    src = tmp_path / "d.c"
    src.write_text(
        '#include "gmpi_render.h"\n'
        "typedef int (*bwd_t)(const GmpiRenderParams *, const GmpiSharedColor *, const GmpiDepthAlpha *, const float *, const float *, const float *, float *,\n"
        "                     const int64_t *, float *, const int64_t *, float *, const int64_t *, void *);\n"
        "int main(void) {\n"
        "    bwd_t pixel = gmpi_mpi_render_depth_backward_launch, tile = gmpi_mpi_render_depth_backward_tile_launch;\n"
        "    return (pixel == 0) + (tile == 0) + (GMPI_ABI_VERSION != 2) + (sizeof(GmpiRenderParams) != 184) + (sizeof(GmpiSharedColor) != 72)\n"
        "           + (sizeof(GmpiDepthAlpha) != 40);\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "d.o")], check=True)


def test_library_exports_the_tile_entry_and_keeps_the_abi():
    from ml_gmpi_amd import _lib
    assert TILE in _lib.EXPORTS and PIXEL in _lib.EXPORTS
    assert _lib.ABI_VERSION == 2 and ctypes.sizeof(_lib.GmpiRenderParams) == 184 and ctypes.sizeof(_lib.GmpiSharedColor) == 72
    assert ctypes.sizeof(_lib.GmpiDepthAlpha) == 40
    lib = _lib.load_library()
    assert list(lib.gmpi_mpi_render_depth_backward_tile_launch.argtypes) == list(lib.gmpi_mpi_render_depth_backward_launch.argtypes)


def test_argument_error_codes_and_the_query_on_the_host():
    """test_depth_alpha_cpu's table, applied to the new entry and, side by side, to the one-pixel entry: the same code for the same arguments.
    Every call is refused (or has no views) before anything is launched: no device is needed, the pointers are never followed."""
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    assert lib.gmpi_query(23) == 128 and lib.gmpi_query(22) == 1 and lib.gmpi_query(21) == -1 and lib.gmpi_query(24) == -1 and lib.gmpi_query(0) == 2
    host = np.zeros(64, dtype=np.float32)
    fake = host.ctypes.data   # (a non-NULL address)

    def params(N=1):
        p = L.GmpiRenderParams()
        p.struct_size = ctypes.sizeof(L.GmpiRenderParams)
        p.flags, p.variant, p.rgba_dtype = L.FLAG_ALIGN_CORNERS, L.VARIANT_AUTO, L.DTYPE_F32
        p.N, p.M, p.D, p.Ht, p.Wt, p.H, p.W, p.views_per_mpi = N, 1, 3, 4, 4, 4, 4, 1
        p.rgba = fake
        p.rgba_stride[:] = [16, 0, 0, 4, 1]   # [1], [2]: ignored
        p.dhw = p.ray_dir = p.eye_pos = p.z_dir = p.rgb_out = p.depth_out = fake
        return p

    def shared(with_bg=True):
        s = L.GmpiSharedColor()
        s.struct_size = ctypes.sizeof(L.GmpiSharedColor)
        s.rgb, s.background = fake, (fake if with_bg else None)
        s.rgb_stride[:] = [48, 16, 4]
        s.background_stride[:] = [48, 16, 4]
        return s

    def ramp(lo=-0.25, hi=0.25, den=0.5):
        d = L.GmpiDepthAlpha()
        d.struct_size = ctypes.sizeof(L.GmpiDepthAlpha)
        d.plane_z, d.plane_z_stride, d.z_lo, d.z_hi, d.z_den = fake, 0, lo, hi, den
        return d

    ref = lambda x: None if x is None else ctypes.byref(x)
    s3 = (ctypes.c_int64 * 3)(48, 16, 4)
    seen = []

    def bwd(p, s, d, go=fake, gr=fake, gd=fake, gb=fake, gds=s3):
        """Both entries; they must agree.  Returns the tile entry's code."""
        rc = [fn(ref(p), ref(s), ref(d), go, None, None, gr, s3, gd, gds, gb, s3, None)
              for fn in (lib.gmpi_mpi_render_depth_backward_tile_launch, lib.gmpi_mpi_render_depth_backward_launch)]
        assert rc[0] == rc[1], rc
        seen.append(rc[0])
        return rc[0]

    call = bwd
    assert call(params(N=0), shared(), ramp()) == 0                                              # no views: nothing to launch
    assert call(None, shared(), ramp()) == -1 and call(params(), None, ramp()) == -1 and call(params(), shared(), None) == -1   # GMPI_E_NULL
    d = ramp(); d.plane_z = None
    assert call(params(), shared(), d) == -1
    s = shared(); s.rgb = None
    assert call(params(), s, ramp()) == -1
    p = params(); p.rgba = None
    assert call(p, shared(), ramp()) == -1
    p = params(); p.rgba_dtype = L.DTYPE_U8
    assert call(p, shared(), ramp()) == -3                                                       # GMPI_E_DTYPE
    for lo, hi, den in ((0.25, 0.25, 0.5), (0.3, 0.25, 0.5), (-0.25, 0.25, 0.0), (-0.25, 0.25, -0.5), (float("nan"), 0.25, 0.5)):
        assert call(params(), shared(), ramp(lo, hi, den)) == -2, (lo, hi, den)                  # bad bounds: GMPI_E_SHAPE
    d = ramp(); d.plane_z_stride = -3
    assert call(params(), shared(), d) == -4                                                     # GMPI_E_STRIDE
    p = params(); p.rgba_stride[4] = 2
    assert call(p, shared(), ramp()) == -4
    d = ramp(); d.struct_size += 8
    assert call(params(), shared(), d) == -5                                                     # GMPI_E_ABI
    p = params(); p.struct_size -= 8
    assert call(p, shared(), ramp()) == -5
    for v in (L.VARIANT_LDS, L.VARIANT_WAVE, L.VARIANT_DMA, L.VARIANT_BAND, 9):
        p = params(); p.variant = v
        assert call(p, shared(), ramp()) == -6, v                                                # GMPI_E_VARIANT
    p = params(); p.flags |= 1 << 30
    assert call(p, shared(), ramp()) == -7                                                       # GMPI_E_FLAGS
    p = params(N=0); p.variant = L.VARIANT_GATHER
    assert call(p, shared(), ramp()) == 0
    p = params(N=0); p.D = 129                                                                   # (more planes than the tile kernel takes: no error)
    assert call(p, shared(), ramp()) == 0
    p = params(); p.rgb_out = p.depth_out = None
    assert bwd(p, shared(), ramp(), go=None) == -1                                                   # the backward needs no outputs, but the upstream gradient
    assert bwd(p, shared(), ramp(), gr=None, gd=None, gb=None) == -1                                 # all three NULL
    assert bwd(p, shared(with_bg=False), ramp()) == -1                                               # a background gradient without a background
    assert bwd(p, shared(), ramp(), gds=None) == -1                                                  # a gradient without its strides
    assert bwd(p, shared(), ramp(), gds=(ctypes.c_int64 * 3)(16, 0, 3)) == -4                        # rows overlap
    p0 = params(N=0); p0.rgb_out = p0.depth_out = None
    assert bwd(p0, shared(), ramp(), gr=None, gb=None) == 0 and bwd(p0, shared(with_bg=False), ramp(), gb=None) == 0
    p = params(N=65536)
    assert bwd(p, shared(), ramp()) == -2                                                            # the view index is a grid dimension
    assert len(seen) >= 30


# ---- the kernels' resources, from their descriptors ----------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_tile_kernels_have_no_scratch_and_two_workgroups_of_lds(tmp_path):
    csrc = os.path.join(ROOT, "ml-gmpi_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
             "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]   # = ml-gmpi_amd/csrc/Makefile
    mk = open(os.path.join(csrc, "Makefile")).read()
    for f in ("-ffp-contract=off", "-fno-slp-vectorize", "-O3", "render_depth_tile.hip", "render_depth.hip"):
        assert f in mk, f"the Makefile no longer has {f}: keep this test in step with it"
    res = subprocess.run([HIPCC, *flags, "-save-temps", "-c", os.path.join(csrc, "render_depth_tile.hip"), "-o", "render_depth_tile.o"], cwd=tmp_path,
                         capture_output=True, timeout=900)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    asm = open(os.path.join(tmp_path, "render_depth_tile-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    kernels = {}
    for name, meta in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel", asm, flags=re.M | re.S):   # the descriptors only
        field = lambda key: int(re.search(r"\.amdhsa_" + key + r"\s+(\d+)", meta).group(1))
        kernels[name] = (field("private_segment_fixed_size"), field("group_segment_fixed_size"))
    tile = {n: v for n, v in kernels.items() if "render_depth_tile_kernel" in n}
    assert len(tile) == 6 and len(kernels) == 6, sorted(kernels)   # 3 storage types x align_corners, and nothing else in the file
    for name, (scratch, lds) in sorted(tile.items()):
        print(name, "scratch", scratch, "lds", lds)
        assert scratch == 0, (name, scratch)
        assert 65536 <= lds <= 81920, (name, lds)   # the 64 KiB window is there; two workgroups fit the 160 KB of a CU
    shutil.rmtree(tmp_path, ignore_errors=True)
