"""compute_depth_ramp / LightRenderer.render_depth (the shading augmentation of the depth-alpha layout) without a GPU: the two C entries in the
header, the binding and the library; every refusal of the entries through raw ctypes (all return before a launch: the pointers are never
followed); the Python refusals; the GPU tests' float64 chain against the oracle; the new kernels' descriptors."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _ramp_cases as rc
from test_depth_alpha_cpu import HIPCC, ROOT

FWD, BWD = "gmpi_ramp_depth_launch", "gmpi_ramp_depth_backward_launch"


def test_header_declares_both_entries_as_plain_c(tmp_path):
    src = tmp_path / "r.c"
    src.write_text(
        '#include "gmpi_render.h"\n'
        "int main(void) {\n"
        "    int (*fwd)(const void *, int32_t, int64_t, int64_t, const GmpiDepthAlpha *, const float *, int32_t, int32_t, int32_t, int32_t, float *,\n"
        "               float *, void *) = gmpi_ramp_depth_launch;\n"
        "    int (*bwd)(const void *, int32_t, int64_t, int64_t, const GmpiDepthAlpha *, const float *, const float *, const float *, const float *,\n"
        "               float *, int64_t, int64_t, int32_t, int32_t, int32_t, int32_t, void *) = gmpi_ramp_depth_backward_launch;\n"
        "    return (fwd == 0) + (bwd == 0);\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "r.o")], check=True)


def test_binding_and_library_carry_both_entries_and_the_query():
    from ml_gmpi_amd import _lib
    assert FWD in _lib.EXPORTS and BWD in _lib.EXPORTS
    assert _lib.ABI_VERSION == 2 and ctypes.sizeof(_lib.GmpiRenderParams) == 184 and ctypes.sizeof(_lib.GmpiDepthAlpha) == 40
    lib = _lib.load_library()
    assert hasattr(lib, FWD) and hasattr(lib, BWD)
    assert len(lib.gmpi_ramp_depth_launch.argtypes) == 13 and len(lib.gmpi_ramp_depth_backward_launch.argtypes) == 17
    assert lib.gmpi_query(32) == 1 and lib.gmpi_query(31) == -1 and lib.gmpi_query(33) == -1 and lib.gmpi_query(0) == 2


def test_entries_refuse_bad_arguments_before_any_launch():
    from ml_gmpi_amd import _lib as L
    lib = L.load_library()
    host = np.zeros(64, dtype=np.float32)
    fake = host.ctypes.data   # (a non-NULL address)
    NULL, SHAPE, DTYPE, STRIDE, ABI = -1, -2, -3, -4, -5
    Wd = 8

    def ramp(lo=-0.25, hi=0.25, den=0.5):
        d = L.GmpiDepthAlpha()
        d.struct_size = ctypes.sizeof(L.GmpiDepthAlpha)
        d.plane_z, d.plane_z_stride, d.z_lo, d.z_hi, d.z_den = fake, 0, lo, hi, den
        return d

    ref = lambda x: None if x is None else ctypes.byref(x)
    base = dict(image=fake, dtype=L.DTYPE_F32, sb=32, sr=Wd, ramp=ramp(), ds=fake, T=None, gz=fake, gt=fake, out=fake, gsb=32, gsr=Wd, B=1, D=3, H=4, W=Wd)
    seen = []

    def fwd(**kw):
        a = dict(base, **kw)
        return lib.gmpi_ramp_depth_launch(a["image"], a["dtype"], a["sb"], a["sr"], ref(a["ramp"]), a["ds"], a["B"], a["D"], a["H"], a["W"], a["out"], None, None)

    def bwd(**kw):
        a = dict(base, **kw)
        return lib.gmpi_ramp_depth_backward_launch(a["image"], a["dtype"], a["sb"], a["sr"], ref(a["ramp"]), a["ds"], a["T"], a["gz"], a["gt"], a["out"],
                                                   a["gsb"], a["gsr"], a["B"], a["D"], a["H"], a["W"], None)

    def both(want, **kw):
        got = (fwd(**kw), bwd(**kw))
        seen.append(got)
        assert got == (want, want), (kw, got, want)

    both(0, B=0)                                                       # no images: nothing to launch
    for name in ("image", "ramp", "ds", "out"):                        # (out: depth_out / grad_depth_image)
        both(NULL, **{name: None})
    d = ramp(); d.plane_z = None
    both(NULL, ramp=d)
    for lo, hi, den in ((0.25, 0.25, 0.5), (0.3, 0.25, 0.5), (-0.25, 0.25, 0.0), (-0.25, 0.25, -0.5), (float("nan"), 0.25, 0.5),
                        (-0.25, float("nan"), 0.5), (-0.25, 0.25, float("nan"))):
        both(SHAPE, ramp=ramp(lo, hi, den))
    for kw in (dict(D=0), dict(D=-1), dict(H=0), dict(W=0), dict(B=-1), dict(B=65536), dict(H=65536)):
        both(SHAPE, **kw)
    d = ramp(); d.plane_z_stride = -3
    both(STRIDE, ramp=d)
    both(STRIDE, sb=-1)
    both(STRIDE, sr=Wd - 1)
    assert bwd(gsb=0) == STRIDE and bwd(gsb=-32) == STRIDE and bwd(gsr=Wd - 1) == STRIDE
    both(DTYPE, dtype=L.DTYPE_U8)
    both(DTYPE, dtype=7)
    both(DTYPE, dtype=-1)
    for delta in (8, -8):
        d = ramp(); d.struct_size += delta
        both(ABI, ramp=d)
    # what gmpi_mpi_render_depth_launch returns for that struct
    p = L.GmpiRenderParams()
    p.struct_size = ctypes.sizeof(L.GmpiRenderParams)
    s = L.GmpiSharedColor()
    s.struct_size = ctypes.sizeof(L.GmpiSharedColor)
    assert lib.gmpi_mpi_render_depth_launch(ctypes.byref(p), ctypes.byref(s), ctypes.byref(d), None) == ABI
    assert bwd(gz=None, gt=None) == 0                                  # both upstream gradients NULL: nothing is added
    assert bwd(gz=None, gt=None, out=None) == NULL and bwd(gz=None, gt=None, gsr=Wd - 1) == STRIDE   # ... but the arguments are still checked
    both(0, B=0, sb=0)
    assert len(seen) >= 28


def test_python_refusals():
    from ml_gmpi_amd import GmpiError, LightRenderer, compute_depth_ramp
    pz, ds = rc.plane_tables(4)
    depth = torch.rand((2, 1, 6, 8))
    with pytest.raises(TypeError, match="uint8"):
        compute_depth_ramp((depth * 255).to(torch.uint8), pz, -0.25, 0.25, ds)
    with pytest.raises(GmpiError, match="ROCm device"):
        compute_depth_ramp(depth, pz, -0.25, 0.25, ds)
    with pytest.raises(GmpiError, match="ROCm device"):
        compute_depth_ramp(depth.clone().requires_grad_(True), pz, -0.25, 0.25, ds, want_transmittance=True)
    with pytest.raises(NotImplementedError, match="plane_z"):
        compute_depth_ramp(depth, pz.clone().requires_grad_(True), -0.25, 0.25, ds)
    with pytest.raises(NotImplementedError, match="plane_ds"):
        compute_depth_ramp(depth, pz, -0.25, 0.25, ds.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="z_lo"):
        compute_depth_ramp(depth, pz, torch.tensor(-0.25, requires_grad=True), 0.25, ds)
    with torch.no_grad():   # (no graph is asked for: the CPU tensor is what is refused)
        with pytest.raises(GmpiError):
            compute_depth_ramp(depth, pz.clone().requires_grad_(True), -0.25, 0.25, ds)
    for bad in (depth[:, 0], depth.expand(2, 3, 6, 8), depth[None]):
        with pytest.raises(AssertionError, match="Expected depth"):
            compute_depth_ramp(bad, pz, -0.25, 0.25, ds)
    for bad in (pz.reshape(1, 1, 4), torch.stack([pz] * 3)):
        with pytest.raises(AssertionError, match="Expected plane_z"):
            compute_depth_ramp(depth, bad, -0.25, 0.25, ds)
    # LightRenderer.render_depth: the same rules, plus the colour images'
    L = LightRenderer(sphere_center_z=1.0, sphere_r=1.0)
    rgb, dhw, xyz = torch.rand((2, 3, 6, 8)), torch.ones((4, 3)), torch.zeros((4, 6, 8, 3))
    kw = dict(plane_z=pz, z_range=1.0, n_z_bins=4)
    with pytest.raises(TypeError, match="uint8"):
        L.render_depth((rgb * 255).to(torch.uint8), depth, dhw, xyz, **kw)
    with pytest.raises(TypeError, match="uint8"):
        L.render_depth(rgb, depth, dhw, xyz, background=(rgb * 255).to(torch.uint8), **kw)
    with pytest.raises(GmpiError, match="ROCm device"):
        L.render_depth(rgb, depth, dhw, xyz, **kw)
    assert L.step == -1   # a refused call does not advance the schedule


def test_check_keeps_its_rules_for_the_colour_images():
    """depth_alpha._check (what render_depth applies once the tensors are on a device) still refuses what it refused before `_check_depth` was
    split off for compute_depth_ramp."""
    from ml_gmpi_amd.depth_alpha import _check
    pz = rc.plane_tables(4)[0]
    depth, rgb = torch.rand((2, 1, 6, 8)), torch.rand((2, 3, 6, 8))
    _check(rgb, depth, pz, rgb)
    for args in ((rgb[:, :2], depth, pz, None), (rgb, depth, pz, rgb[:1]), (rgb, depth[:, 0], pz, None), (rgb, depth, torch.stack([pz] * 3), None)):
        with pytest.raises(AssertionError, match="Expected"):
            _check(*args)


@pytest.mark.parametrize("n_z_bins", [4, 32, 256])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_float64_chain_agrees_with_the_oracle_on_the_planes(n_z_bins, dtype):
    """The yardstick of the GPU tests' backward, pinned without a GPU: the float64 chain on the stored values with the fp32-rounded constants against
    oracle.alpha_depth(depth_alpha_planes(...)), to 2e-6; and the split of the base case the GPU tests rely on."""
    from test_hip_depth_alpha import _bounds
    lo, hi = _bounds(n_z_bins)
    pz, ds = rc.plane_tables()
    for reach in (None, 1.35):
        depth = rc.depth_image(n_z_bins, dtype, reach)
        z64, t64 = rc.ramp_chain(depth, pz, lo, hi, ds)
        z, t = rc.oracle_reference(depth, pz, lo, hi, ds)
        ez, et = float(np.abs(z64.numpy() - z).max()), float(np.abs(t64.numpy() - t).max())
        opaque = float((t < 1e-30).mean())
        print(f"n_z_bins {n_z_bins} {dtype} reach {reach}: |chain64 - oracle| depth {ez:.2e} T {et:.2e}; T_out < 1e-30 on {opaque:.0%} of the texels")
        assert ez <= 2e-6 and et <= 2e-6, (ez, et)
        if reach is None and n_z_bins != 32:
            assert 0.25 <= opaque <= 0.75, opaque   # both the re-walk and the direct start of the backward's sweep are exercised


@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_ramp_kernels_have_no_scratch_and_no_lds(tmp_path):
    csrc = os.path.join(ROOT, "ml-gmpi_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
             "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]   # = ml-gmpi_amd/csrc/Makefile
    mk = open(os.path.join(csrc, "Makefile")).read()
    for f in ("-ffp-contract=off", "-fno-slp-vectorize", "-O3", "light_kernels.hip"):
        assert f in mk, f"the Makefile no longer has {f}: keep this test in step with it"
    res = subprocess.run([HIPCC, *flags, "-save-temps", "-c", os.path.join(csrc, "light_kernels.hip"), "-o", "light_kernels.o"], cwd=tmp_path,
                         capture_output=True, timeout=900)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    asm = open(os.path.join(tmp_path, "light_kernels-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    kernels = {}
    for name, meta in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel", asm, flags=re.M | re.S):   # the descriptors only
        field = lambda key: int(re.search(r"\.amdhsa_" + key + r"\s+(\d+)", meta).group(1))
        kernels[name] = (field("private_segment_fixed_size"), field("group_segment_fixed_size"))
    ramp = {n: v for n, v in kernels.items() if "ramp_depth_kernel" in n or "ramp_depth_backward_kernel" in n}
    assert len(ramp) == 6, sorted(kernels)   # forward and backward x 3 storage types
    for name, (scratch, lds) in sorted(ramp.items()):
        print(name, "scratch", scratch, "lds", lds)
        assert scratch == 0 and lds == 0, (name, scratch, lds)
    shutil.rmtree(tmp_path, ignore_errors=True)
