"""Build-time guard of the band kernel's CARRY instances (render_band_chunk_kernel: the plane-chunked render through the band kernel), next to
tests/test_band_isa.py, which guards their one-shot twins.  The state's five loads per pixel sit in front of the plane loop and its stores behind it,
so the plane loop is the one-shot kernel's -- as long as the ten values more that live across it do not push an instance into scratch: a spill reloaded
in the plane loop is a vector memory operation on the DMA's counter.  Everything here is read from the code object's resource METADATA
(.vgpr_count, .vgpr_spill_count, .private_segment_fixed_size, .group_segment_fixed_size of the .amdgpu_metadata document) and through
tools/isa_pipe.py; no instruction text is searched for opcodes.

Budgets: no scratch at all; 16-bit instances 64 VGPRs (1024 threads, two workgroups per CU = 8 waves per SIMD), fp32 instances 128 (512 threads);
twice the LDS of a workgroup within a CU's 160 KiB."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = (".vgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _metadata(asm):
    """{kernel name: {field: value}} of the listing's .amdgpu_metadata document (one `- .agpr_count:` item per kernel)."""
    doc = asm[asm.index(".amdgpu_metadata"):asm.index(".end_amdgpu_metadata")]
    out = {}
    for item in re.split(r"\n  - \.agpr_count:", doc)[1:]:
        name = re.search(r"\n\s+\.name:\s+(\S+)", item).group(1)
        out[name] = {f: int(re.search(r"\n\s+" + re.escape(f) + r":\s+(\d+)", item).group(1)) for f in FIELDS}
    return out


@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_band_carry_kernels_have_no_scratch_and_fit_two_workgroups_per_cu(tmp_path):
    src = os.path.join(ROOT, "ml-gmpi_amd", "csrc", "render_band.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
             "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src)]   # = ml-gmpi_amd/csrc/Makefile
    mk = open(os.path.join(os.path.dirname(src), "Makefile")).read()
    for f in ("-ffp-contract=off", "-fno-slp-vectorize", "-O3"):
        assert f in mk, f"the Makefile no longer passes {f}: keep this test's flags in step with it"
    subprocess.run([HIPCC, *flags, "-save-temps", "-c", src, "-o", "render_band.o"], cwd=tmp_path, check=True, capture_output=True, timeout=900)
    asm = open(os.path.join(tmp_path, "render_band-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    meta = {n: m for n, m in _metadata(asm).items() if re.fullmatch(r"_ZN4gmpi4band24render_band_chunk_kernel\w+", n)}
    assert len(meta) == 24, sorted(meta)   # {bf16, fp16, fp32} x align_corners x strict order x range check
    assert not any(re.fullmatch(r"_ZN4gmpi4band18render_band_kernel\w+", n) for n in meta)   # (tests/test_band_isa.py counts the one-shot names)
    for name, m in sorted(meta.items()):
        print(name, m)
        assert "6CarryKE" in name, name   # the carry is a kernel argument of its own, not a member of KParams
        assert m[".vgpr_spill_count"] == 0, (name, m)
        assert m[".private_segment_fixed_size"] == 0, (name, m)
        fp32 = "render_band_chunk_kernelIf" in name
        assert m[".vgpr_count"] <= (128 if fp32 else 64), (name, m)
        assert 2 * m[".group_segment_fixed_size"] <= 160 * 1024, (name, m)
    # the software-pipelined taps: no instruction may touch the destination of an LDS read that is still in flight
    isa_pipe = _tool("isa_pipe")
    bodies = isa_pipe.kernel_bodies(asm, "render_band_chunk_kernel")
    assert sorted(bodies) == sorted(meta)
    piped = 0
    for name, body in bodies.items():
        assert isa_pipe.check(body, name) == [], name
        piped += isa_pipe.counted_waits(body) > 0
    assert piped == 12, piped   # the default-mode instances (storage type x align_corners x range check) are the pipelined ones
    shutil.rmtree(tmp_path, ignore_errors=True)
