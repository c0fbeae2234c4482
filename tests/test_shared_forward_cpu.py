"""The staged shared-colour forward without a GPU: the new C entry in the binding and the header, the pinned ABI, and the register budget of
render_shared_forward.hip."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_binding_lists_the_support_query_and_keeps_the_abi():
    from ml_gmpi_amd import _lib
    assert "gmpi_render_shared_supports" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 2 and ctypes.sizeof(_lib.GmpiRenderParams) == 184 and ctypes.sizeof(_lib.GmpiSharedColor) == 72
    assert _lib.VARIANTS["lds"] == _lib.VARIANT_LDS == 2
    if os.path.isfile(_lib.library_path()):
        import torch  # noqa: F401  (torch's ROCm runtime first, as the binding loads it)
        lib = ctypes.CDLL(_lib.library_path())
        assert hasattr(lib, "gmpi_render_shared_supports")
        lib.gmpi_query.restype, lib.gmpi_query.argtypes = ctypes.c_int, [ctypes.c_int32]
        assert lib.gmpi_query(0) == 2 and lib.gmpi_query(1) == 184
        tile_w, cap_w, cap_h = lib.gmpi_query(12), lib.gmpi_query(13), lib.gmpi_query(14)
        assert tile_w > 0 and 512 % tile_w == 0 and cap_w > tile_w and cap_h > 512 // tile_w, (tile_w, cap_w, cap_h)
        assert lib.gmpi_query(15) == -1


def test_header_declares_the_support_query_as_plain_c(tmp_path):
    src = tmp_path / "s.c"
    src.write_text(
        '#include "gmpi_render.h"\n'
        "int main(void) {\n"
        "    int (*sup)(const GmpiRenderParams *, const GmpiSharedColor *) = gmpi_render_shared_supports;\n"
        "    return (sup == 0) + (GMPI_ABI_VERSION != 2) + (sizeof(GmpiRenderParams) != 184) + (sizeof(GmpiSharedColor) != 72) + (GMPI_VARIANT_LDS != 2);\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "s.o")], check=True)


def test_driver_methods_exist_and_share_their_bodies():
    import inspect
    from ml_gmpi_amd import ViewBatchDriver
    sig = inspect.signature(ViewBatchDriver.render_path_shared)
    assert list(sig.parameters)[1:] == ["rgb", "alpha", "render_size", "yaws", "pitches", "background", "indices", "to_uint8", "depth_range",
                                        "want_transmittance", "to_host", "variant"]
    sig = inspect.signature(ViewBatchDriver.render_seeds_shared)
    assert list(sig.parameters)[1:] == ["rgb", "alpha", "render_size", "background", "views_per_mpi", "variant", "render_kwargs"]
    for shared, plain in (("render_path_shared", "render_path"), ("render_seeds_shared", "render_seeds")):
        a, b = inspect.getsource(getattr(ViewBatchDriver, shared)), inspect.getsource(getattr(ViewBatchDriver, plain))
        helper = "_" + plain
        assert helper in a and helper in b, (shared, plain)   # one body for both


def test_the_product_imports_nothing_from_the_oracle():
    pkg = os.path.join(ROOT, "ml-gmpi_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp")) or f == "Makefile":
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", text, flags=re.M), f
                assert not re.search(r"^\s*#\s*include.*oracle", text, flags=re.M), f


@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_staged_forward_compiles_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "ml-gmpi_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
             "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]   # = ml-gmpi_amd/csrc/Makefile
    mk = open(os.path.join(csrc, "Makefile")).read()
    for f in ("-ffp-contract=off", "-fno-slp-vectorize", "-O3", "render_shared_forward.hip"):
        assert f in mk, f"the Makefile no longer has {f}: keep this test in step with it"
    res = subprocess.run([HIPCC, *flags, "-save-temps", "-c", os.path.join(csrc, "render_shared_forward.hip"), "-o", "render_shared_forward.o"],
                         cwd=tmp_path, capture_output=True, timeout=900)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    asm = open(os.path.join(tmp_path, "render_shared_forward-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    seen = set()
    for name in sorted(set(re.findall(r"^(_Z\w*render_shared_forward_kernel\w*):", asm, flags=re.M))):
        meta = asm[asm.index(".amdhsa_kernel " + name):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1)) == 0, name
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", meta).group(1))
        assert lds <= 53 * 1024, (name, lds)   # three workgroups per CU
        seen.add(name)
    assert len(seen) >= 12, sorted(seen)   # 3 storage types x align_corners x order
