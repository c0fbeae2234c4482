"""C ABI of the geometry backward, without a GPU: the header declares the two entry points as plain C, and the built library exports them."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_geometry_backward_as_plain_c(tmp_path):
    src = tmp_path / "g.c"
    src.write_text(
        '#include "gmpi_render.h"\n'
        "int main(void) {\n"
        "    int (*launch)(const GmpiRenderParams *, const float *, const float *, float *, float *, float *, float *, void *) =\n"
        "        gmpi_mpi_render_geometry_backward_launch;\n"
        "    uint64_t (*bytes)(const GmpiRenderParams *, int) = gmpi_render_geometry_backward_workspace_bytes;\n"
        "    return (launch == 0) + (bytes == 0) + (GMPI_E_WORKSPACE >= 0);\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "g.o")], check=True)


def test_library_exports_the_geometry_backward():
    from ml_gmpi_amd import _lib
    assert "gmpi_mpi_render_geometry_backward_launch" in _lib.EXPORTS
    assert "gmpi_render_geometry_backward_workspace_bytes" in _lib.EXPORTS
    if os.path.isfile(_lib.library_path()):
        import torch  # noqa: F401  (torch's ROCm runtime first, as the binding loads it)
        lib = ctypes.CDLL(_lib.library_path())
        assert hasattr(lib, "gmpi_mpi_render_geometry_backward_launch")
        assert hasattr(lib, "gmpi_render_geometry_backward_workspace_bytes")
