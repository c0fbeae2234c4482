"""The band kernel's DMA exec masks in closed form (ml-gmpi_amd/csrc/gmpi_band_masks.hpp) against their per-lane definition, on the host: a
stand-alone program (test_band_masks_cpu.cpp) built with the system C++ compiler enumerates every (items, rows, wave, pass) of every loader
geometry -- 11 * 16 * 4 * 3 cases for 16-bit volumes, 21 * 16 * 4 * 5 for fp32 ones, and the two other geometries the pixels-per-thread build
parameters allow -- once as a plain build and once under the address and undefined-behaviour sanitizers (shifts by 64 or negative counts, the
overflow of the 64-bit product)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def _build_and_run(tmp_path, name, extra):
    exe = os.path.join(tmp_path, name)
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(ROOT, "ml-gmpi_amd", "csrc"),
                    os.path.join(HERE, "test_band_masks_cpu.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    return subprocess.run([exe], capture_output=True, text=True, timeout=300)


@pytest.mark.skipif(CXX is None, reason="needs a C++ compiler")
def test_masks_equal_the_per_lane_definition_in_every_case(tmp_path):
    run = _build_and_run(str(tmp_path), "band_masks", [])
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"{11 * 16 * 4 * 3} cases" in run.stdout and f"{21 * 16 * 4 * 5} cases" in run.stdout, run.stdout
    assert run.stdout.rstrip().endswith("ok"), run.stdout


@pytest.mark.skipif(CXX is None, reason="needs a C++ compiler")
def test_masks_are_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    run = _build_and_run(str(tmp_path), "band_masks_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and run.stdout.rstrip().endswith("ok"), run.stdout + run.stderr
