"""The transmittance gradient without a GPU: the float64 oracle of tests/_transmittance_ref.py against the geometry oracle, the fp32 C oracle,
finite differences and the closed form dT/da_k = -T / om_k; the C ABI of the `_ex` backward entries; and no scratch in the backward sweeps."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
import _transmittance_ref as tr
from _geometry_ref import geometry_render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _cam(N, H, W, seed=0, tilt=0.3):
    g = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.linspace(-0.11, 0.11, H), np.linspace(-0.11, 0.11, W), indexing="ij")
    rays, eyes, zds = [], [], []
    for _ in range(N):
        a = tilt * (g.random() - 0.5) * 2
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        d = np.stack([xs, ys, np.ones_like(xs)]).reshape(3, -1)
        d = d / np.linalg.norm(d, axis=0)
        rays.append((R @ d).reshape(3, H, W))
        eyes.append([-np.sin(a), 0.0, 1 - np.cos(a)])
        zds.append(R[:, 2])
    return np.stack(rays).astype(np.float32), np.array(eyes, np.float32), np.array(zds, np.float32)


def _dhw(M, D, near=0.95, far=1.12, ext=0.25, last=0.5):
    d = 1.0 / np.linspace(1 / near, 1 / far, D)
    t = np.stack([d, np.full(D, ext), np.full(D, ext)], 1)
    t[-1, 1:] = last
    return np.broadcast_to(t[None], (M, D, 3)).astype(np.float32).copy()


def _smooth_rgba(seed, shape):
    M, D, C, Ht, Wt = shape
    g = torch.Generator().manual_seed(seed)
    coarse = 0.25 + 0.5 * torch.rand((M * D, C, 5, 5), generator=g, dtype=torch.float64)
    coarse[:, 3] = 0.1 + 0.5 * coarse[:, 3]
    fine = F.interpolate(coarse, size=(Ht, Wt), mode="bicubic", align_corners=True).clamp(0, 1)
    win = torch.sin(np.pi * (torch.arange(Ht, dtype=torch.float64) + 0.5) / Ht)[:, None] * \
        torch.sin(np.pi * (torch.arange(Wt, dtype=torch.float64) + 0.5) / Wt)[None, :]
    return (fine * win ** 2).reshape(M, D, C, Ht, Wt).float().numpy()


@pytest.mark.parametrize("ac", [True, False])
def test_helper_matches_the_geometry_oracle_and_the_fp32_oracle(ac):
    N, M, D, H, W = 3, 2, 6, 14, 18
    rgba = oracle.synth_rgba(11, (M, D, 4, 20, 24))
    rgba[0, 1:5, 3, :8] = 1.0   # four exactly opaque planes: T ~ 1e-40 there
    ray, eye, zd = _cam(N, H, W, seed=12)
    dhw, v2m = _dhw(M, D), np.array([0, 1, 0])
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    c, z, T = tr.render(t(rgba), t(dhw), t(ray), t(eye), t(zd), v2m, align_corners=ac)
    c0, z0 = geometry_render(t(rgba), t(dhw), t(ray), t(eye), t(zd), v2m, align_corners=ac)
    assert float((c - c0).abs().max()) <= 1e-12 and float((z - z0).abs().max()) <= 1e-12
    ref = oracle.render(rgba, dhw, ray, eye, zd, view_to_mpi=v2m.astype(np.int32), align_corners=ac)
    assert np.abs(T.numpy() - ref["T"].reshape(T.shape)).max() <= 1e-6
    assert float(T.min()) < 1e-30 and float(T.max()) > 1e-3


def test_transmittance_of_the_samples_has_the_closed_form_gradient():
    g = torch.Generator().manual_seed(3)
    smp = torch.rand((7, 5, 4), generator=g, dtype=torch.float64)
    smp[2, 0, 3] = 1.0                      # exactly opaque
    smp[3, 1, 3] = 1.0 - 1e-6               # nearly opaque
    smp[1:5, 2, 3] = 1.0                    # four exactly opaque in a row
    smp.requires_grad_(True)
    _, _, T = tr.composite(smp, torch.rand((7, 5), generator=g, dtype=torch.float64))
    T.sum().backward()
    with torch.no_grad():
        om = 1 - smp[..., 3] + 1e-10
        want = -T[None] / om
    assert torch.equal(smp.grad[..., :3], torch.zeros_like(smp.grad[..., :3]))   # dT/drgb = 0
    assert torch.allclose(smp.grad[..., 3], want, rtol=1e-12, atol=0)
    assert float(-smp.grad[1, 2, 3]) == pytest.approx(1e-30, rel=1e-6)      # T ~ 1e-40, dT/da ~ 1e-30


@pytest.mark.parametrize("ac", [True, False])
def test_transmittance_gradient_matches_central_differences(ac):
    N, M, D, H, W, Ht, Wt = 2, 1, 4, 6, 7, 10, 12
    rgba = _smooth_rgba(21, (M, D, 4, Ht, Wt)).astype(np.float64)
    ray, eye, zd = (a.astype(np.float64) for a in _cam(N, H, W, seed=22))
    dhw, v2m = _dhw(M, D).astype(np.float64), np.zeros(N, np.int64)
    gT = np.random.default_rng(23).standard_normal((N, 1, H, W))
    got = tr.grads(rgba, dhw, ray, eye, zd, v2m, g_T=gT, align_corners=ac)

    def loss(args):
        t = [torch.from_numpy(a) for a in args]
        return float((tr.render(*t, v2m, align_corners=ac)[2].numpy() * gT).sum())
    base = [rgba, dhw, ray, eye, zd]
    rng = np.random.default_rng(24)
    for i, name in ((0, "rgba"), (1, "dhw"), (2, "ray"), (3, "eye")):
        # a random direction: the directional derivative against a central difference (the floors stay put for steps this small)
        for _ in range(2):
            dirn = rng.standard_normal(base[i].shape)
            if i == 0:
                dirn[:, :, :3] = 0.0            # T does not depend on the colour channels
            h = 1e-6
            plus = [a.copy() for a in base]
            minus = [a.copy() for a in base]
            plus[i] = plus[i] + h * dirn
            minus[i] = minus[i] - h * dirn
            fd = (loss(plus) - loss(minus)) / (2 * h)
            an = float((got[i] * dirn).sum())
            assert abs(an - fd) <= 1e-6 * max(1.0, abs(fd)), (name, an, fd)
    assert np.abs(got[0][:, :, :3]).max() == 0.0 and np.abs(got[0][:, :, 3]).max() > 0
    assert np.abs(got[4]).max() == 0.0      # z_dir only enters the depth


def test_header_declares_the_ex_entries_as_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "gmpi_render.h"\n'
        "int main(void) {\n"
        "    int (*bwd)(const GmpiRenderParams *, const float *, const float *, const float *, float *, const int64_t *, void *) =\n"
        "        gmpi_mpi_render_backward_ex_launch;\n"
        "    int (*geo)(const GmpiRenderParams *, const float *, const float *, const float *, float *, float *, float *, float *, void *) =\n"
        "        gmpi_mpi_render_geometry_backward_ex_launch;\n"
        "    int (*dep)(const void *, int32_t, int64_t, int64_t, int64_t, const float *, const float *, const float *, const float *, float *,\n"
        "               int64_t, int64_t, int64_t, int32_t, int32_t, int32_t, int32_t, void *) = gmpi_alpha_depth_backward_ex_launch;\n"
        "    return (bwd == 0) + (geo == 0) + (dep == 0);\n"
        "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_library_exports_the_ex_entries():
    from ml_gmpi_amd import _lib
    names = ("gmpi_mpi_render_backward_ex_launch", "gmpi_mpi_render_geometry_backward_ex_launch", "gmpi_alpha_depth_backward_ex_launch")
    for name in names:
        assert name in _lib.EXPORTS
    if os.path.isfile(_lib.library_path()):
        import torch  # noqa: F401  (torch's ROCm runtime first, as the binding loads it)
        lib = ctypes.CDLL(_lib.library_path())
        for name in names:
            assert hasattr(lib, name)


@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_backward_kernels_have_no_scratch(tmp_path):
    csrc = os.path.join(ROOT, "ml-gmpi_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
             "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]   # = ml-gmpi_amd/csrc/Makefile
    mk = open(os.path.join(csrc, "Makefile")).read()
    for f in ("-ffp-contract=off", "-fno-slp-vectorize", "-O3"):
        assert f in mk, f"the Makefile no longer passes {f}: keep this test's flags in step with it"
    srcs = ("render_backward", "render_backward_gather", "render_backward_geometry", "light_kernels")
    procs = [subprocess.Popen([HIPCC, *flags, "-save-temps", "-c", os.path.join(csrc, s + ".hip"), "-o", s + ".o"], cwd=tmp_path,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE) for s in srcs]
    for p in procs:
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err.decode()[-2000:]
    seen = {}
    for s in srcs:
        asm = open(os.path.join(tmp_path, s + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        # (texel_gather_kernel, the pair's second pass, reads no upstream gradient and is not covered: it keeps a 112-byte stack frame)
        for name in sorted(set(re.findall(r"^(_Z\w*(?:backward|pixel_pass|geometry_pixel|geometry_reduce)\w*):", asm, flags=re.M))):
            a = asm.index(name + ":")
            body = asm[a:asm.index(".Lfunc_end", a)]
            assert "scratch_" not in body, f"{name}: scratch (spill) operations in the kernel"
            meta = asm[asm.index(".amdhsa_kernel " + name):]
            meta = meta[:meta.index(".end_amdhsa_kernel")]
            assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1)) == 0, name
            seen[name] = s
    kinds = ("render_backward_kernel", "render_backward_tile_kernel", "render_backward_tile2_kernel", "pixel_pass_kernel", "geometry_pixel_kernel",
             "alpha_depth_backward_kernel")
    for k in kinds:
        assert any(k in n for n in seen), (k, sorted(seen))
    shutil.rmtree(tmp_path, ignore_errors=True)
