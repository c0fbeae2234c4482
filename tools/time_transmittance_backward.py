"""Times the backward passes with and without a gradient w.r.t. the transmittance output, through the C ABI, at the G-step shapes (32 planes,
fp32, one MPI per view): the tile kernel (zero-filled gradient, atomics), the atomics-free pair (pixel pass + texel gather, with a workspace) and
the geometry pass (rays, eye, z_dir and dhw).  "old" is the entry without a gT argument, "gT" the `_ex` entry with a gT buffer; the two run
interleaved, rep by rep, so that clock drift hits both alike.  usage: python tools/time_transmittance_backward.py [reps]"""
import ctypes
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ml_gmpi_amd  # noqa: E402
from ml_gmpi_amd import _lib  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
lib = _lib.load_library()
dev = torch.device("cuda:0")
cs = torch.cuda.current_stream(dev).cuda_stream


def timed(fn, n=20):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in evs:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in evs)[n // 2]   # median


for S, B in ((256, 8), (512, 4), (1024, 4)):
    D = 32
    r = ml_gmpi_amd.make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise")
    r.set_cam(r.cam_fov, S, S)
    g = torch.Generator(device=dev).manual_seed(7000)
    vol = torch.rand((B, D, 4, S, S), device=dev, generator=g)
    vol[:, -1, 3] = 1.0
    gc = torch.randn((B, 3, S, S), device=dev, generator=g)
    gd = torch.randn((B, 1, S, S), device=dev, generator=g)
    gT = torch.randn((B, 1, S, S), device=dev, generator=g)
    torch.manual_seed(3)
    cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    ray, eye, zd = torch.cat(cam[3]), torch.cat(cam[4]), torch.cat(cam[5])
    dhw = r._dhw_on_device().expand(B, -1, -1).contiguous()
    res = r.mpi.render_views(vol, dhw, ray, eye, zd, views_per_mpi=1, check_last_plane=True, out_pm1=True, want_transmittance=True,
                             defer_status=True, _in_autograd_fn=True)
    p, keep = res["_bwd"]
    p.rgb_out = p.depth_out = p.status = None
    grad = torch.zeros_like(vol)
    gs = (ctypes.c_int64 * 5)(*grad.stride())
    # the pair: its own copy of the parameters with a workspace (every element of the gradient written)
    pp = _lib.GmpiRenderParams.from_buffer_copy(p)
    need = int(lib.gmpi_render_backward_workspace_bytes(ctypes.byref(pp)))
    bws = torch.empty(need, dtype=torch.uint8, device=dev)
    pp.workspace, pp.workspace_bytes = bws.data_ptr(), bws.numel()
    pp.flags |= _lib.FLAG_GRAD_OVERWRITE
    # the geometry pass: d/d rays, eye, z_dir and dhw
    pg = _lib.GmpiRenderParams.from_buffer_copy(p)
    gws = torch.empty(int(lib.gmpi_render_geometry_backward_workspace_bytes(ctypes.byref(pg), 1)), dtype=torch.uint8, device=dev)
    pg.workspace, pg.workspace_bytes = gws.data_ptr(), gws.numel()
    g_ray, g_eye, g_z, g_dhw = (torch.empty(s, device=dev) for s in ((B, 3, S, S), (B, 3), (B, 3), (B, D, 3)))
    geo_out = (g_ray.data_ptr(), g_eye.data_ptr(), g_z.data_ptr(), g_dhw.data_ptr())

    def run(q, with_T):
        def f():
            if with_T:
                _lib.check(lib.gmpi_mpi_render_backward_ex_launch(ctypes.byref(q), gc.data_ptr(), gd.data_ptr(), gT.data_ptr(), grad.data_ptr(), gs, cs), "ex")
            else:
                _lib.check(lib.gmpi_mpi_render_backward_launch(ctypes.byref(q), gc.data_ptr(), gd.data_ptr(), grad.data_ptr(), gs, cs), "old")
        return f

    def run_geo(with_T):
        def f():
            if with_T:
                _lib.check(lib.gmpi_mpi_render_geometry_backward_ex_launch(ctypes.byref(pg), gc.data_ptr(), gd.data_ptr(), gT.data_ptr(), *geo_out, cs), "geo ex")
            else:
                _lib.check(lib.gmpi_mpi_render_geometry_backward_launch(ctypes.byref(pg), gc.data_ptr(), gd.data_ptr(), *geo_out, cs), "geo")
        return f

    parts = {"tile": (run(p, False), run(p, True)), "pair": (run(pp, False), run(pp, True)), "geometry": (run_geo(False), run_geo(True))}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:   # clock ramp
        for a, b in parts.values():
            a(); b()
        torch.cuda.synchronize()
    for name, (a, b) in parts.items():
        ta, tb = [], []
        for _ in range(REPS):
            ta.append(timed(a))
            tb.append(timed(b))
        ta, tb = sorted(ta)[REPS // 2], sorted(tb)[REPS // 2]
        print(f"{name:9s} {S:5d}^2 x {D} x {B}: old {ta:.4f} ms | gT {tb:.4f} ms | {100 * (tb / ta - 1):+.2f} %", flush=True)
