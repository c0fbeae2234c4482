"""Times the geometry backward (gmpi_mpi_render_geometry_backward_launch: d/d rays, eye, z_dir[, dhw]) next to the forward and the volume backward
at the G-step shapes (32 planes, fp32, 4 views, one MPI per view), each part on its own with events.  usage: python tools/time_geometry_backward.py

Lines: forward; volume backward (default: zero-fill + the tile kernel with atomics) and the atomics-free pair (backward="gather": homography + pixel
pass + texel gather); geometry backward without and with the dhw sums (pixel kernel + slab reducer).  Under `rocprofv3 --kernel-trace --stats` the
trace then holds pixel_pass_kernel and geometry_pixel_kernel of one box side by side."""
import ctypes
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ml_gmpi_amd  # noqa: E402
from ml_gmpi_amd import _lib  # noqa: E402

lib = _lib.load_library()
dev = torch.device("cuda:0")
REPS = 20


def timed(fn):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.2:   # clock ramp
        fn()
        torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for e0, e1 in evs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    return ts[len(ts) // 2]


for name, S in (("train256", 256), ("train512", 512), ("train1024", 1024)):
    D, B = 32, 4
    r = ml_gmpi_amd.make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise")
    r.set_cam(r.cam_fov, S, S)
    g = torch.Generator(device=dev).manual_seed(7000)
    vol = torch.rand((B, D, 4, S, S), device=dev, generator=g)
    vol[:, -1, 3] = 1.0
    gc = torch.randn((B, 3, S, S), device=dev, generator=g)
    gd = torch.randn((B, 1, S, S), device=dev, generator=g)
    torch.manual_seed(3)
    cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    ray, eye, zd = torch.cat(cam[3]), torch.cat(cam[4]), torch.cat(cam[5])
    dhw = r._dhw_on_device().expand(B, -1, -1).contiguous()
    res = r.mpi.render_views(vol, dhw, ray, eye, zd, views_per_mpi=1, check_last_plane=True, out_pm1=True, want_transmittance=True,
                             defer_status=True, _in_autograd_fn=True)
    p, keep = res["_bwd"]
    p.status = None
    cs = torch.cuda.current_stream(dev).cuda_stream
    fwd_ws = int(lib.gmpi_render_workspace_bytes(ctypes.byref(p)))
    fws = torch.empty(max(fwd_ws, 1), dtype=torch.uint8, device=dev)
    if fwd_ws:
        p.workspace, p.workspace_bytes = fws.data_ptr(), fws.numel()

    def fwd():
        _lib.check(lib.gmpi_mpi_render_launch(ctypes.byref(p), cs), "forward")
    t_fwd = timed(fwd)

    q = _lib.GmpiRenderParams()
    ctypes.memmove(ctypes.byref(q), ctypes.byref(p), ctypes.sizeof(q))
    q.rgb_out = q.depth_out = None
    q.workspace, q.workspace_bytes = None, 0
    grad = torch.zeros_like(vol)
    gs = (ctypes.c_int64 * 5)(*grad.stride())

    def vol_atomic():
        grad.zero_()
        _lib.check(lib.gmpi_mpi_render_backward_launch(ctypes.byref(q), gc.data_ptr(), gd.data_ptr(), grad.data_ptr(), gs, cs), "volume backward")
    t_vol = timed(vol_atomic)

    qg = _lib.GmpiRenderParams()
    ctypes.memmove(ctypes.byref(qg), ctypes.byref(q), ctypes.sizeof(qg))
    need = int(lib.gmpi_render_backward_workspace_bytes(ctypes.byref(qg)))
    t_gather = None
    if need:
        gws = torch.empty(need, dtype=torch.uint8, device=dev)
        qg.workspace, qg.workspace_bytes = gws.data_ptr(), gws.numel()
        qg.flags |= _lib.FLAG_GRAD_OVERWRITE

        def vol_gather():
            _lib.check(lib.gmpi_mpi_render_backward_launch(ctypes.byref(qg), gc.data_ptr(), gd.data_ptr(), grad.data_ptr(), gs, cs), "gather backward")
        t_gather = timed(vol_gather)
        del gws

    g_ray, g_eye, g_z = torch.empty_like(ray), torch.empty_like(eye), torch.empty_like(zd)
    g_dhw = torch.empty_like(dhw)
    times = {}
    for want_dhw in (False, True):
        qq = _lib.GmpiRenderParams()
        ctypes.memmove(ctypes.byref(qq), ctypes.byref(q), ctypes.sizeof(qq))
        wsb = int(lib.gmpi_render_geometry_backward_workspace_bytes(ctypes.byref(qq), int(want_dhw)))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        qq.workspace, qq.workspace_bytes = ws.data_ptr(), ws.numel()

        def geo(qq=qq, want_dhw=want_dhw):
            _lib.check(lib.gmpi_mpi_render_geometry_backward_launch(ctypes.byref(qq), gc.data_ptr(), gd.data_ptr(), g_ray.data_ptr(), g_eye.data_ptr(),
                                                                    g_z.data_ptr(), g_dhw.data_ptr() if want_dhw else None, cs), "geometry backward")
        times[want_dhw] = (timed(geo), wsb)
        del ws
    tg = "n/a" if t_gather is None else f"{t_gather:.3f}"
    print(f"{name}: {B} views x {S}^2 x {D} planes, fp32 | forward {t_fwd:.3f} ms | volume backward: zero-fill + atomics {t_vol:.3f} ms, "
          f"atomics-free pair {tg} ms | geometry backward: rays+eye+z_dir {times[False][0]:.3f} ms "
          f"(workspace {times[False][1]} B), + dhw {times[True][0]:.3f} ms (workspace {times[True][1]} B)", flush=True)
    del vol, grad, gc, gd, res, keep
    torch.cuda.empty_cache()
