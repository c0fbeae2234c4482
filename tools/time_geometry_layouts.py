"""Times the geometry backward of the two layouts (gmpi_mpi_render_shared_geometry_backward_launch, gmpi_mpi_render_depth_geometry_backward_launch: d/d
rays, eye, z_dir and dhw) against what a user had to do before them: expand the layout to the RGBA volume and run the volume path's geometry backward.
Through the C ABI, HIP events, medians; 256^2 x 32 x 8, 512^2 x 32 x 4 and 1024^2 x 32 x 4 in fp32; the depth layout with n_z_bins = 4 (a ramp several
planes wide: opaque planes behind the surface, the sweep's start is re-walked) and 256 (a step: most planes are skipped).

  layout   the layout's forward (for T_out) is NOT timed; `geo`: the geometry pass alone (pixel kernel + slab reducer, all four outputs)
  volume   `expand`: expand_shared_color / expand_depth_alpha; `vol_geo`: gmpi_mpi_render_geometry_backward_launch on the expanded volume (the same
           pass over a volume that already exists); `volume_total` = expand + vol_geo: the path without the new entries
  peak     torch.cuda.max_memory_allocated above the inputs of: the layout path (forward outputs, T, the four gradients, the workspace) and the volume
           path (the same plus the expanded volume and what the expand allocates on the way)
  check    the largest |layout - volume| / (1e-4 max|volume|) over the four gradients in the default mode (<= 10 is the tests' bar on smooth inputs; these
           inputs are texel noise: informative only)

Every shape runs in a child process of its own under a time limit; the first failure ends the run.
usage: python tools/time_geometry_layouts.py [reps] [passes]"""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(256, 8, 32), (512, 4, 32), (1024, 4, 32)]   # S, MPIs (one view each), planes
CASES = [("shared", 0), ("depth", 4), ("depth", 256)]   # layout, n_z_bins


def one(layout, S, B, D, n_z_bins, reps):
    import torch
    sys.path.insert(0, ROOT)
    import ml_gmpi_amd
    from ml_gmpi_amd import _lib, depth_alpha_bounds, expand_depth_alpha, expand_shared_color
    from ml_gmpi_amd.hip_mpi import _depth_alpha, _depth_layout, _shared_color, _shared_layout
    lib = _lib.load_library()
    dev = torch.device("cuda:0")
    cs = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn, n=reps):
        for _ in range(3):
            fn()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in evs:
            e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return sorted(a.elapsed_time(b) for a, b in evs)[n // 2]   # median

    r = ml_gmpi_amd.make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise")
    r.set_cam(r.cam_fov, S, S)
    g = torch.Generator(device=dev).manual_seed(7000)
    rgb = torch.rand((B, 3, S, S), device=dev, generator=g)
    bg = torch.rand((B, 3, S, S), device=dev, generator=g)
    if layout == "shared":
        mid = torch.rand((B, D, 1, S, S), device=dev, generator=g)
        mid[:, -1] = 1.0
        plane_z = zb = None
    else:   # a smooth surface with texel noise between the planes (tools/time_depth_alpha.py's)
        coarse = torch.rand((B, 1, 5, 5), device=dev, generator=g)
        mid = 0.15 + 0.7 * torch.nn.functional.interpolate(coarse, size=(S, S), mode="bilinear", align_corners=True)
        mid = (mid + 0.02 * (torch.rand((B, 1, S, S), device=dev, generator=g) - 0.5)).contiguous()
        plane_z = torch.linspace(0, 1, D, device=dev)
        zb = depth_alpha_bounds(1, n_z_bins)
    gc = torch.randn((B, 3, S, S), device=dev, generator=g)
    gd = torch.randn((B, 1, S, S), device=dev, generator=g)
    torch.manual_seed(3)
    cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    ray, eye, zd = torch.cat(cam[3]), torch.cat(cam[4]), torch.cat(cam[5])
    dhw = r._dhw_on_device().expand(B, -1, -1).contiguous()
    kw = dict(check_last_plane=True, out_pm1=True, want_transmittance=True, defer_status=True, views_per_mpi=1)
    base_mem = torch.cuda.memory_allocated(dev)
    row = dict(layout=layout, S=S, B=B, D=D, n_z_bins=n_z_bins)

    def geometry_outputs():
        return [torch.empty_like(t) for t in (ray, eye, zd, dhw)]

    def backward_struct(p, want_dhw=True):
        q = _lib.GmpiRenderParams.from_buffer_copy(p)
        q.rgb_out = q.depth_out = q.status = None
        need = int(lib.gmpi_render_geometry_backward_workspace_bytes(ctypes.byref(q), int(want_dhw)))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        q.workspace, q.workspace_bytes = ws.data_ptr(), ws.numel()
        return q, ws

    # ---- the layout path ---------------------------------------------------------------------------------------------------------------------------
    torch.cuda.reset_peak_memory_stats(dev)
    with torch.no_grad():
        if layout == "shared":
            first, lay = _shared_layout(rgb, mid, bg, None)
        else:
            first, lay = _depth_layout(rgb, mid, plane_z, zb, bg, D, None, "pixel", "pixel")
        res = r.mpi.render_views(first, dhw, ray, eye, zd, _layout=lay, _in_autograd_fn=True, **kw)
        del first, lay
    p = res.pop("_bwd")[0]
    row["frac_T_underflow"] = float((res["T"] < 1e-30).float().mean())
    q, ws = backward_struct(p)
    outs = geometry_outputs()
    sc = _shared_color(rgb, bg)
    if layout == "shared":
        def geo():
            _lib.check(lib.gmpi_mpi_render_shared_geometry_backward_launch(ctypes.byref(q), ctypes.byref(sc), gc.data_ptr(), gd.data_ptr(), None,
                                                                           *[t.data_ptr() for t in outs], cs), "shared geometry backward")
    else:
        da = _depth_alpha(plane_z, *zb)

        def geo():
            _lib.check(lib.gmpi_mpi_render_depth_geometry_backward_launch(ctypes.byref(q), ctypes.byref(sc), ctypes.byref(da), gc.data_ptr(), gd.data_ptr(),
                                                                          None, *[t.data_ptr() for t in outs], cs), "depth geometry backward")
    geo()
    torch.cuda.synchronize()
    row["peak_layout_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20
    row["geo"] = timed(geo)
    layout_grads = [t.clone() for t in outs]
    del res, ws, outs

    # ---- the volume path: expand, then the volume entry ---------------------------------------------------------------------------------------------
    torch.cuda.reset_peak_memory_stats(dev)
    expand = (lambda: expand_shared_color(rgb, mid, bg)) if layout == "shared" else (lambda: expand_depth_alpha(rgb, mid, plane_z, *zb, bg))
    with torch.no_grad():
        vol = expand()
        res = r.mpi.render_views(vol, dhw, ray, eye, zd, _in_autograd_fn=True, **kw)
    pv = res.pop("_bwd")[0]
    qv, wsv = backward_struct(pv)
    outs = geometry_outputs()

    def vol_geo():
        _lib.check(lib.gmpi_mpi_render_geometry_backward_launch(ctypes.byref(qv), gc.data_ptr(), gd.data_ptr(), *[t.data_ptr() for t in outs], cs),
                   "volume geometry backward")
    vol_geo()
    torch.cuda.synchronize()
    row["peak_volume_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20
    row["vol_geo"] = timed(vol_geo)
    with torch.no_grad():
        row["expand"] = timed(lambda: expand(), n=max(reps // 2, 3))
    row["volume_total"] = row["expand"] + row["vol_geo"]
    row["check"] = max(float((a - b).abs().max()) / (1e-4 * float(b.abs().max()) + 1e-30) for a, b in zip(layout_grads, outs))
    print("ROW " + " ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        layout, S, B, D, nz, reps = sys.argv[2], *map(int, sys.argv[3:8])
        one(layout, S, B, D, nz, reps)
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    for ps in range(passes):
        print(f"== pass {ps + 1} of {passes}, {reps} repetitions per figure (medians, ms) ==", flush=True)
        for S, B, D in SHAPES:
            for layout, nz in CASES:
                # a fresh child per shape: its own context, its own allocator; a failure (or a time limit) ends the run
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", layout, str(S), str(B), str(D), str(nz), str(reps)], timeout=240).returncode
                if rc != 0:
                    print(f"child {layout} {S} {B} {D} {nz} ended with status {rc}: stopping", flush=True)
                    sys.exit(1)
