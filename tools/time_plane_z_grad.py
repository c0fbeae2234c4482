"""Times the geometry backward of the depth-alpha layout with and without the gradient w.r.t. plane_z: gmpi_mpi_render_depth_geometry_backward_pz_launch
with grad_plane_z (the PZ instances of render_backward_geometry.hip: one more wave sum and slab component per plane, the wider skip rule, the plane_z
reducer) against the same entry with grad_plane_z = NULL -- gmpi_mpi_render_depth_geometry_backward_launch, whose kernels this feature leaves as they
were: the yardstick.  Through the C ABI, HIP events, medians; 256^2 x 32 x 8, 512^2 x 32 x 4 and 1024^2 x 32 x 4 in fp32, n_z_bins = 4 (a ramp several
planes wide) and 256 (a step: most planes are skipped), with dhw (ray, eye, z_dir, dhw wanted) and without (ray, eye, z_dir).

  geo      the pass without plane_z (pixel kernel + slab reducer)
  geo_pz   the pass with plane_z (PZ pixel kernel + slab reducer + plane_z reducer); ratio = geo_pz / geo
  the two are timed alternately, `rounds` times each; the figure is the median of the rounds' medians
  check    that the pass with plane_z gives the other gradients bit for bit (1 = yes)

The layout's forward (for T_out) is not timed.  Every shape runs in a child process of its own under a time limit; the first failure ends the run.
usage: python tools/time_plane_z_grad.py [reps] [passes]"""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(256, 8, 32), (512, 4, 32), (1024, 4, 32)]   # S, MPIs (one view each), planes
CASES = [(4, 1), (4, 0), (256, 1), (256, 0)]            # n_z_bins, with dhw
ROUNDS = 3


def one(S, B, D, n_z_bins, with_dhw, reps):
    import torch
    sys.path.insert(0, ROOT)
    import ml_gmpi_amd
    from ml_gmpi_amd import _lib, depth_alpha_bounds
    from ml_gmpi_amd.hip_mpi import _depth_alpha, _depth_layout, _shared_color
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
    # a smooth surface with texel noise between the planes (tools/time_depth_alpha.py's)
    coarse = torch.rand((B, 1, 5, 5), device=dev, generator=g)
    depth = 0.15 + 0.7 * torch.nn.functional.interpolate(coarse, size=(S, S), mode="bilinear", align_corners=True)
    depth = (depth + 0.02 * (torch.rand((B, 1, S, S), device=dev, generator=g) - 0.5)).contiguous()
    plane_z = torch.linspace(0, 1, D, device=dev)
    zb = depth_alpha_bounds(1, n_z_bins)
    gc = torch.randn((B, 3, S, S), device=dev, generator=g)
    gd = torch.randn((B, 1, S, S), device=dev, generator=g)
    torch.manual_seed(3)
    cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    ray, eye, zd = torch.cat(cam[3]), torch.cat(cam[4]), torch.cat(cam[5])
    dhw = r._dhw_on_device().expand(B, -1, -1).contiguous()
    kw = dict(check_last_plane=True, out_pm1=True, want_transmittance=True, defer_status=True, views_per_mpi=1)
    with torch.no_grad():
        first, lay = _depth_layout(rgb, depth, plane_z, zb, bg, D, None, "pixel", "pixel")
        res = r.mpi.render_views(first, dhw, ray, eye, zd, _layout=lay, _in_autograd_fn=True, **kw)
    p = res.pop("_bwd")[0]
    sc, da = _shared_color(rgb, bg), _depth_alpha(plane_z, *zb)

    def make(want_pz):
        q = _lib.GmpiRenderParams.from_buffer_copy(p)
        q.rgb_out = q.depth_out = q.status = None
        need = int(lib.gmpi_render_depth_geometry_backward_workspace_bytes(ctypes.byref(q), with_dhw, int(want_pz)))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        q.workspace, q.workspace_bytes = ws.data_ptr(), ws.numel()
        outs = [torch.empty_like(t) for t in (ray, eye, zd)] + ([torch.empty_like(dhw)] if with_dhw else [None])
        g_pz = torch.empty_like(plane_z) if want_pz else None
        ptrs = [None if t is None else t.data_ptr() for t in outs + [g_pz]]

        def launch():
            _lib.check(lib.gmpi_mpi_render_depth_geometry_backward_pz_launch(ctypes.byref(q), ctypes.byref(sc), ctypes.byref(da), gc.data_ptr(), gd.data_ptr(),
                                                                             None, *ptrs, cs), "depth geometry backward")
        return launch, outs, g_pz, ws, need

    geo, outs, _, ws0, need0 = make(False)
    geo_pz, outs_pz, g_pz, ws1, need1 = make(True)
    geo(), geo_pz()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(outs, outs_pz) if a is not None)
    a, b = [], []
    for _ in range(ROUNDS):   # alternately: a drift of the clock lands on both
        a.append(timed(geo))
        b.append(timed(geo_pz))
    t0, t1 = sorted(a)[ROUNDS // 2], sorted(b)[ROUNDS // 2]
    row = dict(S=S, B=B, D=D, n_z_bins=n_z_bins, dhw=with_dhw, geo=t0, geo_pz=t1, ratio=t1 / t0, extra_ms=t1 - t0, check=int(same),
               pz_norm=float(g_pz.norm()), ws_mb=need0 / 2 ** 20, ws_pz_mb=need1 / 2 ** 20)
    print("ROW " + " ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        one(*map(int, sys.argv[2:8]))
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    for ps in range(passes):
        print(f"== pass {ps + 1} of {passes}, {reps} repetitions per figure x {ROUNDS} alternating rounds (medians, ms) ==", flush=True)
        for S, B, D in SHAPES:
            for nz, with_dhw in CASES:
                # a fresh child per shape: its own context, its own allocator; a failure (or a time limit) ends the run
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(S), str(B), str(D), str(nz), str(with_dhw), str(reps)],
                                    timeout=240).returncode
                if rc != 0:
                    print(f"child {S} {B} {D} {nz} {with_dhw} ended with status {rc}: stopping", flush=True)
                    sys.exit(1)
