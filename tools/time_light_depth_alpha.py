"""Times the shading augmentation of the depth-alpha layout (compute_depth_ramp, LightRenderer.render_depth: one depth image in, no alpha planes)
against the path that gives the same result through the [B, D, 1, H, W] alpha planes, with HIP events (medians after 3 warm-up launches): fp32 at
256^2 x 32 x 8, 512^2 x 32 x 4, 1024^2 x 32 x 4 and 1024^2 x 96 x 4, each with n_z_bins = 4 (a ramp several planes wide) and 256 (a step), on the
smooth surface with texel noise of tools/time_depth_alpha.py.

  ramp     compute_depth_ramp: `ramp_fwd` the forward with T (gmpi_ramp_depth_launch), `ramp_total` forward + zero-fill of the gradient image +
           backward (gmpi_ramp_depth_backward_launch), both through the C ABI; `ramp_autograd` the same step through the autograd node
  planes   the yardstick: depth_alpha_planes + compute_depth; `planes_fwd` forward (the ramp in torch + gmpi_alpha_depth_launch), `planes_total`
           forward + backward through autograd (zero-fill and gmpi_alpha_depth_backward_ex_launch inside the node, then the clamp's mask and the plane sum)
  light    LightRenderer.render_depth (`light_depth`) against LightRenderer.render_shared on those planes, the planes' construction included
           (`light_shared`), forward + backward of sum(rgb) + sum(background) each
  *_peak_mb  peak device memory of one pass above the inputs (torch.cuda.max_memory_allocated)
  check    1 when the two forwards' depth and T are bit-equal at the timed size; anything else ends the run

Every shape runs in a child process of its own under a time limit; the first failure ends the run.
usage: python tools/time_light_depth_alpha.py [reps] [passes]"""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(256, 8, 32), (512, 4, 32), (1024, 4, 32), (1024, 4, 96)]   # (S, MPIs, planes)
N_Z_BINS = (4, 256)


def one(S, B, D, n_z_bins, reps):
    import torch
    sys.path.insert(0, ROOT)
    import ml_gmpi_amd
    from ml_gmpi_amd import _lib, compute_depth, compute_depth_ramp, depth_alpha_bounds, depth_alpha_planes
    from ml_gmpi_amd.hip_mpi import _depth_alpha
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

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20

    r = ml_gmpi_amd.make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise")
    g = torch.Generator(device=dev).manual_seed(7000)
    rgb = torch.rand((B, 3, S, S), device=dev, generator=g)
    bg = torch.rand((B, 3, S, S), device=dev, generator=g)
    # a smooth surface with texel noise between the planes: 5 x 5 noise upsampled to 0.15 + 0.7 c, + 0.02 (U - 0.5)
    coarse = torch.rand((B, 1, 5, 5), device=dev, generator=g)
    depth = 0.15 + 0.7 * torch.nn.functional.interpolate(coarse, size=(S, S), mode="bilinear", align_corners=True)
    depth = (depth + 0.02 * (torch.rand((B, 1, S, S), device=dev, generator=g) - 0.5)).contiguous()
    plane_z = torch.linspace(0, 1, D, device=dev)
    dhws = r.static_mpi_plane_dhws
    plane_ds = dhws[:, 0].to(dev).contiguous()
    xyz = r.get_xyz_single_res(S, S)[0][-1:].to(dev).contiguous()   # [1,S,S,3]: the augmentation reads the last plane's texel coordinates only
    zb = depth_alpha_bounds(1, n_z_bins)
    gz = torch.randn((B, 1, S, S), device=dev, generator=g)
    gt = torch.randn((B, 1, S, S), device=dev, generator=g)
    row = dict(S=S, B=B, D=D, n_z_bins=n_z_bins)

    # ---- the results at the timed size --------------------------------------------------------------------------------------------------------
    with torch.no_grad():
        z, T = compute_depth_ramp(depth, plane_z, *zb, plane_ds, want_transmittance=True)
        z2, T2 = compute_depth(depth_alpha_planes(depth, plane_z, *zb), plane_ds, want_transmittance=True)
    row["check"] = int(torch.equal(z, z2) and torch.equal(T, T2))
    assert row["check"] == 1, "compute_depth_ramp against compute_depth on the planes"
    row["T_underflow_frac"] = float((T < 1e-30).float().mean())
    del z2, T2

    # ---- ramp: the new entries through the C ABI ------------------------------------------------------------------------------------------------
    da = _depth_alpha(plane_z, *zb)
    grad = torch.zeros_like(depth)
    fwd = lambda: _lib.check(lib.gmpi_ramp_depth_launch(depth.data_ptr(), _lib.DTYPE_F32, depth.stride(0), depth.stride(2), ctypes.byref(da), plane_ds.data_ptr(),
                                                        B, D, S, S, z.data_ptr(), T.data_ptr(), cs), "ramp forward")
    bwd = lambda: _lib.check(lib.gmpi_ramp_depth_backward_launch(depth.data_ptr(), _lib.DTYPE_F32, depth.stride(0), depth.stride(2), ctypes.byref(da),
                                                                 plane_ds.data_ptr(), T.data_ptr(), gz.data_ptr(), gt.data_ptr(), grad.data_ptr(), grad.stride(0),
                                                                 grad.stride(2), B, D, S, S, cs), "ramp backward")
    row["ramp_fwd"] = timed(fwd)
    row["ramp_fill"] = timed(lambda: grad.zero_())
    row["ramp_bwd"] = timed(bwd)
    row["ramp_total"] = row["ramp_fwd"] + row["ramp_fill"] + row["ramp_bwd"]

    def ramp_step():
        d = depth.detach().requires_grad_(True)
        a, b = compute_depth_ramp(d, plane_z, *zb, plane_ds, want_transmittance=True)
        torch.autograd.backward((a, b), (gz, gt))
    row["ramp_autograd"] = timed(ramp_step)
    row["ramp_peak_mb"] = peak(ramp_step)

    # ---- planes: the yardstick ------------------------------------------------------------------------------------------------------------------
    def planes_fwd():
        with torch.no_grad():
            return compute_depth(depth_alpha_planes(depth, plane_z, *zb), plane_ds, want_transmittance=True)

    def planes_step():
        d = depth.detach().requires_grad_(True)
        a, b = compute_depth(depth_alpha_planes(d, plane_z, *zb), plane_ds, want_transmittance=True)
        torch.autograd.backward((a, b), (gz, gt))
    row["planes_fwd"] = timed(planes_fwd)
    row["planes_total"] = timed(planes_step)
    row["planes_fwd_peak_mb"] = peak(planes_fwd)
    row["planes_peak_mb"] = peak(planes_step)

    # ---- LightRenderer: render_depth against render_shared on the planes ---------------------------------------------------------------------
    L = ml_gmpi_amd.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, ka_max=1.3, kd_max=0.9, n_grow_iters=1)
    L.step = 4

    def light_depth():
        ins = [t.detach().requires_grad_(True) for t in (rgb, depth, bg)]
        o_rgb, _, o_bg = L.render_depth(ins[0], ins[1], dhws, xyz, plane_z=plane_z, z_range=1, n_z_bins=n_z_bins, background=ins[2])
        (o_rgb.sum() + o_bg.sum()).backward()

    def light_shared():
        ins = [t.detach().requires_grad_(True) for t in (rgb, depth, bg)]
        o_rgb, _, o_bg = L.render_shared(ins[0], depth_alpha_planes(ins[1], plane_z, *zb), dhws, xyz, background=ins[2])
        (o_rgb.sum() + o_bg.sum()).backward()
    row["light_depth"] = timed(light_depth)
    row["light_shared"] = timed(light_shared)
    row["light_depth_peak_mb"] = peak(light_depth)
    row["light_shared_peak_mb"] = peak(light_shared)
    row["fwd_vs_planes"] = row["ramp_fwd"] / row["planes_fwd"]
    row["total_vs_planes"] = row["ramp_total"] / row["planes_total"]
    row["light_vs_shared"] = row["light_depth"] / row["light_shared"]
    try:
        clock = f"{torch.cuda.clock_rate()} MHz"
    except Exception:  # noqa: BLE001 -- no SMI binding in this torch
        clock = "n/a"
    print("ROW " + " ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()) + f" device={torch.cuda.get_device_name(0)!r} clock={clock}",
          flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(*(int(a) for a in sys.argv[2:7]))
        sys.exit(0)
    reps = sys.argv[1] if len(sys.argv) > 1 else "15"
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    print("times in ms (medians of", reps, "runs after 3 warm-up runs), memory in MiB above the inputs; one child process per shape;", passes, "passes")
    for k in range(passes):
        print(f"== pass {k + 1} ==", flush=True)
        for S, B, D in SHAPES:
            for n in N_Z_BINS:
                try:
                    rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(S), str(B), str(D), str(n), reps], timeout=240).returncode
                except subprocess.TimeoutExpired:   # (run() has killed the child)
                    rc = "time limit of 240 s"
                if rc != 0:
                    print(f"shape {S} x {B} x {D} n_z_bins {n}: exit status {rc}; stopping")
                    sys.exit(1)
