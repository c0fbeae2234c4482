"""Times the shaded render of an RGBA volume (MPI.render_views_shaded: the shading augmentation fused into the render's taps) against the two-step
path it replaces, with HIP events (medians), at 256^2 x 32 x 8, 512^2 x 32 x 4 and 1024^2 x 32 x 4, each in fp32 and bf16.

  forward     fused_fwd_auto    render_views_shaded, the library's choice (the staged kernel: asserted)
              fused_fwd_gather  render_views_shaded, the one-pixel-per-lane kernel
              apply, two_fwd    gmpi_light_apply_launch into a fp32 volume, then render_views (variant auto) of that volume; two_step_fwd = their sum
  G-step      fused_step        LightRenderer.shading_image -> render_views_shaded -> backward of (colour, depth), under autograd: forward, one zero-fill,
                                one backward launch, the in-place chain rule, the image-sized middle
              two_step          LightRenderer.render -> render_views -> backward: today's chain
              *_peak_mb         peak device memory of one such step above the inputs (torch.cuda.max_memory_allocated)
  check       the fused forward's colour, depth and T against the two-step path's at the timed size (default mode: <= 1e-5), the volume gradients of the
              two steps against each other (<= 1e-4 of the largest, + 1e-6; bf16: + 2^-7, four roundings to the storage dtype); anything else ends the run

Every shape runs in a child process of its own under a time limit; the first failure ends the run.
usage: python tools/time_shaded_render.py [reps] [passes]"""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(S, B, 32, dt) for S, B in ((256, 8), (512, 4), (1024, 4)) for dt in ("f32", "bf16")]   # (S, MPIs, planes, storage)


def one(S, B, D, dtype_name, reps):
    import torch
    sys.path.insert(0, ROOT)
    import ml_gmpi_amd
    from ml_gmpi_amd import _lib
    lib = _lib.load_library()
    dev = torch.device("cuda:0")
    cs = torch.cuda.current_stream(dev).cuda_stream
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype_name]

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
    gather = ml_gmpi_amd.MPI(variant="gather", on_out_of_plane="raise")
    g = torch.Generator(device=dev).manual_seed(7000)
    vol = torch.rand((B, D, 4, S, S), device=dev, generator=g)
    vol[:, :, 3] *= 3.0 / D   # (thin planes: every plane counts)
    vol[:, :, 3] += torch.linspace(0, 0.05, S, device=dev).view(1, 1, 1, S)   # (a slope in the expected depth: the Lambert term is not constant)
    vol[:, D - 1, 3] = 1.0
    vol = vol.to(dtype)
    gc = torch.randn((B, 3, S, S), device=dev, generator=g)
    gd = torch.randn((B, 1, S, S), device=dev, generator=g)
    torch.manual_seed(3)
    cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    ray, eye, zd = torch.cat(cam[3]), torch.cat(cam[4]), torch.cat(cam[5])
    dhw = r._dhw_on_device().expand(B, -1, -1).contiguous()
    xyz, _ = r.get_xyz(S, S, ret_single_res=True)
    def light():   # (the end of the ramp: ka = kd = 0.9, a shading between 0.9 and 1.8 -- the clip bites; `clipped` says for how many colour texels)
        L = ml_gmpi_amd.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, ka_max=0.9, kd_max=0.9, n_grow_iters=1)
        L.step = 10
        return L
    kw = dict(check_last_plane=True, out_pm1=True, want_transmittance=True, defer_status=True)
    out = {k: torch.empty(s, device=dev) for k, s in (("color", (B, 3, S, S)), ("depth", (B, 1, S, S)), ("T", (B, 1, S, S)))}
    row = dict(S=S, B=B, D=D, dtype=dtype_name)

    # ---- forward ------------------------------------------------------------------------------------------------------------------------------
    with torch.no_grad():
        L = light()
        torch.manual_seed(5)
        s = L.shading_image(vol, r.static_mpi_plane_dhws, xyz)
        row["clipped"] = float((vol[:, :, :3].float() * s[:, None] > 1).float().mean())
        res = r.mpi.render_views_shaded(vol, s, dhw, ray, eye, zd, _in_autograd_fn=True, **kw)
        assert res.pop("_bwd")[0].variant == _lib.VARIANT_LDS, "the staged kernel did not take this launch"
        fused = {k: res[k].clone() for k in ("color", "depth", "T")}
        shaded = torch.empty((B, D, 4, S, S), dtype=torch.float32, device=dev)
        strides = (ctypes.c_int64 * 5)(*vol.stride())
        apply = lambda: _lib.check(lib.gmpi_light_apply_launch(vol.data_ptr(), _lib.DTYPE_F32 if dtype is torch.float32 else _lib.DTYPE_BF16, strides, s.data_ptr(),
                                                               shaded.data_ptr(), B, D, S, S, cs), "apply")
        apply()
        two = r.mpi.render_views(shaded, dhw, ray, eye, zd, **kw)
        row["fwd_check"] = max(float((fused[k] - two[k]).abs().max()) for k in fused)
        assert row["fwd_check"] <= 1e-5, row
        row["fused_fwd_auto"] = timed(lambda: r.mpi.render_views_shaded(vol, s, dhw, ray, eye, zd, out=out, **kw))
        row["fused_fwd_gather"] = timed(lambda: gather.render_views_shaded(vol, s, dhw, ray, eye, zd, out=out, **kw))
        row["apply"] = timed(apply)
        row["two_fwd"] = timed(lambda: r.mpi.render_views(shaded, dhw, ray, eye, zd, out=out, **kw))
        row["two_step_fwd"] = row["apply"] + row["two_fwd"]
        row["fused_vs_two_step_fwd"] = row["fused_fwd_auto"] / row["two_step_fwd"]
        del shaded, two, res
    torch.cuda.empty_cache()

    # ---- the G-step: forward + zero-fill + backward, under autograd -----------------------------------------------------------------------------
    leaf = vol.clone().requires_grad_(True)
    kw2 = dict(check_last_plane=True, out_pm1=True, defer_status=True)

    def step(fused_path):
        leaf.grad = None
        L = light()
        torch.manual_seed(5)
        if fused_path:
            o = r.mpi.render_views_shaded(leaf, L.shading_image(leaf, r.static_mpi_plane_dhws, xyz), dhw, ray, eye, zd, **kw2)
        else:
            o = r.mpi.render_views(L.render(leaf, r.static_mpi_plane_dhws, xyz), dhw, ray, eye, zd, **kw2)
        torch.autograd.backward([o["color"], o["depth"]], [gc, gd])

    grads = {}
    for name, fused_path in (("fused", True), ("two", False)):
        step(fused_path)
        torch.cuda.synchronize()
        base_mem = torch.cuda.memory_allocated(dev) - leaf.grad.numel() * leaf.grad.element_size()
        torch.cuda.reset_peak_memory_stats(dev)
        step(fused_path)
        torch.cuda.synchronize()
        row[name + "_peak_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20
        grads[name] = leaf.grad.float().clone()
        row[name + "_step"] = timed(lambda: step(fused_path))
    scale = float(grads["two"].abs().max())
    row["grad_check"] = float((grads["fused"] - grads["two"]).abs().max()) / scale
    # bf16: the gradients come back in the storage dtype.  The fused step rounds three times (the render's term, the shading path's term through
    # compute_depth, their sum in autograd's accumulation), today's chain once: four half ulps of bf16 at most, 4 x 2^-9 of the element
    rounding = 2.0 ** -7 if dtype is torch.bfloat16 else 0.0
    assert row["grad_check"] <= 1e-4 + rounding + 1e-6 / scale, row
    row["fused_vs_two_step"] = row["fused_step"] / row["two_step"]
    try:
        clock = f"{torch.cuda.clock_rate()} MHz"
    except Exception:  # noqa: BLE001 -- no SMI binding in this torch
        clock = "n/a"
    print("ROW " + " ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()) + f" device={torch.cuda.get_device_name(0)!r} clock={clock}",
          flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        S, B, D, dt, reps = sys.argv[2:7]
        one(int(S), int(B), int(D), dt, int(reps))
        sys.exit(0)
    reps = sys.argv[1] if len(sys.argv) > 1 else "15"
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    print("times in ms (medians of", reps, "runs after 3 warm-up runs), memory in MiB above the inputs; one child process per shape;", passes, "pass(es)")
    for k in range(passes):
        print(f"== pass {k + 1} ==", flush=True)
        for S, B, D, dt in SHAPES:
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(S), str(B), str(D), dt, reps], timeout=240).returncode
            except subprocess.TimeoutExpired:   # (run() has killed the child)
                rc = "time limit of 240 s"
            if rc != 0:
                print(f"shape {S} x {B} x {D} {dt}: exit status {rc}; stopping")
                sys.exit(1)
