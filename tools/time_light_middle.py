"""Times the image-sized middle of the shading augmentation (blur, point cloud, normals, Lambert) in both modes of LightRenderer(middle=...) --
"torch": autograd over a torch restatement (the default), "hip": the adjoint kernels and the shade-images node -- with HIP events (medians after 3
warm-up runs) at 256^2 x 8, 512^2 x 4 and 1024^2 x 4 MPIs of 32 planes, fp32 and bf16 storage.  Every quantity is measured once per mode (`_torch`,
`_hip`) in the same child process, and `*_ratio` = hip / torch.

  middle_bwd     (a) `_middle_backward` alone: dL/d shading [B,H,W] -> dL/d depth [B,1,H,W]
  render         (b) LightRenderer.render forward + backward of sum(out * g)
  g_step         (c) shading_image -> render_views_shaded -> backward of (colour, depth): the `fused_step` of tools/time_shaded_render.py, same inputs
  light_shared   (d) render_shared forward + backward of sum(rgb) + sum(background); the alpha planes are the depth image's (depth_alpha_planes, their
  light_depth        construction included), and render_depth on that image: the `light_shared` / `light_depth` of tools/time_light_depth_alpha.py,
                     same inputs, n_z_bins = 4 (bf16: colours, background and depth image in bf16)
  *_peak_mb      (e) peak device memory of one such step above the inputs (torch.cuda.max_memory_allocated)
  middle_bwd_err999_*   (a) against float64 autograd of the product's torch restatement on the device, same inputs: the 99.9th percentile of |error| / max|g_ref|
                 per mode.  The run ends unless hip's is within max(2e-4, 4 x torch's): the tests' rule, with a percentile because single cells on the
                 clamp's knife edge flip in fp32 in either mode.  (The error grows with the resolution in both modes: the normals are differences of
                 neighbouring points, whose distance shrinks with the texel pitch while the noise of the depth does not.)
  *_check        the two modes' gradients against each other at the timed size: the fraction of elements further apart than 2e-4 of the largest + 1e-6
                 (bf16: + 2^-7 of it).  A figure, not a bar: it contains the fp32 noise above, and in (d) the texels where the two modes' shadings,
                 ~5e-6 apart (two GEMMs against 81 taps), decide the mask of clip(c * s, 0, 1) differently, each of which reaches the 11 x 11 depth
                 texels around it.  A wrong gradient differs everywhere: more than 0.25 ends the run

Every shape runs in a child process of its own under a time limit; the first failure ends the run.
usage: python tools/time_light_middle.py [reps] [passes]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(S, B, 32, dt) for S, B in ((256, 8), (512, 4), (1024, 4)) for dt in ("f32", "bf16")]   # (S, MPIs, planes, storage)
MODES = ("torch", "hip")


def one(S, B, D, dtype_name, reps):
    import torch
    sys.path.insert(0, ROOT)
    import ml_gmpi_amd
    from ml_gmpi_amd import compute_depth, depth_alpha_planes, depth_alpha_bounds
    from ml_gmpi_amd.light import _blur_matrix, _blur_torch, _middle_backward, _middle_saved, _shading_torch
    dev = torch.device("cuda:0")
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype_name]

    def timed(fn, n=reps):
        for _ in range(3):
            fn()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in evs:
            e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return sorted(a.elapsed_time(b) for a, b in evs)[n // 2]   # median

    def peak(fn):
        fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20

    r = ml_gmpi_amd.make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise")
    r.set_cam(r.cam_fov, S, S)
    dhws = r.static_mpi_plane_dhws
    xyz, _ = r.get_xyz(S, S, ret_single_res=True)
    row = dict(S=S, B=B, D=D, dtype=dtype_name)
    rounding = 2.0 ** -7 if dtype is torch.bfloat16 else 0.0
    grads = {}

    def agree(name):
        a, b = grads.pop((name, "torch")), grads.pop((name, "hip"))
        scale = float(a.abs().max())
        row[name + "_check"] = float(((a - b).abs() > (2e-4 + rounding) * scale + 1e-6).float().mean())
        assert row[name + "_check"] <= 0.25, (name, row)

    # ---- the volume of tools/time_shaded_render.py: (a), (b), (c) ---------------------------------------------------------------------------------
    g = torch.Generator(device=dev).manual_seed(7000)
    vol = torch.rand((B, D, 4, S, S), device=dev, generator=g)
    vol[:, :, 3] *= 3.0 / D   # (thin planes: every plane counts)
    vol[:, :, 3] += torch.linspace(0, 0.05, S, device=dev).view(1, 1, 1, S)   # (a slope in the expected depth: the Lambert term is not constant)
    vol[:, D - 1, 3] = 1.0
    vol = vol.to(dtype)
    gc = torch.randn((B, 3, S, S), device=dev, generator=g)
    gd = torch.randn((B, 1, S, S), device=dev, generator=g)
    g_vol = torch.randn((B, D, 4, S, S), device=dev, generator=g)
    g_s = torch.randn((B, S, S), device=dev, generator=g)
    torch.manual_seed(3)
    cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    ray, eye, zd = torch.cat(cam[3]), torch.cat(cam[4]), torch.cat(cam[5])
    dhw = r._dhw_on_device().expand(B, -1, -1).contiguous()

    def light(mode, ka=0.9, kd=0.9, step=10):   # (the end of the ramp, as tools/time_shaded_render.py)
        L = ml_gmpi_amd.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, ka_max=ka, kd_max=kd, n_grow_iters=1, middle=mode)
        L.step = step
        return L

    leaf = vol.clone().requires_grad_(True)
    kw2 = dict(check_last_plane=True, out_pm1=True, defer_status=True)
    xyz_last = xyz[-1, :, :, :3].to(dev, torch.float32).contiguous()
    for mode in MODES:
        L = light(mode)
        torch.manual_seed(5)
        ld = L._next_light(B).to(dev, torch.float32).contiguous()
        with torch.no_grad():
            depth = compute_depth(vol[:, :, 3:], dhws[:, :1].to(dev))
            saved = _middle_saved(L, depth, L.blurrer_func(depth))
        middle = lambda: _middle_backward(mode, saved, xyz_last, ld, L.cur_ka, L.cur_kd, g_s)
        grads[("middle_bwd", mode)] = middle().clone()
        with torch.enable_grad():   # float64 autograd of the restatement (the same in both passes of this loop: a few ms)
            d64 = depth.double().requires_grad_(True)
            my, mx = (_blur_matrix(S, L._k1d, dev).double() for _ in range(2))
            s64 = _shading_torch(_blur_torch(d64, my, mx), xyz_last.double(), ld.double(), L.cur_ka, L.cur_kd)
            (ref,) = torch.autograd.grad(s64, d64, g_s.double())
        err = ((grads[("middle_bwd", mode)].double() - ref).abs() / ref.abs().max()).flatten().float()
        row[f"middle_bwd_err999_{mode}"] = float(err.kthvalue(int(0.999 * err.numel())).values)
        del d64, s64, ref, err, my, mx
        row[f"middle_bwd_{mode}"] = timed(middle)
        row[f"middle_bwd_peak_mb_{mode}"] = peak(middle)

        def render_step():
            leaf.grad = None
            torch.manual_seed(5)
            light(mode).render(leaf, dhws, xyz).backward(g_vol)

        def g_step():
            leaf.grad = None
            L = light(mode)
            torch.manual_seed(5)
            o = r.mpi.render_views_shaded(leaf, L.shading_image(leaf, dhws, xyz), dhw, ray, eye, zd, **kw2)
            torch.autograd.backward([o["color"], o["depth"]], [gc, gd])

        for name, fn in (("render", render_step), ("g_step", g_step)):
            fn()
            grads[(name, mode)] = leaf.grad.float().clone()
            row[f"{name}_{mode}"] = timed(fn)
            leaf.grad = None
            row[f"{name}_peak_mb_{mode}"] = peak(fn) + leaf.grad.numel() * leaf.grad.element_size() / 2 ** 20   # (the leaf's gradient counts, as in tools/time_shaded_render.py)
        del saved, depth
    assert row["middle_bwd_err999_hip"] <= max(2e-4, 4 * row["middle_bwd_err999_torch"]), row
    for name in ("middle_bwd", "render", "g_step"):
        agree(name)
        row[name + "_ratio"] = row[name + "_hip"] / row[name + "_torch"]
    del leaf, vol, g_vol
    torch.cuda.empty_cache()

    # ---- the images of tools/time_light_depth_alpha.py: (d) -------------------------------------------------------------------------------------------
    n_z_bins = 4
    g = torch.Generator(device=dev).manual_seed(7000)
    rgb = torch.rand((B, 3, S, S), device=dev, generator=g).to(dtype)
    bg = torch.rand((B, 3, S, S), device=dev, generator=g).to(dtype)
    coarse = torch.rand((B, 1, 5, 5), device=dev, generator=g)
    image = 0.15 + 0.7 * torch.nn.functional.interpolate(coarse, size=(S, S), mode="bilinear", align_corners=True)
    image = (image + 0.02 * (torch.rand((B, 1, S, S), device=dev, generator=g) - 0.5)).contiguous().to(dtype)
    plane_z = torch.linspace(0, 1, D, device=dev)
    zb = depth_alpha_bounds(1, n_z_bins)
    xyz1 = r.get_xyz_single_res(S, S)[0][-1:].to(dev).contiguous()   # [1,S,S,3]: the augmentation reads the last plane's texel coordinates only
    for mode in MODES:
        L = light(mode, ka=1.3, kd=0.9, step=4)

        def light_depth():
            ins = [t.detach().requires_grad_(True) for t in (rgb, image, bg)]
            o_rgb, _, o_bg = L.render_depth(ins[0], ins[1], dhws, xyz1, plane_z=plane_z, z_range=1, n_z_bins=n_z_bins, background=ins[2])
            (o_rgb.sum() + o_bg.sum()).backward()
            return ins[1].grad

        def light_shared():
            ins = [t.detach().requires_grad_(True) for t in (rgb, image, bg)]
            o_rgb, _, o_bg = L.render_shared(ins[0], depth_alpha_planes(ins[1], plane_z, *zb), dhws, xyz1, background=ins[2])
            (o_rgb.sum() + o_bg.sum()).backward()
            return ins[1].grad

        for name, fn in (("light_depth", light_depth), ("light_shared", light_shared)):
            torch.manual_seed(5)
            L.step = 4
            grads[(name, mode)] = fn().float().clone()
            row[f"{name}_{mode}"] = timed(fn)
            row[f"{name}_peak_mb_{mode}"] = peak(fn)
    for name in ("light_depth", "light_shared"):
        agree(name)
        row[name + "_ratio"] = row[name + "_hip"] / row[name + "_torch"]
    try:
        clock = f"{torch.cuda.clock_rate()} MHz"
    except Exception:  # noqa: BLE001 -- no SMI binding in this torch
        clock = "n/a"
    fmt = lambda k, v: f"{k}={v}" if not isinstance(v, float) else f"{k}={v:.2e}" if "err999" in k or k.endswith("_check") else f"{k}={v:.3f}"
    print("ROW " + " ".join(fmt(k, v) for k, v in row.items()) + f" device={torch.cuda.get_device_name(0)!r} clock={clock}",
          flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        S, B, D, dt, reps = sys.argv[2:7]
        one(int(S), int(B), int(D), dt, int(reps))
        sys.exit(0)
    reps = sys.argv[1] if len(sys.argv) > 1 else "15"
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
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
