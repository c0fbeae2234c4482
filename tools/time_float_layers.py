"""Times the render of channels-last float layers [M, D, Ht, Wt, 4] read in place (MPI.render_views_layers, gmpi_mpi_render_layers_launch) against what a
holder of such layers did before -- copy into the planar order, then render -- and against the planar kernels on a planar volume that already exists,
with HIP events (medians), forward only, default mode:

  config3   1024^2 x 96 x 4 views                       fp32, bf16, fp16
  config2   256^2 x 96 x 8 views                        fp32, bf16
  config4   8 camera-path views of ONE 512^2 x 96 MPI   fp32, bf16   (a yaw sweep of +-0.3 rad)

  lay_lds, lay_gather      the staged kernel of render_layers.hip and the gather kernel's texel instance over the layers, in place
  copy_plus_auto           `render_views(layers.permute(0, 1, 4, 2, 3))` with variant auto in ONE timed region: the copy render_views makes + the render
  planar_auto / _lds / _gather   the planar kernels on the planar copy of the same values, made beforehand (auto: the band kernel where it applies)

and, per row: the peak device memory above the inputs of one in-place render (lay_peak_mb) and of one copy-and-render (copy_peak_mb), the largest
difference between the staged kernel's default-mode and strict-order results (lds_default_vs_strict), and the assertion that strict-order lay_lds and
lay_gather equal the planar gather kernel's strict result bit for bit.  Every pass runs in a child process of its own under a time limit; the first
failure ends the run.  `passes` repeats the whole pass in one session, each under a "== pass i ==" header; profiles/float_layers.txt records three and
quotes min-max.  usage: python tools/time_float_layers.py [reps [passes]]   (defaults 15 and 3)

`--backward [reps [passes]]` (defaults 10 and 3; profiles/float_layers_backward.txt) times one training step over the layers instead -- forward +
zero-fill + backward of `render_views_layers`, upstream gradients for colour and depth -- at 256^2 x 32 x 8, 512^2 x 32 x 4 and 1024^2 x 32 x 4 MPIs,
one view each, fp32 and bf16:

  step_texel, step_planar   layers_backward="texel" (the layers read and their gradient written in place) | "planar" (the transient planar copy, the
                            planar backward, the permute back: the path of every commit before the keyword)
  step_volume               `render_views` on a planar volume that already exists, the default backward: what a holder of planar data pays
  bwd_texel, bwd_planar     the backward launch alone through the C entry, accumulating into a gradient that exists: the texel tile kernel over the
                            layers | the planar tile kernel over the planar copy;  fill: zero-filling one fp32 gradient
  peak_texel_mb, peak_planar_mb, peak_volume_mb    peak device memory of one step above its inputs (layers / volume, cameras, upstream gradients): the
                            outputs, every transient and the gradient the step leaves behind
  grad_diff                 fp32 rows: max |texel - planar| gradient / the largest gradient (asserted <= 1e-5)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, S, MPIs, planes, views per MPI, dtypes)
SHAPES = [("config3", 1024, 4, 96, 1, ("f32", "bf16", "f16")), ("config2", 256, 8, 96, 1, ("f32", "bf16")), ("config4", 512, 1, 96, 8, ("f32", "bf16"))]


def one(name, S, B, D, V, tag, reps):
    import torch
    import ml_gmpi_amd
    from ml_gmpi_amd import MPI
    dev = torch.device("cuda:0")
    dtype = dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)[tag]

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
    lay = torch.rand((B, D, S, S, 4), device=dev, generator=torch.Generator(device=dev).manual_seed(7200)).to(dtype)
    N = B * V
    torch.manual_seed(3)
    if V == 1:
        cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    else:   # a camera path: V views of every MPI along a yaw sweep
        yaws = torch.linspace(-0.3, 0.3, V).repeat(B).reshape(N, 1)
        cam = r.sample_cam_poses(N, 0.0, 0.0, 0.0, 0.0, False, given_yaws=yaws, given_pitches=torch.zeros((N, 1)))
    ray, eye, zd = torch.cat(cam[3]), torch.cat(cam[4]), torch.cat(cam[5])
    dhw = r._dhw_on_device().expand(B, -1, -1).contiguous()
    out = {k: torch.empty(s, device=dev) for k, s in (("color", (N, 3, S, S)), ("depth", (N, 1, S, S)), ("T", (N, 1, S, S)))}
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    kw = dict(views_per_mpi=V, check_last_plane=True, out_pm1=True, want_transmittance=True, defer_status=True, out=out, status=status)
    mpis = {(v, s): MPI(variant=v, strict_order=s, on_out_of_plane="raise") for v in ("auto", "lds", "gather") for s in (False, True)}
    row = dict(shape=name, dtype=tag, S=S, B=B, D=D, views=N, volume_mb=lay.numel() * lay.element_size() / 2 ** 20)

    def layers(variant, strict=False):
        with torch.no_grad():
            mpis[(variant, strict)].render_views_layers(lay, dhw, ray, eye, zd, **kw)

    def planar_render(variant, vol, strict=False):
        with torch.no_grad():
            mpis[(variant, strict)].render_views(vol, dhw, ray, eye, zd, **kw)

    def copy_and_render():
        planar_render("auto", lay.permute(0, 1, 4, 2, 3))   # (render_views makes the planar copy: _volume_operand)

    layers("lds")
    row["lay_peak_mb"] = peak(lambda: layers("auto"))
    row["copy_peak_mb"] = peak(copy_and_render)
    row["lay_lds"] = timed(lambda: layers("lds"))
    row["lay_gather"] = timed(lambda: layers("gather"))
    row["copy_plus_auto"] = timed(copy_and_render)
    torch.cuda.empty_cache()
    planar = lay.permute(0, 1, 4, 2, 3).contiguous()
    planar_render("auto", planar)   # (the band kernel's workspace exists before anything is measured)
    for v in ("auto", "lds", "gather"):
        row["planar_" + v] = timed(lambda: planar_render(v, planar))
    # the arithmetic contract at the size that is timed
    planar_render("gather", planar, strict=True)
    ref = {k: t.clone() for k, t in out.items()}
    layers("gather", strict=True)
    assert all(torch.equal(out[k], ref[k]) for k in out), "strict layers gather != strict planar gather"
    layers("lds", strict=True)
    assert all(torch.equal(out[k], ref[k]) for k in out), "strict layers lds != strict planar gather"
    layers("lds")
    row["lds_default_vs_strict"] = max(float((out[k] - ref[k]).abs().max()) / (2.0 if k == "color" else 1.0) for k in out)   # (colour is 2 c - 1 here)
    assert row["lds_default_vs_strict"] <= 1e-5, row["lds_default_vs_strict"]
    assert int(status[0].item()) == 0, int(status[0].item())
    for k in ("lay_gather", "copy_plus_auto", "planar_auto", "planar_lds", "planar_gather"):
        row["lay_lds_vs_" + k] = row["lay_lds"] / row[k]
    row["lay_gather_vs_planar_gather"] = row["lay_gather"] / row["planar_gather"]
    row["lay_gather_vs_copy_plus_auto"] = row["lay_gather"] / row["copy_plus_auto"]
    try:
        clock = f"{torch.cuda.clock_rate()} MHz"
    except Exception:  # noqa: BLE001 -- no SMI binding in this torch
        clock = "n/a"
    print("ROW " + " ".join(f"{k}={v:.3f}" if isinstance(v, float) and abs(v) >= 1e-3 else f"{k}={v:.2e}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items())
          + f" device={torch.cuda.get_device_name(0)!r} clock={clock}", flush=True)
    del planar, lay
    torch.cuda.empty_cache()


BACKWARD_SHAPES = [("256x32x8", 256, 8, 32), ("512x32x4", 512, 4, 32), ("1024x32x4", 1024, 4, 32)]


def one_backward(name, S, B, D, tag, reps):
    import ctypes
    import torch
    import ml_gmpi_amd
    from ml_gmpi_amd import MPI, _lib
    dev = torch.device("cuda:0")
    dtype = dict(f32=torch.float32, bf16=torch.bfloat16)[tag]
    lib = _lib.load_library()

    def timed(fn, n=reps):
        for _ in range(3):
            fn()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in evs:
            e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return sorted(a.elapsed_time(b) for a, b in evs)[n // 2]   # median

    def peak(fn, leaf):
        fn()
        leaf.grad = None   # (the warm-up step's gradient is no input: the measured step's own gradient is part of its peak)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20

    r = ml_gmpi_amd.make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise")
    r.set_cam(r.cam_fov, S, S)
    lay = torch.rand((B, D, S, S, 4), device=dev, generator=torch.Generator(device=dev).manual_seed(7300)).to(dtype).requires_grad_(True)
    torch.manual_seed(3)
    cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    ray, eye, zd = torch.cat(cam[3]), torch.cat(cam[4]), torch.cat(cam[5])
    dhw = r._dhw_on_device().expand(B, -1, -1).contiguous()
    g = torch.Generator(device=dev).manual_seed(7301)
    gc, gd = torch.randn((B, 3, S, S), device=dev, generator=g), torch.randn((B, 1, S, S), device=dev, generator=g)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    kw = dict(out_pm1=True, defer_status=True, status=status)
    mpi = MPI(on_out_of_plane="raise")
    row = dict(shape=name, dtype=tag, S=S, B=B, D=D, volume_mb=lay.numel() * lay.element_size() / 2 ** 20, grad_mb=lay.numel() * 4 / 2 ** 20)

    def step(leaf, mode=None):
        leaf.grad = None
        res = mpi.render_views(leaf, dhw, ray, eye, zd, **kw) if mode is None else mpi.render_views_layers(leaf, dhw, ray, eye, zd, layers_backward=mode, **kw)
        torch.autograd.backward([res["color"], res["depth"]], [gc, gd])   # (no loss kernels: the upstream gradients as they are)

    for mode in ("texel", "planar"):
        row[f"peak_{mode}_mb"] = peak(lambda: step(lay, mode), lay)
        row[f"step_{mode}"] = timed(lambda: step(lay, mode))
    grads = {}
    for mode in ("texel", "planar"):
        step(lay, mode)
        grads[mode] = lay.grad.float()
    scale = float(grads["planar"].abs().max())
    row["grad_diff"] = float((grads["texel"] - grads["planar"]).abs().max()) / scale
    if dtype is torch.float32:
        assert row["grad_diff"] <= 1e-5, row["grad_diff"]
    del grads
    lay.grad = None
    torch.cuda.empty_cache()
    # the two backward launches alone, through the C entries, over the structs the bridges build
    stream = torch.cuda.current_stream(dev).cuda_stream

    def struct(vol, **extra):
        with torch.no_grad():
            res = mpi.render_views(vol, dhw, ray, eye, zd, out_pm1=True, want_transmittance=True, _in_autograd_fn=True, **extra)
        return res["_bwd"][0], res   # (res keeps T and the tensors the struct points to alive)
    p_lay, hold_lay = struct(lay.detach(), _layers="auto")
    grad = torch.zeros(tuple(lay.shape), dtype=torch.float32, device=dev)
    gst = (ctypes.c_int64 * 5)(grad.stride(0), grad.stride(1), 1, grad.stride(2), 4)
    assert lib.gmpi_render_layers_backward_supports(ctypes.byref(p_lay), gst) == 1   # the tile kernel
    row["bwd_texel"] = timed(lambda: _lib.check(lib.gmpi_mpi_render_layers_backward_launch(ctypes.byref(p_lay), gc.data_ptr(), gd.data_ptr(), None, grad.data_ptr(), gst, stream),
                                                "layers backward"))
    row["fill"] = timed(lambda: grad.zero_())
    del grad
    planar = lay.detach().permute(0, 1, 4, 2, 3).contiguous()
    p_vol, hold_vol = struct(planar)
    p_vol.workspace, p_vol.workspace_bytes = None, 0   # (the atomic tile kernel: what the planar bridge of the layers launches)
    gradp = torch.zeros(tuple(planar.shape), dtype=torch.float32, device=dev)
    gstp = (ctypes.c_int64 * 5)(*gradp.stride())
    row["bwd_planar"] = timed(lambda: _lib.check(lib.gmpi_mpi_render_backward_launch(ctypes.byref(p_vol), gc.data_ptr(), gd.data_ptr(), gradp.data_ptr(), gstp, stream),
                                                 "planar backward"))
    del gradp, hold_vol
    volume = planar.requires_grad_(True)
    row["peak_volume_mb"] = peak(lambda: step(volume), volume)
    row["step_volume"] = timed(lambda: step(volume))
    assert int(status[0].item()) == 0, int(status[0].item())
    row["step_texel_vs_planar"] = row["step_texel"] / row["step_planar"]
    row["step_texel_vs_volume"] = row["step_texel"] / row["step_volume"]
    row["bwd_texel_vs_planar"] = row["bwd_texel"] / row["bwd_planar"]
    print("BROW " + " ".join(f"{k}={v:.3f}" if isinstance(v, float) and abs(v) >= 1e-3 else f"{k}={v:.2e}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items())
          + f" device={torch.cuda.get_device_name(0)!r}", flush=True)
    del volume, planar, lay, hold_lay
    torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--pass-backward":
        sys.path.insert(0, ROOT)
        for name, S, B, D in BACKWARD_SHAPES:
            for tag in ("f32", "bf16"):
                one_backward(name, S, B, D, tag, int(sys.argv[2]))
        sys.exit(0)
    child = "--pass"
    if len(sys.argv) > 1 and sys.argv[1] == "--backward":
        child = "--pass-backward"
        del sys.argv[1]
        if len(sys.argv) == 1:
            sys.argv.append("10")
    if len(sys.argv) > 1 and sys.argv[1] == "--pass":
        sys.path.insert(0, ROOT)
        for name, S, B, D, V, tags in SHAPES:
            for tag in tags:
                one(name, S, B, D, V, tag, int(sys.argv[2]))
        sys.exit(0)
    reps = sys.argv[1] if len(sys.argv) > 1 else "15"
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    print("times in ms (medians of", reps, "runs after 3 warm-up runs), memory in MiB above the inputs; one child process per pass;", passes, "passes", flush=True)
    for i in range(passes):
        print(f"== pass {i + 1} ==", flush=True)
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), child, reps], timeout=420).returncode
        except subprocess.TimeoutExpired:   # (run() has killed the child)
            rc = "time limit of 420 s"
        if rc != 0:
            print(f"pass {i + 1}: exit status {rc}; stopping")
            sys.exit(1)
