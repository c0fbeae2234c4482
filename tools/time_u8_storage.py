"""Times the render of a uint8 RGBA volume (GMPI_DTYPE_U8: code c = c / 255) against the float storage types on the SAME volume, with HIP events
(medians), forward only, at 1024^2 x 96 x 4 views (config 3), 256^2 x 96 x 8 views (config 2) and 8 camera-path views of ONE 512^2 x 96 MPI
along a yaw sweep of +-0.3 rad (config 4):

  u8_lds, u8_gather        the staged kernel of render_u8.hip and the gather kernel's uint8 instance
  u8i_lds, u8i_gather      the same two kernels over the SAME codes held channels-last (layers_as_volume of [M, D, Ht, Wt, 4] layers), read in place;
                           their results are asserted to be the planar volume's, bit for bit
  u8i_copy_plus_lds        `.contiguous()` of the channels-last view + the planar staged kernel in one timed region: what a holder of layers paid
                           before the layout was read in place
  bf16_auto, bf16_lds      dequantize_volume(q, bfloat16) rendered with variant auto (the band kernel where it applies) and with the tile kernel
  f32_auto, f32_lds        the same on dequantize_volume(q)
  deq_bf16_plus_auto       dequantise to bf16 + variant auto in one timed region: what a holder of 8-bit data pays without the type

and the peak device memory above the inputs of one u8 render, of one in-place render of the channels-last volume (u8i_peak_mb), of one
copy-and-render of it (u8i_copy_peak_mb) and of one dequantise-and-render (torch.cuda.max_memory_allocated).  Every shape
runs in a child process of its own under a time limit; the first failure ends the run.  One pass over the shapes says nothing about the spread
between passes (clocks settle, boxes differ): `passes` repeats the whole pass in one session, each under a "== pass i ==" header, and
profiles/u8_storage.txt and profiles/u8_interleaved.txt record three.  usage: python tools/time_u8_storage.py [reps [passes]]   (defaults 15 and 3)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, S, MPIs, planes, views per MPI)
SHAPES = [("config3", 1024, 4, 96, 1), ("config2", 256, 8, 96, 1), ("config4", 512, 1, 96, 8)]


def one(name, S, B, D, V, reps):
    import torch
    sys.path.insert(0, ROOT)
    import ml_gmpi_amd
    from ml_gmpi_amd import MPI, dequantize_volume, layers_as_volume
    dev = torch.device("cuda:0")

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
    q = torch.randint(0, 256, (B, D, 4, S, S), device=dev, dtype=torch.uint8, generator=torch.Generator(device=dev).manual_seed(7100))
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
    mpis = {v: MPI(variant=v, on_out_of_plane="raise") for v in ("auto", "lds", "gather")}
    row = dict(shape=name, S=S, B=B, D=D, views=N, volume_u8_mb=q.numel() / 2 ** 20)

    def render(variant, vol):
        with torch.no_grad():
            mpis[variant].render_views(vol, dhw, ray, eye, zd, **kw)

    render("auto", q)   # (the workspace and the status words exist before anything is measured)
    torch.cuda.synchronize()
    base_mem = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    render("auto", q)
    torch.cuda.synchronize()
    row["u8_peak_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20
    row["u8_lds"] = timed(lambda: render("lds", q))
    row["u8_gather"] = timed(lambda: render("gather", q))
    ref = {k: v.clone() for k, v in out.items()}   # (the gather kernel's default-mode result: what the float renders are held against below)

    # the same codes channels-last, read in place
    qi = layers_as_volume(q.permute(0, 1, 3, 4, 2).contiguous())
    assert qi.stride(2) == 1 and qi.stride(4) == 4
    row["u8i_gather"] = timed(lambda: render("gather", qi))
    assert all(torch.equal(out[k], ref[k]) for k in out), "interleaved gather != planar gather"
    render("lds", q)
    staged = {k: v.clone() for k, v in out.items()}
    row["u8i_lds"] = timed(lambda: render("lds", qi))
    assert all(torch.equal(out[k], staged[k]) for k in out), "interleaved staged != planar staged"
    del staged

    def copy_and_render():
        render("lds", qi.contiguous())
    for key, fn in (("u8i_peak_mb", lambda: render("auto", qi)), ("u8i_copy_peak_mb", copy_and_render)):
        fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base_mem = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        row[key] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20
    row["u8i_copy_plus_lds"] = timed(copy_and_render)
    del qi
    torch.cuda.empty_cache()

    def deq_and_render():
        render("auto", dequantize_volume(q, torch.bfloat16))
    deq_and_render()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base_mem = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    deq_and_render()
    torch.cuda.synchronize()
    row["deq_bf16_peak_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20
    row["deq_bf16_plus_auto"] = timed(deq_and_render)
    torch.cuda.empty_cache()
    for tag, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        vol = dequantize_volume(q, dtype)
        row[tag + "_auto"] = timed(lambda: render("auto", vol))
        row[tag + "_lds"] = timed(lambda: render("lds", vol))
        if dtype is torch.float32:   # the same volume by definition: the three kernels agree to the default-mode bars
            err = max(float((out[k] - ref[k]).abs().max()) for k in out)
            assert err <= 2e-5, err
            row["f32_lds_vs_u8_gather_maxerr"] = err
        del vol
        torch.cuda.empty_cache()
    assert int(status[0].item()) == 0, int(status[0].item())
    for k in ("u8_gather", "bf16_auto", "bf16_lds", "f32_auto", "f32_lds", "deq_bf16_plus_auto"):
        row["u8_lds_vs_" + k] = row["u8_lds"] / row[k]
    for k in ("u8_lds", "u8i_gather", "bf16_auto", "bf16_lds", "u8i_copy_plus_lds"):
        row["u8i_lds_vs_" + k] = row["u8i_lds"] / row[k]
    row["u8i_gather_vs_u8_gather"] = row["u8i_gather"] / row["u8_gather"]
    try:
        clock = f"{torch.cuda.clock_rate()} MHz"
    except Exception:  # noqa: BLE001 -- no SMI binding in this torch
        clock = "n/a"
    print("ROW " + " ".join(f"{k}={v:.3f}" if isinstance(v, float) and abs(v) >= 1e-3 else f"{k}={v:.2e}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items())
          + f" device={torch.cuda.get_device_name(0)!r} clock={clock}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        name, S, B, D, V, reps = sys.argv[2:8]
        one(name, int(S), int(B), int(D), int(V), int(reps))
        sys.exit(0)
    reps = sys.argv[1] if len(sys.argv) > 1 else "15"
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    print("times in ms (medians of", reps, "runs after 3 warm-up runs), memory in MiB above the inputs; one child process per shape;", passes, "passes", flush=True)
    for i in range(passes):
        print(f"== pass {i + 1} ==", flush=True)
        for name, S, B, D, V in SHAPES:
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, str(S), str(B), str(D), str(V), reps], timeout=240).returncode
            except subprocess.TimeoutExpired:   # (run() has killed the child)
                rc = "time limit of 240 s"
            if rc != 0:
                print(f"shape {name}: exit status {rc}; stopping")
                sys.exit(1)
