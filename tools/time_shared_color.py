"""Times the shared-colour layout (one colour image per MPI + D alpha planes + a background image) against the volume path it replaces, through the
C ABI, with HIP events (medians): at 256^2 x 8, 512^2 x 4 and 1024^2 x 4 with 32 planes in fp32 the whole G-step (forward, zero-fill, backward),
at 1024^2 x 96 x 4 (fp32, bf16) the forward only, and one camera-path launch (8 views of ONE 512^2 x 96 MPI along a yaw sweep of +-0.3 rad), forward only.
The shared forward is timed twice: the one-pixel-per-lane kernel ("shared_fwd": variant auto) and the staged kernel ("shared_fwd_staged": variant lds).

  baseline  materialise the expanded volume as the generator does (expand + two cat), forward (variant auto), zero-fill of the volume gradient,
            volume backward (tile kernels), plane sum of the colour gradient (the backward of the generator's expand)
  shared    forward, zero-fill of the three gradients, shared backward: one-pixel-per-lane kernel ("gather") and tile kernel separately
  shared, atomics-free pair    the same forward with gmpi_mpi_render_shared_backward_gather_launch (render_backward_gather.hip: pixel pass + texel gather,
            every gradient cell written once: no zero-fill): columns `shared_bwd_pair`, `shared_total_pair` (forward + pair), `pair_ws_mb` (the scratch
            it is lent), `pair_peak_mb` (peak memory of one pass, scratch included), `pair_runs` (plane runs per texel tile).  `pair_check`: the largest
            |pair - tile| / (1e-5 max|tile| + 1e-7) over the three gradients (<= 1 passes), `pair_repro`: 1 when two launches give the same bits;
            anything else ends the run

and the peak device memory of one pass of each (torch.cuda.max_memory_allocated).  Every shape runs in a child process of its own under a time
limit; the first failure ends the run.  usage: python tools/time_shared_color.py [--backward] [reps] [passes]   (--backward: only the shapes with a backward)"""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (S, MPIs, planes, storage, with backward, views per MPI)
SHAPES = [("256", 8, 32, "f32", 1, 1), ("512", 4, 32, "f32", 1, 1), ("1024", 4, 32, "f32", 1, 1), ("1024", 4, 96, "f32", 0, 1), ("1024", 4, 96, "bf16", 0, 1),
          ("512", 1, 96, "f32", 0, 8)]


def one(S, B, D, dtype_name, with_backward, reps, V=1):
    import torch
    sys.path.insert(0, ROOT)
    import ml_gmpi_amd
    from ml_gmpi_amd import _lib, expand_shared_color
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
    g = torch.Generator(device=dev).manual_seed(7000)
    rgb = torch.rand((B, 3, S, S), device=dev, generator=g).to(dtype)
    alpha = torch.rand((B, D, 1, S, S), device=dev, generator=g).to(dtype)
    bg = torch.rand((B, 3, S, S), device=dev, generator=g).to(dtype)
    N = B * V
    gc = torch.randn((N, 3, S, S), device=dev, generator=g)
    gd = torch.randn((N, 1, S, S), device=dev, generator=g)
    torch.manual_seed(3)
    if V == 1:
        cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    else:   # a camera path: V views of every MPI along a yaw sweep
        yaws = torch.linspace(-0.3, 0.3, V).repeat(B).reshape(N, 1)
        cam = r.sample_cam_poses(N, 0.0, 0.0, 0.0, 0.0, False, given_yaws=yaws, given_pitches=torch.zeros((N, 1)))
    ray, eye, zd = torch.cat(cam[3]), torch.cat(cam[4]), torch.cat(cam[5])
    dhw = r._dhw_on_device().expand(B, -1, -1).contiguous()
    kw = dict(views_per_mpi=V, check_last_plane=True, out_pm1=True, want_transmittance=True, defer_status=True)
    base_mem = torch.cuda.memory_allocated(dev)
    row = dict(S=S, B=B, D=D, dtype=dtype_name, views=N)

    # ---- baseline: the volume path of the parent commit ------------------------------------------------------------------------------------------
    torch.cuda.reset_peak_memory_stats(dev)
    vol = expand_shared_color(rgb, alpha, bg)
    out = {k: torch.empty(s, device=dev) for k, s in (("color", (N, 3, S, S)), ("depth", (N, 1, S, S)), ("T", (N, 1, S, S)))}
    with torch.no_grad():
        res = r.mpi.render_views(vol, dhw, ray, eye, zd, out=out, _in_autograd_fn=True, **kw)
    p = res.pop("_bwd")[0]   # (the tuple also holds the volume: dropped here, so that `del vol` below frees it)
    if with_backward:
        pb = _lib.GmpiRenderParams.from_buffer_copy(p)
        pb.rgb_out = pb.depth_out = pb.status = None
        grad = torch.zeros_like(vol, dtype=torch.float32)
        gs = (ctypes.c_int64 * 5)(*grad.stride())
        bwd = lambda: _lib.check(lib.gmpi_mpi_render_backward_launch(ctypes.byref(pb), gc.data_ptr(), gd.data_ptr(), grad.data_ptr(), gs, cs), "backward")
        bwd()
        plane_sum = lambda: (grad[:, :D - 1, :3].sum(1), grad[:, D - 1, :3].contiguous())
        plane_sum()
    torch.cuda.synchronize()
    row["base_peak_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20
    row["base_expand"] = timed(lambda: expand_shared_color(rgb, alpha, bg))
    with torch.no_grad():
        row["base_fwd"] = timed(lambda: r.mpi.render_views(vol, dhw, ray, eye, zd, out=out, **kw))
    if with_backward:
        row["base_fill"] = timed(lambda: grad.zero_())
        row["base_bwd"] = timed(bwd)
        row["base_sum"] = timed(plane_sum)
        del grad, bwd, plane_sum
    del vol, res, p
    torch.cuda.empty_cache()
    assert torch.cuda.memory_allocated(dev) - base_mem <= 4 * out["color"].numel() * 8, "the baseline's volume is still alive"

    # ---- shared --------------------------------------------------------------------------------------------------------------------------------
    torch.cuda.reset_peak_memory_stats(dev)
    with torch.no_grad():
        res = r.mpi.render_views_shared(rgb, alpha, dhw, ray, eye, zd, background=bg, out=out, _in_autograd_fn=True, **kw)
    p = res.pop("_bwd")[0]
    if with_backward:
        sc = _lib.GmpiSharedColor()
        sc.struct_size = ctypes.sizeof(_lib.GmpiSharedColor)
        sc.rgb, sc.background = rgb.data_ptr(), bg.data_ptr()
        for i in range(3):
            sc.rgb_stride[i], sc.background_stride[i] = rgb.stride(i), bg.stride(i)
        g_rgb, g_alpha, g_bg = torch.zeros_like(rgb, dtype=torch.float32), torch.zeros_like(alpha, dtype=torch.float32), torch.zeros_like(bg, dtype=torch.float32)
        s3 = lambda t, dims: (ctypes.c_int64 * 3)(*[t.stride(d) for d in dims])
        strides = (s3(g_rgb, (0, 1, 2)), s3(g_alpha, (0, 1, 3)), s3(g_bg, (0, 1, 2)))

        def shared_bwd(variant):
            q = _lib.GmpiRenderParams.from_buffer_copy(p)
            q.rgb_out = q.depth_out = q.status = None
            q.variant = variant
            return lambda: _lib.check(lib.gmpi_mpi_render_shared_backward_launch(
                ctypes.byref(q), ctypes.byref(sc), gc.data_ptr(), gd.data_ptr(), None, g_rgb.data_ptr(), strides[0], g_alpha.data_ptr(), strides[1],
                g_bg.data_ptr(), strides[2], cs), "shared backward")
        tile, gather = shared_bwd(_lib.VARIANT_AUTO), shared_bwd(_lib.VARIANT_GATHER)
        tile()
    torch.cuda.synchronize()
    row["shared_peak_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20
    if with_backward:
        # the atomics-free pair: its scratch, one pass's peak memory, twice the same bits, and its results at the timed size against the tile kernel's
        qp = _lib.GmpiRenderParams.from_buffer_copy(p)
        qp.rgb_out = qp.depth_out = qp.status = None
        qp.variant = _lib.VARIANT_AUTO
        need = int(lib.gmpi_render_layout_backward_gather_workspace_bytes(ctypes.byref(qp), ctypes.byref(sc), None))
        assert need > 0, "the pair does not take this launch"
        row["pair_runs"] = int(lib.gmpi_render_layout_backward_gather_runs(ctypes.byref(qp), ctypes.byref(sc), None))
        torch.cuda.reset_peak_memory_stats(dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        qp.workspace, qp.workspace_bytes = ws.data_ptr(), need
        qp.flags |= _lib.FLAG_GRAD_OVERWRITE
        pair = lambda: _lib.check(lib.gmpi_mpi_render_shared_backward_gather_launch(
            ctypes.byref(qp), ctypes.byref(sc), gc.data_ptr(), gd.data_ptr(), None, g_rgb.data_ptr(), strides[0], g_alpha.data_ptr(), strides[1],
            g_bg.data_ptr(), strides[2], cs), "shared backward, atomics-free pair")
        for t in (g_rgb, g_alpha, g_bg):
            t.fill_(float("nan"))
        pair()
        torch.cuda.synchronize()
        row["pair_ws_mb"] = need / 2 ** 20
        row["pair_peak_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20   # outputs, gradients and the scratch: shared_peak_mb + pair_ws_mb
        first = [t.clone() for t in (g_rgb, g_alpha, g_bg)]
        pair()
        row["pair_repro"] = int(all(torch.equal(t, f) for t, f in zip((g_rgb, g_alpha, g_bg), first)))
        for t in (g_rgb, g_alpha, g_bg):
            t.zero_()
        tile()
        row["pair_check"] = max(float((f - w).abs().max()) / (1e-5 * float(w.abs().max()) + 1e-7) for f, w in zip(first, (g_rgb, g_alpha, g_bg)))
        assert row["pair_check"] <= 1.0 and row["pair_repro"] == 1, ("the pair against the tile backward", row["pair_check"], row["pair_repro"])
        del first
    with torch.no_grad():
        row["shared_fwd"] = timed(lambda: r.mpi.render_views_shared(rgb, alpha, dhw, ray, eye, zd, background=bg, out=out, **kw))
        staged = r.mpi.render_views_shared(rgb, alpha, dhw, ray, eye, zd, background=bg, out=out, variant="lds", _in_autograd_fn=True, **kw)
        assert staged.pop("_bwd")[0].variant == _lib.VARIANT_LDS, "the staged kernel did not take this launch"
        row["shared_fwd_staged"] = timed(lambda: r.mpi.render_views_shared(rgb, alpha, dhw, ray, eye, zd, background=bg, out=out, variant="lds", **kw))
        row["staged_vs_one_pixel"] = row["shared_fwd_staged"] / row["shared_fwd"]
        row["staged_vs_auto_on_volume"] = row["shared_fwd_staged"] / row["base_fwd"]
        row["staged_vs_expand_plus_auto"] = row["shared_fwd_staged"] / (row["base_expand"] + row["base_fwd"])
    if with_backward:
        row["shared_fill"] = timed(lambda: (g_rgb.zero_(), g_alpha.zero_(), g_bg.zero_()))
        row["shared_bwd_tile"] = timed(tile)
        row["shared_bwd_gather"] = timed(gather)
        row["shared_bwd_pair"] = timed(pair)
        row["shared_total_pair"] = row["shared_fwd"] + row["shared_bwd_pair"]   # (no zero-fill: every cell is written)
        row["pair_vs_fill_plus_tile"] = row["shared_bwd_pair"] / (row["shared_fill"] + row["shared_bwd_tile"])
        row["base_total"] = row["base_expand"] + row["base_fwd"] + row["base_fill"] + row["base_bwd"] + row["base_sum"]
        row["shared_total_tile"] = row["shared_fwd"] + row["shared_fill"] + row["shared_bwd_tile"]
        row["shared_total_gather"] = row["shared_fwd"] + row["shared_fill"] + row["shared_bwd_gather"]
    try:
        clock = f"{torch.cuda.clock_rate()} MHz"
    except Exception:  # noqa: BLE001 -- no SMI binding in this torch
        clock = "n/a"
    print("ROW " + " ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()) + f" device={torch.cuda.get_device_name(0)!r} clock={clock}",
          flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        S, B, D, dt, bw, reps, V = sys.argv[2:9]
        one(int(S), int(B), int(D), dt, int(bw), int(reps), int(V))
        sys.exit(0)
    argv = [a for a in sys.argv[1:] if a != "--backward"]
    backward_only = len(argv) != len(sys.argv) - 1
    reps = argv[0] if len(argv) > 0 else "15"
    passes = int(argv[1]) if len(argv) > 1 else 1
    print("times in ms (medians of", reps, "runs after 3 warm-up runs), memory in MiB above the inputs; one child process per shape;", passes, "pass(es)")
    for k in range(passes):
        print(f"== pass {k + 1} ==", flush=True)
        for S, B, D, dt, bw, V in SHAPES:
            if backward_only and not bw:
                continue
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", S, str(B), str(D), dt, str(bw), reps, str(V)], timeout=240).returncode
            except subprocess.TimeoutExpired:   # (run() has killed the child)
                rc = "time limit of 240 s"
            if rc != 0:
                print(f"shape {S} x {B} x {D} {dt}: exit status {rc}; stopping")
                sys.exit(1)
