"""Times the depth-alpha layout (one colour image, one depth image and a background image per MPI; the alpha of plane k is a ramp of plane_z[k] - depth)
against the two paths that render it through tensors the layout does not need, through the C ABI, with HIP events (medians): 256^2 x 32 x 8, 512^2 x 32 x 4
and 1024^2 x 32 x 4 in fp32 the forward and the whole step (forward, zero-fill, backward), 1024^2 x 96 x 4 the forward only; each with n_z_bins = 4 (a ramp
several planes wide) and 256 (a step).

  depth    the new path: forward, zero-fill of the three gradient images, backward (render_depth.hip: one pixel per lane, both)
  depth, tile backward    the same forward and zero-fill with gmpi_mpi_render_depth_backward_tile_launch (render_depth_tile.hip: one workgroup per
           32 x 16 pixel tile, one LDS window for all planes): columns `depth_bwd_tile`, `depth_total_tile`.  The two depth backwards are timed
           ALTERNATELY in the same child (pixel, tile, pixel, tile, ...), and their gradients are compared per image (`tile_check`: the largest
           |tile - pixel| / (1e-5 max|pixel| + 1e-7) over the three images, <= 1 passes; a failure ends the run)
  depth, atomics-free pair    the same forward with gmpi_mpi_render_depth_backward_gather_launch (render_backward_gather.hip: pixel pass + texel gather,
           every gradient cell written once: no zero-fill): columns `depth_bwd_pair`, `depth_total_pair` (forward + pair), `pair_ws_mb` (the scratch it is
           lent), `pair_peak_mb` (peak memory of one pass, scratch included), `pair_runs` (plane runs per texel tile).  `pair_check`: the largest
           |pair - pixel| / (1e-5 max|pixel| + 1e-7) over the three images (<= 1 passes), `pair_repro`: 1 when two launches give the same bits; anything
           else ends the run
  volume   expand_depth_alpha (the ramp + the generator's expand and two cat), forward (variant auto), zero-fill of the volume gradient, volume backward
           (tile kernels), autograd through the expand (plane sums of the colour gradient, the clamp's mask and the plane sum for the depth)
  shared   the alpha planes materialised (depth_alpha_planes), render_views_shared (variant auto: one pixel per lane), zero-fill of the three gradients,
           shared backward (tile kernel), autograd through the ramp

  depth, window forward   `depth_forward="window"` (render_depth_window.hip: one workgroup per 32 x 16 pixel tile, every tap from one moving LDS window, planes
           in front of the window's nearest depth skipped): column `depth_fwd_window`.  The two forwards are timed ALTERNATELY in the same child (pixel,
           window, pixel, window, ...) -- `depth_fwd` is the one-pixel kernel's median of that interleaved run -- and their outputs are compared
           (`window_check`: 1 when colour, depth and T are bit-equal; anything else ends the run).  `window_vs_pixel` = depth_fwd_window / depth_fwd.
           A last shape is the 8-view camera path of ONE 512^2 x 96 MPI (views_per_mpi = 8), forward only.

and the peak device memory of one pass of each above the inputs (torch.cuda.max_memory_allocated).  Every shape runs in a child process of its own under a
time limit; the first failure ends the run.  usage: python tools/time_depth_alpha.py [--forward | --backward] [reps] [passes]   (--forward: no backward at
any shape; --backward: only the shapes with a backward)"""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (S, MPIs, planes, with backward, views per MPI)
SHAPES = [("256", 8, 32, 1, 1), ("512", 4, 32, 1, 1), ("1024", 4, 32, 1, 1), ("1024", 4, 96, 0, 1), ("512", 1, 96, 0, 8)]
N_Z_BINS = (4, 256)


def one(S, B, D, n_z_bins, with_backward, reps, views=1):
    import torch
    sys.path.insert(0, ROOT)
    import ml_gmpi_amd
    from ml_gmpi_amd import _lib, depth_alpha_bounds, depth_alpha_planes, expand_depth_alpha
    from ml_gmpi_amd.hip_mpi import _depth_alpha, _shared_color
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

    def timed_alternately(fa, fb, n=reps):
        for _ in range(3):
            fa(); fb()
        evs = [tuple(torch.cuda.Event(enable_timing=True) for _ in range(4)) for _ in range(n)]
        for e0, e1, e2, e3 in evs:
            e0.record(); fa(); e1.record()
            e2.record(); fb(); e3.record()
        torch.cuda.synchronize()
        return sorted(e[0].elapsed_time(e[1]) for e in evs)[n // 2], sorted(e[2].elapsed_time(e[3]) for e in evs)[n // 2]

    r = ml_gmpi_amd.make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise")
    r.set_cam(r.cam_fov, S, S)
    g = torch.Generator(device=dev).manual_seed(7000)
    rgb = torch.rand((B, 3, S, S), device=dev, generator=g)
    bg = torch.rand((B, 3, S, S), device=dev, generator=g)
    # a smooth surface with texel noise between the planes: 5 x 5 noise upsampled to 0.15 + 0.7 c, + 0.02 (U - 0.5)
    coarse = torch.rand((B, 1, 5, 5), device=dev, generator=g)
    depth = 0.15 + 0.7 * torch.nn.functional.interpolate(coarse, size=(S, S), mode="bilinear", align_corners=True)
    depth = (depth + 0.02 * (torch.rand((B, 1, S, S), device=dev, generator=g) - 0.5)).contiguous()
    plane_z = torch.linspace(0, 1, D, device=dev)
    zb = depth_alpha_bounds(1, n_z_bins)
    N = B * views
    gc = torch.randn((N, 3, S, S), device=dev, generator=g)
    gd = torch.randn((N, 1, S, S), device=dev, generator=g)
    torch.manual_seed(3)
    if views > 1:   # a camera path: yaw across the pose range, a little pitch
        gy = torch.linspace(-1, 1, N).reshape(N, 1) * (2 * r.horizontal_std)
        gp = torch.linspace(-1, 1, N).reshape(N, 1) * r.vertical_std
        cam = r.sample_cam_poses(N, 0.0, 0.0, 0.0, 0.0, False, given_yaws=gy, given_pitches=gp)
    else:
        cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    ray, eye, zd = torch.cat(cam[3]), torch.cat(cam[4]), torch.cat(cam[5])
    dhw = r._dhw_on_device().expand(B, -1, -1).contiguous()
    kw = dict(check_last_plane=True, out_pm1=True, want_transmittance=True, defer_status=True, views_per_mpi=views)
    out = {k: torch.empty(s, device=dev) for k, s in (("color", (N, 3, S, S)), ("depth", (N, 1, S, S)), ("T", (N, 1, S, S)))}
    s3 = lambda t, dims: (ctypes.c_int64 * 3)(*[t.stride(d) for d in dims])
    base_mem = torch.cuda.memory_allocated(dev)
    row = dict(S=S, B=B, D=D, n_z_bins=n_z_bins, views=N)

    def backward_struct(p):
        q = _lib.GmpiRenderParams.from_buffer_copy(p)
        q.rgb_out = q.depth_out = q.status = None
        return q

    # ---- volume: the expanded volume through the volume kernels --------------------------------------------------------------------------------
    torch.cuda.reset_peak_memory_stats(dev)
    ins = [t.clone().requires_grad_(True) for t in (rgb, depth, bg)] if with_backward else [rgb, depth, bg]
    vol_graph = expand_depth_alpha(ins[0], ins[1], plane_z, *zb, ins[2])
    vol = vol_graph.detach()
    with torch.no_grad():
        res = r.mpi.render_views(vol, dhw, ray, eye, zd, out=out, _in_autograd_fn=True, **kw)
    p = res.pop("_bwd")[0]
    frac_T = float((out["T"] < 1e-30).float().mean())   # pixels whose forward transmittance underflows: the backward re-walks those
    if with_backward:
        pb = backward_struct(p)
        grad = torch.zeros_like(vol)
        gs = (ctypes.c_int64 * 5)(*grad.stride())
        bwd = lambda: _lib.check(lib.gmpi_mpi_render_backward_launch(ctypes.byref(pb), gc.data_ptr(), gd.data_ptr(), grad.data_ptr(), gs, cs), "backward")
        bwd()
        through_expand = lambda: torch.autograd.grad(vol_graph, ins, grad, retain_graph=True)
        through_expand()
    torch.cuda.synchronize()
    row["volume_peak_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20
    with torch.no_grad():
        row["volume_expand"] = timed(lambda: expand_depth_alpha(rgb, depth, plane_z, *zb, bg))
        row["volume_fwd"] = timed(lambda: r.mpi.render_views(vol, dhw, ray, eye, zd, out=out, **kw))
    if with_backward:
        row["volume_fill"] = timed(lambda: grad.zero_())
        row["volume_bwd"] = timed(bwd)
        row["volume_expand_bwd"] = timed(through_expand)
        del grad, bwd, through_expand
    del vol, vol_graph, res, p, ins
    torch.cuda.empty_cache()
    assert torch.cuda.memory_allocated(dev) - base_mem <= 4 * out["color"].numel() * 8, "the volume is still alive"

    # ---- shared: the alpha planes materialised, shared-colour kernels ---------------------------------------------------------------------------
    torch.cuda.reset_peak_memory_stats(dev)
    dep_in = depth.clone().requires_grad_(True) if with_backward else depth
    alpha_graph = depth_alpha_planes(dep_in, plane_z, *zb)
    alpha = alpha_graph.detach()
    with torch.no_grad():
        res = r.mpi.render_views_shared(rgb, alpha, dhw, ray, eye, zd, background=bg, out=out, _in_autograd_fn=True, **kw)
    p = res.pop("_bwd")[0]
    sc = _shared_color(rgb, bg)
    if with_backward:
        ps = backward_struct(p)
        g_rgb, g_alpha, g_bg = torch.zeros_like(rgb), torch.zeros_like(alpha), torch.zeros_like(bg)
        st = (s3(g_rgb, (0, 1, 2)), s3(g_alpha, (0, 1, 3)), s3(g_bg, (0, 1, 2)))
        sbwd = lambda: _lib.check(lib.gmpi_mpi_render_shared_backward_launch(
            ctypes.byref(ps), ctypes.byref(sc), gc.data_ptr(), gd.data_ptr(), None, g_rgb.data_ptr(), st[0], g_alpha.data_ptr(), st[1], g_bg.data_ptr(), st[2], cs),
            "shared backward")
        sbwd()
        through_ramp = lambda: torch.autograd.grad(alpha_graph, dep_in, g_alpha, retain_graph=True)
        through_ramp()
    torch.cuda.synchronize()
    row["shared_peak_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20
    with torch.no_grad():
        row["shared_planes"] = timed(lambda: depth_alpha_planes(depth, plane_z, *zb))
        row["shared_fwd"] = timed(lambda: r.mpi.render_views_shared(rgb, alpha, dhw, ray, eye, zd, background=bg, out=out, **kw))
    if with_backward:
        row["shared_fill"] = timed(lambda: (g_rgb.zero_(), g_alpha.zero_(), g_bg.zero_()))
        row["shared_bwd"] = timed(sbwd)
        row["shared_planes_bwd"] = timed(through_ramp)
        del g_alpha, sbwd, through_ramp
    del alpha, alpha_graph, res, p, dep_in
    torch.cuda.empty_cache()

    # ---- depth: the new path ---------------------------------------------------------------------------------------------------------------------
    torch.cuda.reset_peak_memory_stats(dev)
    with torch.no_grad():
        res = r.mpi.render_views_depth(rgb, depth, plane_z, zb, dhw, ray, eye, zd, background=bg, out=out, _in_autograd_fn=True, **kw)
    p = res.pop("_bwd")[0]
    da = _depth_alpha(plane_z, *zb)
    if with_backward:
        pd = backward_struct(p)
        d_rgb, d_dep, d_bg = torch.zeros_like(rgb), torch.zeros_like(depth), torch.zeros_like(bg)
        st = (s3(d_rgb, (0, 1, 2)), s3(d_dep, (0, 1, 2)), s3(d_bg, (0, 1, 2)))
        depth_backward = lambda entry: lambda: _lib.check(entry(
            ctypes.byref(pd), ctypes.byref(sc), ctypes.byref(da), gc.data_ptr(), gd.data_ptr(), None, d_rgb.data_ptr(), st[0], d_dep.data_ptr(), st[1],
            d_bg.data_ptr(), st[2], cs), "depth backward")
        dbwd, dbwd_tile = depth_backward(lib.gmpi_mpi_render_depth_backward_launch), depth_backward(lib.gmpi_mpi_render_depth_backward_tile_launch)
        # the results at the timed size: tile against one pixel per lane, per gradient image
        dbwd()
        want = [t.clone() for t in (d_rgb, d_dep, d_bg)]
        for t in (d_rgb, d_dep, d_bg):
            t.zero_()
        dbwd_tile()
        row["tile_check"] = max(float((t - w).abs().max()) / (1e-5 * float(w.abs().max()) + 1e-7) for t, w in zip((d_rgb, d_dep, d_bg), want))
        assert all(float(w.abs().max()) > 0 for w in want) and row["tile_check"] <= 1.0, ("tile backward against the one-pixel backward", row["tile_check"])
        del want
    torch.cuda.synchronize()
    row["depth_peak_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20
    if with_backward:
        # the atomics-free pair: its scratch, one pass's peak memory, twice the same bits, and its results at the timed size against the one-pixel kernel's
        pg = backward_struct(p)
        pg.variant = _lib.VARIANT_AUTO
        need = int(lib.gmpi_render_layout_backward_gather_workspace_bytes(ctypes.byref(pg), ctypes.byref(sc), ctypes.byref(da)))
        assert need > 0, "the pair does not take this launch"
        row["pair_runs"] = int(lib.gmpi_render_layout_backward_gather_runs(ctypes.byref(pg), ctypes.byref(sc), ctypes.byref(da)))
        torch.cuda.reset_peak_memory_stats(dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        pg.workspace, pg.workspace_bytes = ws.data_ptr(), need
        pg.flags |= _lib.FLAG_GRAD_OVERWRITE
        dbwd_pair = lambda: _lib.check(lib.gmpi_mpi_render_depth_backward_gather_launch(
            ctypes.byref(pg), ctypes.byref(sc), ctypes.byref(da), gc.data_ptr(), gd.data_ptr(), None, d_rgb.data_ptr(), st[0], d_dep.data_ptr(), st[1],
            d_bg.data_ptr(), st[2], cs), "depth backward, atomics-free pair")
        for t in (d_rgb, d_dep, d_bg):
            t.fill_(float("nan"))
        dbwd_pair()
        torch.cuda.synchronize()
        row["pair_ws_mb"] = need / 2 ** 20
        row["pair_peak_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20   # outputs, gradients and the scratch: depth_peak_mb + pair_ws_mb
        first = [t.clone() for t in (d_rgb, d_dep, d_bg)]
        dbwd_pair()
        row["pair_repro"] = int(all(torch.equal(t, f) for t, f in zip((d_rgb, d_dep, d_bg), first)))
        for t in (d_rgb, d_dep, d_bg):
            t.zero_()
        dbwd()
        row["pair_check"] = max(float((f - w).abs().max()) / (1e-5 * float(w.abs().max()) + 1e-7) for f, w in zip(first, (d_rgb, d_dep, d_bg)))
        assert row["pair_check"] <= 1.0 and row["pair_repro"] == 1, ("the pair against the one-pixel backward", row["pair_check"], row["pair_repro"])
        del first
    with torch.no_grad():
        # the two forwards at the timed size: the window kernel must give the one-pixel kernel's bits
        fwd = lambda how: lambda: r.mpi.render_views_depth(rgb, depth, plane_z, zb, dhw, ray, eye, zd, background=bg, out=out, depth_forward=how, **kw)
        fwd("pixel")()
        want = {k: v.clone() for k, v in out.items()}
        for v in out.values():
            v.fill_(-7.0)
        fwd("window")()
        row["window_check"] = int(all(torch.equal(out[k], want[k]) for k in out) and r.mpi.depth_window_fallbacks == 0)
        assert row["window_check"] == 1, "window forward against the one-pixel forward"
        del want
        row["depth_fwd"], row["depth_fwd_window"] = timed_alternately(fwd("pixel"), fwd("window"))
    row["window_vs_pixel"] = row["depth_fwd_window"] / row["depth_fwd"]
    row["window_vs_auto_on_existing_volume"] = row["depth_fwd_window"] / row["volume_fwd"]
    row["window_vs_volume"] = row["depth_fwd_window"] / (row["volume_expand"] + row["volume_fwd"])
    if with_backward:
        row["depth_fill"] = timed(lambda: (d_rgb.zero_(), d_dep.zero_(), d_bg.zero_()))
        row["depth_bwd"], row["depth_bwd_tile"] = timed_alternately(dbwd, dbwd_tile)
        row["volume_total"] = row["volume_expand"] + row["volume_fwd"] + row["volume_fill"] + row["volume_bwd"] + row["volume_expand_bwd"]
        row["shared_total"] = row["shared_planes"] + row["shared_fwd"] + row["shared_fill"] + row["shared_bwd"] + row["shared_planes_bwd"]
        row["depth_total"] = row["depth_fwd"] + row["depth_fill"] + row["depth_bwd"]
        row["depth_total_tile"] = row["depth_fwd"] + row["depth_fill"] + row["depth_bwd_tile"]
        row["depth_bwd_pair"] = timed(dbwd_pair)
        row["depth_total_pair"] = row["depth_fwd"] + row["depth_bwd_pair"]   # (no zero-fill: every cell is written)
        row["pair_vs_fill_plus_pixel"] = row["depth_bwd_pair"] / (row["depth_fill"] + row["depth_bwd"])
        row["pair_vs_fill_plus_tile"] = row["depth_bwd_pair"] / (row["depth_fill"] + row["depth_bwd_tile"])
    row["fwd_vs_volume"] = row["depth_fwd"] / (row["volume_expand"] + row["volume_fwd"])
    row["fwd_vs_shared"] = row["depth_fwd"] / (row["shared_planes"] + row["shared_fwd"])
    row["fwd_vs_auto_on_existing_volume"] = row["depth_fwd"] / row["volume_fwd"]
    row["T_underflow_frac"] = frac_T
    try:
        clock = f"{torch.cuda.clock_rate()} MHz"
    except Exception:  # noqa: BLE001 -- no SMI binding in this torch
        clock = "n/a"
    print("ROW " + " ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()) + f" device={torch.cuda.get_device_name(0)!r} clock={clock}",
          flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        S, B, D, n, bw, reps, views = sys.argv[2:9]
        one(int(S), int(B), int(D), int(n), int(bw), int(reps), int(views))
        sys.exit(0)
    argv = [a for a in sys.argv[1:] if a not in ("--forward", "--backward")]
    forward_only, backward_only = "--forward" in sys.argv[1:], "--backward" in sys.argv[1:]
    reps = argv[0] if len(argv) > 0 else "15"
    passes = int(argv[1]) if len(argv) > 1 else 3
    print("times in ms (medians of", reps, "runs after 3 warm-up runs), memory in MiB above the inputs; one child process per shape;", passes, "passes")
    for k in range(passes):
        print(f"== pass {k + 1} ==", flush=True)
        for S, B, D, bw, views in SHAPES:
            if backward_only and not bw:
                continue
            for n in N_Z_BINS:
                try:
                    rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", S, str(B), str(D), str(n), str(0 if forward_only else bw), reps, str(views)], timeout=240).returncode
                except subprocess.TimeoutExpired:   # (run() has killed the child)
                    rc = "time limit of 240 s"
                if rc != 0:
                    print(f"shape {S} x {B} x {D} n_z_bins {n}: exit status {rc}; stopping")
                    sys.exit(1)
