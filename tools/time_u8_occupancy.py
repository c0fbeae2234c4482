"""Times the sparse render of uint8 RGBA volumes (`occupancy=`, gmpi_mpi_render_u8_sparse_launch) against the dense staged uint8 kernel of the same build,
with HIP events (medians), forward only, at 1024^2 x 96 x 4 views (config 3), 256^2 x 96 x 8 views (config 2) and 8 camera-path views of ONE 512^2 x 96
MPI along a yaw sweep of +-0.3 rad (config 4), on three volumes built from a seed, each held planar and channels-last:

  noise   white-noise codes, alpha in 1..255: nothing can be skipped -- the price of asking
  ramp    the depth-alpha ramp of a dome depth image, quantized: empty in front of the surface, opaque behind it
  shell   the same dome, alpha non-zero for about two plane spacings around the surface and exactly 0 elsewhere: what a stored MPI looks like

Rows, per shape, volume and layout (all in one child process, on one box):

  dense       the staged uint8 kernel (variant "lds"), no occupancy
  sparse      the same launch with occupancy=; dense and sparse ALTERNATE run by run inside the timed loop; the results are asserted equal bit for bit
  map_build   build_occupancy(q) alone (once per volume, not per render)
  skipped     the share of (tile, plane) pairs the sparse launch skipped, read from its counters
  bf16_auto   variant "auto" (the band kernel where it applies) on dequantize_volume(q, bfloat16): the "convert once" comparison

Every shape runs in a child process of its own under a time limit; the first failure ends the run.  The whole pass is repeated `passes` times in one session
and the table holds min-max over the passes.  Nothing is routed by these numbers.
usage: python tools/time_u8_occupancy.py [reps [passes [out]]]   (defaults 15, 3 and profiles/u8_occupancy.txt)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, S, MPIs, planes, views per MPI)
SHAPES = [("config3", 1024, 4, 96, 1), ("config2", 256, 8, 96, 1), ("config4", 512, 1, 96, 8)]
KINDS = ("noise", "ramp", "shell")
SEED = 7200


def make_volume(kind, B, D, S, dev):
    """uint8 codes [B,D,4,S,S] on the device: white-noise colours; the alpha of `kind` (the constructions of tests/_u8_occupancy_cases.py)."""
    import torch
    from ml_gmpi_amd import depth_alpha_planes
    g = torch.Generator(device=dev).manual_seed(SEED + S + D)
    q = torch.randint(0, 256, (B, D, 4, S, S), device=dev, dtype=torch.uint8, generator=g)
    if kind == "noise":
        q[:, :, 3] = torch.randint(1, 256, (B, D, S, S), device=dev, dtype=torch.uint8, generator=g)
        return q
    c = torch.arange(S, device=dev, dtype=torch.float32) + 0.5
    r2 = ((c[None, :] - S / 2) ** 2 + (c[:, None] - S / 2) ** 2) / (0.45 * S) ** 2
    depth = torch.where(r2 <= 1.0, 0.8 - 0.6 * torch.sqrt((1.0 - r2).clamp(0.0, 1.0)), torch.full_like(r2, 4.0)).reshape(1, 1, S, S)
    plane_z, sp = torch.linspace(0.0, 1.0, D, device=dev), 1.0 / (D - 1)
    a = depth_alpha_planes(depth, plane_z, -0.5 * sp, 0.5 * sp)
    if kind == "shell":
        a = a - depth_alpha_planes(depth + sp, plane_z, -0.5 * sp, 0.5 * sp)
    q[:, :, 3] = torch.round(a[:, :, 0].clamp(0, 1) * 255.0).to(torch.uint8)   # (one MPI's planes, broadcast over the batch)
    return q


def one(name, S, B, D, V, reps):
    import torch
    sys.path.insert(0, ROOT)
    import ml_gmpi_amd
    from ml_gmpi_amd import MPI, build_occupancy, dequantize_volume, layers_as_volume, occupancy_reference
    dev = torch.device("cuda:0")

    def events(n):
        return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]

    def median(evs):
        return sorted(a.elapsed_time(b) for a, b in evs)[len(evs) // 2]

    def timed(fn, n=reps):
        for _ in range(3):
            fn()
        evs = events(n)
        for e0, e1 in evs:
            e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return median(evs)

    r = ml_gmpi_amd.make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise")
    r.set_cam(r.cam_fov, S, S)
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
    lds, auto = MPI(variant="lds", on_out_of_plane="raise"), MPI(variant="auto", on_out_of_plane="raise")

    def render(mpi, vol, occ=None):
        with torch.no_grad():
            mpi.render_views(vol, dhw, ray, eye, zd, **({} if occ is None else {"occupancy": occ}), **kw)

    for kind in KINDS:
        planar = make_volume(kind, B, D, S, dev)
        bf16 = dequantize_volume(planar, torch.bfloat16)
        bf16_auto = timed(lambda: render(auto, bf16))
        del bf16
        torch.cuda.empty_cache()
        for layout in ("planar", "channels_last"):
            q = planar if layout == "planar" else layers_as_volume(planar.permute(0, 1, 3, 4, 2).contiguous())
            occ = build_occupancy(q, stats=True)
            assert torch.equal(occ.map, occupancy_reference(q))
            render(lds, q)
            dense_out = {k: v.clone() for k, v in out.items()}
            occ.stats.zero_()
            render(lds, q, occ)
            torch.cuda.synchronize()
            assert all(torch.equal(out[k].view(torch.int32), dense_out[k].view(torch.int32)) for k in out), "sparse != dense"
            skipped, staged = (int(v) for v in occ.stats.cpu().to(torch.int64).tolist())
            del dense_out
            for _ in range(3):
                render(lds, q), render(lds, q, occ)
            ev_d, ev_s = events(reps), events(reps)
            for (d0, d1), (s0, s1) in zip(ev_d, ev_s):   # dense and sparse alternate
                d0.record(); render(lds, q); d1.record()
                s0.record(); render(lds, q, occ); s1.record()
            torch.cuda.synchronize()
            row = dict(shape=name, kind=kind, layout=layout, dense=median(ev_d), sparse=median(ev_s), map_build=timed(lambda: build_occupancy(q)),
                       skipped=skipped / max(skipped + staged, 1), bf16_auto=bf16_auto, empty_blocks=float((occ.map == 0).float().mean()))
            assert lds.occupancy_fallbacks == 0 and int(status[0].item()) == 0
            print("ROW " + " ".join(f"{k}={v:.4f}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()), flush=True)
            del q, occ
        del planar
        torch.cuda.empty_cache()
    print(f"DEVICE {torch.cuda.get_device_name(0)!r}", flush=True)


def table(rows, passes):
    """min-max over the passes of every figure, one line per shape, volume and layout; sparse / dense per pass."""
    keys, seen = {}, []
    for r in rows:
        k = (r["shape"], r["kind"], r["layout"])
        if k not in keys:
            seen.append(k)
        keys.setdefault(k, []).append(r)

    def span(rs, f, fmt="{:.3f}"):
        v = [f(r) for r in rs]
        return f"{fmt.format(min(v))}-{fmt.format(max(v))}"
    lines = [f"min-max over {passes} passes; times in ms", f"{'shape':8s} {'volume':6s} {'layout':13s} {'dense':>13s} {'sparse':>13s} {'sparse/dense':>13s} {'map_build':>13s} "
             f"{'skipped':>11s} {'empty_blocks':>12s} {'bf16_auto':>13s} {'sparse/bf16':>13s}"]
    for k in seen:
        rs = keys[k]
        lines.append(f"{k[0]:8s} {k[1]:6s} {k[2]:13s} {span(rs, lambda r: r['dense']):>13s} {span(rs, lambda r: r['sparse']):>13s} "
                     f"{span(rs, lambda r: r['sparse'] / r['dense'], '{:.2f}'):>13s} {span(rs, lambda r: r['map_build']):>13s} {span(rs, lambda r: r['skipped'], '{:.3f}'):>11s} "
                     f"{rs[0]['empty_blocks']:12.3f} {span(rs, lambda r: r['bf16_auto']):>13s} {span(rs, lambda r: r['sparse'] / r['bf16_auto'], '{:.2f}'):>13s}")
    return lines


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        name, S, B, D, V, reps = sys.argv[2:8]
        one(name, int(S), int(B), int(D), int(V), int(reps))
        sys.exit(0)
    reps = sys.argv[1] if len(sys.argv) > 1 else "15"
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "u8_occupancy.txt")
    log = [f"tools/time_u8_occupancy.py: times in ms (medians of {reps} runs after 3 warm-up runs, dense and sparse alternating); one child process per shape; {passes} passes"]
    print(log[0], flush=True)
    rows = []
    for i in range(passes):
        log.append(f"== pass {i + 1} ==")
        print(log[-1], flush=True)
        for name, S, B, D, V in SHAPES:
            try:
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, str(S), str(B), str(D), str(V), reps], timeout=240,
                                     stdout=subprocess.PIPE, text=True)
                rc, text = res.returncode, res.stdout
            except subprocess.TimeoutExpired:   # (run() has killed the child)
                rc, text = "time limit of 240 s", ""
            print(text, end="", flush=True)
            log.extend(text.splitlines())
            if rc != 0:
                print(f"shape {name}: exit status {rc}; stopping")
                sys.exit(1)
            for line in text.splitlines():
                if line.startswith("ROW "):
                    row = dict(f.split("=", 1) for f in line[4:].split())
                    rows.append({k: (v if k in ("shape", "kind", "layout") else float(v)) for k, v in row.items()})
    lines = table(rows, passes)
    print("\n".join(lines), flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines + [""] + log) + "\n")
