"""Times the plane-chunked render (MPI.render_views_chunks: gmpi_mpi_render_chunk_launch per chunk, the per-pixel state carried in place) against what
it replaces, with HIP events (medians): 1024^2 x 96 x 1 view and 256^2 x 96 x 8 views, fp32 and bf16, chunks of 8, 16 and 32 planes, forward only; and
forward + backward at the 32-plane G-step shapes (256^2 x 8, 512^2 x 4, 1024^2 x 4, fp32; chunks of 8 and 16).  The chunks are views of ONE volume
tensor (it has to exist for the one-shot columns): what is timed is the launches, not a generator.

  chunked        render_views_chunks over the chunks, variant "lds" (what "auto" means for a chunk launch wherever the tile kernel takes the tensors)
  chunked_band   the same through the band kernel's carry instances (chunk_kernel="band": gmpi_mpi_render_chunk_band_launch, a table kernel per chunk)
  chunked_band_tile  chunk_kernel="band+tile": the band carry kernel and the gated tile carry kernel behind it, per chunk
  one_lds        the one-shot render_views of the whole volume with the same variant
  one_auto       the one-shot render_views with variant "auto" (the band kernel at these sizes, with its workspace)
  emulated       what the parent commit allows: per chunk render_views(..., want_transmittance=True) -- "auto" --, combined with image-sized torch ops
                 (C += T C_c, Z += T Z_c, T *= T_c: three passes per chunk); not bit-identical to the one-shot render
  *_peak_mb      peak device memory of one call above the inputs (volume, camera tensors): outputs, state, workspace
  err_*          max |colour difference| of `chunked`, `chunked_band` (against one_auto: the band kernel's own one-shot render) and `emulated` against one_lds (chunked: 0 is expected and asserted in strict order by the tests;
                 here the default mode runs)
  G-step rows    fwd+bwd of render_views (tile backward, zero-fill included) against render_views_chunks under autograd (one zero-filled buffer per chunk)

Every shape runs in a child process of its own under a time limit; the first failure ends the run.
usage: python tools/time_chunks.py [reps] [passes]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (S, MPIs = views, planes, storage, with backward, chunk sizes)
SHAPES = [("1024", 1, 96, "f32", 0, "8,16,32"), ("1024", 1, 96, "bf16", 0, "8,16,32"), ("256", 8, 96, "f32", 0, "8,16,32"), ("256", 8, 96, "bf16", 0, "8,16,32"),
          ("256", 8, 32, "f32", 1, "8,16"), ("512", 4, 32, "f32", 1, "8,16"), ("1024", 4, 32, "f32", 1, "8,16")]


def one(S, B, D, dtype_name, with_backward, reps, sizes):
    import torch
    sys.path.insert(0, ROOT)
    import ml_gmpi_amd
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
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        keep = fn()   # (the outputs stay alive while the peak is read)
        torch.cuda.synchronize()
        mb = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
        del keep
        return mb

    make = lambda variant: ml_gmpi_amd.make_renderer("FFHQ", n_planes=D, device=dev, on_out_of_plane="raise", kernel_variant=variant)
    r_lds, r_auto = make("lds"), make("auto")
    r_lds.set_cam(r_lds.cam_fov, S, S)
    g = torch.Generator(device=dev).manual_seed(7100)
    vol = torch.rand((B, D, 4, S, S), device=dev, generator=g)
    vol[:, :, 3] *= 0.25   # (every plane counts: nothing can be skipped behind an opaque one)
    vol = vol.to(dtype)
    torch.manual_seed(3)
    cam = r_lds.sample_cam_poses(B, r_lds.horizontal_mean, r_lds.horizontal_std, r_lds.vertical_mean, r_lds.vertical_std, True)
    ray, eye, zd = torch.cat(cam[3]), torch.cat(cam[4]), torch.cat(cam[5])
    dhw = r_lds._dhw_on_device().expand(B, -1, -1).contiguous()
    kw = dict(check_last_plane=True, out_pm1=False, want_transmittance=True, defer_status=True)
    cut = lambda t, Dc: [t[:, k:k + Dc] for k in range(0, D, Dc)]

    def emulated(Dc):
        C = Z = T = None
        for k in range(0, D, Dc):
            last = k + Dc >= D
            res = r_auto.mpi.render_views(vol[:, k:k + Dc], dhw[:, k:k + Dc].contiguous(), ray, eye, zd, **dict(kw, check_last_plane=last))
            if C is None:
                C, Z, T = res["color"], res["depth"], res["T"]
            else:
                C, Z, T = C + T * res["color"], Z + T * res["depth"], T * res["T"]
        return C, Z, T

    row = dict(S=S, views=B, D=D, dtype=dtype_name, stack_mb=vol.numel() * vol.element_size() / 2 ** 20)
    if not with_backward:
        with torch.no_grad():
            one_lds = lambda: r_lds.mpi.render_views(vol, dhw, ray, eye, zd, **kw)
            one_auto = lambda: r_auto.mpi.render_views(vol, dhw, ray, eye, zd, **kw)
            ref = one_lds()["color"].clone()
            ref_auto = one_auto()["color"].clone()
            row["one_lds"], row["one_auto"] = timed(one_lds), timed(one_auto)
            row["one_lds_peak_mb"], row["one_auto_peak_mb"] = peak(one_lds), peak(one_auto)
            for Dc in sizes:
                chunks = cut(vol, Dc)
                chunked = lambda: r_lds.mpi.render_views_chunks(chunks, dhw, ray, eye, zd, **kw)
                row[f"chunked_{Dc}"], row[f"emulated_{Dc}"] = timed(chunked), timed(lambda: emulated(Dc))
                row[f"chunked_{Dc}_peak_mb"], row[f"emulated_{Dc}_peak_mb"] = peak(chunked), peak(lambda: emulated(Dc))
                row[f"err_chunked_{Dc}"] = float((chunked()["color"] - ref).abs().max())
                for name, kernel in (("chunked_band", "band"), ("chunked_band_tile", "band+tile")):
                    banded = lambda: r_lds.mpi.render_views_chunks(chunks, dhw, ray, eye, zd, chunk_kernel=kernel, **kw)
                    row[f"{name}_{Dc}"], row[f"{name}_{Dc}_peak_mb"] = timed(banded), peak(banded)
                    row[f"err_{name}_{Dc}"] = float((banded()["color"] - ref_auto).abs().max())
                assert r_lds.mpi.chunk_band_fallbacks == 0
                row[f"err_emulated_{Dc}"] = float((emulated(Dc)[0] - ref).abs().max())
    else:
        gc = torch.randn((B, 3, S, S), device=dev, generator=g)
        gd = torch.randn((B, 1, S, S), device=dev, generator=g)
        kw = dict(check_last_plane=True, out_pm1=True, defer_status=True)

        def step(leaves, render):
            for t in leaves:
                t.grad = None
            res = render()
            ((res["color"] * gc).sum() + (res["depth"] * gd).sum()).backward()
            return [t.grad for t in leaves]

        whole = vol.clone().requires_grad_(True)
        one_step = lambda: step([whole], lambda: r_lds.mpi.render_views(whole, dhw, ray, eye, zd, **kw))
        ref = one_step()[0].clone()
        row["one_fwd_bwd"], row["one_fwd_bwd_peak_mb"] = timed(one_step), peak(one_step)
        for Dc in sizes:
            leaves = [c.clone().requires_grad_(True) for c in cut(vol, Dc)]
            chunk_step = lambda: step(leaves, lambda: r_lds.mpi.render_views_chunks(leaves, dhw, ray, eye, zd, **kw))
            got = torch.cat(chunk_step(), 1)
            row[f"grad_check_{Dc}"] = float((got - ref).abs().max()) / (1e-5 * float(ref.abs().max()))   # (<= 1: this project's bar between two kernels)
            assert row[f"grad_check_{Dc}"] <= 1.0, ("chunked gradients against the one-shot backward", Dc, row[f"grad_check_{Dc}"])
            del got
            row[f"chunked_fwd_bwd_{Dc}"], row[f"chunked_fwd_bwd_{Dc}_peak_mb"] = timed(chunk_step), peak(chunk_step)
    try:
        clock = f"{torch.cuda.clock_rate()} MHz"
    except Exception:  # noqa: BLE001 -- no SMI binding in this torch
        clock = "n/a"
    print("ROW " + " ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()) + f" device={torch.cuda.get_device_name(0)!r} clock={clock}",
          flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        S, B, D, dt, bw, reps, sizes = sys.argv[2:9]
        one(int(S), int(B), int(D), dt, int(bw), int(reps), [int(s) for s in sizes.split(",")])
        sys.exit(0)
    reps = sys.argv[1] if len(sys.argv) > 1 else "15"
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    print("times in ms (medians of", reps, "runs after 3 warm-up runs), memory in MiB above the inputs; one child process per shape;", passes, "pass(es)")
    for k in range(passes):
        print(f"== pass {k + 1} ==", flush=True)
        for S, B, D, dt, bw, sizes in SHAPES:
            try:
                rc = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "--one", S, str(B), str(D), dt, str(bw), reps, sizes],
                                    timeout=180).returncode
            except subprocess.TimeoutExpired:   # (run() has killed the child)
                rc = "time limit of 180 s"
            if rc != 0:
                print(f"shape {S} x {B} x {D} {dt}: exit status {rc}; stopping")
                sys.exit(1)
