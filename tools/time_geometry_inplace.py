"""Times the geometry backward over the volume AS STORED (gmpi_mpi_render_u8_geometry_backward_launch: planar and channels-last uint8 codes;
gmpi_mpi_render_layers_geometry_backward_launch: channels-last fp32 and bf16 layers -- d/d rays, eye, z_dir and dhw, read in place) against what a user
had to do before them: make the planar float volume and run the volume entry's geometry backward on it.  Through the C ABI, HIP events, medians;
256^2 x 32 x 8, 512^2 x 32 x 4 and 1024^2 x 32 x 4 (the shapes of profiles/geometry_backward_layouts.txt), texel noise, default mode.

  in place   the storage's forward (for T_out) is NOT timed; `geo`: the geometry pass alone (pixel kernel + slab reducer, all four outputs)
  before     `convert`: dequantize_volume(q) for the two uint8 layouts, layers.permute(0, 1, 4, 2, 3).contiguous() for the layers (the layers' own
             dtype); `vol_geo`: gmpi_mpi_render_geometry_backward_launch on that planar volume -- the same pass over a planar volume that already
             exists; `before_total` = convert + vol_geo: the path without the new entries
  peak       torch.cuda.max_memory_allocated above the inputs of: the in-place path (forward outputs, T, the four gradients, the workspace) and the
             path before (the same plus the planar volume and what the conversion allocates on the way), MiB; `storage_mb`: the stored volume itself
  check      the largest |in place - before| / (1e-4 max|before|) over the four gradients (<= 10 is the tests' bar on smooth inputs; these inputs
             are texel noise and the forwards of the two paths are different kernels: informative only)

Every shape runs in a child process of its own under a time limit; the first failure ends the run.
usage: python tools/time_geometry_inplace.py [reps] [passes]"""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(256, 8, 32), (512, 4, 32), (1024, 4, 32)]   # S, MPIs (one view each), planes
STORAGES = ("u8", "u8cl", "lay_f32", "lay_bf16")


def one(S, B, D, reps):
    import torch
    sys.path.insert(0, ROOT)
    import ml_gmpi_amd
    from ml_gmpi_amd import _lib, dequantize_volume, layers_as_volume
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
    gc = torch.randn((B, 3, S, S), device=dev, generator=g)
    gd = torch.randn((B, 1, S, S), device=dev, generator=g)
    torch.manual_seed(3)
    cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    ray, eye, zd = torch.cat(cam[3]), torch.cat(cam[4]), torch.cat(cam[5])
    dhw = r._dhw_on_device().expand(B, -1, -1).contiguous()
    kw = dict(check_last_plane=True, out_pm1=True, want_transmittance=True, defer_status=True, views_per_mpi=1)

    def geometry_outputs():
        return [torch.empty_like(t) for t in (ray, eye, zd, dhw)]

    def backward_struct(p, query):
        q = _lib.GmpiRenderParams.from_buffer_copy(p)
        q.rgb_out = q.depth_out = q.status = None
        need = int(getattr(lib, query)(ctypes.byref(q), 1))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        q.workspace, q.workspace_bytes = ws.data_ptr(), ws.numel()
        return q, ws

    for storage in STORAGES:
        codes = torch.randint(0, 256, (B, D, S, S, 4), device=dev, generator=g, dtype=torch.uint8)   # texel noise, channels-last
        codes[:, -1, :, :, 3] = 255
        if storage == "u8":
            store = codes.permute(0, 1, 4, 2, 3).contiguous()
        elif storage == "u8cl":
            store = layers_as_volume(codes)
        else:
            store = dequantize_volume(codes, torch.float32 if storage == "lay_f32" else torch.bfloat16)
        if storage != "u8cl":
            del codes
        layers = storage.startswith("lay")
        convert = (lambda: store.permute(0, 1, 4, 2, 3).contiguous()) if layers else (lambda: dequantize_volume(store).contiguous())
        entry = "gmpi_mpi_render_layers_geometry_backward_launch" if layers else "gmpi_mpi_render_u8_geometry_backward_launch"
        torch.cuda.synchronize()
        base_mem = torch.cuda.memory_allocated(dev)
        row = dict(storage=storage, S=S, B=B, D=D, storage_mb=store.numel() * store.element_size() / 2 ** 20)

        # ---- in place ---------------------------------------------------------------------------------------------------------------------------------
        torch.cuda.reset_peak_memory_stats(dev)
        with torch.no_grad():
            res = r.mpi.render_views(store, dhw, ray, eye, zd, _in_autograd_fn=True, **(dict(kw, _layers="auto") if layers else kw))
        q, ws = backward_struct(res.pop("_bwd")[0], "gmpi_render_geometry_inplace_workspace_bytes")
        outs = geometry_outputs()

        def geo():
            _lib.check(getattr(lib, entry)(ctypes.byref(q), gc.data_ptr(), gd.data_ptr(), None, *[t.data_ptr() for t in outs], cs), entry)
        geo()
        torch.cuda.synchronize()
        row["peak_inplace_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20
        row["geo"] = timed(geo)
        inplace_grads = [t.clone() for t in outs]
        del res, ws, outs, q

        # ---- before: the planar float volume, then the volume entry -----------------------------------------------------------------------------------
        torch.cuda.reset_peak_memory_stats(dev)
        with torch.no_grad():
            vol = convert()
            res = r.mpi.render_views(vol, dhw, ray, eye, zd, _in_autograd_fn=True, **kw)
        qv, wsv = backward_struct(res.pop("_bwd")[0], "gmpi_render_geometry_backward_workspace_bytes")
        outs = geometry_outputs()

        def vol_geo():
            _lib.check(lib.gmpi_mpi_render_geometry_backward_launch(ctypes.byref(qv), gc.data_ptr(), gd.data_ptr(), *[t.data_ptr() for t in outs], cs),
                       "volume geometry backward")
        vol_geo()
        torch.cuda.synchronize()
        row["peak_before_mb"] = (torch.cuda.max_memory_allocated(dev) - base_mem) / 2 ** 20
        row["vol_geo"] = timed(vol_geo)
        with torch.no_grad():
            row["convert"] = timed(lambda: convert(), n=max(reps // 2, 3))
        row["before_total"] = row["convert"] + row["vol_geo"]
        row["check"] = max(float((a - b).abs().max()) / (1e-4 * float(b.abs().max()) + 1e-30) for a, b in zip(inplace_grads, outs))
        print("ROW " + " ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()), flush=True)
        del res, wsv, outs, qv, vol, store, inplace_grads, convert
        if storage == "u8cl":
            del codes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        one(*map(int, sys.argv[2:6]))
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    for ps in range(passes):
        print(f"== pass {ps + 1} of {passes}, {reps} repetitions per figure (medians, ms) ==", flush=True)
        for S, B, D in SHAPES:
            # a fresh child per shape: its own context, its own allocator; a failure (or a time limit) ends the run
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(S), str(B), str(D), str(reps)], timeout=240).returncode
            if rc != 0:
                print(f"child {S} {B} {D} ended with status {rc}: stopping", flush=True)
                sys.exit(1)
