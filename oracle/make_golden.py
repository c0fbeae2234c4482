"""Generates tests/golden/*.npz by RUNNING THE REFERENCE ITSELF on CPU (fp32).

Run in the build container only (needs /root/reference):   python oracle/make_golden.py

The reference has no golden vectors of its own, so these fixtures are the
pin for the oracle (oracle/mpi_oracle.c), for the host-side geometry mirror and for the HIP path:

  render_*.npz   inputs (rgba by seed via oracle.synth_rgba, camera tensors exactly as the
                 reference's `sample_cam_poses` produced them) + outputs of the reference
                 `MPIRenderer.render` / `MPI.forward` (gmpi/core/mpi_renderer.py:387, mpi.py:308)
  backward_*.npz gradient of the reference w.r.t. the RGBA volume (autograd through MPIRenderer.render / MPI.forward,
                 the G-step's backward, train.py:740-779) for seeded output gradients
  geometry.npz   plane depths / dhws / c2w / rays / sampled poses of the reference's host-side
                 helpers (mpi_utils.py:21,787,652; cam_utils.py:734; camera.py:182;
                 mpi_renderer.py:337) for the dataset presets
  light_render_nonsquare.npz  LightRenderer.render and its intermediate quantities at two shapes with H != W (`python oracle/make_golden.py
                 light-nonsquare`, run_light_render_nonsquare)
  reference_seams.npz  what the reference hands this package at its seams (`python oracle/make_golden.py seams`,
                 run_seams): replayed by tests/test_install_reference.py without the reference
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle  # noqa: E402
import ref_import  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")

# name, preset, D, (Ht, Wt), S (render size), B views, align_corners, pose spec, rgba options
RENDER_CASES = [
    dict(name="ffhq_d8_32_ac1", preset="FFHQ", D=8, tex=(32, 32), S=32, B=2, ac=True, pose="random", seed=11),
    dict(name="ffhq_d8_32_ac0", preset="FFHQ", D=8, tex=(32, 32), S=32, B=2, ac=False, pose="random", seed=12),
    dict(name="ffhq_d6_tex48x40_extreme", preset="FFHQ", D=6, tex=(48, 40), S=24, B=2, ac=True,
         pose=[(0.578, 0.254), (-0.578, -0.254)], seed=13),
    dict(name="metfaces_d16_64_bf16", preset="MetFaces", D=16, tex=(64, 64), S=64, B=1, ac=True, pose="random",
         seed=14, bf16=True, last_alpha_one=True),
    dict(name="afhq_d5_tex20_img36", preset="AFHQCat", D=5, tex=(20, 20), S=36, B=1, ac=False, pose="random",
         seed=15),
    dict(name="ffhq_d4_alpha01", preset="FFHQ", D=4, tex=(16, 16), S=16, B=1, ac=True, pose=[(0.1, -0.05)],
         seed=16, alpha_binary=True),
    dict(name="ffhq_d32_256_cfg1", preset="FFHQ", D=32, tex=(256, 256), S=256, B=1, ac=True, pose="random",
         seed=1000),  # BASELINE.json configs[0]
]


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def build_rgba(case):
    Ht, Wt = case["tex"]
    rgba = oracle.synth_rgba(case["seed"], (case["B"], case["D"], 4, Ht, Wt),
                             last_alpha_one=case.get("last_alpha_one", False), bf16_round=case.get("bf16", False))
    if case.get("alpha_binary"):
        rgba[:, :, 3] = (rgba[:, :, 3] > 0.5).astype(np.float32)  # exercises a==1 (the 1e-10 term) and a==0
    return rgba


def run_render_case(ns, case):
    with quiet():
        r = ref_import.make_reference_renderer(ns, case["preset"], case["D"], align_corners=case["ac"])
        r.set_cam(r.cam_fov, case["S"], case["S"])
    B = case["B"]
    torch.manual_seed(case["seed"])
    if case["pose"] == "random":
        cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
    else:
        yaws = torch.tensor([[p[0]] for p in case["pose"]], dtype=torch.float32)
        pitches = torch.tensor([[p[1]] for p in case["pose"]], dtype=torch.float32)
        cam = r.sample_cam_poses(B, 0.0, 0.0, 0.0, 0.0, False, given_yaws=yaws, given_pitches=pitches)
    keys = ["batch_yaws", "batch_pitches", "batch_tf_c2w", "batch_ray_dir", "batch_eye_pos", "batch_z_dir"]
    infos = dict(zip(keys, cam))
    rgba = build_rgba(case)
    t_rgba = torch.from_numpy(rgba)
    if case.get("bf16"):
        t_rgba = t_rgba.to(torch.bfloat16)  # exact (values were rounded); reference upcasts, mpi_renderer.py:446
    with quiet():
        rgb, depth, c2w, angles = r.render(t_rgba, case["S"], case["S"], given_cam_infos=infos,
                                            assert_not_out_of_last_plane=True)
    # second formulation of the same composite (mpi.py:218-306) as an extra pin
    dhw = r.dynamic_mpi_plane_dhws.reshape(1, -1, 3).expand(B, -1, -1)
    with quiet():
        c_old, d_old = r.mpi.old_forward(batch_rgba=t_rgba.float(), batch_dhw=dhw, batch_ray_dir=cam[3],
                                         batch_eye_pos=cam[4], batch_z_dir=cam[5], separate_background=None)
    meta = {k: v for k, v in case.items()}
    np.savez(
        os.path.join(OUT, f"render_{case['name']}.npz"),
        meta=json.dumps(meta),
        dhw=dhw.contiguous().numpy().astype(np.float32),
        ray_dir=torch.cat(cam[3]).numpy(), eye=torch.cat(cam[4]).numpy(), zdir=torch.cat(cam[5]).numpy(),
        yaws=cam[0].numpy(), pitches=cam[1].numpy(), c2w=cam[2].numpy(),
        ref_rgb_pm1=rgb.numpy(), ref_depth=depth.numpy(), ref_angles=angles.numpy(),
        ref_old_color01=c_old.numpy(), ref_old_depth=d_old.numpy(),
    )
    print("wrote", case["name"], "rgb range", float(rgb.min()), float(rgb.max()))


def run_multiview_case(ns):
    """MPI.forward called directly with a ragged views-per-MPI list (mpi.py:331-354): M=2 MPIs, (2,1) views."""
    with quiet():
        r = ref_import.make_reference_renderer(ns, "FFHQ", 5)
        r.set_cam(r.cam_fov, 20, 20)
    torch.manual_seed(21)
    cam = r.sample_cam_poses(3, 0.0, 0.289, 0.0, 0.127, True)
    rgba = oracle.synth_rgba(21, (2, 5, 4, 24, 28))
    dhw = r.dynamic_mpi_plane_dhws.reshape(1, -1, 3).expand(2, -1, -1).contiguous()
    ray = [torch.cat(cam[3][:2]), cam[3][2]]
    eye = [torch.cat(cam[4][:2]), cam[4][2]]
    zd = [torch.cat(cam[5][:2]), cam[5][2]]
    color, depth = r.mpi(batch_rgba=torch.from_numpy(rgba), batch_dhw=dhw, batch_ray_dir=ray, batch_eye_pos=eye,
                         batch_z_dir=zd, separate_background=None, assert_not_out_of_last_plane=True)
    np.savez(os.path.join(OUT, "forward_ragged_views.npz"),
             meta=json.dumps(dict(seed=21, M=2, D=5, tex=(24, 28), S=20, views_per_mpi=[2, 1], ac=True)),
             dhw=dhw.numpy(), ray_dir=torch.cat(cam[3]).numpy(), eye=torch.cat(cam[4]).numpy(),
             zdir=torch.cat(cam[5]).numpy(), view_to_mpi=np.array([0, 0, 1], np.int32),
             ref_color01=color.numpy(), ref_depth=depth.numpy())
    print("wrote forward_ragged_views")


def run_geometry(ns):
    out = {}
    meta = {"presets": {}, "poses": []}
    for preset in ("FFHQ", "MetFaces", "AFHQCat"):
        for confined in (True, False):
            for D in (4, 32, 96):
                if not confined and D != 32:
                    continue
                with quiet():
                    r = ref_import.make_reference_renderer(ns, preset, D, confined=confined)
                key = f"dhw_{preset}_{'conf' if confined else 'free'}_{D}"
                out[key] = r.static_mpi_plane_dhws.numpy()
                meta["presets"][key] = dict(preset=preset, confined=confined, D=D)
    for method in ("uniform", "log-uniform", "sqrt", "squared", "inverse"):
        out[f"dist_{method}"] = ns.mpi_utils.sample_distance(0.95, 1.12, 12, method)
    # c2w + rays for given angles, 3 sphere setups
    with quiet():
        r = ref_import.make_reference_renderer(ns, "FFHQ", 4)
    for i, (S, yaw, pitch) in enumerate([(8, 0.0, 0.0), (8, 0.3, -0.1), (16, -0.578, 0.254), (5, 0.01, 0.2)]):
        with quiet():
            r.set_cam(r.cam_fov, S, S)
        cam = r.sample_cam_poses(1, 0.0, 0.0, 0.0, 0.0, False, given_yaws=torch.tensor([[yaw]]),
                                 given_pitches=torch.tensor([[pitch]]))
        out[f"pose{i}_c2w"] = cam[2].numpy()
        out[f"pose{i}_ray"] = cam[3][0].numpy()
        out[f"pose{i}_eye"] = cam[4][0].numpy()
        out[f"pose{i}_zdir"] = cam[5][0].numpy()
        meta["poses"].append(dict(S=S, yaw=yaw, pitch=pitch))
    with quiet():
        ra = ref_import.make_reference_renderer(ns, "AFHQCat", 4)
        ra.set_cam(ra.cam_fov, 6, 6)
    cam = ra.sample_cam_poses(2, 0.0, 0.0, 0.0, 0.0, False, given_yaws=torch.tensor([[0.2], [-0.4]]),
                              given_pitches=torch.tensor([[0.1], [0.3]]))
    out["afhq_c2w"] = cam[2].numpy()
    out["afhq_ray"] = torch.cat(cam[3]).numpy()
    # RNG-consuming pose sampling (truncated_gaussian / uniform / gaussian; random + deterministic sweeps)
    with quiet():
        r.set_cam(r.cam_fov, 4, 4)
    for j, (method, rnd, B) in enumerate([("truncated_gaussian", True, 5), ("uniform", True, 3),
                                         ("gaussian", True, 3), ("truncated_gaussian", False, 4)]):
        r.cam_sample_method = method
        torch.manual_seed(100 + j)
        cam = r.sample_cam_poses(B, 0.05, 0.289, -0.02, 0.127, rnd)
        out[f"sample{j}_yaws"] = cam[0].numpy()
        out[f"sample{j}_pitches"] = cam[1].numpy()
        out[f"sample{j}_c2w"] = cam[2].numpy()
        out[f"sample{j}_after"] = torch.rand(2).numpy()  # RNG stream position after the call
        meta.setdefault("samples", []).append(dict(method=method, random=rnd, B=B, seed=100 + j))
    # video-style call: std 0 through the truncated_gaussian sampler (render_video.py:236-237 pattern)
    r.cam_sample_method = "truncated_gaussian"
    torch.manual_seed(200)
    cam = r.sample_cam_poses(1, 0.25, 0.0, 0.0, 0.0, True)
    out["video_yaws"] = cam[0].numpy()
    out["video_c2w"] = cam[2].numpy()
    out["video_after"] = torch.rand(2).numpy()
    np.savez(os.path.join(OUT, "geometry.npz"), meta=json.dumps(meta), **out)
    print("wrote geometry", len(out), "arrays")


def run_light_depth():
    """LightRenderer.compute_depth (light_renderer.py:82-100).  The module imports torchvision at import time (not
    installed here, not on this function's path): a stand-in module is registered first."""
    import importlib
    import types
    if "torchvision" not in sys.modules:
        tv = types.ModuleType("torchvision")
        tv.transforms = types.SimpleNamespace(GaussianBlur=lambda **k: None)
        sys.modules["torchvision"] = tv
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    ref_import._install_stubs()
    lr = importlib.import_module("gmpi.core.light_renderer")
    B, D, S = 2, 12, 40
    rgba = oracle.synth_rgba(77, (B, D, 4, S, S))
    rgba[0, :, 3] = (rgba[0, :, 3] > 0.7).astype(np.float32)  # exact 0/1 alphas in one batch element
    alpha = torch.from_numpy(rgba)[:, :, 3:]
    ds = torch.from_numpy(ref_import.import_reference().mpi_utils.sample_distance(0.95, 1.12, D, "inverse"))
    depth = lr.LightRenderer.compute_depth(None, alpha, ds.reshape(-1, 1))
    np.savez(os.path.join(OUT, "light_compute_depth.npz"), meta=json.dumps(dict(seed=77, B=B, D=D, S=S)),
             plane_ds=ds.numpy(), ref_depth=depth.numpy())
    print("wrote light_compute_depth", tuple(depth.shape))


def _torchvision_stand_in():
    """torchvision is not installed in this image.  `LightRenderer.__init__` only needs
    torchvision.transforms.GaussianBlur(kernel_size, sigma); the stand-in restates torchvision's functional
    `gaussian_blur` (transforms/_functional_tensor.py): 1-D kernels = pdf samples on linspace(-(k-1)/2, (k-1)/2, k)
    normalised to 1, 2-D kernel = their outer product, reflect padding by k//2, depthwise conv2d.  Everything else on
    the path (compute_depth, compute_pcl, get_normal, the shading and the pose sampling) is the reference's own code."""
    import types

    class GaussianBlur(torch.nn.Module):
        def __init__(self, kernel_size, sigma):
            super().__init__()
            self.kernel_size, self.sigma = tuple(kernel_size), tuple(sigma)

        @staticmethod
        def _k1d(k, s):
            lim = (k - 1) * 0.5
            x = torch.linspace(-lim, lim, steps=k)
            pdf = torch.exp(-0.5 * (x / s).pow(2))
            return pdf / pdf.sum()

        def forward(self, img):
            kx, ky = self._k1d(self.kernel_size[0], self.sigma[0]), self._k1d(self.kernel_size[1], self.sigma[1])
            k2d = torch.mm(ky[:, None], kx[None, :]).to(img.dtype)
            c = img.shape[-3]
            k2d = k2d.expand(c, 1, k2d.shape[0], k2d.shape[1])
            pad = [self.kernel_size[0] // 2, self.kernel_size[0] // 2, self.kernel_size[1] // 2, self.kernel_size[1] // 2]
            return torch.nn.functional.conv2d(torch.nn.functional.pad(img, pad, mode="reflect"), k2d, groups=c)

    tv = types.ModuleType("torchvision")
    tv.transforms = types.SimpleNamespace(GaussianBlur=GaussianBlur)
    return tv


def run_light_render():
    """LightRenderer.render (light_renderer.py:122-199) on a small MPI: the reference class end to end (seeded light
    pose), with the torchvision stand-in above for the blur."""
    import importlib
    sys.modules["torchvision"] = _torchvision_stand_in()
    sys.modules.pop("gmpi.core.light_renderer", None)
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    ns = ref_import.import_reference()
    lr = importlib.import_module("gmpi.core.light_renderer")
    B, D, S = 2, 6, 32
    r = ref_import.make_reference_renderer(ns, "FFHQ", D)
    xyz, _ = r.get_xyz(S, S, ret_single_res=True)  # [D,S,S,3]
    rgba = oracle.synth_rgba(79, (B, D, 4, S, S), last_alpha_one=True)
    # smooth alpha so that the surface (and its normals) are not pure noise
    a = torch.from_numpy(rgba[:, :, 3:4].reshape(B * D, 1, S, S))
    a = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(a, (3, 3, 3, 3), mode="replicate"), 7, stride=1)
    rgba[:, :, 3] = a.reshape(B, D, S, S).numpy()
    rgba[:, -1, 3] = 1.0
    out = {}
    for name, kw, steps in (("kd", dict(ka_max=0.6, kd_max=0.9, n_grow_iters=4), 3), ("ambient", dict(ka_max=1.0, kd_max=0.0, n_grow_iters=2), 2)):
        L = lr.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, **kw)
        torch.manual_seed(123)
        res = None
        for _ in range(steps):  # `step` ramps ka/kd (light_renderer.py:176-179)
            res = L.render(torch.from_numpy(rgba), r.static_mpi_plane_dhws, xyz)
        out[f"ref_{name}"] = res.numpy()
        torch.manual_seed(123)  # the light direction of the LAST step, re-derived with the reference's own sampler
        for _ in range(steps):
            c2w, _, _ = ns.cam_utils.gen_sphere_path(n_cams=B, sphere_center=L.sphere_center, sphere_r=L.sphere_r,
                                                     yaw_mean=L.l_h_mean, yaw_std=L.l_h_std, pitch_mean=L.l_v_mean,
                                                     pitch_std=L.l_v_std, n_truncated_stds=2, flag_rnd=True,
                                                     sample_method="truncated_gaussian", given_yaws=None, given_pitches=None)
        pos = torch.as_tensor(c2w[:, :3, 3], dtype=torch.float32)
        out[f"light_dir_{name}"] = ns.torch_utils.normalize_vecs(torch.FloatTensor(L.sphere_center).reshape(1, 3) - pos).numpy()
        out[f"ka_kd_{name}"] = np.array([L.cur_ka, L.cur_kd], dtype=np.float64)
        out[f"rng_after_{name}"] = torch.rand(2).numpy()
    np.savez(os.path.join(OUT, "light_render.npz"), meta=json.dumps(dict(seed=79, B=B, D=D, S=S)), rgba=rgba,
             dhw=r.static_mpi_plane_dhws.numpy(), xyz=xyz.numpy(), **out)
    print("wrote light_render", {k: v.shape for k, v in out.items()})


NONSQUARE_LIGHT_CASES = (("21x37", 21, 37, 81), ("50x18", 50, 18, 82))   # name, H, W, seed: W % 4 != 0, H < W and H > W
LIGHT_TEXEL_PITCH = 0.2473 / 32


def light_grid(plane_ds, H, W, pitch=LIGHT_TEXEL_PITCH):
    """A synthetic `mpi_tex_pix_xyz` [D,H,W,3]: texel centres on a grid of constant pitch in x (along W) and y (along H), centred on the
    axis, z = the plane's distance.  `LightRenderer.render` reads only the last plane's grid."""
    D = len(plane_ds)
    xyz = np.empty((D, H, W, 3), np.float32)
    xyz[..., 0] = ((np.arange(W, dtype=np.float64) - (W - 1) / 2) * pitch).astype(np.float32)[None, None, :]
    xyz[..., 1] = ((np.arange(H, dtype=np.float64) - (H - 1) / 2) * pitch).astype(np.float32)[None, :, None]
    xyz[..., 2] = np.asarray(plane_ds, np.float32).reshape(D, 1, 1)
    return xyz


def run_light_render_nonsquare():
    """tests/golden/light_render_nonsquare.npz: the reference's `LightRenderer.render` (and its `compute_depth`, `blurrer_func`, `compute_pcl`,
    `get_normal`, for the intermediate quantities) at two shapes with H != W, on a synthetic texel grid; same torchvision stand-in as
    run_light_render.  ka + kd > 1: some rgb * shading clip at 1."""
    import importlib
    sys.modules["torchvision"] = _torchvision_stand_in()
    sys.modules.pop("gmpi.core.light_renderer", None)
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    ns = ref_import.import_reference()
    lr = importlib.import_module("gmpi.core.light_renderer")
    B, D = 2, 5
    with quiet():
        dhw = ref_import.make_reference_renderer(ns, "FFHQ", D).static_mpi_plane_dhws
    out = {"dhw": dhw.numpy()}
    for name, H, W, seed in NONSQUARE_LIGHT_CASES:
        xyz = torch.from_numpy(light_grid(dhw[:, 0].numpy(), H, W))
        rgba = oracle.synth_rgba(seed, (B, D, 4, H, W), last_alpha_one=True)
        a = torch.from_numpy(rgba[:, :, 3:4].reshape(B * D, 1, H, W))
        for _ in range(3):   # (one pass, as run_light_render, leaves the fp32 chain 1.1e-5 from float64 at this pitch: above the 1e-5 the tests ask)
            a = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(a, (3, 3, 3, 3), mode="replicate"), 7, stride=1)
        rgba[:, :, 3] = a.reshape(B, D, H, W).numpy()
        rgba[:, -1, 3] = 1.0
        vol = torch.from_numpy(rgba)
        L = lr.LightRenderer(sphere_center_z=1.0, sphere_r=1.0, ka_max=0.6, kd_max=0.9, n_grow_iters=2)
        torch.manual_seed(321)
        for _ in range(3):   # the third call renders with the full ka, kd
            res = L.render(vol, dhw, xyz)
        torch.manual_seed(321)
        for _ in range(3):
            c2w, _, _ = ns.cam_utils.gen_sphere_path(n_cams=B, sphere_center=L.sphere_center, sphere_r=L.sphere_r,
                                                     yaw_mean=L.l_h_mean, yaw_std=L.l_h_std, pitch_mean=L.l_v_mean,
                                                     pitch_std=L.l_v_std, n_truncated_stds=2, flag_rnd=True,
                                                     sample_method="truncated_gaussian", given_yaws=None, given_pitches=None)
        pos = torch.as_tensor(c2w[:, :3, 3], dtype=torch.float32)
        depth = L.compute_depth(vol[:, :, 3:], dhw[:, :1])
        pcl = L.compute_pcl(vol[:, :, 3:], dhw, xyz)
        out.update({f"rgba_{name}": rgba, f"xyz_last_{name}": xyz[-1].numpy(), f"ref_{name}": res.numpy(),
                    f"light_dir_{name}": ns.torch_utils.normalize_vecs(torch.FloatTensor(L.sphere_center).reshape(1, 3) - pos).numpy(),
                    f"ka_kd_{name}": np.array([L.cur_ka, L.cur_kd], dtype=np.float64),
                    f"ref_depth_{name}": depth.numpy(), f"ref_blurred_{name}": L.blurrer_func(depth).numpy(),
                    f"ref_normal_{name}": L.get_normal(pcl).numpy()})
    np.savez(os.path.join(OUT, "light_render_nonsquare.npz"),
             meta=json.dumps(dict(B=B, D=D, pitch=LIGHT_TEXEL_PITCH, cases=[list(c) for c in NONSQUARE_LIGHT_CASES])), **out)
    print("wrote light_render_nonsquare", {k: v.shape for k, v in out.items()})


def run_backward_cases(ns):
    """Gradient of the reference w.r.t. the RGBA volume: autograd through the reference's own MPIRenderer.render /
    MPI.forward (mpi.py:308-436), exactly what the G-step back-propagates (train.py:740-779), fp32 on the CPU.
    loss = sum(rgb * g_rgb) + sum(depth * g_depth) with seeded normal g's."""
    keys = ["batch_yaws", "batch_pitches", "batch_tf_c2w", "batch_ray_dir", "batch_eye_pos", "batch_z_dir"]
    cases = [
        dict(name="ffhq_d8_32", D=8, S=32, B=2, seed=31, ac=True),
        dict(name="ffhq_d8_32_opaque", D=8, S=32, B=1, seed=32, ac=True, opaque=True),
        dict(name="ffhq_d6_tex40_img24_ac0", D=6, S=24, tex=40, B=2, seed=33, ac=False),
    ]
    for case in cases:
        with quiet():
            r = ref_import.make_reference_renderer(ns, "FFHQ", case["D"], align_corners=case["ac"])
            r.set_cam(r.cam_fov, case["S"], case["S"])
        B, D, S, T = case["B"], case["D"], case["S"], case.get("tex", case["S"])
        torch.manual_seed(case["seed"])
        cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
        rgba = oracle.synth_rgba(case["seed"], (B, D, 4, T, T), last_alpha_one=True)
        if case.get("opaque"):  # exactly and nearly opaque planes in the middle of the stack (the 1e-10 term matters)
            rgba[:, 2, 3, :, : T // 2] = 1.0
            rgba[:, 4, 3, :, T // 4:] = np.float32(1.0 - 1e-6)
            rgba[:, 3:6, 3, : T // 3, :] = 1.0
        vol = torch.from_numpy(rgba).requires_grad_(True)
        with quiet():
            rgb, depth, _, _ = r.render(vol, S, S, given_cam_infos=dict(zip(keys, cam)))
        g = torch.Generator().manual_seed(case["seed"] + 100)
        g_rgb, g_depth = torch.randn(rgb.shape, generator=g), torch.randn(depth.shape, generator=g)
        ((rgb * g_rgb).sum() + (depth * g_depth).sum()).backward()
        dhw = r.dynamic_mpi_plane_dhws.reshape(1, -1, 3).expand(B, -1, -1)
        np.savez(os.path.join(OUT, f"backward_{case['name']}.npz"), meta=json.dumps(case), rgba=rgba,
                 dhw=dhw.contiguous().numpy().astype(np.float32), ray_dir=torch.cat(cam[3]).numpy(),
                 eye=torch.cat(cam[4]).numpy(), zdir=torch.cat(cam[5]).numpy(), g_rgb=g_rgb.numpy(), g_depth=g_depth.numpy(),
                 ref_rgb_pm1=rgb.detach().numpy(), ref_depth=depth.detach().numpy(), ref_grad_rgba=vol.grad.numpy())
        print("wrote backward", case["name"], "max |grad|", float(vol.grad.abs().max()))
    # MPI.forward called directly with a ragged views-per-MPI list (M = 2 MPIs, (2, 1) views): gradients of two views
    # accumulate into MPI 0
    with quiet():
        r = ref_import.make_reference_renderer(ns, "FFHQ", 5)
        r.set_cam(r.cam_fov, 20, 20)
    torch.manual_seed(34)
    cam = r.sample_cam_poses(3, 0.0, 0.289, 0.0, 0.127, True)
    rgba = oracle.synth_rgba(34, (2, 5, 4, 24, 28))
    vol = torch.from_numpy(rgba).requires_grad_(True)
    dhw = r.dynamic_mpi_plane_dhws.reshape(1, -1, 3).expand(2, -1, -1).contiguous()
    color, depth = r.mpi(batch_rgba=vol, batch_dhw=dhw, batch_ray_dir=[torch.cat(cam[3][:2]), cam[3][2]],
                         batch_eye_pos=[torch.cat(cam[4][:2]), cam[4][2]], batch_z_dir=[torch.cat(cam[5][:2]), cam[5][2]],
                         separate_background=None)
    g = torch.Generator().manual_seed(134)
    g_rgb, g_depth = torch.randn(color.shape, generator=g), torch.randn(depth.shape, generator=g)
    ((color * g_rgb).sum() + (depth * g_depth).sum()).backward()
    np.savez(os.path.join(OUT, "backward_forward_ragged_views.npz"),
             meta=json.dumps(dict(seed=34, M=2, D=5, tex=(24, 28), S=20, views_per_mpi=[2, 1], ac=True)), rgba=rgba,
             dhw=dhw.numpy(), ray_dir=torch.cat(cam[3]).numpy(), eye=torch.cat(cam[4]).numpy(), zdir=torch.cat(cam[5]).numpy(),
             view_to_mpi=np.array([0, 0, 1], np.int32), g_rgb=g_rgb.numpy(), g_depth=g_depth.numpy(),
             ref_color01=color.detach().numpy(), ref_depth=depth.detach().numpy(), ref_grad_rgba=vol.grad.numpy())
    print("wrote backward_forward_ragged_views")


def _seam_value(out, meta, key, v):
    """One keyword argument of a recorded call: tensors (and lists of them, stacked) into the npz, everything else into meta."""
    if torch.is_tensor(v):
        out[key] = v.detach().numpy()
        meta[key] = "tensor"
    elif isinstance(v, (list, tuple)) and v and all(torch.is_tensor(x) for x in v):
        out[key] = torch.stack([x.detach() for x in v]).numpy()
        meta[key] = "tensor_list"
    elif isinstance(v, (list, tuple)):
        out[key] = np.asarray(v, dtype=np.float32)
        meta[key] = "number_list"
    else:
        meta[key] = {"value": v}


def run_seams(ns):
    """reference_seams.npz: what the reference hands this package at its seams, replayed without the reference by
    tests/test_install_reference.py and tests/test_host_geometry.py:
      rng_after_ctor  torch.rand(3) after torch.manual_seed(77) and the reference's FFHQ renderer with 4 planes (the RNG its constructor draws)
      cam_dirs_*      its camera's unit directions [3, S*S] (camera.py:117), the right operand of its ray product (camera.py:200)
      ctor_*          the keyword arguments its MPIRenderer gives `MPI(...)` (mpi_renderer.py:47), and that renderer's plane dhws
      fwd_*           the keyword arguments its MPIRenderer.render gives `MPI.forward` (mpi_renderer.py:451-461): FFHQ, 6 planes, 3 views of
                      20^2 over 24^2 textures drawn after torch.manual_seed(5)
      video_*         the calls its video driver `generate_img` (eval/vis/render_video.py:95-130) makes to MPIRenderer.render for 5 angles
                      (a fake generator -- seeded torch.rand volumes -- stands in for the network)"""
    import importlib
    import types
    out, meta = {}, {}
    torch.manual_seed(77)
    with quiet():
        ref_import.make_reference_renderer(ns, "FFHQ", 4)
    out["rng_after_ctor"] = torch.rand(3).numpy()
    # the camera-space unit directions the reference's ray product multiplies (camera.py:117, 200), for the image sizes of geometry.npz's poses
    for preset, size in (("FFHQ", 8), ("FFHQ", 16), ("FFHQ", 5), ("AFHQCat", 6)):
        with quiet():
            r = ref_import.make_reference_renderer(ns, preset, 4)
            r.set_cam(r.cam_fov, size, size)
        out[f"cam_dirs_{preset}_{size}"] = r.cam.ray_dir_torch.numpy()

    ctor, seen = {}, {}

    class SpyMPI(ns.mpi.MPI):
        def __init__(self, *a, **kw):
            assert not a, a
            ctor.update(kw)
            super().__init__(**kw)

        def forward(self, **kw):
            seen.update(kw)
            return super().forward(**kw)

    saved = ns.mpi_renderer.MPI
    ns.mpi_renderer.MPI = SpyMPI
    try:
        with quiet():
            r = ref_import.make_reference_renderer(ns, "FFHQ", 4)
        meta["ctor"] = {"kwargs": ctor, "preset": "FFHQ", "D": 4}
        out["ctor_static_dhws"] = r.static_mpi_plane_dhws.numpy()
        B, D, S, T = 3, 6, 20, 24
        with quiet():
            r = ref_import.make_reference_renderer(ns, "FFHQ", D)
            r.set_cam(r.cam_fov, S, S)
        torch.manual_seed(5)
        rgba = torch.rand(B, D, 4, T, T)
        with quiet():
            r.render(rgba, S, S, assert_not_out_of_last_plane=True)
    finally:
        ns.mpi_renderer.MPI = saved
    fwd_meta = {}
    for k, v in seen.items():
        _seam_value(out, fwd_meta, "fwd_" + k, v)
    meta["fwd"] = dict(B=B, D=D, S=S, T=T, seed=5, kwargs=fwd_meta)

    # the video driver: torchvision / imageio / torch_ema are imported by render_video.py but are not on the render path
    def stub(name, **attrs):
        m = sys.modules.get(name) or types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules.setdefault(name, m)
        return m
    if importlib.util.find_spec("torchvision") is None:
        stub("torchvision").utils = stub("torchvision.utils", save_image=lambda *a, **k: None)
        stub("torchvision.transforms")
    if importlib.util.find_spec("imageio") is None:
        stub("imageio", mimwrite=lambda *a, **k: None, imwrite=lambda *a, **k: None)
    if importlib.util.find_spec("torch_ema") is None:
        stub("torch_ema", ExponentialMovingAverage=type("ExponentialMovingAverage", (), {"__init__": lambda self, *a, **k: None}))
    rv = importlib.import_module("gmpi.eval.vis.render_video")
    D, S, T = 5, 24, 32
    kw = dict(ref_import.PRESETS["FFHQ"])
    kw.update(n_mpi_planes=D, plan_spatial_enlarge_factor=1.001, plane_distances_sample_method="inverse",
              cam_sample_method="truncated_gaussian", mpi_align_corners=True, use_xyz_ztype="depth", use_normalized_xyz=False,
              normalized_xyz_range="-11", use_confined_volume=True, device=torch.device("cpu"))
    with quiet():
        renderer = rv.MPIRenderer(**kw)                           # as render_video.py:168-189
        ws = renderer.get_xyz_interpolate_ws(D, D)                # :193
        renderer.set_cam(kw["cam_fov"], S, S)                     # :198
        xyz, _ = renderer.get_xyz(T, T, ret_single_res=False, only_z=False)   # :200-205
    calls, gen_calls = [], []
    ref_render = renderer.render

    def spy_render(*a, **k):
        calls.append((a, k))
        return ref_render(*a, **k)
    renderer.render = spy_render
    rv.mpi_renderer = renderer                                    # the module global generate_img reads (:104)

    def fake_generator(z, c, xyz_input, only_z, n_planes, z_interpolation_ws=None, truncation_psi=1.0):
        gen_calls.append(n_planes)
        return torch.rand((z.shape[0], n_planes, 4, T, T), generator=torch.Generator().manual_seed(11))

    angles = np.linspace(0.5, -0.5, 5).tolist()                   # :236-237 (100 angles there)
    metadata = dict(img_size=S, h_mean=0.0, v_mean=0.0, h_stddev=0.0, v_stddev=0.0, ray_start=kw["plane_min_d"], ray_end=kw["plane_max_d"])
    torch.manual_seed(0)
    z = torch.randn((1, 16))
    with quiet():
        rv.generate_img(device=torch.device("cpu"), face_angles=angles, generator=fake_generator, z=z, mpi_xyz_input=xyz, metadata=metadata,
                        horizontal_cam_move=True, mpi_xyz_only_z=False, z_interpolation_ws=ws, n_planes=D, truncation_psi=1.0,
                        render_single_image=False, chunk_n_planes=-1, disable_tqdm=True)
    assert gen_calls == [D, D] and len(calls) == len(angles), (gen_calls, len(calls))
    vol = calls[0][0][0]
    assert all(a[0] is vol or torch.equal(a[0], vol) for a, _ in calls)   # one unchanged volume for the whole path
    out["video_rgba"] = vol.detach().numpy()
    meta["video"] = dict(D=D, S=S, T=T, angles=angles, renderer_kwargs={k: v for k, v in kw.items() if k != "device"},
                         generator_calls=gen_calls, calls=[dict(size=[a[1], a[2]], kwargs=k) for a, k in calls])
    np.savez(os.path.join(OUT, "reference_seams.npz"), meta=json.dumps(meta, default=lambda o: np.asarray(o).tolist()), **out)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "seams":
        torch.set_num_threads(1)
        run_seams(ref_import.import_reference())
        return
    if len(sys.argv) > 1 and sys.argv[1] == "backward":
        torch.set_num_threads(1)
        run_backward_cases(ref_import.import_reference())
        return
    if len(sys.argv) > 1 and sys.argv[1] == "light":
        os.makedirs(OUT, exist_ok=True)
        torch.set_num_threads(1)
        run_light_depth()
        run_light_render()
        run_light_render_nonsquare()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "light-nonsquare":
        os.makedirs(OUT, exist_ok=True)
        torch.set_num_threads(1)
        run_light_render_nonsquare()
        return
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(1)
    ns = ref_import.import_reference()
    for case in RENDER_CASES:
        run_render_case(ns, case)
    run_multiview_case(ns)
    run_backward_cases(ns)
    run_geometry(ns)
    run_light_depth()
    run_light_render()
    run_light_render_nonsquare()
    with open(os.path.join(OUT, "PROVENANCE.txt"), "w") as f:
        f.write("Generated by oracle/make_golden.py from the reference at /root/reference "
                "(apple/ml-gmpi @ 2024_08_07), CPU fp32, torch %s, numpy %s.\n" % (torch.__version__, np.__version__))


if __name__ == "__main__":
    main()
