"""The inputs of the shading-augmentation shape tests, in one place: tests/test_light_shapes_cpu.py checks on the CPU that every case's bar means
something (noise floor of the fp32 chain, discriminating power against a transposed grid and a shifted depth, a gradient that reaches every tensor),
tests/test_hip_light_shapes.py runs the kernels on exactly these inputs.  CPU only (numpy / torch), never imported by the product."""
import numpy as np
import torch
import torch.nn.functional as F

import oracle
from _torch_ref import torch_light_render

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
B, D = 2, 5
KA, KD = 0.6, 0.9                      # ka + kd > 1: rgb * shading clips at 1 where the surface faces the light
PITCH = 0.2473 / 32                    # texel pitch of the grid, both axes
PLANE_DS = (1.0 / np.linspace(1.0 / 0.95, 1.0 / 1.12, D)).astype(np.float32)   # inverse-depth spacing, as the presets
LIGHT_DIRS = np.array([[0.06, 0.25, 0.966], [-0.14, 0.23, 0.962]], dtype=np.float64)
LIGHT_DIRS = (LIGHT_DIRS / np.linalg.norm(LIGHT_DIRS, axis=1, keepdims=True)).astype(np.float32)   # towards +z, as the augmentation's lights
BLUR_KSIZE = 9
SMOOTHING_PASSES = 3

# (5, 7): the smallest the 9-tap reflect blur allows; W % 4 = 1, 2, 3; (24, 260) / (8, 1032): a second x-block of the scalar / vector instances
SHAPES = [(21, 37), (50, 18), (5, 7), (9, 6), (32, 33), (32, 34), (32, 35), (24, 260), (8, 1032), (40, 256)]
LAYOUTS = ("contiguous", "rowpad4", "rowpad1", "expand", "offset1", "chanslice")
WIDE = 64                             # shapes wider than this are exempt from the 1e-5 cap on n0 (see NOISE_CAP)
NOISE_CAP = 1e-5


def _cases():
    out = {}
    for i, (H, W) in enumerate(SHAPES):
        for dt in DTYPES:
            out[f"{H}x{W}-{dt}-contiguous"] = dict(H=H, W=W, dtype=dt, layout="contiguous", seed=100 + i)
    for lay in LAYOUTS[1:]:
        for dt in DTYPES:               # W % 4 == 0: "rowpad4" and "chanslice" stay on the vector instances, the others leave them
            out[f"40x256-{dt}-{lay}"] = dict(H=40, W=256, dtype=dt, layout=lay, seed=109)
    for lay in ("rowpad1", "expand", "offset1", "chanslice"):
        out[f"21x37-f32-{lay}"] = dict(H=21, W=37, dtype="f32", layout=lay, seed=100)
    out["24x260-bf16-rowpad4"] = dict(H=24, W=260, dtype="bf16", layout="rowpad4", seed=107)
    out["8x1032-f16-rowpad4"] = dict(H=8, W=1032, dtype="f16", layout="rowpad4", seed=108)
    return out


CASES = _cases()

# n0 = max |oracle.light_shade (fp32) - float64 torch_light_render| on the case's stored values, as tests/test_light_shapes_cpu.py computes and
# prints it (rounded up to two digits); the expanded batch renders element 0 under both lights and has a floor of its own.
# The GPU bar of a case is max(1e-5, 4 * n0).
N0 = {
    "21x37-f32-contiguous": 7.9e-06,
    "21x37-bf16-contiguous": 6.8e-06,
    "21x37-f16-contiguous": 7.0e-06,
    "50x18-f32-contiguous": 9.8e-06,
    "50x18-bf16-contiguous": 8.1e-06,
    "50x18-f16-contiguous": 8.3e-06,
    "5x7-f32-contiguous": 4.3e-06,
    "5x7-bf16-contiguous": 4.5e-06,
    "5x7-f16-contiguous": 4.6e-06,
    "9x6-f32-contiguous": 4.8e-06,
    "9x6-bf16-contiguous": 5.4e-06,
    "9x6-f16-contiguous": 5.8e-06,
    "32x33-f32-contiguous": 8.1e-06,
    "32x33-bf16-contiguous": 7.4e-06,
    "32x33-f16-contiguous": 7.4e-06,
    "32x34-f32-contiguous": 6.3e-06,
    "32x34-bf16-contiguous": 6.8e-06,
    "32x34-f16-contiguous": 6.5e-06,
    "32x35-f32-contiguous": 7.8e-06,
    "32x35-bf16-contiguous": 6.8e-06,
    "32x35-f16-contiguous": 7.8e-06,
    "24x260-f32-contiguous": 9.5e-06,
    "24x260-bf16-contiguous": 8.8e-06,
    "24x260-f16-contiguous": 1.1e-05,
    "8x1032-f32-contiguous": 1.4e-05,
    "8x1032-bf16-contiguous": 1.8e-05,
    "8x1032-f16-contiguous": 2.6e-05,
    "40x256-f32-contiguous": 8.9e-06,
    "40x256-bf16-contiguous": 8.8e-06,
    "40x256-f16-contiguous": 9.0e-06,
    "40x256-f32-rowpad4": 8.9e-06,
    "40x256-bf16-rowpad4": 8.8e-06,
    "40x256-f16-rowpad4": 9.0e-06,
    "40x256-f32-rowpad1": 8.9e-06,
    "40x256-bf16-rowpad1": 8.8e-06,
    "40x256-f16-rowpad1": 9.0e-06,
    "40x256-f32-expand": 8.9e-06,
    "40x256-bf16-expand": 8.6e-06,
    "40x256-f16-expand": 8.8e-06,
    "40x256-f32-offset1": 8.9e-06,
    "40x256-bf16-offset1": 8.8e-06,
    "40x256-f16-offset1": 9.0e-06,
    "40x256-f32-chanslice": 8.9e-06,
    "40x256-bf16-chanslice": 8.8e-06,
    "40x256-f16-chanslice": 9.0e-06,
    "21x37-f32-rowpad1": 7.9e-06,
    "21x37-f32-expand": 7.9e-06,
    "21x37-f32-offset1": 7.9e-06,
    "21x37-f32-chanslice": 7.9e-06,
    "24x260-bf16-rowpad4": 8.8e-06,
    "8x1032-f16-rowpad4": 2.6e-05,
}


def bar(name):
    return max(1e-5, 4 * N0[name])


def texel_grid(H, W, z=float(PLANE_DS[-1]), pitch=PITCH):
    """xyz of the last plane [H,W,3] float32: x along W, y along H, constant pitch, centred on the axis."""
    xyz = np.empty((H, W, 3), np.float32)
    xyz[..., 0] = ((np.arange(W, dtype=np.float64) - (W - 1) / 2) * pitch).astype(np.float32)[None, :]
    xyz[..., 1] = ((np.arange(H, dtype=np.float64) - (H - 1) / 2) * pitch).astype(np.float32)[:, None]
    xyz[..., 2] = np.float32(z)
    return xyz


def stored_volume(seed, H, W, dtype, batch=B, planes=D):
    """White-noise colours, 7x7 box-smoothed alpha (replicate border), last alpha 1, a block with rgb == 0 and one with rgb == 1, rounded to the
    storage dtype -> [batch, planes, 4, H, W] tensor of that dtype on the CPU."""
    rgba = oracle.synth_rgba(seed, (batch, planes, 4, H, W), last_alpha_one=True)
    a = torch.from_numpy(rgba[:, :, 3:4].reshape(batch * planes, 1, H, W))
    for _ in range(SMOOTHING_PASSES):
        a = F.avg_pool2d(F.pad(a, (3, 3, 3, 3), mode="replicate"), 7, stride=1)
    rgba[:, :, 3] = a.reshape(batch, planes, H, W).numpy()
    rgba[:, -1, 3] = 1.0
    rgba[:, 1, :3, :, : max(W // 4, 1)] = 0.0
    rgba[:, 2, :3, : max(H // 4, 1), :] = 1.0
    return torch.from_numpy(rgba).to(dtype)


def lay_out(stored, layout):
    """A view with the case's memory layout, on the device of `stored`, holding its values (the expanded batch: element 0 in every element)."""
    b, d, _, H, W = stored.shape
    z = lambda *shape: torch.zeros(shape, dtype=stored.dtype, device=stored.device)
    if layout == "contiguous":
        return stored
    if layout in ("rowpad4", "rowpad1"):              # row stride W + 4 (every stride stays a multiple of 4) / W + 1 (none does)
        buf = z(b, d, 4, H, W + (4 if layout == "rowpad4" else 1))
        buf[..., :W] = stored
        return buf[..., :W]
    if layout == "expand":                            # stride(0) == 0: every batch element is element 0
        return stored[:1].expand(b, d, 4, H, W)
    if layout == "offset1":                           # storage offset of one element: no 16-byte (8-byte) alignment
        flat = z(stored.numel() + 1)
        flat[1:] = stored.reshape(-1)
        return flat[1:].view(stored.shape)
    if layout == "chanslice":                         # channels 1..4 of a six-channel tensor
        wide = z(b, d, 6, H, W)
        wide[:, :, 1:5] = stored
        return wide[:, :, 1:5]
    raise KeyError(layout)


def takes_vector_instance(view):
    """The launch condition of light_apply_kernel<T, 4> / light_apply_backward_kernel<T, 4> for a volume view (the fp32 side buffers the product
    allocates are 16-byte aligned)."""
    W = view.shape[-1]
    return W % 4 == 0 and all(s % 4 == 0 for s in view.stride()[:4]) and view.data_ptr() % (4 * view.element_size()) == 0


CLIP_BAND = 1e-2   # no rgb * shading within this of the upper clip bound (except rgb == 1 blocks far inside the clipped side, see inputs)


def inputs(name):
    """-> dict(stored [B,D,4,H,W] in the storage dtype (before the layout), values float64 [B,D,4,H,W] (what the kernels see: after the layout),
    xyz [H,W,3], plane_ds [D], light_dir [B,3], ka, kd, g [B,D,4,H,W] float32 upstream gradient, layout, dtype).

    A texel whose rgb * shading lies within CLIP_BAND of 1 gets rgb = 0.5: there the clip's mask -- and with it an O(1) part of the gradient --
    would hang on the last bits of the shading, which fp32 and float64 do not share (the exact bounds are the subject of a test of their own)."""
    c = CASES[name]
    H, W, dtype = c["H"], c["W"], DTYPES[c["dtype"]]
    stored = stored_volume(c["seed"], H, W, dtype)
    g = np.random.default_rng(c["seed"]).standard_normal((B, D, 4, H, W)).astype(np.float32)
    inp = dict(stored=stored, values=lay_out(stored, c["layout"]).double().contiguous(), xyz=texel_grid(H, W), plane_ds=PLANE_DS,
               light_dir=LIGHT_DIRS, ka=KA, kd=KD, g=g, layout=c["layout"], dtype=dtype, H=H, W=W)
    near = np.abs(inp["values"][:, :, :3].numpy() * shading_of(inp)[:, None, None] - 1.0) < CLIP_BAND
    if c["layout"] == "expand":
        near = np.broadcast_to(near.any(0, keepdims=True), near.shape)
    stored[:, :, :3][torch.from_numpy(near.copy())] = 0.5
    inp["values"] = lay_out(stored, c["layout"]).double().contiguous()
    inp["nudged"] = float(near.mean())
    return inp


def shading_of(inp):
    """The float64 shading image [B,H,W] of the case, read off torch_light_render on a volume of constant colour 1/16 (never clips)."""
    v = inp["values"].clone()
    v[:, :, :3] = 1.0 / 16
    return reference(dict(inp, values=v))[:, 0, 0] * 16


def k1d():
    from ml_gmpi_amd.light import gaussian_kernel1d
    return gaussian_kernel1d(BLUR_KSIZE, 0.3 * ((BLUR_KSIZE - 1) * 0.5 - 1) + 0.8)


def reference(inp, dtype=torch.float64, xyz=None, values=None, grad=False, ka=None, kd=None):
    """torch_light_render on the case's values in `dtype` -> out (numpy float64) [, d sum(out * g) / d values (numpy float64; for the expanded batch
    summed over the copies, [1,D,4,H,W])]."""
    v = (inp["values"] if values is None else values).to(dtype)
    if grad:
        leaf = (v[:1] if inp["layout"] == "expand" else v).clone().requires_grad_(True)
        v = leaf.expand(v.shape) if inp["layout"] == "expand" else leaf
    t = lambda a: torch.as_tensor(a).to(dtype)
    out = torch_light_render(v, t(inp["plane_ds"]), t(inp["xyz"] if xyz is None else xyz), t(inp["light_dir"]),
                             inp["ka"] if ka is None else ka, inp["kd"] if kd is None else kd, k1d().to(dtype))
    if not grad:
        return out.double().numpy()
    (out * t(inp["g"])).sum().backward()
    return out.detach().double().numpy(), leaf.grad.double().numpy()


def noise_floor(inp):
    """n0: the fp32 oracle against float64, both on the CPU."""
    got, _ = oracle.light_shade(inp["values"].float().numpy(), inp["plane_ds"], inp["xyz"], inp["light_dir"], inp["ka"], inp["kd"])
    return float(np.abs(got - reference(inp)).max())


def transposed_grid(inp):
    """The grid read as if H and W were exchanged: the [H,W,3] buffer taken for a [W,H,3] one."""
    H, W = inp["H"], inp["W"]
    return np.ascontiguousarray(inp["xyz"].reshape(W, H, 3).transpose(1, 0, 2))


def shifted_alpha(inp):
    """The values with every alpha plane moved one texel in x (the colours stay): the depth the shading sees is shifted."""
    v = inp["values"].clone()
    v[:, :, 3] = torch.roll(v[:, :, 3], 1, dims=-1)
    return v


def shading_numpy(blurred, xyz, light_dir, ka, kd, dtype):
    """light_shading_kernel restated in numpy in `dtype`: blurred [B,H,W], xyz [H,W,3], light_dir [B,3] -> shading [B,H,W]."""
    f = dtype
    blur, xyz = np.asarray(blurred).astype(f), np.asarray(xyz).astype(f)[None]
    g = (xyz * (blur[..., None] / (xyz[..., 2:] + f(1e-8)))).astype(f)
    c = g[:, 1:-1, 1:-1]
    up, down, left, right = g[:, :-2, 1:-1], g[:, 2:, 1:-1], g[:, 1:-1, :-2], g[:, 1:-1, 2:]
    n = np.cross(up - c, left - c) + np.cross(left - c, down - c) + np.cross(down - c, right - c) + np.cross(right - c, up - c)
    n = np.pad(n.astype(f), ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    n = n / (np.sqrt((n ** 2).sum(3, keepdims=True, dtype=f)) + f(1e-8))
    diffuse = np.maximum(f(-1.0) * (n * np.asarray(light_dir).astype(f).reshape(-1, 1, 1, 3)).sum(3, dtype=f), f(0.0))
    return (f(ka) + diffuse * f(kd)).astype(f)
