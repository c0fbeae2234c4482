"""The reference's shading augmentation (gmpi/core/light_renderer.py `LightRenderer`) on the device.

`compute_depth` (light_renderer.py:82-100): the reference builds `[B, D+1, 1, H, W]` shifted alphas, a cumprod tensor,
the weights and a weighted sum (five full passes over the alpha planes); here the alpha channel is read once by one
streaming HIP kernel and the running transmittance lives in a register -- the renderer's composite with the identity
warp.  `LightRenderer.render` chains it with three more kernels (csrc/light_kernels.hip): Gaussian blur of the depth,
point cloud -> normals -> Lambert shading per texel, and `clip(rgb * shading, 0, 1)` over the volume.

The reference applies the augmentation inside the G-step (train.py:535-541): when the volume requires grad the same
kernels run under a `torch.autograd.Function` whose backward uses two more streaming kernels for the volume-sized ops
(clip(rgb*shading) and the alpha compositing of the depth) and, for the B*H*W middle (blur, normals, Lambert), torch autograd
over a torch restatement (`LightRenderer(middle="torch")`, the default) or two adjoint kernels (`middle="hip"`).

`render_shared` and `render_depth` are the augmentation for the shared-colour and the depth-alpha layout: there the shaded MPI is an MPI of
the same layout, and only the expected depth needs a kernel (`compute_depth`; `compute_depth_ramp`, which reads one depth image and no planes).
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, poses
from .hip_mpi import _DTYPES, _call, _depth_alpha, _ptr, _refuse_uint8

EPS = 1e-8  # light_renderer.py:8


def compute_depth(mpi_alpha: torch.Tensor, plane_ds: torch.Tensor, want_transmittance: bool = False):
    """mpi_alpha [B, D, 1, H, W] (any float storage dtype; may be the strided view `mpi[:, :, 3:]` of an RGBA volume),
    plane_ds [D] or [D,1] plane distances -> depth [B, 1, H, W] (float32) [, transmittance [B,1,H,W]].

    Differentiable w.r.t. mpi_alpha (as the reference's plain-torch `LightRenderer.compute_depth`, light_renderer.py:82-100), through both
    outputs: the backward is gmpi_alpha_depth_backward_ex_launch.  plane_ds gets no gradient."""
    _refuse_uint8("compute_depth", mpi_alpha)
    if not mpi_alpha.is_cuda:
        raise _lib.GmpiError("compute_depth needs tensors on a ROCm device (no CPU path)")
    assert mpi_alpha.ndim == 5 and mpi_alpha.shape[2] == 1, f"{mpi_alpha.shape}"
    if torch.is_grad_enabled() and isinstance(plane_ds, torch.Tensor) and plane_ds.requires_grad:
        raise NotImplementedError("compute_depth provides no gradient w.r.t. plane_ds")
    if torch.is_grad_enabled() and mpi_alpha.requires_grad:
        depth, T = _DepthFunction.apply(mpi_alpha, plane_ds)
    else:
        with torch.no_grad():
            depth, T = _alpha_depth(mpi_alpha, plane_ds, want_transmittance)
    return (depth, T) if want_transmittance else depth


def _alpha_operand(mpi_alpha: torch.Tensor) -> torch.Tensor:
    """The alpha view the kernels read: a storage dtype they take, innermost stride 1, no negative strides."""
    if mpi_alpha.dtype not in _DTYPES:
        mpi_alpha = mpi_alpha.float()
    # (a plane stride of 0 -- one plane expanded over D -- or overlapping rows are legal torch views that the entries refuse with GMPI_E_STRIDE:
    # tests/test_hip_light_shapes.py::test_render_takes_a_volume_expanded_over_the_planes)
    if mpi_alpha.stride(4) != 1 or any(s < 0 for s in mpi_alpha.stride()) or mpi_alpha.stride(1) == 0 or mpi_alpha.stride(3) < mpi_alpha.shape[4]:
        mpi_alpha = mpi_alpha.contiguous()
    return mpi_alpha


def _alpha_depth(mpi_alpha: torch.Tensor, plane_ds: torch.Tensor, want_transmittance: bool):
    """gmpi_alpha_depth_launch -> (depth, T or None), both float32 [B,1,H,W]."""
    mpi_alpha = _alpha_operand(mpi_alpha)
    B, D, _, H, W = mpi_alpha.shape
    ds = plane_ds.reshape(-1).to(mpi_alpha.device, torch.float32).contiguous()
    assert ds.numel() == D, f"{ds.shape}, {D}"
    depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=mpi_alpha.device)
    T = torch.empty((B, 1, H, W), dtype=torch.float32, device=mpi_alpha.device) if want_transmittance else None
    _call("gmpi_alpha_depth_launch", mpi_alpha.device, mpi_alpha.data_ptr(), _DTYPES[mpi_alpha.dtype], mpi_alpha.stride(0),
          mpi_alpha.stride(1), mpi_alpha.stride(3), ds.data_ptr(), B, D, H, W, depth.data_ptr(), _ptr(T))
    return depth, T


class _DepthFunction(torch.autograd.Function):
    """autograd bridge of compute_depth: forward = gmpi_alpha_depth_launch (T always, into a buffer private to this node: the backward
    sweeps back to front from it), backward = gmpi_alpha_depth_backward_ex_launch into a zero-filled fp32 gradient.  An output the loss
    does not use arrives as None (set_materialize_grads(False)) and is passed as NULL."""

    @staticmethod
    def forward(ctx, mpi_alpha, plane_ds):
        depth, T = _alpha_depth(mpi_alpha.detach(), plane_ds.detach(), True)
        ds = plane_ds.detach().reshape(-1).to(mpi_alpha.device, torch.float32).contiguous()
        ctx.save_for_backward(mpi_alpha, ds, T)
        ctx.in_dtype = mpi_alpha.dtype
        ctx.set_materialize_grads(False)
        return depth, T

    @staticmethod
    def backward(ctx, g_depth, g_T):
        mpi_alpha, ds, T = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or (g_depth is None and g_T is None):
            return None, None
        alpha = _alpha_operand(mpi_alpha.detach())
        B, D, _, H, W = alpha.shape
        dev = alpha.device
        g_depth = None if g_depth is None else g_depth.to(torch.float32).contiguous()
        g_T = None if g_T is None else g_T.to(torch.float32).contiguous()
        grad = torch.zeros((B, D, 1, H, W), dtype=torch.float32, device=dev)
        _call("gmpi_alpha_depth_backward_ex_launch", dev, alpha.data_ptr(), _DTYPES[alpha.dtype], alpha.stride(0), alpha.stride(1),
              alpha.stride(3), ds.data_ptr(), T.data_ptr(), _ptr(g_depth), _ptr(g_T), grad.data_ptr(), grad.stride(0), grad.stride(1),
              grad.stride(3), B, D, H, W)
        return grad.to(ctx.in_dtype), None


def compute_depth_ramp(depth: torch.Tensor, plane_z: torch.Tensor, z_lo: float, z_hi: float, plane_ds: torch.Tensor,
                       want_transmittance: bool = False):
    """`compute_depth` for a depth-alpha MPI, without the alpha planes: depth [B,1,H,W] (any float storage dtype; may be a strided view such as
    channel 3 of an RGB-D tensor or an expanded batch), plane_z [D] or [B,D], the ramp's bounds as `depth_alpha_planes` takes them, plane_ds [D]
    or [D,1] metric plane distances -> expected depth [B,1,H,W] (float32) [, transmittance [B,1,H,W]].

    By definition `compute_depth(depth_alpha_planes(depth, plane_z, z_lo, z_hi), plane_ds, ...)`, bit for bit (gmpi_ramp_depth_launch: the texel
    is held in a register, the [B,D,1,H,W] planes are never built).  Differentiable w.r.t. depth through both outputs
    (gmpi_ramp_depth_backward_launch); plane_z, plane_ds and the bounds get no gradient."""
    from .depth_alpha import _check_depth
    _refuse_uint8("compute_depth_ramp", depth)
    _check_depth(depth, plane_z)
    if torch.is_grad_enabled():
        for name, v in (("plane_z", plane_z), ("plane_ds", plane_ds), ("z_lo", z_lo), ("z_hi", z_hi)):
            if isinstance(v, torch.Tensor) and v.requires_grad:
                raise NotImplementedError(f"compute_depth_ramp provides no gradient w.r.t. {name}")
    if not depth.is_cuda:
        raise _lib.GmpiError("compute_depth_ramp needs tensors on a ROCm device (no CPU path)")
    z_lo, z_hi = float(z_lo), float(z_hi)
    if torch.is_grad_enabled() and depth.requires_grad:
        out, T = _RampDepthFunction.apply(depth, plane_z, plane_ds, z_lo, z_hi)
    else:
        with torch.no_grad():
            out, T = _ramp_depth(_ramp_operands(depth, plane_z, plane_ds), z_lo, z_hi, want_transmittance)
    return (out, T) if want_transmittance else out


def _ramp_operands(depth: torch.Tensor, plane_z: torch.Tensor, plane_ds: torch.Tensor):
    """What the ramp entries read: the depth image in a storage dtype they take (innermost stride 1, rows that do not overlap, no negative stride:
    such views are passed as they are), plane_z [D] or [B,D] and plane_ds [D] in fp32 on its device."""
    if depth.dtype not in _DTYPES:
        depth = depth.float()
    if depth.stride(3) != 1 or depth.stride(0) < 0 or depth.stride(2) < depth.shape[3]:
        depth = depth.contiguous()
    pz = plane_z.detach().to(depth.device, torch.float32).contiguous()
    ds = plane_ds.detach().reshape(-1).to(depth.device, torch.float32).contiguous()
    assert ds.numel() == pz.shape[-1], f"{tuple(ds.shape)}, {tuple(pz.shape)}"
    return depth, pz, ds


def _ramp_depth(operands, z_lo: float, z_hi: float, want_transmittance: bool):
    """gmpi_ramp_depth_launch -> (depth, T or None), both float32 [B,1,H,W]."""
    image, pz, ds = operands
    B, _, H, W = image.shape
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=image.device)
    T = torch.empty((B, 1, H, W), dtype=torch.float32, device=image.device) if want_transmittance else None
    ramp = _depth_alpha(pz, z_lo, z_hi)
    _call("gmpi_ramp_depth_launch", image.device, image.data_ptr(), _DTYPES[image.dtype], image.stride(0), image.stride(2), ctypes.byref(ramp),
          ds.data_ptr(), B, pz.shape[-1], H, W, out.data_ptr(), _ptr(T))
    return out, T


class _RampDepthFunction(torch.autograd.Function):
    """autograd bridge of compute_depth_ramp, as _DepthFunction: forward = gmpi_ramp_depth_launch (T always, kept for the backward's sweep),
    backward = gmpi_ramp_depth_backward_launch into a zero-filled fp32 image.  An output the loss does not use arrives as None and is passed as
    NULL."""

    @staticmethod
    def forward(ctx, depth, plane_z, plane_ds, z_lo, z_hi):
        operands = _ramp_operands(depth.detach(), plane_z, plane_ds)
        out, T = _ramp_depth(operands, z_lo, z_hi, True)
        ctx.save_for_backward(*operands, T)
        ctx.misc = (z_lo, z_hi, depth.dtype)
        ctx.set_materialize_grads(False)
        return out, T

    @staticmethod
    def backward(ctx, g_depth, g_T):
        image, pz, ds, T = ctx.saved_tensors
        z_lo, z_hi, in_dtype = ctx.misc
        if not ctx.needs_input_grad[0] or (g_depth is None and g_T is None):
            return None, None, None, None, None
        B, _, H, W = image.shape
        dev = image.device
        g_depth = None if g_depth is None else g_depth.to(torch.float32).contiguous()
        g_T = None if g_T is None else g_T.to(torch.float32).contiguous()
        grad = torch.zeros((B, 1, H, W), dtype=torch.float32, device=dev)
        ramp = _depth_alpha(pz, z_lo, z_hi)
        _call("gmpi_ramp_depth_backward_launch", dev, image.data_ptr(), _DTYPES[image.dtype], image.stride(0), image.stride(2), ctypes.byref(ramp),
              ds.data_ptr(), T.data_ptr(), _ptr(g_depth), _ptr(g_T), grad.data_ptr(), grad.stride(0), grad.stride(2), B, pz.shape[-1], H, W)
        return grad.to(in_dtype), None, None, None, None


def gaussian_kernel1d(ksize: int, sigma: float) -> torch.Tensor:
    """1-D kernel of torchvision.transforms.GaussianBlur (functional `_get_gaussian_kernel1d`): samples of the pdf on
    linspace(-(k-1)/2, (k-1)/2, k), normalised to sum 1, float32."""
    lim = (ksize - 1) * 0.5
    x = torch.linspace(-lim, lim, steps=ksize)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


_BLUR_MATRICES = {}


def _blur_matrix(n: int, k1d: torch.Tensor, device) -> torch.Tensor:
    """[n,n] matrix of the 1-D reflect-padded blur (row i = weights of output i over the inputs); cached."""
    k1d = k1d.detach().cpu()
    key = (n, tuple(k1d.tolist()), str(device))
    m = _BLUR_MATRICES.get(key)
    if m is None:
        k, r = k1d.numel(), k1d.numel() // 2
        src = torch.arange(n).view(n, 1) + torch.arange(k).view(1, k) - r          # [n,k] unpadded source index
        src = src.abs()
        src = torch.where(src >= n, 2 * (n - 1) - src, src)                       # padding_mode="reflect"
        m = torch.zeros((n, n), dtype=torch.float32)
        m.index_put_((torch.arange(n).view(n, 1).expand(n, k), src), k1d.to(torch.float32).view(1, k).expand(n, k), accumulate=True)
        m = m.to(device)
        if len(_BLUR_MATRICES) < 16:
            _BLUR_MATRICES[key] = m
    return m


def _blur_torch(depth: torch.Tensor, my: torch.Tensor, mx: torch.Tensor) -> torch.Tensor:
    """Differentiable restatement of gaussian_blur_kernel ([B,1,H,W]) for the backward of the pipeline's middle: the
    separable blur as two GEMMs with the reflect-padded 1-D operators `_blur_matrix` (equal to the 81-tap sum up to
    rounding; a 9x9 `F.conv2d` on B single-channel images costs milliseconds in MIOpen, the GEMMs microseconds)."""
    return torch.matmul(torch.matmul(my, depth), mx.t())


def _shading_torch(depth_blurred: torch.Tensor, xyz_last: torch.Tensor, light_dir: torch.Tensor, ka: float, kd: float) -> torch.Tensor:
    """torch restatement of light_shading_kernel (compute_pcl :102-120, get_normal :57-80, Lambert :163-190) -> [B,H,W]."""
    xyz = xyz_last.to(depth_blurred)[None]
    g = xyz * (depth_blurred[:, 0].unsqueeze(-1) / (xyz[..., 2:] + EPS))
    c = g[:, 1:-1, 1:-1]
    up, down, left, right = g[:, :-2, 1:-1], g[:, 2:, 1:-1], g[:, 1:-1, :-2], g[:, 1:-1, 2:]
    n = (torch.cross(up - c, left - c, dim=3) + torch.cross(left - c, down - c, dim=3)
         + torch.cross(down - c, right - c, dim=3) + torch.cross(right - c, up - c, dim=3))
    n = F.pad(n.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate").permute(0, 2, 3, 1)
    n = n / (((n ** 2).sum(3, keepdim=True)) ** 0.5 + EPS)
    diffuse = (-1 * (n * light_dir.to(depth_blurred).view(-1, 1, 1, 3)).sum(3)).clamp(min=0)
    return ka + diffuse * kd


MIDDLES = ("torch", "hip")


def _middle_saved(renderer, depth, blurred):
    """What a node saves in its forward for `_middle_backward`, all on the device already.  "torch": the expected depth and the two `_blur_matrix`
    operands; "hip": the forward's blurred depth and the 1-D kernel (the matrices are never built)."""
    dev = depth.device
    H, W = depth.shape[-2:]
    if renderer.middle == "hip":
        return blurred, renderer._k1d.to(dev, torch.float32)
    return depth, _blur_matrix(H, renderer._k1d, dev), _blur_matrix(W, renderer._k1d, dev)


def _middle_backward(mode, saved, xyz_last, light_dir, ka, kd, g_shading):
    """dL/d depth [B,1,H,W] from dL/d shading [B,H,W] through the image-sized middle (blur, point cloud, normals, Lambert); `saved` is what
    `_middle_saved` returned for `mode`.  The ONE backward of the middle: `_LightFunction`, `_ShadingFunction` and `_ShadeImagesFunction` call it.

    "torch": torch autograd over the torch restatement of the two kernels.
    "hip": gmpi_light_shading_backward_launch on the forward's blurred depth, then gmpi_light_blur_backward_launch: two gathers, no atomics, the
    same bits on every run.  Where a cell's un-normalised normal is exactly 0 it contributes 0; the restatement yields NaN there (pow(0.5) at 0)."""
    if mode == "hip":
        blurred, k1d = saved
        B, _, H, W = blurred.shape
        dev = blurred.device
        g_shading = g_shading.to(torch.float32).contiguous()
        g_blurred = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        g_depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        _call("gmpi_light_shading_backward_launch", dev, blurred.data_ptr(), xyz_last.data_ptr(), light_dir.data_ptr(), float(kd), g_shading.data_ptr(),
              B, H, W, g_blurred.data_ptr())
        _call("gmpi_light_blur_backward_launch", dev, g_blurred.data_ptr(), g_depth.data_ptr(), B, H, W, k1d.data_ptr(), k1d.numel())
        return g_depth
    depth, my, mx = saved
    with torch.enable_grad():
        d = depth.detach().requires_grad_(True)
        s = _shading_torch(_blur_torch(d, my, mx), xyz_last, light_dir, ka, kd)
        (g_depth,) = torch.autograd.grad(s, d, g_shading)
    return g_depth


class _LightFunction(torch.autograd.Function):
    """LightRenderer.render as one autograd node: forward = the four kernels, backward = apply-backward kernel, torch
    autograd through the B*H*W middle, alpha-depth-backward kernel (adds into the alpha channel of the gradient)."""

    @staticmethod
    def forward(ctx, vol, renderer, plane_ds, xyz_last, light_dir, ka, kd):
        out, depth, T, shading, blurred = renderer._forward_kernels(vol.detach(), plane_ds, xyz_last, light_dir, ka, kd, want_blurred=True)
        dev = vol.device
        # everything the backward needs is put on the device here: CPU tensor ops inside the autograd worker thread start
        # a second OpenMP pool, and the two pools then fight for the cores (milliseconds per tiny host op)
        ctx.save_for_backward(vol.detach(), T, shading, xyz_last.to(dev, torch.float32).contiguous(), light_dir.to(dev, torch.float32).contiguous(),
                              plane_ds.reshape(-1).to(dev, torch.float32).contiguous(), *_middle_saved(renderer, depth, blurred))
        ctx.misc = (ka, kd, vol.dtype, renderer.middle)
        return out

    @staticmethod
    def backward(ctx, g_out):
        vol, T, shading, xyz_last, light_dir, ds, *middle = ctx.saved_tensors
        ka, kd, in_dtype, mode = ctx.misc
        dev = vol.device
        B, D, _, H, W = vol.shape
        g_out = g_out.to(torch.float32).contiguous()
        g_rgba = torch.empty((B, D, 4, H, W), dtype=torch.float32, device=dev)
        g_shading = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        strides = (ctypes.c_int64 * 5)(*vol.stride())
        stream = torch.cuda.current_stream(dev).cuda_stream
        _call("gmpi_light_apply_backward_launch", dev, vol.data_ptr(), _DTYPES[vol.dtype], strides, shading.data_ptr(), g_out.data_ptr(),
              g_rgba.data_ptr(), g_shading.data_ptr(), B, D, H, W, stream=stream)
        g_depth = _middle_backward(mode, middle, xyz_last, light_dir, ka, kd, g_shading).contiguous()
        alpha = vol[:, :, 3:]
        plane = H * W
        _call("gmpi_alpha_depth_backward_launch", dev, alpha.data_ptr(), _DTYPES[vol.dtype], alpha.stride(0), alpha.stride(1), alpha.stride(3),
              ds.data_ptr(), T.data_ptr(), g_depth.data_ptr(), g_rgba.data_ptr() + 3 * plane * 4, D * 4 * plane, 4 * plane, W, B, D, H, W,
              stream=stream)
        return g_rgba.to(in_dtype), None, None, None, None, None, None


class _ShadingFunction(torch.autograd.Function):
    """The image-sized middle of `LightRenderer.shading_image` as one autograd node: forward = the blur and shading kernels `render` runs (the
    same bits), backward = `_middle_backward` in the renderer's mode, as in `_LightFunction.backward`."""

    @staticmethod
    def forward(ctx, depth, renderer, xyz_last, light_dir, ka, kd):
        dev = depth.device
        d = depth.detach()
        blurred = renderer.blurrer_func(d)
        shading = renderer.shading(blurred, xyz_last, light_dir, ka, kd).unsqueeze(1)
        ctx.save_for_backward(xyz_last.to(dev, torch.float32).contiguous(), light_dir.to(dev, torch.float32).contiguous(),
                              *_middle_saved(renderer, d, blurred))
        ctx.misc = (ka, kd, renderer.middle)
        return shading

    @staticmethod
    def backward(ctx, g_shading):
        xyz_last, light_dir, *middle = ctx.saved_tensors
        ka, kd, mode = ctx.misc
        return _middle_backward(mode, middle, xyz_last, light_dir, ka, kd, g_shading[:, 0].to(torch.float32)), None, None, None, None, None


def _image_operand(image: torch.Tensor) -> torch.Tensor:
    """The colour image the shade-images entries read: a storage dtype they take, innermost stride 1, rows that do not overlap, a channel stride
    above 0, no negative MPI stride (such views are passed as they are; an expanded batch is one of them)."""
    if image.dtype not in _DTYPES:
        image = image.float()
    if image.stride(3) != 1 or image.stride(0) < 0 or image.stride(1) <= 0 or image.stride(2) < image.shape[3]:
        image = image.contiguous()
    return image


def _image_args(image):
    """(pointer, dtype code, strides {MPI, channel, row}) of an image operand, NULLs for None."""
    if image is None:
        return None, 0, None
    return image.data_ptr(), _DTYPES[image.dtype], (ctypes.c_int64 * 3)(image.stride(0), image.stride(1), image.stride(2))


class _ShadeImagesFunction(torch.autograd.Function):
    """`LightRenderer._shade_images` with middle="hip" as one autograd node: expected depth [B,1,H,W] fp32, colour image, background image or None
    -> (clip(rgb * shading, 0, 1), clip(background * shading, 0, 1) or None), float32.  Forward = the blur and shading kernels `render` runs (the
    shading has the bits of `shading_image()`), then gmpi_light_shade_images_launch.  Backward = gmpi_light_shade_images_backward_launch (both
    images and grad_shading in one launch), then `_middle_backward`: the gradient w.r.t. the expected depth goes on to `compute_depth` /
    `compute_depth_ramp`.  Each gradient comes back in its input's dtype; what requires no grad gets no buffer, and the middle is skipped when the
    depth requires none.  An output the loss does not use arrives as None and is passed as NULL."""

    @staticmethod
    def forward(ctx, depth, rgb, background, renderer, xyz_last, light_dir, ka, kd):
        dev = depth.device
        d = depth.detach()
        B, _, H, W = d.shape
        blurred = renderer.blurrer_func(d)
        shading = renderer.shading(blurred, xyz_last, light_dir, ka, kd)
        c, bg = _image_operand(rgb.detach()), (None if background is None else _image_operand(background.detach()))
        o_rgb = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        o_bg = None if bg is None else torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        _call("gmpi_light_shade_images_launch", dev, *_image_args(c), *_image_args(bg), shading.data_ptr(), o_rgb.data_ptr(), _ptr(o_bg), B, H, W)
        ctx.save_for_backward(c, shading, xyz_last.to(dev, torch.float32).contiguous(), light_dir.to(dev, torch.float32).contiguous(),
                              blurred, renderer._k1d.to(dev, torch.float32), *(() if bg is None else (bg,)))
        ctx.misc = (ka, kd, rgb.dtype, None if background is None else background.dtype)
        ctx.set_materialize_grads(False)
        return o_rgb, o_bg

    @staticmethod
    def backward(ctx, g_rgb, g_bg):
        c, shading, xyz_last, light_dir, blurred, k1d, *rest = ctx.saved_tensors
        bg = rest[0] if rest else None
        ka, kd, rgb_dtype, bg_dtype = ctx.misc
        need_depth, need_rgb, need_bg = ctx.needs_input_grad[0], ctx.needs_input_grad[1], bg is not None and ctx.needs_input_grad[2]
        if (g_rgb is None and g_bg is None) or not (need_depth or need_rgb or need_bg):
            return (None,) * 8
        dev = c.device
        B, _, H, W = c.shape
        g_rgb = None if g_rgb is None else g_rgb.to(torch.float32).contiguous()
        g_bg = None if g_bg is None or bg is None else g_bg.to(torch.float32).contiguous()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        grad_rgb, grad_bg, g_shading = (new(B, 3, H, W) if need_rgb else None, new(B, 3, H, W) if need_bg else None,
                                        new(B, H, W) if need_depth else None)
        _call("gmpi_light_shade_images_backward_launch", dev, *_image_args(c), *_image_args(bg), shading.data_ptr(), _ptr(g_rgb), _ptr(g_bg),
              _ptr(grad_rgb), _ptr(grad_bg), _ptr(g_shading), B, H, W)
        g_depth = _middle_backward("hip", (blurred, k1d), xyz_last, light_dir, ka, kd, g_shading) if need_depth else None
        return (g_depth, None if grad_rgb is None else grad_rgb.to(rgb_dtype), None if grad_bg is None else grad_bg.to(bg_dtype),
                None, None, None, None, None)


class LightRenderer:
    """Same constructor, attributes (`step`, `cur_ka`, `cur_kd`, `sphere_center`, ...) and method signatures as the
    reference class (light_renderer.py:11-199); tensors live on the ROCm device of `batch_mpi`.

    One keyword of this package's own: `middle` says how the image-sized middle of the augmentation (blur, point cloud, normals, Lambert) is
    differentiated, and how `render_shared` / `render_depth` run it.  "torch" (the default): torch autograd over a torch restatement of the two
    kernels.  "hip": the adjoint kernels of csrc/light_kernels.hip (`_middle_backward`), atomics-free and bit-reproducible, and one autograd node
    of kernels for the two layouts (`_ShadeImagesFunction`).  The forward of `render` and `shading_image` is the same kernels in both modes."""

    def __init__(self, *, sphere_center_z, sphere_r, ka_max=1.0, kd_max=0.0, n_grow_iters=1000, l_h_mean=0.0, l_h_std=0.2,
                 l_v_mean=0.2, l_v_std=0.05, blur_ksize=9, middle="torch"):
        if middle not in MIDDLES:
            raise ValueError(f"middle must be one of {MIDDLES}, got {middle!r}")
        self.middle = middle
        self.ka_max, self.kd_max, self.n_grow_iters = ka_max, kd_max, n_grow_iters
        self.cur_ka = self.cur_kd = 0.0
        self.l_h_mean, self.l_h_std, self.l_v_mean, self.l_v_std = l_h_mean, l_h_std, l_v_mean, l_v_std
        self.sphere_center = torch.FloatTensor(np.array([0, 0, sphere_center_z]))
        self.sphere_r = sphere_r
        self.blur_ksize = blur_ksize
        self.blur_sigma = 0.3 * ((blur_ksize - 1) * 0.5 - 1) + 0.8  # OpenCV's rule, light_renderer.py:50
        self._k1d = gaussian_kernel1d(blur_ksize, self.blur_sigma)
        self.step = -1

    # -- pieces (same names as the reference) ------------------------------------------------------------------
    compute_depth = staticmethod(lambda mpi_alpha, plane_ds: compute_depth(mpi_alpha, plane_ds))

    @torch.no_grad()
    def blurrer_func(self, depth: torch.Tensor) -> torch.Tensor:
        """[B,1,H,W] -> blurred [B,1,H,W] (torchvision GaussianBlur: reflect padding, ksize x ksize)."""
        d = depth.to(torch.float32).contiguous()
        B, _, H, W = d.shape
        out = torch.empty_like(d)
        k = self._k1d.to(d.device)
        _call("gmpi_light_blur_launch", d.device, d.data_ptr(), out.data_ptr(), B, H, W, k.data_ptr(), self.blur_ksize)
        return out

    @torch.no_grad()
    def shading(self, depth_blurred: torch.Tensor, xyz_last: torch.Tensor, light_direction: torch.Tensor, ka: float,
                kd: float) -> torch.Tensor:
        """compute_pcl + get_normal + Lambert term: [B,1,H,W], [H,W,3], [B,3] -> shading [B,H,W] = ka + kd*max(-n.l, 0)."""
        d = depth_blurred.to(torch.float32).contiguous()
        B, _, H, W = d.shape
        xyz = xyz_last.to(d.device, torch.float32).reshape(H, W, 3).contiguous()
        ld = light_direction.to(d.device, torch.float32).reshape(B, 3).contiguous()
        out = torch.empty((B, H, W), dtype=torch.float32, device=d.device)
        _call("gmpi_light_shading_launch", d.device, d.data_ptr(), xyz.data_ptr(), ld.data_ptr(), float(ka), float(kd), B, H, W, out.data_ptr())
        return out

    # -- light_renderer.py:122-199 ------------------------------------------------------------------------------
    @torch.no_grad()
    def _forward_kernels(self, vol, plane_ds, xyz_last, light_direction, ka, kd, want_blurred=False):
        dev = vol.device
        B, D, _, H, W = vol.shape
        depth, T = compute_depth(vol[:, :, 3:], plane_ds, want_transmittance=True)
        blurred = self.blurrer_func(depth)
        shading = self.shading(blurred, xyz_last, light_direction, ka, kd)
        out = torch.empty((B, D, 4, H, W), dtype=torch.float32, device=dev)
        strides = (ctypes.c_int64 * 5)(*vol.stride())
        _call("gmpi_light_apply_launch", dev, vol.data_ptr(), _DTYPES[vol.dtype], strides, shading.data_ptr(), out.data_ptr(), B, D, H, W)
        return (out, depth, T, shading, blurred) if want_blurred else (out, depth, T, shading)

    def render_shared(self, rgb: torch.Tensor, alpha: torch.Tensor, mpi_plane_dhws: torch.Tensor, mpi_tex_pix_xyz: torch.Tensor,
                      background: torch.Tensor = None):
        """`render` for a shared-colour MPI (rgb [B,3,H,W], alpha [B,D,1,H,W], background [B,3,H,W] or None): the shading is one value per
        texel, the same for every plane, so the shaded MPI is a shared-colour MPI again -- (clip(rgb * shading, 0, 1), alpha, clip(background
        * shading, 0, 1) or None), colours in float32.  Equal to `render(expand_shared_color(rgb, alpha, background))` split again; the step
        counter, cur_ka / cur_kd and the torch RNG advance as in `render`.  The depth comes from the differentiable `compute_depth` kernel (one
        pass over the alpha planes).  The rest is image-sized torch with middle="torch"; with middle="hip" it is one autograd node of kernels
        (`_ShadeImagesFunction`: the shading has the bits of `shading_image()`, the colours are within one fp32 rounding of the torch mode's, the
        backward is bit-reproducible).  Differentiable w.r.t. rgb, alpha and background, each gradient in its tensor's dtype."""
        _refuse_uint8("LightRenderer.render_shared", rgb, alpha, background)
        if not alpha.is_cuda:
            raise _lib.GmpiError("LightRenderer.render_shared needs tensors on a ROCm device (no CPU path)")
        from .shared_color import _check
        _check(rgb, alpha, background)
        dev = alpha.device
        light_direction = self._next_light(alpha.shape[0])
        plane_ds = mpi_plane_dhws[:, :1].detach().to(dev)
        depth = compute_depth(alpha, plane_ds)                                                      # [B,1,H,W] float32
        o_rgb, o_bg = self._shade_images(depth, mpi_tex_pix_xyz, light_direction, rgb, background)
        return o_rgb, alpha, o_bg

    def render_depth(self, rgb: torch.Tensor, depth: torch.Tensor, mpi_plane_dhws: torch.Tensor, mpi_tex_pix_xyz: torch.Tensor, *,
                     plane_z: torch.Tensor, z_range: float, n_z_bins: int, background: torch.Tensor = None):
        """`render` for a depth-alpha MPI (rgb [B,3,H,W], depth [B,1,H,W], plane_z [D] or [B,D], background [B,3,H,W] or None; the ramp's bounds
        are `depth_alpha_bounds(z_range, n_z_bins)`): the shading is one value per texel and multiplies the colour images, so the shaded MPI is a
        depth-alpha MPI again -- (clip(rgb * shading, 0, 1), depth, clip(background * shading, 0, 1) or None), colours in float32, the depth
        image as it was handed in.  Equal to `render(expand_depth_alpha(rgb, depth, plane_z, z_lo, z_hi, background))` read back as such an MPI;
        the step counter, cur_ka / cur_kd and the torch RNG advance as in `render`.  The expected depth comes from the differentiable
        `compute_depth_ramp` kernel (no alpha planes).  The rest is image-sized torch with middle="torch", one autograd node of kernels with
        middle="hip", as in `render_shared`.  Differentiable w.r.t. rgb, depth and background, each gradient in its tensor's dtype."""
        from .depth_alpha import _check, depth_alpha_bounds
        _refuse_uint8("LightRenderer.render_depth", rgb, depth, background)
        if not depth.is_cuda:
            raise _lib.GmpiError("LightRenderer.render_depth needs tensors on a ROCm device (no CPU path)")
        _check(rgb, depth, plane_z, background)
        z_lo, z_hi = depth_alpha_bounds(z_range, n_z_bins)
        light_direction = self._next_light(depth.shape[0])
        plane_ds = mpi_plane_dhws[:, :1].detach().to(depth.device)
        z = compute_depth_ramp(depth, plane_z, z_lo, z_hi, plane_ds)                                # [B,1,H,W] float32
        o_rgb, o_bg = self._shade_images(z, mpi_tex_pix_xyz, light_direction, rgb, background)
        return o_rgb, depth, o_bg

    def shading_image(self, batch_mpi: torch.Tensor, mpi_plane_dhws: torch.Tensor, mpi_tex_pix_xyz: torch.Tensor) -> torch.Tensor:
        """The shading `render` multiplies the colours by, as an image: batch_mpi [B,D,4,H,W], mpi_plane_dhws [D,3], mpi_tex_pix_xyz [D,H,W,>=3]
        -> [B,1,H,W] float32, for `MPI.render_views_shaded` / `MPIRenderer.render_shaded`, which shade on the taps: `render(mpi)` equals
        `apply_shading(mpi, shading_image(mpi))` bit for bit (the depth, blur and shading kernels are `render`'s).  One step of the schedule: the
        step counter, cur_ka / cur_kd and the torch RNG advance exactly as in `render` -- call one or the other per step.  Nothing volume-sized is
        allocated in the forward.  Differentiable w.r.t. the alpha channel of batch_mpi: the expected depth comes from the differentiable
        `compute_depth`; the image-sized middle back-propagates through its torch restatement (the one `_shade_images` runs) with
        middle="torch", through the two adjoint kernels of `_middle_backward` with middle="hip".  The forward is the same in both modes."""
        _refuse_uint8("LightRenderer.shading_image", batch_mpi)
        if not batch_mpi.is_cuda:
            raise _lib.GmpiError("LightRenderer.shading_image needs tensors on a ROCm device (no CPU path)")
        assert batch_mpi.ndim == 5 and batch_mpi.shape[2] == 4, f"Expected an RGBA volume (#mpi, #planes, 4, h, w), got {tuple(batch_mpi.shape)}"
        light_direction = self._next_light(batch_mpi.shape[0])
        plane_ds = mpi_plane_dhws[:, :1].detach().to(batch_mpi.device)
        xyz_last = mpi_tex_pix_xyz[-1, :, :, :3].detach()
        depth = compute_depth(batch_mpi[:, :, 3:], plane_ds)                                        # [B,1,H,W] float32
        if torch.is_grad_enabled() and depth.requires_grad:
            return _ShadingFunction.apply(depth, self, xyz_last, light_direction, self.cur_ka, self.cur_kd)
        return self.shading(self.blurrer_func(depth), xyz_last, light_direction, self.cur_ka, self.cur_kd).unsqueeze(1)

    def _shade_images(self, depth: torch.Tensor, mpi_tex_pix_xyz: torch.Tensor, light_direction: torch.Tensor, rgb: torch.Tensor,
                      background: torch.Tensor):
        """The image-sized middle of the augmentation (blur, point cloud, normals, Lambert) and the shading of the colour images, shared by
        `render_shared` and `render_depth`: expected depth [B,1,H,W] fp32, rgb, background or None -> (clip(rgb * shading, 0, 1),
        clip(background * shading, 0, 1) or None) in float32.  middle="torch": torch ops under autograd; middle="hip": `_ShadeImagesFunction`."""
        dev = depth.device
        H, W = depth.shape[-2:]
        if self.middle == "hip":
            return _ShadeImagesFunction.apply(depth, rgb, background, self, mpi_tex_pix_xyz[-1, :, :, :3].detach(), light_direction, self.cur_ka,
                                              self.cur_kd)
        xyz_last = mpi_tex_pix_xyz[-1, :, :, :3].detach().to(dev, torch.float32)
        blurred = _blur_torch(depth, _blur_matrix(H, self._k1d, dev), _blur_matrix(W, self._k1d, dev))
        shading = _shading_torch(blurred, xyz_last, light_direction.to(dev, torch.float32), self.cur_ka, self.cur_kd).unsqueeze(1)   # [B,1,H,W]
        shade = lambda c: torch.clip(c.to(torch.float32) * shading, min=0.0, max=1.0)
        return shade(rgb), (None if background is None else shade(background))

    def _next_light(self, B: int) -> torch.Tensor:
        """One step of the augmentation's schedule: advances `step`, draws the light position on the sphere (consumes the torch RNG exactly as
        the reference's gen_sphere_path call), sets cur_ka / cur_kd; returns the light direction [B,3] (host tensor)."""
        self.step += 1
        c2w, _, _ = poses.gen_sphere_path(n_cams=B, sphere_center=self.sphere_center, sphere_r=self.sphere_r,
                                          yaw_mean=self.l_h_mean, yaw_std=self.l_h_std, pitch_mean=self.l_v_mean,
                                          pitch_std=self.l_v_std, n_truncated_stds=2, flag_rnd=True,
                                          sample_method="truncated_gaussian", given_yaws=None, given_pitches=None)
        with poses.host_math():
            light_pos = c2w[:, :3, 3]
            light_pos = light_pos if isinstance(light_pos, torch.Tensor) else torch.FloatTensor(light_pos)
            light_direction = poses._unit(self.sphere_center.reshape(1, 3) - light_pos)  # towards the sphere centre
        cur_ratio = min(1.0, self.step / self.n_grow_iters)
        self.cur_ka, self.cur_kd = cur_ratio * self.ka_max, cur_ratio * self.kd_max
        return light_direction

    def render(self, batch_mpi: torch.Tensor, mpi_plane_dhws: torch.Tensor, mpi_tex_pix_xyz: torch.Tensor) -> torch.Tensor:
        """batch_mpi [B,D,4,H,W], mpi_plane_dhws [D,3], mpi_tex_pix_xyz [D,H,W,>=3] -> shaded MPI [B,D,4,H,W] float32
        (differentiable w.r.t. batch_mpi: two streaming kernels for the volume-sized ends, the image-sized middle by `_middle_backward` in the
        mode of this renderer -- torch autograd over a restatement, or with middle="hip" two adjoint kernels, where a cell whose un-normalised
        normal is exactly 0 contributes 0 instead of the restatement's NaN; the forward does not depend on the mode)."""
        _refuse_uint8("LightRenderer.render", batch_mpi)
        if not batch_mpi.is_cuda:
            raise _lib.GmpiError("LightRenderer.render needs tensors on a ROCm device (no CPU path)")
        dev = batch_mpi.device
        vol = batch_mpi if batch_mpi.dtype in _DTYPES else batch_mpi.float()
        if vol.stride(4) != 1 or any(s < 0 for s in vol.stride()) or vol.stride(1) == 0 or vol.stride(2) == 0 or vol.stride(3) < vol.shape[4]:
            vol = vol.contiguous()   # (what the apply entries refuse, see _alpha_operand; a batch stride of 0 they take)
        light_direction = self._next_light(vol.shape[0])
        plane_ds = mpi_plane_dhws[:, :1].detach().to(dev)
        xyz_last = mpi_tex_pix_xyz[-1, :, :, :3].detach()
        if torch.is_grad_enabled() and vol.requires_grad:
            return _LightFunction.apply(vol, self, plane_ds, xyz_last, light_direction, self.cur_ka, self.cur_kd)
        return self._forward_kernels(vol, plane_ds, xyz_last, light_direction, self.cur_ka, self.cur_kd)[0]
