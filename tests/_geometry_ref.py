"""Test-only differentiable restatement of the render w.r.t. the sample POSITIONS (the plane geometry dhw, the rays, the eye positions and the
optical axes): the oracle of the geometry backward (render_backward_geometry.hip).  Unlike tests/_torch_ref.py nothing runs under no_grad:

  * the coordinate chain (gmpi/core/mpi.py:74-99 + grid_sampler's unnormalize) runs in float64 for the derivatives;
  * the bilinear corners x0 = floor(ix), y0 = floor(iy) come from the fp32 strict-order chain (one rounding per op, evaluated without grad):
    then they are the kernel's floors bit for bit -- on white noise the position gradient jumps by O(1) at a texel edge, so a floor decided
    differently would be a false failure;
  * the bilinear sample is written out (zero-padded taps, differentiable in the fractions tx = ix - x0, ty = iy - y0), composited in float64
    with om = 1 - a + 1e-10 and depth_k = s * dot.
Never imported by the product."""
import torch


def f32_coords(zdiff, pw, ph, ex, ey, rx, ry, rz, Ht, Wt, align_corners):
    """The forward's fp32 chain (gmpi_device.hpp plane_coord), all float32 tensors (broadcast): (ix, iy, narrowed_u, narrowed_v)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    s = zdiff / rz
    x = ex + rx * s
    y = ey + ry * s
    u = (2.0 * x) / pw
    v = (2.0 * y) / ph
    if align_corners:
        ix = (u + 1.0) * f((Wt - 1) * 0.5)
        iy = (v + 1.0) * f((Ht - 1) * 0.5)
        return ix, iy, None, None
    nv = (v >= -1.0) & (v <= 1.0)
    nu = (u >= -1.0) & (u <= 1.0)
    v = torch.where(nv, v * f(0.95), v)
    u = torch.where(nu, u * f(0.95), u)
    ix = ((u + 1.0) * f(float(Wt)) - 1.0) * f(0.5)
    iy = ((v + 1.0) * f(float(Ht)) - 1.0) * f(0.5)
    return ix, iy, nu, nv


def unnormalize(u, size, align_corners):
    """grid_sampler's unnormalize in float64 (differentiable)."""
    return (u + 1) * (size - 1) / 2 if align_corners else ((u + 1) * size - 1) / 2


def bilinear(vol, ix, iy, x0, y0):
    """Zero-padded bilinear sample of vol [P,C,Ht,Wt] at (ix, iy) [P,...] with the given integer corners (int64, same shape):
    [P,...,C].  Differentiable in vol, ix and iy (through the fractions)."""
    P, C, Ht, Wt = vol.shape
    pad = torch.nn.functional.pad(vol, (2, 2, 2, 2))            # taps at -2 .. Wt + 1 read zeros
    x0 = x0.clamp(-2, Wt)
    y0 = y0.clamp(-2, Ht)
    tx = ix - x0.to(ix.dtype)
    ty = iy - y0.to(iy.dtype)
    kk = torch.arange(P).view((P,) + (1,) * (ix.dim() - 1)).expand_as(x0)

    def tap(dy, dx):
        return pad[kk, :, y0 + dy + 2, x0 + dx + 2]               # [P,...,C]
    tx, ty = tx.unsqueeze(-1), ty.unsqueeze(-1)
    return (tap(0, 0) * (1 - tx) * (1 - ty) + tap(0, 1) * tx * (1 - ty) + tap(1, 0) * (1 - tx) * ty + tap(1, 1) * tx * ty)


def geometry_render(rgba, dhw, ray_dir, eye, zdir, view_to_mpi, align_corners=True):
    """rgba [M,D,4,Ht,Wt], dhw [M,D,3], ray_dir [N,3,H,W], eye / zdir [N,3] (float64, any of them may require grad) ->
    color [N,3,H,W], depth [N,1,H,W]."""
    N, _, H, W = ray_dir.shape
    M, D, _, Ht, Wt = rgba.shape
    colors, depths = [], []
    for n in range(N):
        m = int(view_to_mpi[n])
        d, ph, pw = dhw[m, :, 0].view(D, 1, 1), dhw[m, :, 1].view(D, 1, 1), dhw[m, :, 2].view(D, 1, 1)
        rx, ry, rz = ray_dir[n, 0][None], ray_dir[n, 1][None], ray_dir[n, 2][None]
        ex, ey, ez = eye[n, 0], eye[n, 1], eye[n, 2]
        with torch.no_grad():
            f = lambda t: t.detach().float()
            ix32, iy32, nu, nv = f32_coords(f(d) - f(ez), f(pw), f(ph), f(ex), f(ey), f(rx), f(ry), f(rz), Ht, Wt, align_corners)
            x0, y0 = torch.floor(ix32).long(), torch.floor(iy32).long()
        s = (d - ez) / rz
        x = ex + rx * s
        y = ey + ry * s
        u = 2 * x / pw
        v = 2 * y / ph
        if not align_corners:
            u = torch.where(nu, u * 0.95, u)
            v = torch.where(nv, v * 0.95, v)
        ix, iy = unnormalize(u, Wt, align_corners), unnormalize(v, Ht, align_corners)
        smp = bilinear(rgba[m], ix, iy, x0, y0)                     # [D,H,W,4]
        dot = ray_dir[n, 0] * zdir[n, 0] + ray_dir[n, 1] * zdir[n, 1] + ray_dir[n, 2] * zdir[n, 2]
        depth_k = s * dot[None]
        a = smp[..., 3]
        om = 1 - a + 1e-10
        T = torch.cumprod(torch.cat([torch.ones_like(om[:1]), om[:-1]], 0), 0)
        w = a * T
        colors.append((w[..., None] * smp[..., :3]).sum(0).permute(2, 0, 1))
        depths.append((w * depth_k).sum(0)[None])
    return torch.stack(colors), torch.stack(depths)


def geometry_grads(rgba, dhw, ray_dir, eye, zdir, view_to_mpi, g_color, g_depth, align_corners=True, out_pm1=False):
    """d(sum g_color * color + sum g_depth * depth) / d(dhw, ray_dir, eye, zdir) in float64, as numpy arrays.  g_depth may be None; with out_pm1
    the colour is 2 C - 1 (mpi_renderer.py:467)."""
    t = lambda a: torch.as_tensor(a).double()
    vol = t(rgba)
    geo = [t(a).clone().requires_grad_(True) for a in (dhw, ray_dir, eye, zdir)]
    color, depth = geometry_render(vol, *geo, view_to_mpi, align_corners=align_corners)
    if out_pm1:
        color = 2 * color - 1
    loss = (color * t(g_color)).sum()
    if g_depth is not None:
        loss = loss + (depth * t(g_depth)).sum()
    loss.backward()
    return [(g.grad if g.grad is not None else torch.zeros_like(g)).detach().numpy() for g in geo]   # (z_dir: none without g_depth)
