"""Test-only float64 restatement of the render that also returns the final transmittance T = prod_k (1 - a_k + 1e-10), differentiable w.r.t.
the volume and the geometry (dhw, rays, eye positions, optical axes): the oracle of the transmittance gradient (the `_ex` backward entries of
include/gmpi_render.h).  The coordinate chain, the fp32 floors and the zero-padded bilinear sample are tests/_geometry_ref.py's, so the taps are
the kernel's.  Never imported by the product."""
import torch

from _geometry_ref import bilinear, f32_coords, unnormalize


def composite(smp, depth_k):
    """smp [D,...,4] bilinear samples (front plane first), depth_k [D,...] -> color [...,3], depth [...], T [...] (the forward of mpi.py:421-434
    with the element the reference slices off kept: T_out = T_D)."""
    a = smp[..., 3]
    om = 1 - a + 1e-10
    Tk = torch.cumprod(torch.cat([torch.ones_like(om[:1]), om], 0), 0)   # T_0 .. T_D
    w = a * Tk[:-1]
    return (w[..., None] * smp[..., :3]).sum(0), (w * depth_k).sum(0), Tk[-1]


def render(rgba, dhw, ray_dir, eye, zdir, view_to_mpi, align_corners=True):
    """rgba [M,D,4,Ht,Wt], dhw [M,D,3], ray_dir [N,3,H,W], eye / zdir [N,3] (float64, any of them may require grad) ->
    color [N,3,H,W], depth [N,1,H,W], T [N,1,H,W]."""
    N, _, H, W = ray_dir.shape
    M, D, _, Ht, Wt = rgba.shape
    colors, depths, Ts = [], [], []
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
        u = 2 * (ex + rx * s) / pw
        v = 2 * (ey + ry * s) / ph
        if not align_corners:
            u = torch.where(nu, u * 0.95, u)
            v = torch.where(nv, v * 0.95, v)
        ix, iy = unnormalize(u, Wt, align_corners), unnormalize(v, Ht, align_corners)
        smp = bilinear(rgba[m], ix, iy, x0, y0)                     # [D,H,W,4]
        dot = ray_dir[n, 0] * zdir[n, 0] + ray_dir[n, 1] * zdir[n, 1] + ray_dir[n, 2] * zdir[n, 2]
        c, z, t = composite(smp, s * dot[None])
        colors.append(c.permute(2, 0, 1))
        depths.append(z[None])
        Ts.append(t[None])
    return torch.stack(colors), torch.stack(depths), torch.stack(Ts)


def grads(rgba, dhw, ray_dir, eye, zdir, view_to_mpi, g_color=None, g_depth=None, g_T=None, align_corners=True, out_pm1=False):
    """d(sum gC * color + sum gZ * depth + sum gT * T) / d(rgba, dhw, ray_dir, eye, zdir) in float64, as numpy arrays (any of the upstream
    gradients may be None; with out_pm1 the colour is 2 C - 1, mpi_renderer.py:467)."""
    t = lambda a: torch.as_tensor(a).double()
    args = [t(a).clone().requires_grad_(True) for a in (rgba, dhw, ray_dir, eye, zdir)]
    color, depth, T = render(*args, view_to_mpi, align_corners=align_corners)
    if out_pm1:
        color = 2 * color - 1
    loss = torch.zeros((), dtype=torch.float64)
    for out, g in ((color, g_color), (depth, g_depth), (T, g_T)):
        if g is not None:
            loss = loss + (out * t(g)).sum()
    loss.backward()
    return [(a.grad if a.grad is not None else torch.zeros_like(a)).detach().numpy() for a in args]


def alpha_depth(alpha, plane_ds):
    """compute_depth in float64 (light_renderer.py:82-100, plus the final transmittance): alpha [B,D,1,H,W] (may require grad), plane_ds [D]
    -> depth [B,1,H,W], T [B,1,H,W]."""
    om = 1 - alpha + 1e-10
    Tk = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), om], 1), 1)
    w = alpha * Tk[:, :-1]
    return (w * torch.as_tensor(plane_ds, dtype=alpha.dtype).reshape(1, -1, 1, 1, 1)).sum(1), Tk[:, -1]
