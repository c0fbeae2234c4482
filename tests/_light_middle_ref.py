"""References for the backward of the shading augmentation's image-sized middle (blur, point cloud, normals, Lambert), in one place:
tests/test_light_middle_cpu.py pins the gather-form adjoints below to torch autograd without a GPU, tests/test_hip_light_middle.py runs the kernels
(csrc/light_kernels.hip: light_shading_backward_kernel, gaussian_blur_backward_kernel) against the same autograd.  CPU only (numpy / torch float64),
never imported by the product."""
import numpy as np
import torch
import torch.nn.functional as F

import _light_cases as lc
from _torch_ref import torch_light_render

EPS = 1e-8
B = lc.B


def surface(seed, H, W, batch=B, noise=0.02, bump=0.08):
    """A blurred-depth-like image [batch,1,H,W] float32 around 1: a smooth bump per image plus 2 % texel noise (normals that tilt both ways;
    noise=0 and a bump of 0.002: a slope below 0.2 at every shape used, every normal within 12 degrees of the axis)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    out = np.empty((batch, 1, H, W), np.float32)
    for b in range(batch):
        cy, cx = rng.uniform(-0.5, 0.5, 2)
        out[b, 0] = 1.0 + bump * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) * 2) + noise * (rng.random((H, W)) - 0.5)
    return out


def blur64(depth, k1d):
    """The reflect-padded blur of torch_light_render (its own expression) on [B,1,H,W], in the dtype of `depth`; differentiable."""
    r = k1d.numel() // 2
    k2d = torch.outer(k1d.to(depth), k1d.to(depth))[None, None]
    return F.conv2d(F.pad(depth, (r, r, r, r), mode="reflect"), k2d)


def middle_autograd(depth, xyz, light_dir, ka, kd, k1d, g_shading, dtype=torch.float64):
    """(shading [B,H,W], d sum(shading * g_shading) / d depth [B,1,H,W]) through torch_light_render's OWN middle, numpy in `dtype`: a one-plane
    volume with plane distance 1 has the expected depth alpha, and a colour of 1/16 never clips, so out[:, 0, 0] * 16 is the shading of `depth`.
    k1d = [1.0] is the identity blur: the shading formula alone."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    leaf = t(depth).clone().requires_grad_(True)
    b, _, H, W = leaf.shape
    rgba = torch.cat((torch.full((b, 1, 3, H, W), 1.0 / 16, dtype=dtype), leaf[:, None]), 2)
    out = torch_light_render(rgba, torch.ones(1, dtype=dtype), t(xyz), t(light_dir), ka, kd, torch.as_tensor(k1d).to(dtype))
    s = out[:, 0, 0] * 16
    (g,) = torch.autograd.grad(s, leaf, t(g_shading))
    return s.detach().numpy(), g.numpy()


# ---- the gather-form adjoints, restated in numpy float64 with explicit index loops -------------------------------------------------------------
def shading_backward_gather(blurred, xyz, light_dir, kd, g_shading, parts=False):
    """Adjoint of the shading formula in the form the kernel uses.  blurred [B,H,W], xyz [H,W,3], light_dir [B,3], g_shading [B,H,W] ->
    grad_blurred [B,H,W] float64.  (1) replica sums: the upstream gradient of interior cell (cy, cx) is the sum of g_shading over the pixels that
    clamp to it.  (2) per cell the chain through ka + kd diffuse, clamp(min=0) (closed), n / (|n| + EPS) and the four cross products gives one
    gradient per point of the cell (centre, up, down, left, right).  (3) five-cell gather: a texel's point collects from itself as centre and from
    its four neighbours' cells.  (4) grad_blurred = g_p . xyz / (xyz_z + EPS).  With parts=True also returns the per-role arrays."""
    d, xyz, L, gs = (np.asarray(a, np.float64) for a in (blurred, xyz, light_dir, g_shading))
    Bn, H, W = d.shape
    p = xyz[None] * (d[..., None] / (xyz[None, ..., 2:] + EPS))                       # [B,H,W,3]
    roles = {k: np.zeros((Bn, H, W, 3)) for k in ("c", "u", "d", "l", "r")}            # gradient of each point of cell (y, x), stored AT the cell
    for b in range(Bn):
        for cy in range(1, H - 1):
            for cx in range(1, W - 1):
                rows = [cy] + ([0] if cy == 1 else []) + ([H - 1] if cy == H - 2 else [])
                cols = [cx] + ([0] if cx == 1 else []) + ([W - 1] if cx == W - 2 else [])
                G = sum(gs[b, yy, xx] for yy in rows for xx in cols)                   # (1)
                c = p[b, cy, cx]
                u, dn, l, r = p[b, cy - 1, cx] - c, p[b, cy + 1, cx] - c, p[b, cy, cx - 1] - c, p[b, cy, cx + 1] - c
                n = np.cross(u, l) + np.cross(l, dn) + np.cross(dn, r) + np.cross(r, u)
                norm = np.sqrt((n * n).sum())
                nh = n / (norm + EPS)
                if not (-(nh * L[b]).sum() >= 0) or norm == 0:
                    continue
                g_nh = -kd * G * L[b]
                g_n = g_nh / (norm + EPS) - nh * (g_nh * nh).sum() / norm
                # (a x b) . g: the gradient w.r.t. a is b x g, w.r.t. b it is g x a
                g_u = np.cross(l, g_n) + np.cross(g_n, r)
                g_l = np.cross(g_n, u) + np.cross(dn, g_n)
                g_d = np.cross(g_n, l) + np.cross(r, g_n)
                g_r = np.cross(g_n, dn) + np.cross(u, g_n)
                for k, v in (("u", g_u), ("l", g_l), ("d", g_d), ("r", g_r), ("c", -(g_u + g_l + g_d + g_r))):
                    roles[k][b, cy, cx] = v
    g_p = np.zeros((Bn, H, W, 3))
    for y in range(H):
        for x in range(W):                                                              # (3): cells outside the interior hold zeros
            g_p[:, y, x] = roles["c"][:, y, x]
            if y + 1 < H:
                g_p[:, y, x] += roles["u"][:, y + 1, x]                                 # this texel is the `up` of the cell below it
            if y - 1 >= 0:
                g_p[:, y, x] += roles["d"][:, y - 1, x]
            if x + 1 < W:
                g_p[:, y, x] += roles["l"][:, y, x + 1]
            if x - 1 >= 0:
                g_p[:, y, x] += roles["r"][:, y, x - 1]
    out = (g_p * xyz[None]).sum(3) / (xyz[None, ..., 2] + EPS)                          # (4)
    return (out, roles) if parts else out


def _blur_adjoint_1d(g, k, axis):
    """Along `axis` of length n: input i receives k[t] g[j] for every tap t and every j in [0, n) with refl(j + t - r) == i.  The unpadded
    sources are s = i, s = -i (i != 0), s = 2(n-1) - i (i != n-1), and j = s - t + r."""
    g = np.moveaxis(np.asarray(g, np.float64), axis, -1)
    n, r = g.shape[-1], len(k) // 2
    out = np.zeros_like(g)
    for i in range(n):
        sources = [i] + ([-i] if i != 0 else []) + ([2 * (n - 1) - i] if i != n - 1 else [])
        for s in sources:
            for t in range(len(k)):
                j = s - t + r
                if 0 <= j < n:
                    out[..., i] += k[t] * g[..., j]
    return np.moveaxis(out, -1, axis)


def blur_backward_gather(g_blurred, k1d):
    """Adjoint of the reflect-padded separable blur, [B,H,W] -> [B,H,W] float64, one axis after the other."""
    k = np.asarray(k1d, np.float64)
    return _blur_adjoint_1d(_blur_adjoint_1d(g_blurred, k, 2), k, 1)


def blur_matrix(n, k1d):
    """The dense [n,n] operator of the 1-D reflect-padded blur in float64 (row j = weights of output j over the inputs), built from the forward's
    definition alone: out[j] = sum_t k[t] in[refl(j + t - r)]."""
    k = np.asarray(k1d, np.float64)
    r = len(k) // 2
    m = np.zeros((n, n))
    for j in range(n):
        for t in range(len(k)):
            s = abs(j + t - r)
            m[j, 2 * (n - 1) - s if s >= n else s] += k[t]
    return m
