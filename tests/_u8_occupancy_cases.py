"""Inputs of the occupancy tests (tests/test_u8_occupancy_cpu.py, tests/test_hip_u8_occupancy.py): synthetic uint8 MPIs that are mostly empty, the
stridings the map is built from, and the brute-force definition of the map.  CPU only; nothing here is imported by the product.

    shell   a dome depth image; the alpha of plane k is non-zero for about two plane spacings around the surface (the difference of two
            `depth_alpha_planes` ramps half a spacing wide, one shifted by a spacing), exactly 0 elsewhere and outside the dome: what a stored MPI looks like
    ramp    the depth-alpha ramp itself, quantized: empty in front of the surface, opaque behind it
    noise   codes 1..255 everywhere: nothing can be skipped

Colours are white-noise codes: a kernel that skipped a box whose alpha is not all zero would show."""
import functools

import numpy as np
import torch

BLOCK = 16


def _dome(S):
    """Normalised depth [1,1,S,S] of a dome: 0.2 at the centre, 0.8 at its rim (radius 0.45 S); outside it 4.0, behind every plane."""
    y, x = np.meshgrid(np.arange(S) + 0.5, np.arange(S) + 0.5, indexing="ij")
    r2 = ((x - S / 2) ** 2 + (y - S / 2) ** 2) / (0.45 * S) ** 2
    d = np.where(r2 <= 1.0, 0.8 - 0.6 * np.sqrt(np.clip(1.0 - r2, 0.0, 1.0)), 4.0)
    return torch.from_numpy(d.astype(np.float32)).reshape(1, 1, S, S)


@functools.lru_cache(maxsize=None)
def volume(kind, S, D, seed=0, M=1):
    """uint8 codes [M,D,4,S,S], planar and contiguous, computed once and left unchanged (callers clone before they write)."""
    from ml_gmpi_amd import depth_alpha_planes
    g = torch.Generator().manual_seed(1000 * seed + 7 * S + D)
    q = torch.randint(0, 256, (M, D, 4, S, S), generator=g, dtype=torch.uint8)
    if kind == "noise":
        q[:, :, 3] = torch.randint(1, 256, (M, D, S, S), generator=g, dtype=torch.uint8)
        return q
    plane_z = torch.linspace(0.0, 1.0, D)
    sp = 1.0 / max(D - 1, 1)
    depth = _dome(S).expand(M, -1, -1, -1)
    if kind == "ramp":
        a = depth_alpha_planes(depth, plane_z, -0.5 * sp, 0.5 * sp)
    elif kind == "shell":
        a = depth_alpha_planes(depth, plane_z, -0.5 * sp, 0.5 * sp) - depth_alpha_planes(depth + sp, plane_z, -0.5 * sp, 0.5 * sp)
    else:
        raise KeyError(kind)
    q[:, :, 3] = torch.round(a[:, :, 0].clamp(0, 1) * 255.0).to(torch.uint8)
    return q


def stridings(q):
    """{name: a view holding q's codes (or, for the batch slice, those of q's even MPIs)}: planar, channels-last, a batch slice `[::2]`, rows padded by a slice."""
    from ml_gmpi_amd import layers_as_volume
    M, D, _, Ht, Wt = q.shape
    padded = torch.zeros((M, D, 4, Ht, Wt + 12), dtype=torch.uint8)
    padded[..., 4:4 + Wt] = q
    padded[..., :4] = 255          # (what lies in the padding must not be looked at)
    padded[..., 4 + Wt:] = 255
    return {"planar": q, "channels_last": layers_as_volume(q.permute(0, 1, 3, 4, 2).contiguous()), "batch_slice": q[::2],
            "padded_rows": padded[..., 4:4 + Wt]}


def brute_force_map(q):
    """The definition, as a loop: per block the largest alpha code among the texels that exist."""
    M, D, _, Ht, Wt = q.shape
    a = q[:, :, 3].numpy()
    nby, nbx = -(-Ht // BLOCK), -(-Wt // BLOCK)
    out = np.zeros((M, D, nby, nbx), dtype=np.uint8)
    for by in range(nby):
        for bx in range(nbx):
            out[:, :, by, bx] = a[:, :, by * BLOCK:min((by + 1) * BLOCK, Ht), bx * BLOCK:min((bx + 1) * BLOCK, Wt)].reshape(M, D, -1).max(-1)
    return torch.from_numpy(out)


def sparse_codes(seed, shape, p_zero=0.9):
    """Codes that are zero with probability p_zero."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(1, 256, tuple(shape), generator=g, dtype=torch.uint8)
    return torch.where(torch.rand(tuple(shape), generator=g) < p_zero, torch.zeros((), dtype=torch.uint8), q)


def corner_volumes(M, D, Ht, Wt):
    """Four volumes, alpha 0 but for a lone code at one corner texel (by its position: 0 = top left .. 3 = bottom right) of every block; colours 255."""
    out = []
    for c in range(4):
        q = torch.full((M, D, 4, Ht, Wt), 255, dtype=torch.uint8)
        q[:, :, 3] = 0
        for y0 in range(0, Ht, BLOCK):
            for x0 in range(0, Wt, BLOCK):
                y = min(y0 + BLOCK, Ht) - 1 if c & 2 else y0
                x = min(x0 + BLOCK, Wt) - 1 if c & 1 else x0
                q[:, :, 3, y, x] = 1 + (y * Wt + x) % 255
        out.append(q)
    return out


def empty_shares(q):
    """(share of all-zero 16 x 16 blocks, share of 5 x 3-block neighbourhoods (x by y, clipped at the border) that are entirely empty)."""
    m = brute_force_map(q).numpy() == 0
    nby, nbx = m.shape[-2:]
    hood = np.ones_like(m)
    for by in range(nby):
        for bx in range(nbx):
            hood[..., by, bx] = m[..., max(by - 1, 0):by + 2, max(bx - 2, 0):bx + 3].all(axis=(-1, -2))
    return float(m.mean()), float(hood.mean())
