"""Test-only inputs in which every plane of a deep stack counts, and the per-plane gradient comparison that goes with them.

A white-noise alpha channel (U[0,1)) lets the transmittance fall by about e per plane: behind plane ~30 nothing changes an output by as much
as half an ulp, so the chunk boundaries, the table ring, the plane split and the back half of every backward sweep are never looked at.
`thin` and `surface` keep T healthy through hundreds of planes; `plane_visibility` measures, on a reference render, how much an output moves
when one plane is taken out (tests/test_visible_stacks_cpu.py holds the inputs of the GPU tests to >= 100 x the bar those tests apply);
`slab_compare` checks a volume gradient per (MPI, plane, channel) image instead of per tensor.  Never imported by the product."""
import numpy as np
import torch

ALPHA_LAWS = ("noise", "thin", "surface")
SLAB_REL = 5e-5        # the project's gradient bar (tests/test_hip_shared_color.py `_compare`), applied to the slab's own maximum
SLAB_REF_FACTOR = 4    # ... or 4 x the deviation of the same chain in fp32 from float64 (another summation order), whichever is larger
E_REF_CAP = 1e-4       # the inputs are chosen so that e_ref stays below this in every slab: the self-calibrating bar cannot hide anything
_SIG_BITS = {torch.bfloat16: 8, torch.float16: 11}


def _store(t, dtype, like):
    """Round to the storage dtype.  torch in -> tensor of that dtype; numpy in -> float32 array holding the stored values."""
    if isinstance(like, np.ndarray):
        return (t if dtype is None else t.to(dtype)).float().numpy()
    return t if dtype is None else t.to(dtype)


def _f32(rgba):
    return (torch.from_numpy(rgba) if isinstance(rgba, np.ndarray) else rgba).float().clone()


def thin(rgba, budget=1.5, dtype=None):
    """rgba [M,D,4,Ht,Wt] with alpha ~ U[0,1): alpha scaled by 2 budget / D (never up), so that sum_k alpha_k ~ budget and T_out ~ e^-budget
    whatever D is, then rounded to `dtype`."""
    v = _f32(rgba)
    v[:, :, 3] *= min(1.0, 2.0 * budget / v.shape[1])
    return _store(v, dtype, rgba)


def surface(rgba, width=1.5, peak=0.9, floor=0.5, dtype=None):
    """An MPI-like stack: alpha_k(x, y) = peak exp(-((k - s(x, y)) / width)^2) + noise floor / D, where the surface position s ramps along
    the diagonal of the texture from -1 to D over its central half (the corners, which a camera may not see, stay at -1 and D): every plane
    is the dominant one somewhere, depth spans the whole range, and every plane has nearly opaque texels with planes behind them.  The
    colours and the noise are rgba's own."""
    v = _f32(rgba)
    M, D, _, Ht, Wt = v.shape
    y = torch.arange(Ht, dtype=torch.float64, device=v.device).view(Ht, 1) / max(Ht - 1, 1)
    x = torch.arange(Wt, dtype=torch.float64, device=v.device).view(1, Wt) / max(Wt - 1, 1)
    t = ((0.5 * (x + y) - 0.25) / 0.5).clamp(0.0, 1.0)
    s = -1.0 + (D + 1.0) * t                                                  # [Ht,Wt]
    k = torch.arange(D, dtype=torch.float64, device=v.device).view(D, 1, 1)
    bump = peak * torch.exp(-((k - s[None]) / width) ** 2)                    # [D,Ht,Wt]
    v[:, :, 3] = (bump[None].float() + v[:, :, 3] * (floor / D)).clamp(max=1.0)
    return _store(v, dtype, rgba)


def make_alpha(rgba, alpha="noise", dtype=None):
    """Apply one of ALPHA_LAWS to a white-noise volume ("noise": as it is), rounded to `dtype`."""
    if alpha == "noise":
        return _store(_f32(rgba), dtype, rgba)
    return {"thin": thin, "surface": surface}[alpha](rgba, dtype=dtype)


def listed_planes(D):
    """Every plane for D <= 98; for deeper stacks the first, the last and the ones around the ring (32) and chunk (96) boundaries."""
    if D <= 98:
        return list(range(D))
    return sorted({k for k in (0, 1, 31, 32, 33, 95, 96, 97, D // 2, D - 2, D - 1) if 0 <= k < D})


def plane_visibility(render_fn, rgba, planes):
    """Reference only.  render_fn(rgba) -> (color, depth) arrays; returns {k: (max |d color|, max |d depth|)} when plane k's alpha is zeroed."""
    vol = np.array(rgba, dtype=np.float32, copy=True)
    c0, z0 = render_fn(vol)
    out = {}
    for k in planes:
        keep = vol[:, k, 3].copy()
        vol[:, k, 3] = 0.0
        c, z = render_fn(vol)
        vol[:, k, 3] = keep
        out[k] = (float(np.abs(c - c0).max()), float(np.abs(z - z0).max()))
    return out


def half_ulp(x, dtype):
    """Half a unit in the last place of every element of x in `dtype` (0 for fp32: the gradient is not rounded again)."""
    if dtype not in _SIG_BITS:
        return np.zeros_like(x)
    _, e = np.frexp(np.abs(x))
    return np.where(x == 0, 0.0, np.ldexp(1.0, e - 1 - _SIG_BITS[dtype]))


def slab_stats(ref64, ref32):
    """Per slab (all leading axes but the last two): scale = max |ref64|, e_ref = max |ref32 - ref64| / scale (0 where scale is 0)."""
    lead = ref64.shape[:-2]
    r64 = np.asarray(ref64, dtype=np.float64).reshape(-1, *ref64.shape[-2:])
    r32 = np.asarray(ref32, dtype=np.float64).reshape(r64.shape)
    scale = np.abs(r64).max(axis=(1, 2))
    dev = np.abs(r32 - r64).max(axis=(1, 2))
    e_ref = np.divide(dev, scale, out=np.zeros_like(dev), where=scale > 0)
    return scale.reshape(lead), e_ref.reshape(lead)


def slab_compare(got, ref64, ref32, dtype=torch.float32, min_rel_scale=0.0, label=""):
    """Gradient check per slab -- one (MPI, plane, channel) image of a volume gradient [M,D,C,Ht,Wt] (any leading axes: the last two are the
    image).  Every element of a slab may deviate from float64 by max(5e-5, 4 e_ref) * scale (+ half an ulp of the element for a gradient
    that comes back in 16-bit storage), scale = max |ref64| over the slab, e_ref = max |ref32 - ref64| over the slab / scale; no absolute
    term.  A slab whose scale is exactly 0 must be exactly 0.  Slabs whose scale is below min_rel_scale * (the tensor's maximum) are left
    out and counted (0: none is -- the thin and surface stacks; the white-noise cases pass 1e-6).
    Returns dict(worst=largest deviation / allowed, where=its slab, failures=[...], skipped=n, slabs=n, e_ref_max=..., scale_min_rel=...)."""
    g = np.asarray(got, dtype=np.float64)
    r64 = np.asarray(ref64, dtype=np.float64)
    assert g.shape == r64.shape, (g.shape, r64.shape)
    scale, e_ref = slab_stats(r64, ref32)
    top = float(scale.max())
    lead = r64.shape[:-2]
    res = dict(worst=0.0, where=None, failures=[], skipped=0, slabs=int(scale.size), e_ref_max=0.0,
               scale_min_rel=float(scale.min() / top) if top > 0 else 0.0)
    for idx in np.ndindex(*lead):
        sc = float(scale[idx])
        if sc == 0.0:
            if np.any(g[idx] != 0.0):
                res["failures"].append((idx, "nonzero where the reference is exactly 0", float(np.abs(g[idx]).max())))
                res["worst"], res["where"] = float("inf"), idx
            continue
        if sc < min_rel_scale * top:
            res["skipped"] += 1
            continue
        e = float(e_ref[idx])
        res["e_ref_max"] = max(res["e_ref_max"], e)
        allowed = max(SLAB_REL, SLAB_REF_FACTOR * e) * sc + half_ulp(np.maximum(np.abs(g[idx]), np.abs(r64[idx])), dtype)
        ratio = float((np.abs(g[idx] - r64[idx]) / allowed).max())
        if not np.isfinite(ratio):
            ratio = float("inf")
        if ratio > res["worst"]:
            res["worst"], res["where"] = ratio, idx
        if ratio > 1.0:
            res["failures"].append((idx, ratio, sc, e))
    print(f"{label} slabs {res['slabs']} skipped {res['skipped']} worst ratio {res['worst']:.3f} at {res['where']} "
          f"e_ref max {res['e_ref_max']:.2e} min scale / max {res['scale_min_rel']:.2e}")
    return res
