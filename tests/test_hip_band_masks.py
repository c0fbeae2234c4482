"""GPU tests of the band kernel's DMA exec masks (ml-gmpi_amd/csrc/gmpi_band_masks.hpp: closed-form scalar arithmetic on the box shape, where the
kernel used to ballot a per-lane predicate).  The masks decide which texels of a box are staged, so a wrong one shows as a pixel that samples
texels of another plane.  Smallest launches that have every wave role -- one or two band rows (16-bit volumes: 256 x 16 pixels, fp32: 128 x 16),
12 planes, textures of 208^2 and 296^2 texels under a 256^2 camera, so that the items per line AND the rows of a sub-block's box change between
consecutive planes (asserted on the host replay of the table kernel, tools/band_shape_changes.py: the tests cannot pass vacuously) -- under
four cameras: frontal; tilted until a box needs the last DMA pass (the third; fp32: the fourth and the fifth); boxes that hang over the texture
edge (zeros padding: the loader's predicated form); one sub-block whose box does not fit (its band takes the direct gather next to a staged band).
Bars: strict-order mode bit-identical to kernel_variant="gather" (colour, depth, T), default mode within 1e-5 of it; the [0,1] test still
fires on ONE bad texel in the last row / the last item column of a box -- the lanes a wrong mask would switch off."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from test_hip_parity import TOL, hip_render

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, S = 12, 256
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


@functools.lru_cache(maxsize=None)
def _replay():
    spec = importlib.util.spec_from_file_location("band_shape_changes", os.path.join(ROOT, "tools", "band_shape_changes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _renderer():
    from ml_gmpi_amd.renderer import MPIRenderer, PRESETS
    kw = dict(PRESETS["FFHQ"])
    kw.update(n_mpi_planes=D, plan_spatial_enlarge_factor=1.001, plane_distances_sample_method="inverse", cam_sample_method="truncated_gaussian",
              mpi_align_corners=True, use_confined_volume=True, device=torch.device("cpu"), ray_backend="torch")
    r = MPIRenderer(**kw)
    r.set_cam(r.cam_fov, S, S)
    return r


@functools.lru_cache(maxsize=None)
def _camera(yaw, pitch):
    """Rays [3, S, S], eye [3], z axis [3] of the 256^2 pinhole camera at (yaw, pitch); the tests render windows of it (any window of a pinhole
    ray field is one)."""
    r = _renderer()
    cam = r.sample_cam_poses(1, 0, 0, 0, 0, False, given_yaws=torch.tensor([[float(yaw)]]), given_pitches=torch.tensor([[float(pitch)]]))
    return cam[3][0][0].contiguous(), cam[4][0][0].contiguous(), cam[5][0][0].contiguous()


def _dhw():
    return _renderer().static_mpi_plane_dhws.reshape(-1, 3).float().contiguous()


def _elem_size(dtype):
    return 4 if dtype == torch.float32 else 2


@functools.lru_cache(maxsize=None)
def _volume(T, dtype):
    g = torch.Generator().manual_seed(1000 + T)
    return torch.rand((1, D, 4, T, T), generator=g).to(dtype)


# camera -> candidate (yaw, pitch) and what the host replay must show for a window of H rows
POSES = {
    "frontal": [(0.0, 0.0)],
    "last_pass": [(0.25, -0.2), (0.25, 0.25), (0.2, 0.25), (0.1, -0.2), (0.1, 0.2), (0.05, 0.25)],
    "padded": [(0.3, 0.0), (0.1, -0.2), (0.2, 0.1)],
    "unfit": [(0.0, 0.0)],
}
# textures per camera and element size (a tilted camera's boxes over the 296-texel texture are wider than the 10 items of a 16-bit box)
TEXTURES = {("frontal", 2): (208, 296), ("frontal", 4): (208, 296), ("last_pass", 2): (208,), ("last_pass", 4): (208, 296),
            ("padded", 2): (208,), ("padded", 4): (208, 296), ("unfit", 2): (208, 296), ("unfit", 4): (208, 296)}


def _wanted(camera, boxes, es):
    """Does this window show what the camera is there for?  (host replay of the table kernel)"""
    rp = _replay()
    ch = rp.shape_changes(boxes)
    if boxes["unfit"].any() or ch["changes"].max() < 4 or ch["nq"].max() < 1 or ch["rows"].max() < 1:
        return False
    rows, padded = boxes["rows"], boxes["padded"]
    if camera == "frontal":
        return not padded.any()
    if camera == "last_pass":   # the last pass on the plain path; fp32 (passes of 3 rows): the fourth pass (10..12 rows) as well
        return bool(((rows > 12) & ~padded).any()) and (es == 2 or bool(((rows > 9) & (rows <= 12) & ~padded).any()))
    if camera == "padded":
        return bool(padded.any()) and bool((~padded).any())
    return not padded.any()


def _case(camera, dtype, T, H=16):
    """(ray [1,3,H,W], eye [1,3], zd [1,3], dhw [1,D,3], boxes): the first window of the first candidate pose that shows what `camera` is for."""
    rp = _replay()
    es = _elem_size(dtype)
    W = 256 if es == 2 else 128
    dhw = _dhw()
    for yaw, pitch in POSES[camera]:
        ray, eye, zd = _camera(yaw, pitch)
        for y0 in range(0, S - H + 1, 8):
            for x0 in range(0, S - W + 1, 64):
                win = ray[:, y0:y0 + H, x0:x0 + W].contiguous()
                boxes = rp.box_shapes(win.numpy(), eye.numpy(), dhw.numpy(), T, T, es)
                if not _wanted(camera, boxes, es):
                    continue
                if camera == "unfit":
                    # one corner pixel of ONE sub-block (second band row, first sub-block) looks where a pixel 40 columns to its right looks: the box of that
                    # sub-block grows past the item columns a buffer holds, its band takes the direct gather, the band above stays staged
                    win = win.clone()
                    win[:, 8, 63] = win[:, 8, 103]
                    boxes = rp.box_shapes(win.numpy(), eye.numpy(), dhw.numpy(), T, T, es)
                    unfit = boxes["unfit"].any(0)
                    assert unfit.sum() == 1 and unfit[1, 0], unfit
                return win[None], eye[None], zd[None], dhw[None], boxes
    raise AssertionError(f"no window of {POSES[camera]} shows a '{camera}' case for element size {es}, texture {T}")


@functools.lru_cache(maxsize=None)
def _gather(camera, dtype, T):
    ray, eye, zd, dhw, _ = _case(camera, dtype, T)
    return hip_render(_volume(T, dtype), dhw, ray, eye, zd, variant="gather", strict=True, check_last=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("camera", list(POSES))
def test_band_matches_gather_when_box_shapes_change_every_plane(camera, dtype):
    rp = _replay()
    for T in TEXTURES[camera, _elem_size(dtype)]:
        ray, eye, zd, dhw, boxes = _case(camera, dtype, T)
        staged = {k: v[:, ~boxes["unfit"].any(0)] for k, v in boxes.items() if k in ("shape", "nq", "rows")}
        changes = (staged["shape"][1:] != staged["shape"][:-1]).sum(0)
        assert changes.max() >= 4 and (staged["nq"][1:] != staged["nq"][:-1]).any() and (staged["rows"][1:] != staged["rows"][:-1]).any(), (camera, T, changes)
        vol = _volume(T, dtype)
        ref = _gather(camera, dtype, T)
        assert int(ref["status"][0]) == 0
        strict = hip_render(vol, dhw, ray, eye, zd, variant="band", strict=True, check_last=False)
        assert int(strict["status"][0]) == 0, (camera, T)
        for k in ("color", "depth", "T"):
            assert np.array_equal(strict[k], ref[k]), (camera, T, k, np.abs(strict[k] - ref[k]).max())
        fast = hip_render(vol, dhw, ray, eye, zd, variant="band", check_last=False)
        assert int(fast["status"][0]) == 0, (camera, T)
        for k in ("color", "depth", "T"):
            err = float(np.abs(fast[k] - ref[k]).max())
            print(f"{camera} {dtype} texture {T}: default mode against the strict gather, {k}: {err:.3e}")
            assert err <= TOL, (camera, T, k, err)


def _edge_texel(boxes, ray, eye, dhw, T, es, which):
    """A texel in the last row (`which` = "row") / the last item column ("col") of some sub-block's box that a pixel of THAT sub-block samples and no
    pixel of another sub-block does: (plane, texel row, texel column).  The window is one band row (no band below); a last-row texel is taken
    from a pixel at least 4 pixels inside its sub-block, a last-column texel from the rightmost sub-block (nothing to its right); the pixel's
    coordinates stay 0.1 texel clear of the texel borders, so the default mode's reciprocal divisions sample the same texels."""
    rp = _replay()
    tpi = rp.geometry(es)["kTPI"]
    _, H, W = ray.shape
    ix, iy = rp.plane_coords(ray, eye, dhw, T, T)            # [D, H, W]
    fx, fy = ix - np.floor(ix), iy - np.floor(iy)
    clear = (fx > 0.1) & (fx < 0.9) & (fy > 0.1) & (fy < 0.9)
    n_sub = boxes["nq"].shape[2]
    for k in range(1, D):
        for b in (range(n_sub) if which == "row" else [n_sub - 1]):
            if boxes["padded"][k, 0, b] or boxes["unfit"][k, 0, b]:
                continue
            qx0, by0, nq, rows = (int(boxes[n][k, 0, b]) for n in ("qx0", "by0", "nq", "rows"))
            for py in range(H):
                for px in range(b * 64 + (4 if which == "row" else 0), min(b * 64 + 64, W) - (4 if which == "row" else 0)):
                    if not clear[k, py, px]:
                        continue
                    x0, y0 = int(np.floor(ix[k, py, px])), int(np.floor(iy[k, py, px]))
                    if which == "row" and y0 + 1 == by0 + rows - 1:
                        return k, y0 + 1, x0
                    if which == "col" and (x0 + 1 - qx0) // tpi == nq - 1:
                        return k, y0, x0 + 1
    raise AssertionError(f"no pixel samples the last {which} of a box")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_range_check_sees_the_last_row_and_the_last_item_column_of_a_box(dtype):
    es = _elem_size(dtype)
    T = 208
    ray, eye, zd, dhw, boxes = _case("frontal", dtype, T, H=8)
    vol = _volume(T, dtype)
    assert int(hip_render(vol, dhw, ray, eye, zd, variant="band", check_last=False)["status"][0]) == 0
    for which, chan, value in (("row", 3, 1.5), ("col", 1, -0.25)):
        k, ty, tx = _edge_texel(boxes, ray[0].numpy(), eye[0].numpy(), dhw[0].numpy(), T, es, which)
        assert 0 <= ty < T and 0 <= tx < T
        bad = vol.clone()
        bad[0, k, chan, ty, tx] = value
        for strict in (False, True):
            with pytest.raises(AssertionError):
                hip_render(bad, dhw, ray, eye, zd, variant="band", strict=strict, check_last=False)
