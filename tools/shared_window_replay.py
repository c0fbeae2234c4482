"""CPU replay of the colour window of render_shared_tile_kernel (ml-gmpi_amd/csrc/render_shared.hip): per 32 x 16 pixel tile the texel boxes of the
planes (from the tile's corner pixels, fp32 coordinate chain), the `inside` test and the re-anchor rule, and from them how often a tile flushes
its colour window to global memory -- at the shapes and poses tools/time_shared_color.py times (FFHQ preset, 32 planes, torch.manual_seed(3)) and
at the 2-sigma corner of the pose range.  No GPU needed.  usage: python tools/shared_window_replay.py [--window WxH] [--box WxH] [--one-window | --forward]

--window / --box: the window and the largest staged box in texels (defaults: the shared kernel's 64x32 and 56x27).  --one-window replays
render_depth_tile_kernel (ml-gmpi_amd/csrc/render_depth_tile.hip): the box limit is the window itself unless --box is given, and the background's
flush after the last plane empties the colour channels only -- the window stays filled (its depth channel), so that flush is not counted as a
window flush: with a background every tile has one colour-channel flush on top of the counts printed.  --forward replays
render_depth_window_kernel (ml-gmpi_amd/csrc/render_depth_window.hip): the front-to-back sweep, a box staged when it fits the window once widened to
whole loader items of 4 texels, the anchor column a multiple of 4, the drift direction taken from the next staged box of the 64-plane table chunk;
it counts whole-window LOADS per tile (with a background one reload of the colour channels on top) and the planes that are not staged."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ml_gmpi_amd.renderer import MPIRenderer, PRESETS  # noqa: E402

TW, TH, AP, AR, CW, CH = 32, 16, 56, 27, 64, 32   # kTileW, kTileH (gmpi_backward.hpp), kSAP, kSAR (render_shared.hip), kCW, kCH (gmpi_backward.hpp)


def boxes(dhw, ray, eye, S):
    """[N, D, tiles, 4] int boxes (x, y, nx (0: not staged), ny) of every view, plane and tile; align_corners=True, texture S x S."""
    f = np.float32
    N, _, H, W = ray.shape
    D = dhw.shape[0]
    ys0 = np.arange(0, H, TH); ys1 = np.minimum(ys0 + TH - 1, H - 1)
    xs0 = np.arange(0, W, TW); xs1 = np.minimum(xs0 + TW - 1, W - 1)
    cy = np.stack([ys0, ys0, ys1, ys1], 0)[:, :, None] + 0 * xs0[None, None, :]     # [4, ty, tx]
    cx = np.stack([xs0, xs1, xs0, xs1], 0)[:, None, :] + 0 * ys0[None, :, None]
    c = f((S - 1) * 0.5)
    out = np.zeros((N, D, cy.shape[1] * cy.shape[2], 4), np.int64)
    for n in range(N):
        r = ray[n][:, cy, cx].astype(f)                                              # [3, 4, ty, tx]
        for k in range(D):
            s = (f(dhw[k, 0]) - f(eye[n, 2])) / r[2]
            ix = ((f(2) * (f(eye[n, 0]) + r[0] * s)) / f(dhw[k, 2]) + f(1)) * c
            iy = ((f(2) * (f(eye[n, 1]) + r[1] * s)) / f(dhw[k, 1]) + f(1)) * c
            fin = (np.abs(ix) < 1e6).all(0) & (np.abs(iy) < 1e6).all(0)
            eps = f(1 / 64)
            bx, by = np.floor(ix.min(0) - eps), np.floor(iy.min(0) - eps)
            nx, ny = np.floor(ix.max(0) + eps) + 2 - bx, np.floor(iy.max(0) + eps) + 2 - by
            nx = np.where(fin & (nx <= AP) & (ny <= AR), nx, 0)
            out[n, k] = np.stack([np.where(fin, bx, 0), np.where(fin, by, 0), nx, np.where(fin, ny, 0)], -1).reshape(-1, 4)
    return out


def flushes(bb, background, one_window=False):
    """bb [D, 4] of one tile -> number of non-empty flushes of the colour window (the kernel's sweep, every gradient wanted).  one_window: the
    background's flush leaves the window filled (render_depth_tile_kernel) and is not counted."""
    D = bb.shape[0]
    wx0 = wy0 = 0
    is_open = filled = False
    count = 0
    front = bb[0]
    for k in range(D - 1, -1, -1):
        x, y, nx, ny = bb[k]
        if nx > 0:
            inside = is_open and x >= wx0 and y >= wy0 and x + nx <= wx0 + CW and y + ny <= wy0 + CH
            if not inside:
                count += filled
                filled = False
                wx0 = x + nx - CW if (front[2] > 0 and front[0] < x) else x
                wy0 = y + ny - CH if (front[2] > 0 and front[1] < y) else y
                is_open = True
            filled = True
        if k == D - 1 and background and is_open and D > 1 and not one_window:
            count += filled
            filled = False
    return count + filled


FWD_CHUNK, FWD_ITEM = 64, 4   # kWChunk, kWTPI (render_depth_window.hip)


def forward_staged(bb):
    """bb [..., 4] boxes staged against the window itself (boxes(..) with AP, AR = CW, CH) -> the same with nx = 0 where the box, widened to whole
    loader items, exceeds the window."""
    x, nx = bb[..., 0], bb[..., 2]
    wide = -(-(x + nx) // FWD_ITEM) * FWD_ITEM - (x // FWD_ITEM) * FWD_ITEM
    out = bb.copy()
    out[..., 2] = np.where(wide <= CW, nx, 0)
    return out


def loads(bb):
    """bb [D, 4] of one tile -> number of whole-window loads of the forward's front-to-back sweep."""
    D = bb.shape[0]
    wx0 = wy0 = dx = dy = 0
    is_open = False
    count = 0
    for k in range(D):
        x, y, nx, ny = (int(v) for v in bb[k])
        if nx == 0:
            continue
        if not (is_open and x >= wx0 and y >= wy0 and x + nx <= wx0 + CW and y + ny <= wy0 + CH):
            ahead = [b for b in bb[k + 1:min(k - k % FWD_CHUNK + FWD_CHUNK, D)] if b[2] > 0]
            if ahead:   # the drift: centres of this box and of the next staged one of the chunk
                ddx, ddy = 2 * int(ahead[0][0]) + int(ahead[0][2]) - (2 * x + nx), 2 * int(ahead[0][1]) + int(ahead[0][3]) - (2 * y + ny)
                dx, dy = ddx or dx, ddy or dy
            wx0 = -(-(x + nx) // FWD_ITEM) * FWD_ITEM - CW if dx < 0 else (x // FWD_ITEM) * FWD_ITEM
            wy0 = y + ny - CH if dy < 0 else y
            is_open = True
            count += 1
    return count


def main():
    global AP, AR, CW, CH
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", default=None, help="WxH of the window in texels")
    ap.add_argument("--box", default=None, help="WxH of the largest box that is staged")
    ap.add_argument("--one-window", action="store_true", help="replay render_depth_tile_kernel: one window for colour and depth")
    ap.add_argument("--forward", action="store_true", help="replay render_depth_window_kernel: window loads of the front-to-back sweep")
    args = ap.parse_args()
    if args.window:
        CW, CH = (int(v) for v in args.window.lower().split("x"))
    if args.one_window or args.forward:
        AP, AR = CW, CH
    if args.box:
        AP, AR = (int(v) for v in args.box.lower().split("x"))
    assert AP <= CW and AR <= CH, "a staged box must fit the window"
    one_window = args.one_window
    D = 32
    if args.forward:
        print(f"window loads per tile (whole reloads of the {CW} x {CH} window, all four channels; boxes that fit it once widened to items of {FWD_ITEM} texels are "
              "staged; with a background one reload of the colour channels on top), D = 32, FFHQ preset")
    elif one_window:
        print(f"window flushes per tile (non-empty flushes of the {CW} x {CH} window, all four channels; boxes up to {AP} x {AR} are staged; with a background one "
              "flush of the colour channels on top), D = 32, FFHQ preset")
    else:
        print(f"colour-window flushes per tile (non-empty flushes of the {CW} x {CH} window; alpha is flushed once per plane on top), D = 32, FFHQ preset")
    what = "loads" if args.forward else "flushes"
    print(f"{'case':34s} {'tiles':>6s} {'mean':>6s} {'max':>4s} {'tiles with 1 / 2 ' + what:>26s} {'not staged planes':>18s}")
    for S, B, extreme in ((256, 8, False), (512, 4, False), (1024, 4, False), (256, 2, True), (512, 2, True), (1024, 2, True)):
        kw = dict(PRESETS["FFHQ"])
        kw.update(n_mpi_planes=D, plan_spatial_enlarge_factor=1.001, plane_distances_sample_method="inverse", cam_sample_method="truncated_gaussian",
                  mpi_align_corners=True, use_confined_volume=True, device=torch.device("cpu"))
        r = MPIRenderer(**kw)
        r.set_cam(r.cam_fov, S, S)
        torch.manual_seed(3)
        if extreme:
            n = r.cam_pose_n_truncated_stds
            gy = torch.tensor([[(-1) ** i * n * r.horizontal_std] for i in range(B)], dtype=torch.float32)
            gp = torch.tensor([[(-1) ** (i // 2) * n * r.vertical_std] for i in range(B)], dtype=torch.float32)
            cam = r.sample_cam_poses(B, 0, 0, 0, 0, False, given_yaws=gy, given_pitches=gp)
        else:
            cam = r.sample_cam_poses(B, r.horizontal_mean, r.horizontal_std, r.vertical_mean, r.vertical_std, True)
        ray, eye = torch.cat(cam[3]).numpy(), torch.cat(cam[4]).numpy()
        dhw = r.static_mpi_plane_dhws.reshape(-1, 3).numpy()
        bb = boxes(dhw, ray, eye, S)
        if args.forward:
            bb = forward_staged(bb)
        for background in (True, False):
            if args.forward:
                cnt = np.array([loads(bb[n, :, t]) for n in range(bb.shape[0]) for t in range(bb.shape[2])])
            else:
                cnt = np.array([flushes(bb[n, :, t], background, one_window) for n in range(bb.shape[0]) for t in range(bb.shape[2])])
            name = f"{S}^2 x {B} {'2-sigma poses' if extreme else 'timed poses'} {'bg' if background else 'no bg'}"
            print(f"{name:34s} {cnt.size:6d} {cnt.mean():6.2f} {cnt.max():4d} {(cnt == 1).sum():12d} / {(cnt == 2).sum():<11d} {int((bb[..., 2] == 0).sum()):18d}")
        if not extreme:
            d = np.abs(np.diff(bb[:, :D - 1, :, :2], axis=1))
            print(f"    box drift between neighbouring planes 0..D-2: x mean {d[..., 0].mean():.1f} max {d[..., 0].max()} texels, y mean {d[..., 1].mean():.1f} max {d[..., 1].max()};"
                  f" plane widths {dhw[0, 2]:.4f} .. {dhw[D - 2, 2]:.4f}, last plane {dhw[D - 1, 2]:.4f} x {dhw[D - 1, 1]:.4f}")


if __name__ == "__main__":
    main()
