"""What colour input costs on the device.  Not a test.

    python tests/validation/gray_cost.py                          step time with the switch off (grey device images) and on (RGB8 device images
                                                                  of the same frames): 157 streams and 1 stream at 1241 x 376
    python tests/validation/gray_cost.py --kernels rgb8 dense     60 frames of 157 streams on random colour images with the colour switch and the
    python tests/validation/gray_cost.py --kernels rgba8 aligned  equalisation on and nothing else: run under a kernel trace, k_gray_u8 and the
                                                                  yardstick k_equalize_apply are read off its statistics.  dense: rows of
                                                                  channels * cols bytes (three channels: every alignment); aligned: rows
                                                                  padded to a multiple of 16 bytes

The step-time legs play four rendered worlds forwards and backwards over ten frames, so that the trackers keep tracking."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from _oracle import Oracle      # noqa: E402
from color_cases import colourise      # noqa: E402
from vslam_pose_estimation_framework_amd import color, hip      # noqa: E402

WORLDS, RING = 4, 10


def step_times(cfg, frames, B, fmt, steps=60, warmup=20):
    """Median wall time per step of B streams, every step submitted and waited for (ms).  fmt GRAY8: the numpy grey of the same frames."""
    dev = torch.device("cuda", 0)
    g = hip.load()
    g.create(cfg, 0, B)
    g.set_color_input(fmt)
    rows, cols, ch = int(cfg.rows), int(cfg.cols), color.channels(fmt)
    side = 0 if fmt == color.GRAY8 else 2
    L = torch.stack([torch.stack([torch.from_numpy(frames[s % WORLDS][j][side]) for s in range(B)]) for j in range(RING)]).to(dev)
    R = torch.stack([torch.stack([torch.from_numpy(frames[s % WORLDS][j][side + 1]) for s in range(B)]) for j in range(RING)]).to(dev)
    torch.cuda.synchronize()
    ts = []
    for k in range(warmup + steps):
        j = k % (2 * RING - 2)
        j = j if j < RING else 2 * RING - 2 - j
        t0 = time.perf_counter()
        g.process_device(L[j].data_ptr(), R[j].data_ptr(), cols * ch, rows * cols * ch)
        g.synchronize()
        ts.append(time.perf_counter() - t0)
    fi = g.frame_info(0)
    g.destroy()
    return 1e3 * float(np.median(ts[warmup:])), fi.n_keypoints_left, fi.status


def kernels_only(cfg, fmt, aligned, B=157, frames=60):
    dev = torch.device("cuda", 0)
    rows, cols, ch = int(cfg.rows), int(cfg.cols), color.channels(fmt)
    stride = (ch * cols + 15) & ~15 if aligned else ch * cols
    L = torch.randint(0, 256, (B, rows, stride), dtype=torch.uint8, device=dev)
    R = torch.randint(0, 256, (B, rows, stride), dtype=torch.uint8, device=dev)      # 157 x 2 different images: 440 MB of RGB8, more than the last-level cache
    g = hip.load()
    g.create(cfg, 0, B)
    g.set_color_input(fmt)
    g.set_equalization(True)
    torch.cuda.synchronize()
    for _ in range(frames):
        g.process_device(L.data_ptr(), R.data_ptr(), stride, rows * stride)
    g.synchronize()
    g.destroy()
    px = 2 * B * rows * cols
    print("%s %s (row stride %d): %d frames of %d streams; per step k_gray_u8 moves %.1f MB (%d B per pixel), k_equalize_apply %.1f MB (2 B per pixel)" % (
        color.NAMES[fmt], "aligned" if aligned else "dense", stride, frames, B, px * (ch + 1) / 1e6, ch + 1, px * 2 / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", nargs=2, metavar=("FORMAT", "ROWS"), default=None, help="rgb8 | rgba8 | bgr8 | bgra8, dense | aligned")
    a = ap.parse_args()
    o = Oracle()
    scene = o.scene_kitti()
    cfg = o.config_for_scene(scene)
    if a.kernels:
        fmt = {v: k for k, v in color.NAMES.items()}[a.kernels[0]]
        kernels_only(cfg, fmt, a.kernels[1] == "aligned")
        return
    frames = []
    for w in range(WORLDS):
        sc = o.scene_kitti(seed=7 + 2 * w)
        rng = np.random.default_rng(100 + 7 + 2 * w)
        world = []
        for k in range(RING):
            cl, cr = (colourise(im, rng) for im in o.render(sc, k))
            world.append((color.to_gray_u8(cl, color.RGB8), color.to_gray_u8(cr, color.RGB8), cl, cr))
        frames.append(world)
    o.destroy()
    for B in (157, 1):
        off, kp0, st0 = step_times(cfg, frames, B, color.GRAY8)
        on, kp1, st1 = step_times(cfg, frames, B, color.RGB8)
        print("%3d streams at %d x %d: step %.3f ms off, %.3f ms on (+%.3f ms, +%.1f %%); keypoints left %d / %d, status %d / %d" % (
            B, int(cfg.cols), int(cfg.rows), off, on, on - off, 100.0 * (on - off) / off, kp0, kp1, st0, st1))


if __name__ == "__main__":
    main()
