"""What CLAHE costs on the device, next to global equalisation.  Not a test.

    python tests/validation/clahe_cost.py                      step time with the slot off, with global equalisation and with CLAHE (clip 40, 8 x 8):
                                                               157 streams and 1 stream at 1241 x 376, device images (the caller's memory is read,
                                                               the pair lands in the input slabs)
    python tests/validation/clahe_cost.py --kernels random     60 frames of 157 streams on random images under global equalisation, then 60 under CLAHE,
    python tests/validation/clahe_cost.py --kernels flat       and nothing else: run under a kernel trace, the four kernels are read off its statistics

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
from vslam_pose_estimation_framework_amd import hip      # noqa: E402

WORLDS, RING = 4, 10
CLIP, TILES = 40.0, (8, 8)


def switch(g, mode):
    if mode == "global":
        g.set_equalization(True)
    elif mode == "clahe":
        g.set_clahe(True, CLIP, TILES)


def step_times(cfg, frames, B, mode, steps=60, warmup=20):
    """Median wall time per step of B streams, every step submitted and waited for (ms)."""
    dev = torch.device("cuda", 0)
    g = hip.load()
    g.create(cfg, 0, B)
    switch(g, mode)
    rows, cols = int(cfg.rows), int(cfg.cols)
    L = torch.stack([torch.stack([torch.from_numpy(frames[s % WORLDS][j][0]) for s in range(B)]) for j in range(RING)]).to(dev)
    R = torch.stack([torch.stack([torch.from_numpy(frames[s % WORLDS][j][1]) for s in range(B)]) for j in range(RING)]).to(dev)
    torch.cuda.synchronize()
    ts = []
    for k in range(warmup + steps):
        j = k % (2 * RING - 2)
        j = j if j < RING else 2 * RING - 2 - j
        t0 = time.perf_counter()
        g.process_device(L[j].data_ptr(), R[j].data_ptr(), cols, rows * cols)
        g.synchronize()
        ts.append(time.perf_counter() - t0)
    fi = g.frame_info(0)
    g.destroy()
    return 1e3 * float(np.median(ts[warmup:])), fi.n_keypoints_left, fi.status


def kernels_only(cfg, content, B=157, frames=60):
    dev = torch.device("cuda", 0)
    rows, cols = int(cfg.rows), int(cfg.cols)
    if content == "random":
        L = torch.randint(0, 256, (B, rows, cols), dtype=torch.uint8, device=dev)
    else:
        L = torch.full((B, rows, cols), 117, dtype=torch.uint8, device=dev)
    for mode in ("global", "clahe"):
        g = hip.load()
        g.create(cfg, 0, B)
        switch(g, mode)
        torch.cuda.synchronize()
        for _ in range(frames):
            g.process_device(L.data_ptr(), L.data_ptr(), cols, rows * cols)
        g.synchronize()
        g.destroy()
    print("%s: %d frames of %d streams per mode, %.1f MB per step read by each kernel" % (content, frames, B, 2 * B * rows * cols / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", choices=("random", "flat"), default=None)
    ap.add_argument("--frames", type=int, default=60, help="frames per mode of the --kernels legs (fewer under a counter collection)")
    a = ap.parse_args()
    o = Oracle()
    scene = o.scene_kitti()
    cfg = o.config_for_scene(scene)
    if a.kernels:
        kernels_only(cfg, a.kernels, frames=a.frames)
        return
    frames = []
    for w in range(WORLDS):
        sc = o.scene_kitti(seed=7 + 2 * w)
        frames.append([o.render(sc, k) for k in range(RING)])
    o.destroy()
    for B in (157, 1):
        res = {mode: step_times(cfg, frames, B, mode) for mode in ("off", "global", "clahe")}
        off = res["off"][0]
        print("%3d streams at %d x %d: step %.3f ms off, %.3f ms global equalisation (+%.3f ms, +%.1f %%), %.3f ms CLAHE %g %dx%d (+%.3f ms, +%.1f %%); "
              "keypoints left %d / %d / %d, status %d / %d / %d" % (
                  B, int(cfg.cols), int(cfg.rows), off, res["global"][0], res["global"][0] - off, 100.0 * (res["global"][0] - off) / off,
                  res["clahe"][0], CLIP, TILES[0], TILES[1], res["clahe"][0] - off, 100.0 * (res["clahe"][0] - off) / off,
                  res["off"][1], res["global"][1], res["clahe"][1], res["off"][2], res["global"][2], res["clahe"][2]))


if __name__ == "__main__":
    main()
