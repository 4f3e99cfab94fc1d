#!/usr/bin/env python3
"""Cost of the detection masks at KITTI size: one leg per process, meant to run under a kernel trace of its own,

    rocprofv3 --kernel-trace --stats -d DIR -- python tests/validation/mask_cost.py --streams 157 --leg frame

legs: `static` (the static mask only: k_mask_apply), `frame` (static + per-frame device masks: the fused k_mask_pack), `off` (no mask);
every leg rectifies through identity maps, so that k_rectify, which walks the same 2 W H B bytes, appears in the same trace as the yardstick
beside k_emit.  Prints the wall time per frame as well (device frames, submitted back to back, synchronised at the end)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1)
    ap.add_argument("--leg", choices=("off", "static", "frame"), default="static")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--margin", type=int, default=4)
    a = ap.parse_args()
    import torch
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip
    o = Oracle()
    scene = o.scene_kitti(scale=1.0, seed=7)
    cfg = o.config_for_scene(scene)
    rows, cols, B = scene.rows, scene.cols, a.streams
    cfg.max_history_frames = 64
    g = hip.load()
    g.create(cfg, 0, B)
    yy, xx = np.mgrid[0:rows, 0:cols]
    xy = np.ascontiguousarray(np.stack([xx, yy], axis=2).astype(np.int16))
    fa = np.zeros((rows, cols), np.uint16)
    p16, pu16 = C.POINTER(C.c_int16), C.POINTER(C.c_uint16)
    g.check(g.fn("set_rectification")(g.ctx, C.c_int32(rows), C.c_int32(cols), xy.ctypes.data_as(p16), fa.ctypes.data_as(pu16),
                                      xy.ctypes.data_as(p16), fa.ctypes.data_as(pu16)))
    pairs = [o.render(scene, k) for k in range(4)]
    dev = [(torch.from_numpy(np.repeat(L[None], B, 0)).cuda(), torch.from_numpy(np.repeat(R[None], B, 0)).cuda()) for L, R in pairs]
    blob = np.where(((xx - 0.4 * cols) / (0.36 * cols)) ** 2 + ((yy - 0.55 * rows) / (0.36 * rows)) ** 2 <= 1.0, 0, 255).astype(np.uint8)
    if a.leg != "off":
        g.set_detection_mask(blob, blob, a.margin)
    fm = None
    if a.leg == "frame":
        rect = np.full((rows, cols), 255, np.uint8)
        rect[rows // 4:rows // 2, cols // 2:cols // 2 + cols // 5] = 0
        fm = torch.from_numpy(np.repeat(rect[None], B, 0)).cuda()
    torch.cuda.synchronize()

    def frame(k):
        L, R = dev[k % 4]
        if fm is not None:
            g.set_frame_masks(fm, fm, a.margin)
        g.process_device(L.data_ptr(), R.data_ptr(), cols, rows * cols)
    for k in range(10):
        frame(k)
    g.synchronize()
    t0 = time.perf_counter()
    for k in range(a.frames):
        frame(k)
    g.synchronize()
    dt = (time.perf_counter() - t0) / a.frames
    fi = g.frame_info(0)
    print("mask_cost leg=%s streams=%d margin=%d: %.4f ms per frame, n_detected_left %d, n_keypoints_left %d" % (
        a.leg, B, a.margin, dt * 1e3, fi.n_detected_left, fi.n_keypoints_left))
    g.destroy()
    o.destroy()


if __name__ == "__main__":
    main()
