#!/usr/bin/env python3
"""Cost of the per-frame masks in RGB-D mode and of k_map_valid.

    python tests/validation/rgbd_mask_cost.py [--repeats 5] [--json OUT.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/validation/rgbd_mask_cost.py --repeats 1

Frame masks: the tum configuration on the synthetic street at 188 x 620 and 480 x 640, one sequence, 12 frames per pass (reset between
passes), host frames through process(); legs `static` (the static mask only: k_mask_apply per attempt), `frame-host` (static + a host
frame mask per frame: its copy, one k_mask_pack, k_mask_apply on the effective words), `frame-device` (the same from a device mask)
and `frame-device-keep` (an all-255 device mask: the frame-mask machinery with the detections of the static leg).  The figure is the
wall time per frame, the median over the repeats; `frame-device-keep` minus `static` is what the machinery costs, the other two legs
also do less work behind the detector because their rectangle removes detections.
k_map_valid: vslam_set_rectification_mask on a context that rectifies 376 x 1241 through identity maps, both sides, margin 4: the wall
time of the setter (allocation, one launch, the synchronisation) - the kernel's own time is in the trace of the second form."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

FRAMES = 12
MARGIN = 4


def rgbd_legs(o, g, rows, cols, repeats):
    import run_rgbd
    import torch
    from vslam_pose_estimation_framework_amd.capi import RgbdTracker
    scene = o.scene_kitti(scale=0.5, seed=26)
    scene.speed_m = 0.25; scene.sway_m = 0.4
    scene.rows, scene.cols = rows, cols
    scene.cx, scene.cy = cols / 2.0, rows / 2.0
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    cfg, p = run_rgbd.configure(g, "tum", rows, cols, K, 2e-3, 1, 0, 4.0)
    frames = [(o.render(scene, k)[0], o.render_depth(scene, k, 2e-3)) for k in range(FRAMES)]
    yy, xx = np.mgrid[0:rows, 0:cols]
    blob = np.where(((xx - 0.15 * cols) / (0.04 * cols)) ** 2 + ((yy - 0.25 * rows) / (0.12 * rows)) ** 2 <= 1.0, 0, 255).astype(np.uint8)
    masks = []
    for k in range(FRAMES):
        m = np.full((rows, cols), 255, np.uint8)
        x0 = (41 * k + cols // 4) % (cols - cols // 3)
        m[rows // 10:rows // 10 + (2 * rows) // 3, x0:x0 + cols // 3] = 0
        masks.append(m)
    dev_masks = [torch.from_numpy(m).cuda() for m in masks]
    torch.cuda.synchronize()
    out = {}
    keep_mask = torch.full((rows, cols), 255, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    for leg in ("static", "frame-device-keep", "frame-host", "frame-device"):
        t = RgbdTracker(g, cfg, p)
        t.set_detection_mask(blob, MARGIN)
        per_frame = []
        detected = 0
        for rep in range(repeats + 1):               # the first pass warms up
            t.reset()
            t0 = time.perf_counter()
            for k, (L, D) in enumerate(frames):
                if leg == "frame-host":
                    t.set_frame_mask(masks[k], MARGIN)
                elif leg == "frame-device":
                    t.set_frame_mask(dev_masks[k], MARGIN)
                elif leg == "frame-device-keep":
                    t.set_frame_mask(keep_mask, MARGIN)
                fi, _ = t.process(L, D)
            dt = (time.perf_counter() - t0) / FRAMES
            detected = fi.n_detected_left
            if rep:
                per_frame.append(dt * 1e3)
        t.destroy()
        out[leg] = {"ms_per_frame": per_frame, "median_ms": float(np.median(per_frame)), "n_detected_left_last": int(detected)}
    return out


def map_valid_setter(o, g, repeats):
    import ctypes as C
    scene = o.scene_kitti(scale=1.0, seed=7)
    cfg = o.config_for_scene(scene)
    rows, cols = scene.rows, scene.cols
    g.create(cfg, 0, 1)
    yy, xx = np.mgrid[0:rows, 0:cols]
    xy = np.ascontiguousarray(np.stack([xx, yy], axis=2).astype(np.int16))
    xy[:, :40, 0] = -1                                # a seam on the left, so that the words are not all-keep
    fa = np.zeros((rows, cols), np.uint16)
    p16, pu16 = C.POINTER(C.c_int16), C.POINTER(C.c_uint16)
    g.check(g.fn("set_rectification")(g.ctx, C.c_int32(rows), C.c_int32(cols), xy.ctypes.data_as(p16), fa.ctypes.data_as(pu16),
                                      xy.ctypes.data_as(p16), fa.ctypes.data_as(pu16)))
    times = []
    for rep in range(repeats + 1):
        g.set_rectification_mask(False)
        t0 = time.perf_counter()
        g.set_rectification_mask(True, MARGIN)
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    g.destroy()
    return {"rows": rows, "cols": cols, "sides": 2, "margin": MARGIN, "setter_ms": times, "median_ms": float(np.median(times))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip
    os.environ["VSLAM_RGBD_HOST"] = "0"
    o = Oracle()
    g = hip.load()
    res = {"rgbd_frame_masks": {}, "margin": MARGIN, "frames_per_pass": FRAMES, "repeats": a.repeats}
    for rows, cols in ((188, 620), (480, 640)):
        legs = rgbd_legs(o, g, rows, cols, a.repeats)
        res["rgbd_frame_masks"]["%dx%d" % (rows, cols)] = legs
        for leg, v in legs.items():
            print("rgbd_mask_cost %dx%d leg=%s: median %.4f ms per frame (%s), n_detected_left %d" % (
                rows, cols, leg, v["median_ms"], " ".join("%.4f" % x for x in v["ms_per_frame"]), v["n_detected_left_last"]))
    res["map_valid_setter"] = map_valid_setter(o, g, a.repeats)
    v = res["map_valid_setter"]
    print("rgbd_mask_cost k_map_valid via vslam_set_rectification_mask at %dx%d, 2 sides, margin %d: median %.4f ms per call (%s)" % (
        v["rows"], v["cols"], v["margin"], v["median_ms"], " ".join("%.4f" % x for x in v["setter_ms"])))
    o.destroy()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
