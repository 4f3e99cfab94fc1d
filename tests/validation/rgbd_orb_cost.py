#!/usr/bin/env python3
"""Cost of detector_type ORB in RGB-D mode on the two loops.

    python tests/validation/rgbd_orb_cost.py [--repeats 5] [--json OUT.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/validation/rgbd_orb_cost.py --leg device-188x620 --repeats 1

The tum configuration with the OrbDetector and the ORB extractor on the synthetic street, 12 frames per pass (reset between passes), host
frames through process().  Legs, one process each (the loop is chosen by the environment when the tracker is created; the parent opens no
GPU and runs them one after the other):
  device-188x620, device-480x640   the device-resident loop, one sequence
  host-188x620, host-480x640       the host-driven loop (VSLAM_RGBD_HOST=1): what served this mode before, the yardstick
  batch8-188x620                   the device-resident loop, eight sequences in one context (the figure is per step of eight frames)
  graph-188x620                    the device-resident loop, one sequence, captured launch sequence (VSLAM_RGBD_GRAPH=1)
The figure is the wall time per frame (per step for the batch), the median over the repeats after one warm-up pass."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FRAMES = 12
LEGS = ("device-188x620", "host-188x620", "device-480x640", "host-480x640", "batch8-188x620", "graph-188x620")


def run_leg(leg, repeats):
    import numpy as np
    kind, size = leg.split("-")
    rows, cols = (int(v) for v in size.split("x"))
    os.environ["VSLAM_RGBD_HOST"] = "1" if kind == "host" else "0"
    os.environ["VSLAM_RGBD_GRAPH"] = "1" if kind == "graph" else "0"
    import run_rgbd
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip
    from vslam_pose_estimation_framework_amd.capi import RgbdBatch, RgbdTracker
    o = Oracle()
    g = hip.load()
    B = 8 if kind == "batch8" else 1
    worlds = []
    for s in range(B):
        scene = o.scene_kitti(scale=0.5, seed=26 + s)
        scene.speed_m = 0.25; scene.sway_m = 0.4
        scene.rows, scene.cols = rows, cols
        scene.cx, scene.cy = cols / 2.0, rows / 2.0
        worlds.append([(o.render(scene, k)[0], o.render_depth(scene, k, 2e-3)) for k in range(FRAMES)])
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    cfg, p = run_rgbd.configure(g, "tum", rows, cols, K, 2e-3, 1, 1, 4.0)
    o.destroy()
    t = RgbdTracker(g, cfg, p) if B == 1 else RgbdBatch(g, cfg, p, B)
    steps = [(np.stack([w[k][0] for w in worlds]), np.stack([w[k][1] for w in worlds])) for k in range(FRAMES)] if B > 1 else worlds[0]
    per_frame, last = [], None
    for rep in range(repeats + 1):               # the first pass warms up
        t.reset()
        t0 = time.perf_counter()
        for L, D in steps:
            last = t.process(L, D)
        dt = (time.perf_counter() - t0) / FRAMES
        if rep:
            per_frame.append(dt * 1e3)
    fi = last[0][0] if B > 1 else last[0]
    t.destroy()
    return {"leg": leg, "sequences": B, "ms_per_frame": per_frame, "median_ms": float(np.median(per_frame)), "n_keypoints_left_last": int(fi.n_keypoints_left),
            "n_points_last": int(fi.n_points), "status_last": int(fi.status)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--leg", default="", choices=("",) + LEGS)
    a = ap.parse_args()
    if a.leg:
        print("RGBD_ORB_COST " + json.dumps(run_leg(a.leg, a.repeats)))
        return
    res = {"frames_per_pass": FRAMES, "repeats": a.repeats, "legs": {}}
    for leg in LEGS:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--repeats", str(a.repeats)], stdout=subprocess.PIPE, timeout=600, check=True).stdout.decode()
        v = json.loads([ln for ln in out.split("\n") if ln.startswith("RGBD_ORB_COST ")][-1][len("RGBD_ORB_COST "):])
        res["legs"][leg] = v
        print("rgbd_orb_cost leg=%s: median %.4f ms per %s (%s), n_keypoints_left %d, n_points %d, status %d" % (
            leg, v["median_ms"], "step of %d frames" % v["sequences"] if v["sequences"] > 1 else "frame", " ".join("%.4f" % x for x in v["ms_per_frame"]),
            v["n_keypoints_left_last"], v["n_points_last"], v["status_last"]), flush=True)
    for size in ("188x620", "480x640"):
        d, h = res["legs"]["device-" + size]["median_ms"], res["legs"]["host-" + size]["median_ms"]
        print("rgbd_orb_cost %s: device loop %.4f ms, host-driven loop %.4f ms per frame: %s" % (size, d, h, "device loop not above" if d <= h else "DEVICE LOOP ABOVE THE HOST-DRIVEN LOOP"))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
