"""What the depth image's bilateral filter costs on the device.  Not a test.

    python tests/validation/bilateral_cost.py                  RGB-D frame time (submit + wait, host frames) with the switch off and on, direct and under
                                                               VSLAM_RGBD_GRAPH=1, 1 and 32 sequences of the noisy tum scenes (620 x 188) of bilateral_cases.py
    python tests/validation/bilateral_cost.py --off            the off legs alone (direct and captured): run once per library (VSLAM_HIP_LIB names another
                                                               build) to set this commit beside its parent
    python tests/validation/bilateral_cost.py --kernels B      40 frames of B sequences at 640 x 480 with undistortion and the filter on, and nothing else:
                                                               run under a kernel trace, the three kernels and k_undistort_depth are read off its statistics

The frame-time legs play the twelve frames forwards and backwards, so that the trackers keep tracking."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np      # noqa: E402

import bilateral_cases as bc      # noqa: E402
from vslam_pose_estimation_framework_amd import hip, io_formats, rectify      # noqa: E402
from vslam_pose_estimation_framework_amd.capi import RgbdBatch      # noqa: E402


def frame_times(g, seqs, B, on, graph, steps=120, warmup=30):
    """Median wall time of process() on B sequences (ms), and the last frame's status and points of sequence 0."""
    os.environ["VSLAM_RGBD_HOST"] = "0"
    os.environ["VSLAM_RGBD_GRAPH"] = "1" if graph else "0"
    cfg, p = seqs[0]["cfg"], seqs[0]["p"]
    t = RgbdBatch(g, cfg, p, B)
    ring = len(seqs[0]["frames"])
    L = [np.ascontiguousarray(np.stack([seqs[s % len(seqs)]["frames"][j][0] for s in range(B)])) for j in range(ring)]
    D = [np.ascontiguousarray(np.stack([seqs[s % len(seqs)]["frames"][j][1] for s in range(B)])) for j in range(ring)]
    try:
        if on:
            t.set_bilateral(True)
        ts = []
        for k in range(warmup + steps):
            j = k % (2 * ring - 2)
            j = j if j < ring else 2 * ring - 2 - j
            t0 = time.perf_counter()
            infos = t.process(L[j], D[j])
            ts.append(time.perf_counter() - t0)
        fi = infos[0][0]
    finally:
        t.destroy()
    return 1e3 * float(np.median(ts[warmup:])), fi.status, fi.n_points


def kernels_only(g, B, frames=40):
    import run_rgbd
    rows, cols, unit = 480, 640, 1e-3
    fx, fy, cx, cy = io_formats.TUM_INTRINSICS["freiburg1"]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    cfg, p = run_rgbd.configure(g, "tum", rows, cols, K, unit)
    os.environ["VSLAM_RGBD_HOST"] = "0"
    os.environ["VSLAM_RGBD_GRAPH"] = "0"
    rng = np.random.default_rng(3)
    # a tilted wall 1 .. 5 m away with 10 % holes and the sensor noise of the test scenes; a smooth image (few corners: the trackers stay LOCALIZING)
    wall = np.rint((1.0 + 4.0 * np.linspace(0, 1, cols)[None, :] + 0.5 * np.linspace(0, 1, rows)[:, None]) / unit)
    depth = np.stack([bc.add_noise(np.where(rng.random((rows, cols)) < 0.1, 0, wall).astype(np.uint16), rng) for _ in range(B)])
    image = np.broadcast_to((np.arange(cols) * 200 // cols + 20).astype(np.uint8), (B, rows, cols)).copy()
    t = RgbdBatch(g, cfg, p, B)
    try:
        t.set_undistortion(rectify.undistortion(rectify.CameraModel(K, io_formats.TUM_DISTORTION["freiburg1"], rows, cols)))
        t.set_bilateral(True)
        for _ in range(frames):
            t.process(image, depth)
        changed = float((t.filtered_depth(0)[0] != t.undistorted(0)[1]).mean())
    finally:
        t.destroy()
    print("%d frames of %d sequences at %d x %d, undistortion and bilateral filter on; the filter changed %.1f %% of the pixels of the last frame" % (
        frames, B, cols, rows, 100 * changed))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", type=int, default=0, metavar="B")
    ap.add_argument("--off", action="store_true")
    a = ap.parse_args()
    g = hip.load()
    if a.kernels:
        kernels_only(g, a.kernels)
        return
    seqs = [bc.sequence(seed) for seed in bc.SEEDS]
    tag = os.environ.get("VSLAM_HIP_LIB") or "this build"
    for B in (1, 32):
        for graph in (0, 1):
            off = frame_times(g, seqs, B, False, graph)
            line = "%-40s %2d sequences %s: frame %.4f ms off (status %d, %d points)" % (tag, B, "captured" if graph else "direct  ", off[0], off[1], off[2])
            if not a.off:
                on = frame_times(g, seqs, B, True, graph)
                line += ", %.4f ms on (%+.4f ms; status %d, %d points)" % (on[0], on[0] - off[0], on[1], on[2])
            print(line, flush=True)


if __name__ == "__main__":
    main()
