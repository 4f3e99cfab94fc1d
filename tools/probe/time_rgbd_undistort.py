"""Cost of undistorting raw RGB-D frames per step: vslam_rgbd_submit_batch_device + vslam_rgbd_wait on device-resident frames with the
feature on (rendered frames as a freiburg1 lens would have delivered them: k_rectify on the image queue and k_undistort_depth on the space
map's queue ahead of everything else), with the feature off on the same raw frames undistorted beforehand in numpy (everything behind
the two kernels then sees the same bits), and a second tracker with the feature off as the control (the spread between two identical
trackers).  One process, alternating the trackers in rounds.  Usage:
    python tools/probe/time_rgbd_undistort.py [sequences] [frames] [rows] [cols]     (one JSON line)
The two kernels' own time: run this under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from _oracle import Oracle  # noqa: E402  (renderer only)
from test_rgbd_mode import DEPTH_SCALE  # noqa: E402
from vslam_pose_estimation_framework_amd import hip, io_formats, rectify  # noqa: E402
from vslam_pose_estimation_framework_amd.capi import RgbdBatch  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1
N = int(sys.argv[2]) if len(sys.argv) > 2 else 24
ROWS = int(sys.argv[3]) if len(sys.argv) > 3 else 480
COLS = int(sys.argv[4]) if len(sys.argv) > 4 else 640
ROUNDS = 3
os.environ["VSLAM_RGBD_HOST"] = "0"
sys.path.insert(0, os.path.join(ROOT, "tools"))
import run_rgbd  # noqa: E402  (the tum configuration's values)

o = Oracle()
g = hip.load()
W = min(B, 4)          # rendered worlds, reused round-robin
raws, fixed = [], []
for i in range(W):
    scene = o.scene_kitti(scale=0.5, seed=23 + 7 * i)
    scene.speed_m = 0.25; scene.sway_m = 0.4
    scene.rows, scene.cols = ROWS, COLS
    scene.cx, scene.cy = COLS / 2.0, ROWS / 2.0
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    cam = rectify.CameraModel(K, io_formats.TUM_DISTORTION["freiburg1"], ROWS, COLS)
    if i == 0:
        und = rectify.undistortion(cam)
        # per raw pixel, where it looks in the pinhole image: the lens
        vv, uu = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
        xy = cam.undistort_normalized(np.stack([uu.ravel(), vv.ravel()], axis=1))
        lens = rectify.encode_map((K[0, 0] * xy[:, 0] + K[0, 2]).reshape(ROWS, COLS), (K[1, 1] * xy[:, 1] + K[1, 2]).reshape(ROWS, COLS))
    frames = [(o.render(scene, k)[0], o.render_depth(scene, k, 2e-3)) for k in range(N)]
    raws.append([(rectify.remap_u8(L, *lens), rectify.remap_nearest_u16(D, *lens)) for L, D in frames])
    fixed.append([und.apply(L, D) for L, D in raws[-1]])
cfg, p = run_rgbd.configure(g, "tum", ROWS, COLS, K, 2e-3, 1, 0, DEPTH_SCALE)
cfg.max_points = 4096; cfg.max_keypoints = 8192; cfg.max_history_frames = 64
dev = torch.device("cuda", 0)


def resident(src):
    Ld = [torch.from_numpy(np.stack([src[i % W][f][0] for i in range(B)])).to(dev) for f in range(N)]
    Dd = [torch.from_numpy(np.stack([src[i % W][f][1] for i in range(B)]).view(np.int16)).to(dev) for f in range(N)]
    return Ld, Dd


inputs = {"off": resident(fixed), "on": resident(raws)}
inputs["off_control"] = inputs["off"]
torch.cuda.synchronize()

trackers = {}
for name in ("off", "off_control", "on"):
    t = RgbdBatch(g, cfg, p, B)
    if name == "on":
        t.set_undistortion(und)
    trackers[name] = t


def run(name, first, count):
    t = trackers[name]
    Ld, Dd = inputs[name]
    for f in range(first, first + count):
        t.submit_device(Ld[f].data_ptr(), COLS, ROWS * COLS, Dd[f].data_ptr(), COLS, ROWS * COLS)
        t.wait(infos=False)


warm = min(8, N // 4)
ms = {name: [] for name in trackers}
for rnd in range(ROUNDS):
    for name, t in trackers.items():
        t.reset()
        run(name, 0, warm)
        t0 = time.perf_counter()
        run(name, warm, N - warm)
        ms[name].append((time.perf_counter() - t0) / (N - warm) * 1e3)
info = {name: [t.frame_info(s)[0] for s in range(B)] for name, t in trackers.items()}
best = {name: min(v) for name, v in ms.items()}
print(json.dumps({"config": "tum", "sequences": B, "rows": ROWS, "cols": COLS, "frames": N, "rounds": ROUNDS,
                  "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                  "best_ms_per_step": {k: round(v, 4) for k, v in best.items()},
                  "undistortion_cost_ms": round(best["on"] - best["off"], 4),
                  "control_ms_off_control_minus_off": round(best["off_control"] - best["off"], 4),
                  "points_per_sequence_mean": {k: round(float(np.mean([fi.n_points for fi in v])), 1) for k, v in info.items()},
                  "tracking": {k: int(sum(fi.status == 1 for fi in v)) for k, v in info.items()},
                  "error_flags": {k: int(max(fi.error_flags for fi in v)) for k, v in info.items()}}), flush=True)
for t in trackers.values():
    t.destroy()
o.destroy()
