"""Cost of rectification per step: vslam_process_device on the same device-resident frames with rectification off, on with identity
maps (the downstream work is then bit-identical to "off", so the difference is k_rectify and its launch alone) and on with the maps of a
distorted EuRoC-like rig (k1 = -0.28, rotations ~1 degree; the detector sees different images, so that difference also carries the
changed downstream work).  A second context without rectification is the control: the spread between two identical contexts.  One
process, alternating the contexts in rounds.  Usage:
    python tools/probe/time_rectify.py [kitti|euroc] [streams] [frames]     (one JSON line)"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vslam_pose_estimation_framework_amd import hip, rectify, synth  # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else "kitti"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1
N = int(sys.argv[3]) if len(sys.argv) > 3 else 120
ROUNDS = 3

sy = synth.Synth()
dev = torch.device("cuda", 0)
scene = sy.scene_kitti(7) if which == "kitti" else sy.scene_euroc(7)
probe_api = hip.load()
cfg = synth.config_for_scene(probe_api, scene, which)
cfg.max_history_frames = N + 8
rows, cols = int(cfg.rows), int(cfg.cols)
stride = (cols + 63) & ~63
img = rows * stride
L = torch.empty((N, B, rows, stride), dtype=torch.uint8, device=dev)
R = torch.empty_like(L)
for s in range(B):
    sc = sy.scene_kitti(7 + 13 * s) if which == "kitti" else sy.scene_euroc(7 + 13 * s)
    sy.render_device(sc, 0, N, L[0, s].data_ptr(), R[0, s].data_ptr(), stride, B * img, torch.cuda.current_stream().cuda_stream)
torch.cuda.synchronize()


class Maps(object):
    def __init__(self, maps):
        self.rows, self.cols, self.raw_rows, self.raw_cols = rows, cols, rows, cols
        (self.map_xy_left, self.map_a_left), (self.map_xy_right, self.map_a_right) = maps


yy, xx = np.mgrid[0:rows, 0:cols]
ident = (np.stack([xx, yy], -1).astype(np.int16), np.zeros((rows, cols), np.uint16))
K = np.array(cfg.K).reshape(3, 3)
B_m = -cfg.baseline_h[0] / K[0, 0]
left = rectify.CameraModel(K, [-0.28, 0.074, 0.0002, 1.8e-5], rows, cols)
right = rectify.CameraModel(K * [[1.003], [1.002], [1]], [-0.283, 0.075, -0.0001, -3.6e-5], rows, cols)
rig = rectify.rectification(left, right, rectify.rodrigues(np.radians([0.4, -0.9, 0.3])), [-B_m, 0.002, -0.001])

apis = {}
for name, maps in (("off", None), ("off_control", None), ("identity", Maps([ident, ident])), ("rig", rig)):
    a = hip.load()
    a.create(cfg, 0, B)
    if maps is not None:
        a.set_rectification(maps)
    apis[name] = a


def run(a, first, count):
    for k in range(first, first + count):
        a.process_device(L[k].data_ptr(), R[k].data_ptr(), stride, img)
    a.synchronize()


warm = min(20, N // 4)
ms = {name: [] for name in apis}
for rnd in range(ROUNDS):
    for name, a in apis.items():
        a.reset()
        run(a, 0, warm)
        t0 = time.perf_counter()
        run(a, warm, N - warm)
        ms[name].append((time.perf_counter() - t0) / (N - warm) * 1e3)
flags = {name: int(max(a.frame_info(s).error_flags for s in range(B))) for name, a in apis.items()}
best = {name: min(v) for name, v in ms.items()}
print(json.dumps({"which": which, "streams": B, "rows": rows, "cols": cols, "frames": N, "rounds": ROUNDS,
                  "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                  "best_ms_per_step": {k: round(v, 4) for k, v in best.items()},
                  "rectify_cost_ms_identity_minus_off": round(best["identity"] - best["off"], 4),
                  "rig_minus_off_ms": round(best["rig"] - best["off"], 4),
                  "control_ms_off_control_minus_off": round(best["off_control"] - best["off"], 4),
                  "error_flags": flags}), flush=True)
for a in apis.values():
    a.destroy()
