"""Cost of the RGB-D landmark map and observation log per step: vslam_rgbd_submit_batch_device + vslam_rgbd_wait on the same device-resident
frames with the feature off, with the map on, with map + log on (one k_rgbd_map_commit launch behind every tail), and a second tracker
with the feature off as the control (the spread between two identical trackers).  One process, alternating the trackers in rounds.  Usage:
    python tools/probe/time_rgbd_map.py [icl|tum|xtion] [sequences] [frames] [scale]     (one JSON line)
k_rgbd_map_commit's own time: run this under rocprofv3 --kernel-trace --stats."""
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
from test_rgbd_mode import setup  # noqa: E402
from vslam_pose_estimation_framework_amd import hip  # noqa: E402
from vslam_pose_estimation_framework_amd.capi import RgbdBatch  # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else "tum"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1
N = int(sys.argv[3]) if len(sys.argv) > 3 else 40
scale = float(sys.argv[4]) if len(sys.argv) > 4 else 0.5
ROUNDS = 3
os.environ["VSLAM_RGBD_HOST"] = "0"

o = Oracle()
g = hip.load()
W = min(B, 8)          # rendered worlds, reused round-robin (tests/validation/rgbd_batch.py)
worlds = []
for i in range(W):
    scene, cfg, p = setup(o, which, scale=scale, seed=23 + 7 * i)
    worlds.append([(o.render(scene, k)[0], o.render_depth(scene, k, 2e-3)) for k in range(N)])
cfg.max_points = 4096; cfg.max_keypoints = 8192; cfg.max_history_frames = 64
rows, cols = int(cfg.rows), int(cfg.cols)
dev = torch.device("cuda", 0)
Ld = [torch.from_numpy(np.stack([worlds[i % W][f][0] for i in range(B)])).to(dev) for f in range(N)]
Dd = [torch.from_numpy(np.stack([worlds[i % W][f][1] for i in range(B)]).view(np.int16)).to(dev) for f in range(N)]
torch.cuda.synchronize()

trackers = {}
for name in ("off", "off_control", "map", "map_log"):
    t = RgbdBatch(g, cfg, p, B)
    if name in ("map", "map_log"):
        t.enable_map(200 * N)
    if name == "map_log":
        t.enable_observations(N * int(cfg.max_points))
    trackers[name] = t


def run(t, first, count):
    for f in range(first, first + count):
        t.submit_device(Ld[f].data_ptr(), cols, rows * cols, Dd[f].data_ptr(), cols, rows * cols)
        t.wait(infos=False)


warm = min(8, N // 4)
ms = {name: [] for name in trackers}
for rnd in range(ROUNDS):
    for name, t in trackers.items():
        t.reset()
        run(t, 0, warm)
        t0 = time.perf_counter()
        run(t, warm, N - warm)
        ms[name].append((time.perf_counter() - t0) / (N - warm) * 1e3)
flags = {name: int(max(t.frame_info(s)[0].error_flags for s in range(B))) for name, t in trackers.items()}
sizes = [trackers["map_log"].map_size(s) for s in range(B)]
counts = [trackers["map_log"].observation_count(s) for s in range(B)]
best = {name: min(v) for name, v in ms.items()}
print(json.dumps({"config": which, "sequences": B, "rows": rows, "cols": cols, "frames": N, "rounds": ROUNDS,
                  "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                  "best_ms_per_step": {k: round(v, 4) for k, v in best.items()},
                  "map_cost_ms": round(best["map"] - best["off"], 4), "map_log_cost_ms": round(best["map_log"] - best["off"], 4),
                  "control_ms_off_control_minus_off": round(best["off_control"] - best["off"], 4),
                  "landmarks_per_sequence_mean": round(sum(sizes) / B, 1), "observations_per_sequence_mean": round(sum(counts) / B, 1),
                  "error_flags": flags}), flush=True)
for t in trackers.values():
    t.destroy()
o.destroy()
