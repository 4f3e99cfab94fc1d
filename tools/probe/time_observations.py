"""Cost of the observation log per step: vslam_process_device on the same device-resident frames with the map on and the log off, with
the log on (vslam_enable_observations: one k_obs_append launch behind k_map_commit), and a second context with the log off as the control
(the spread between two identical contexts).  One process, alternating the contexts in rounds.  Usage:
    python tools/probe/time_observations.py [kitti|euroc] [streams] [frames]     (one JSON line)
k_obs_append's and k_map_commit's own times: run this under rocprofv3 --kernel-trace --stats; both are in the same trace."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from vslam_pose_estimation_framework_amd import hip, synth  # noqa: E402

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

apis = {}
for name in ("off", "off_control", "on"):
    a = hip.load()
    a.create(cfg, 0, B)
    a.enable_map(200 * N)
    if name == "on":
        a.enable_observations(N * int(cfg.max_points))      # cannot overflow
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
counts = [apis["on"].observation_count(s) for s in range(B)]
sizes = [apis["on"].map_size(s) for s in range(B)]
best = {name: min(v) for name, v in ms.items()}
print(json.dumps({"which": which, "streams": B, "rows": rows, "cols": cols, "frames": N, "rounds": ROUNDS,
                  "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                  "best_ms_per_step": {k: round(v, 4) for k, v in best.items()},
                  "log_cost_ms_on_minus_off": round(best["on"] - best["off"], 4),
                  "control_ms_off_control_minus_off": round(best["off_control"] - best["off"], 4),
                  "observations_per_stream_mean": round(sum(counts) / B, 1), "observations_per_stream_and_frame": round(sum(counts) / B / N, 1),
                  "landmarks_per_stream_mean": round(sum(sizes) / B, 1), "error_flags": flags}), flush=True)
for a in apis.values():
    a.destroy()
