"""Cost of the map's colours per step: vslam_process_device on device-resident colour frames (RGB8) with the landmark map on, with and
without vslam_enable_map_colors (one k_map_color launch behind k_map_commit), and a third context with the colours off as the control (the
spread between two identical contexts), alternating the contexts in rounds.  Usage:
    python tools/probe/time_map_color.py [streams] [frames] [rectify]     (one JSON line)
`rectify`: 1 sets a rectification of mildly distorted cameras at the frames' own size, so that the colours are fetched through the maps.
The kernels' own times (k_map_color against k_map_commit, which walks the same points): run this under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vslam_pose_estimation_framework_amd import color, hip, rectify, synth  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1
N = int(sys.argv[2]) if len(sys.argv) > 2 else 24
RECT = len(sys.argv) > 3 and int(sys.argv[3]) != 0
ROUNDS = 3

sy = synth.Synth()
dev = torch.device("cuda", 0)
probe_api = hip.load()
cfg = synth.config_for_scene(probe_api, sy.scene_kitti(7), "kitti")
cfg.max_history_frames = N + 8
rows, cols = int(cfg.rows), int(cfg.cols)
stride = (cols + 63) & ~63
img = rows * stride
G = torch.empty((2, N, B, rows, stride), dtype=torch.uint8, device=dev)
for s in range(B):
    sy.render_device(sy.scene_kitti(7 + 13 * s), 0, N, G[0, 0, s].data_ptr(), G[1, 0, s].data_ptr(), stride, B * img, torch.cuda.current_stream().cuda_stream)
torch.cuda.synchronize()
# a warm cast, as tests/color_cases.colourise gives the grey frames: R = 1.15 g, G = g, B = 0.70 g
g = G[..., :cols].to(torch.float32)
C = torch.stack([(1.15 * g).clamp(0, 255), g, 0.70 * g], dim=-1).round().to(torch.uint8).contiguous()      # [2, N, B, rows, cols, 3]
del G, g
torch.cuda.synchronize()
rect = None
if RECT:
    K = np.array(cfg.K, np.float64).reshape(3, 3)
    cams = [rectify.CameraModel(K, d, rows, cols) for d in ([-0.05, 0.01, 0.0005, -0.0005], [-0.045, 0.012, -0.0004, 0.0003])]
    rect = rectify.rectification(cams[0], cams[1], np.eye(3), np.array([float(cfg.baseline_h[0]) / K[0, 0], 0.0, 0.0]))
    rectify.apply_to_config(cfg, rect)

apis = {}
for name in ("off", "off_control", "on"):     # the order of tools/probe/time_map.py: the SECOND context of a process is the slow one there
    a = hip.load()
    a.create(cfg, 0, B)
    a.set_color_input(color.RGB8)
    if rect is not None:
        a.set_rectification(rect)
    a.enable_map(200 * N)
    if name == "on":
        a.enable_map_colors(True)
    apis[name] = a


def run(a, first, count):
    for k in range(first, first + count):
        a.process_device(C[0, k].data_ptr(), C[1, k].data_ptr(), 3 * cols, 3 * rows * cols)
    a.synchronize()


warm = min(8, N // 4)
ms = {name: [] for name in apis}
for rnd in range(ROUNDS):
    for name, a in apis.items():
        a.reset()
        run(a, 0, warm)
        t0 = time.perf_counter()
        run(a, warm, N - warm)
        ms[name].append((time.perf_counter() - t0) / (N - warm) * 1e3)
sizes = [apis["on"].map_size(s) for s in range(B)]
points = [apis["on"].frame_info(s).n_points for s in range(B)]
lit = float(np.mean([apis["on"].map_colors(s).any(axis=1).mean() for s in range(min(B, 4))]))
best = {name: min(v) for name, v in ms.items()}
print(json.dumps({"streams": B, "rows": rows, "cols": cols, "frames": N, "rounds": ROUNDS, "rectify": bool(RECT),
                  "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "best_ms_per_step": {k: round(v, 4) for k, v in best.items()},
                  "colour_cost_ms_on_minus_off": round(best["on"] - best["off"], 4),
                  "control_ms_off_control_minus_off": round(best["off_control"] - best["off"], 4), "landmarks_per_stream_mean": round(sum(sizes) / B, 1),
                  "points_per_stream_last_frame_mean": round(sum(points) / B, 1), "share_of_entries_with_a_colour": round(lit, 4)}), flush=True)
for a in apis.values():
    a.destroy()
