"""What downscaling costs on the device.  Not a test.

    python tests/validation/downscale_cost.py [--out DIR]         every leg below in a process of its own, each under its own time limit;
                                                                  the kernel legs under rocprofv3 --kernel-trace --stats, their rows and
                                                                  the bytes per second read off the statistics.  A leg that fails or runs
                                                                  out of time ends the run.
    python tests/validation/downscale_cost.py --leg kernels F B   60 frames of B streams of random RGB8 device images of 1241 x 376 with the
                                                                  colour switch and the downscale by F on and nothing else: k_gray_u8 (the
                                                                  yardstick: 4 B per full pixel) and k_downscale_u8 (F F + 1 B per reduced
                                                                  pixel) in one trace
    python tests/validation/downscale_cost.py --leg depth B       30 frames of a batch of B RGB-D sequences on device frames of 1281 x 401, the
                                                                  downscale by 2 ahead of the undistortion (raw 640 x 200 -> 620 x 188):
                                                                  k_downscale_depth_u16 beside k_undistort_depth on the tracker's own planes
    python tests/validation/downscale_cost.py --leg steps B       step time of a full-resolution context against a context that downscales the
                                                                  same device frames by 2 (median of 60 steps behind 20 warm-up steps)

The step-time leg plays four rendered worlds forwards and backwards over ten frames, so that the trackers keep tracking."""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ROWS, COLS = 376, 1241
WORLDS, RING = 4, 10


def leg_kernels(f, B, frames=60):
    import torch
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import color, downscale, hip
    o = Oracle()
    cfg = downscale.apply_to_config(o.config_for_scene(o.scene_kitti()), f)
    o.destroy()
    assert (int(cfg.rows), int(cfg.cols)) == (ROWS // f, COLS // f)
    dev = torch.device("cuda", 0)
    stride = 3 * COLS
    L = torch.randint(0, 256, (B, ROWS, stride), dtype=torch.uint8, device=dev)
    R = torch.randint(0, 256, (B, ROWS, stride), dtype=torch.uint8, device=dev)
    g = hip.load()
    g.create(cfg, 0, B)
    g.set_color_input(color.RGB8)
    g.set_downscale(f, ROWS, COLS)
    torch.cuda.synchronize()
    for _ in range(frames):
        g.process_device(L.data_ptr(), R.data_ptr(), stride, ROWS * stride)
    g.synchronize()
    g.destroy()
    print("factor %d, %d streams, %d frames; per step k_gray_u8 moves %.1f MB, k_downscale_u8 %.1f MB" % (
        f, B, frames, gray_bytes(B) / 1e6, downscale_bytes(f, B) / 1e6))


def gray_bytes(B):
    return 2 * B * ROWS * COLS * 4


def downscale_bytes(f, B):
    return 2 * B * (ROWS // f) * (COLS // f) * (f * f + 1)


DEPTH_FULL, DEPTH_RAW = (401, 1281), (200, 640)      # full frames, the raw size behind the downscale by 2 (undistorted: 188 x 620)


def leg_depth(B, frames=30):
    """The RGB-D tracker's own planes: a batch of B sequences on device frames with the downscale by 2 ahead of the undistortion."""
    import numpy as np
    import torch
    import downscale_cases as dc
    import undistort_cases as uc
    from _oracle import Oracle
    from test_undistort_gpu import SHIFT
    from vslam_pose_estimation_framework_amd import hip, rectify
    from vslam_pose_estimation_framework_amd.capi import RgbdBatch
    os.environ["VSLAM_RGBD_HOST"] = "0"
    o = Oracle()
    cfg, p, K, world = dc.rgbd_world(o, 26, 2, frames=2)
    o.destroy()
    und = rectify.undistortion(uc.raw_camera(K, uc.FREIBURG1, DEPTH_RAW[0], DEPTH_RAW[1], SHIFT), K, int(cfg.rows), int(cfg.cols))
    # the rendered full frame, cut / padded to the full size of this rig, the same for every sequence but for a shift: real texture and depth
    L0 = np.zeros(DEPTH_FULL, np.uint8); D0 = np.zeros(DEPTH_FULL, np.uint16)
    L0[:376, :1241] = world[0][0]; D0[:376, :1241] = world[0][1]
    L = np.stack([np.roll(L0, 3 * s, axis=1) for s in range(B)]); D = np.stack([np.roll(D0, 3 * s, axis=1) for s in range(B)])
    dev = torch.device("cuda", 0)
    Ld = torch.from_numpy(L).to(dev); Dd = torch.from_numpy(D.view(np.int16)).to(dev)
    torch.cuda.synchronize()
    g = hip.load()
    t = RgbdBatch(g, cfg, p, B)
    t.set_undistortion(und)
    t.set_downscale(2, *DEPTH_FULL)
    for _ in range(frames):
        t.submit_device(Ld.data_ptr(), DEPTH_FULL[1], DEPTH_FULL[0] * DEPTH_FULL[1], Dd.data_ptr(), DEPTH_FULL[1], DEPTH_FULL[0] * DEPTH_FULL[1])
        t.wait(infos=False)
    t.destroy()
    print("depth: %d sequences, %d frames; per frame k_downscale_depth_u16 moves %.1f MB, k_undistort_depth %.1f MB" % (
        B, frames, depth_downscale_bytes(B) / 1e6, depth_undistort_bytes(B) / 1e6))


def depth_downscale_bytes(B):
    return B * DEPTH_RAW[0] * DEPTH_RAW[1] * (4 * 2 + 2)          # four elements read, one written per reduced pixel


def depth_undistort_bytes(B):
    return B * 188 * 620 * (2 + 2) + ((B + 7) // 8) * 188 * 620 * 6      # one element gathered and one written per pixel; the maps once per 8 sequences


def leg_steps(B, steps=60, warmup=20):
    import numpy as np
    import torch
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import downscale, hip
    o = Oracle()
    cfg_full = o.config_for_scene(o.scene_kitti())
    cfg_red = downscale.apply_to_config(o.config_for_scene(o.scene_kitti()), 2)
    frames = [[o.render(o.scene_kitti(seed=7 + 2 * w), k) for k in range(RING)] for w in range(WORLDS)]
    o.destroy()
    dev = torch.device("cuda", 0)
    L = torch.stack([torch.stack([torch.from_numpy(frames[s % WORLDS][j][0]) for s in range(B)]) for j in range(RING)]).to(dev)
    R = torch.stack([torch.stack([torch.from_numpy(frames[s % WORLDS][j][1]) for s in range(B)]) for j in range(RING)]).to(dev)
    torch.cuda.synchronize()
    out = []
    for cfg, f in ((cfg_full, 1), (cfg_red, 2)):
        g = hip.load()
        g.create(cfg, 0, B)
        if f > 1:
            g.set_downscale(f, ROWS, COLS)
        ts = []
        for k in range(warmup + steps):
            j = k % (2 * RING - 2)
            j = j if j < RING else 2 * RING - 2 - j
            t0 = time.perf_counter()
            g.process_device(L[j].data_ptr(), R[j].data_ptr(), COLS, ROWS * COLS)
            g.synchronize()
            ts.append(time.perf_counter() - t0)
        fi = g.frame_info(0)
        out.append((1e3 * float(np.median(ts[warmup:])), fi.n_keypoints_left, fi.status))
        g.destroy()
    (t1, kp1, st1), (t2, kp2, st2) = out
    print("%3d streams, device frames of %d x %d: step %.3f ms at full resolution, %.3f ms downscaled by 2 (x %.2f); keypoints left %d / %d, status %d / %d" % (
        B, COLS, ROWS, t1, t2, t2 / t1, kp1, kp2, st1, st2))


def run_leg(args, limit, out_dir, trace=None):
    """One leg in a process of its own under `limit` seconds; trace: the folder rocprofv3 writes its statistics to.  -> its rows"""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg"] + [str(a) for a in args]
    if trace:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--"] + cmd
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    text = "\n".join(l for l in r.stdout.splitlines() if l.startswith(("factor", "depth:", " ")) or "streams" in l)
    print(text, flush=True)
    if r.returncode != 0:
        print(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit("leg %s ended with status %d: nothing further is started" % (" ".join(str(a) for a in args), r.returncode))
    rows = {}
    if trace:
        for path in glob.glob(os.path.join(trace, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row["Name"].split("(")[0].split("<")[0].split()[-1]      # "void k_downscale_u8<2>(DownscaleArgs)" -> k_downscale_u8
                if name not in rows or float(row["TotalDurationNs"]) > float(rows[name]["TotalDurationNs"]):
                    rows[name] = row
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", nargs="+", default=None)
    ap.add_argument("--out", default="downscale_cost_trace", help="folder for the traces (removed afterwards)")
    a = ap.parse_args()
    if a.leg:
        if a.leg[0] == "kernels":
            leg_kernels(int(a.leg[1]), int(a.leg[2]))
        elif a.leg[0] == "depth":
            leg_depth(int(a.leg[1]))
        else:
            leg_steps(int(a.leg[1]))
        return
    show = ("Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs")
    for B in (157, 1):
        for f in (2, 3, 4):
            trace = os.path.join(a.out, "k%d_%d" % (f, B))
            rows = run_leg(["kernels", f, B], 240, a.out, trace)
            for name in ("k_gray_u8", "k_downscale_u8"):
                print('"%s",%s' % (name, ",".join(rows[name][c] for c in show)))
            tg, td = float(rows["k_gray_u8"]["AverageNs"]), float(rows["k_downscale_u8"]["AverageNs"])
            bg, bd = gray_bytes(B) / tg, downscale_bytes(f, B) / td        # bytes per ns = GB/s
            print("k_gray_u8 %.3f TB/s, k_downscale_u8 %.3f TB/s, ratio %.2f\n" % (bg / 1e3, bd / 1e3, bd / bg), flush=True)
    for B in (128, 1):
        trace = os.path.join(a.out, "depth%d" % B)
        rows = run_leg(["depth", B], 300, a.out, trace)
        for name in ("k_downscale_depth_u16", "k_undistort_depth"):
            print('"%s",%s' % (name, ",".join(rows[name][c] for c in show)))
        td, tu = float(rows["k_downscale_depth_u16"]["AverageNs"]), float(rows["k_undistort_depth"]["AverageNs"])
        print("k_downscale_depth_u16 %.3f TB/s, k_undistort_depth %.3f TB/s\n" % (depth_downscale_bytes(B) / td / 1e3, depth_undistort_bytes(B) / tu / 1e3), flush=True)
    for B in (157, 1):
        run_leg(["steps", B], 420, a.out)
    shutil.rmtree(a.out, ignore_errors=True)


if __name__ == "__main__":
    main()
