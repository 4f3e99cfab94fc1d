"""What smoothing costs on the device.  Not a test.

    python tests/validation/smooth_cost.py [--out DIR]              every leg below in a process of its own, each under its own time limit;
                                                                    the kernel legs under rocprofv3 --kernel-trace --stats with nothing else
                                                                    traced, their rows and the rates read off the statistics.  A leg that
                                                                    fails or runs out of time ends the run.
    python tests/validation/smooth_cost.py --leg kernels MODE K B   60 frames of B streams of random RGB8 device pairs of 1241 x 376 in a context
                                                                    with the ORB extractor, the colour switch and smoothing MODE:K on:
                                                                    k_gray_u8 (4 B per pixel), k_smooth (2 B per pixel) and k_gauss7 (the
                                                                    extractor's 7 x 7 Gaussian on the same pair, 2 B per pixel) in one trace
    python tests/validation/smooth_cost.py --leg pmc MODE K B       the same workload, 10 frames, under rocprofv3 --pmc alone (no tracing beside
                                                                    it): k_smooth's SQ_ACTIVE_INST_VALU, SQ_ACTIVE_INST_ANY, SQ_WAIT_ANY and
                                                                    SQ_WAIT_INST_ANY over SQ_WAVE_CYCLES — the VALU issue share of a wavefront's
                                                                    lifetime and what the rest of it is
    python tests/validation/smooth_cost.py --leg steps B            step time (submit and wait, median of 60 steps behind 20 warm-up steps) of
                                                                    grey device pairs with the stage off, gaussian:5 and median:3

Yardstick 1 (a condition, every Gaussian and median 3): k_smooth's pixels per second >= 0.9 x k_gauss7's in the same trace.
Yardstick 2 (reported): k_smooth's bytes per second over k_gray_u8's, target 0.75.  A miss of yardstick 1 at the first stream count ends the
run with a non-zero status."""
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
MODES = [("gaussian", 3), ("gaussian", 5), ("gaussian", 7), ("median", 3), ("median", 5)]


def pixels(B):
    return 2 * B * ROWS * COLS


def leg_kernels(mode, ksize, B, frames=60):
    import torch
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import color, hip, smooth
    o = Oracle()
    cfg = o.config_for_scene(o.scene_kitti())
    o.destroy()
    assert (int(cfg.rows), int(cfg.cols)) == (ROWS, COLS)
    cfg.descriptor_type = 1                    # the ORB extractor: k_gauss7 runs on the pair the detector read
    dev = torch.device("cuda", 0)
    stride = 3 * COLS
    L = torch.randint(0, 256, (B, ROWS, stride), dtype=torch.uint8, device=dev)
    R = torch.randint(0, 256, (B, ROWS, stride), dtype=torch.uint8, device=dev)
    g = hip.load()
    g.create(cfg, 0, B)
    g.set_color_input(color.RGB8)
    g.set_smoothing(smooth.MODES[mode], ksize)
    torch.cuda.synchronize()
    for _ in range(frames):
        g.process_device(L.data_ptr(), R.data_ptr(), stride, ROWS * stride)
    g.synchronize()
    g.destroy()
    print("%s:%d, %d streams, %d frames; per step %.1f M pixels: k_gray_u8 moves %.1f MB, k_smooth and k_gauss7 %.1f MB each" % (
        mode, ksize, B, frames, pixels(B) / 1e6, 4 * pixels(B) / 1e6, 2 * pixels(B) / 1e6))


def leg_steps(B, steps=60, warmup=20):
    import numpy as np
    import torch
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip, smooth
    o = Oracle()
    cfg = o.config_for_scene(o.scene_kitti())
    frames = [[o.render(o.scene_kitti(seed=7 + 2 * w), k) for k in range(RING)] for w in range(WORLDS)]
    o.destroy()
    dev = torch.device("cuda", 0)
    L = torch.stack([torch.stack([torch.from_numpy(frames[s % WORLDS][j][0]) for s in range(B)]) for j in range(RING)]).to(dev)
    R = torch.stack([torch.stack([torch.from_numpy(frames[s % WORLDS][j][1]) for s in range(B)]) for j in range(RING)]).to(dev)
    torch.cuda.synchronize()
    out = []
    for sm in (None, ("gaussian", 5), ("median", 3)):
        g = hip.load()
        g.create(cfg, 0, B)
        if sm:
            g.set_smoothing(smooth.MODES[sm[0]], sm[1])
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
    print("%3d streams, device frames of %d x %d: step %.3f ms with the stage off, %.3f ms gaussian:5, %.3f ms median:3; keypoints left %d / %d / %d, status %d / %d / %d" % (
        (B, COLS, ROWS) + tuple(o_[0] for o_ in out) + tuple(o_[1] for o_ in out) + tuple(o_[2] for o_ in out)))


PMC = ("SQ_WAVE_CYCLES", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_ANY", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY")


def pmc_shares(trace):
    """the counters of every k_smooth dispatch summed -> {counter: share of SQ_WAVE_CYCLES}"""
    total = {}
    for path in glob.glob(os.path.join(trace, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "k_smooth" in row.get("Kernel_Name", ""):
                total[row["Counter_Name"]] = total.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    cycles = total.get("SQ_WAVE_CYCLES", 0.0)
    return {k: v / cycles for k, v in total.items()} if cycles else {}


def run_leg(args, limit, trace=None, pmc=False):
    """One leg in a process of its own under `limit` seconds; trace: the folder rocprofv3 writes its statistics (pmc: its counters alone)
    to.  -> its rows"""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg"] + [str(a) for a in args]
    if trace and pmc:
        cmd = ["rocprofv3", "--pmc"] + list(PMC) + ["--output-format", "csv", "-d", trace, "--"] + cmd
    elif trace:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--"] + cmd
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    print("\n".join(l for l in r.stdout.splitlines() if "streams" in l), flush=True)
    if r.returncode != 0:
        print(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit("leg %s ended with status %d: nothing further is started" % (" ".join(str(a) for a in args), r.returncode))
    rows = {}
    if trace:
        for path in glob.glob(os.path.join(trace, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row["Name"].split("(")[0].split("<")[0].split()[-1]      # "void k_smooth<1, 2>(SmoothArgs)" -> k_smooth
                if name not in rows or float(row["TotalDurationNs"]) > float(rows[name]["TotalDurationNs"]):
                    rows[name] = row
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", nargs="+", default=None)
    ap.add_argument("--out", default="smooth_cost_trace", help="folder for the traces (removed afterwards)")
    ap.add_argument("--streams", default="157,1", help="stream counts of the legs")
    ap.add_argument("--modes", default=",".join("%s:%d" % m for m in MODES), help="the kernel legs' modes")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-pmc", action="store_true")
    a = ap.parse_args()
    if a.leg:
        if a.leg[0] in ("kernels", "pmc"):
            leg_kernels(a.leg[1], int(a.leg[2]), int(a.leg[3]), 60 if a.leg[0] == "kernels" else 10)
        else:
            leg_steps(int(a.leg[1]))
        return
    show = ("Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs")
    counts = [int(x) for x in a.streams.split(",")]
    missed = []
    modes = [(m.split(":")[0], int(m.split(":")[1])) for m in a.modes.split(",")]
    for B in counts:
        for mode, ksize in modes:
            trace = os.path.join(a.out, "%s%d_%d" % (mode, ksize, B))
            rows = run_leg(["kernels", mode, ksize, B], 240, trace)
            for name in ("k_gray_u8", "k_smooth", "k_gauss7"):
                print('"%s",%s' % (name, ",".join(rows[name][c] for c in show)))
            tg, ts, t7 = (float(rows[n]["AverageNs"]) for n in ("k_gray_u8", "k_smooth", "k_gauss7"))
            px = pixels(B)
            y1, y2 = t7 / ts, (2 * px / ts) / (4 * px / tg)
            bound = (mode, ksize) != ("median", 5)
            if bound and y1 < 0.9 and B == counts[0]:
                missed.append((mode, ksize, y1))
            print("k_smooth %.1f Gpixel/s = %.3f TB/s, k_gauss7 %.1f Gpixel/s, k_gray_u8 %.3f TB/s; yardstick 1 (k_smooth / k_gauss7 pixels per second) %.2f%s, "
                  "yardstick 2 (k_smooth / k_gray_u8 bytes per second) %.2f\n" % (px / ts, 2 * px / ts / 1e3, px / t7, 4 * px / tg / 1e3, y1,
                                                                                   "" if bound else " (no condition)", y2), flush=True)
    for mode, ksize in ([] if a.no_pmc else modes):          # counters in runs of their own, nothing traced beside them
        trace = os.path.join(a.out, "pmc_%s%d" % (mode, ksize))
        run_leg(["pmc", mode, ksize, counts[0]], 240, trace, pmc=True)
        sh = pmc_shares(trace)
        print("%s:%d, %d streams, k_smooth, shares of SQ_WAVE_CYCLES: %s\n" % (mode, ksize, counts[0], ", ".join("%s %.3f" % (k, sh[k]) for k in PMC[1:] if k in sh) or "no counter rows found"), flush=True)
    for B in ([] if a.no_steps else counts):
        run_leg(["steps", B], 420)
    shutil.rmtree(a.out, ignore_errors=True)
    if missed:
        raise SystemExit("yardstick 1 missed: %s" % ", ".join("%s:%d %.2f" % m for m in missed))


if __name__ == "__main__":
    main()
