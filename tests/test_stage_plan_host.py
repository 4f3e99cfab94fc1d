"""The stereo context's stage plan (csrc/stage_plan.h) on the host, no GPU: which slabs exist and how a frame is routed in every switch
state, and the one function that allocates and frees the slabs under a walk of switch flips with allocation failures injected."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_stage_plan_walk(tmp_path):
    """tests/cpp/stage_plan_walk.cpp: all 96 switch states (colour off / 3 / 4 channels, factor 1 / 2, remap, smoothing, slot, host /
    device source) — the wanted slabs against the six existence conditions and their geometry, the route against the table of DESIGN.md
    6.1, both restated there; every id a route names exists; caller memory is never written; only the slot works in place, smoothing
    never; the detector reads upload[parity] unless no stage ran on a device pair."""
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = str(tmp_path / "stage_plan_walk")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "vslam_pose_estimation_framework_amd", "csrc"), "-o", exe,
                           os.path.join(CPP, "stage_plan_walk.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "stage plan walk: ok (96 states)" in out.stdout, out.stdout + out.stderr


def test_stage_slabs_follow_the_plan_through_failing_switches():
    """tests/cpp/test_stage_reconcile.cpp under ASan + UBSan: stage_slabs_reconcile on counting stand-ins, 2000 seeded switch flips per
    pass in the setters' shape, the k-th allocation of a flip failing for every k a reconcile reaches — live allocations are the plan's
    wanted set at the right byte counts after every flip, a failed flip leaves its switch off, everything is freed exactly once."""
    subprocess.run(["make", "-C", CPP, "test_stage_reconcile"], check=True, capture_output=True)
    out = subprocess.run([os.path.join(CPP, "test_stage_reconcile")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "live allocations follow the plan, every allocation freed exactly once" in out.stdout
