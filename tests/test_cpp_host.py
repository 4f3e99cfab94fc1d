"""C++ above the C ABI, compiled with plain g++ (no hipcc, no torch) and run as separate processes:
  - the test-only host mirror of the reference's plug-in interface (tests/cpp/proslam_hip_mirror.hpp) against the oracle;
  - the SHIM (shim/proslam_hip_plugin.h: HipStereoFramePointGenerator / HipStereoUVAligner deriving from the reference's
    classes) against minimal declaration stubs of the reference interfaces it touches (tests/shim_stubs/, test-only): it
    must compile (signature drift against base_framepoint_generator.h / base_aligner.h / frame.h fails here), link, and —
    on the GPU box — reproduce the fused device path frame by frame, host objects included;
  - csrc/device_store.h (the memory a switchable feature owns on the device) on counting malloc / free stand-ins, under
    AddressSanitizer and UndefinedBehaviorSanitizer: host code only, no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _build(target):
    subprocess.run(["make", "-C", CPP, target], check=True, capture_output=True)
    return os.path.join(CPP, target)


def test_cpp_host_mirror_compiles_against_c_abi_only():
    exe = _build("test_host_tracker")
    assert os.access(exe, os.X_OK)
    with open(os.path.join(CPP, "proslam_hip_mirror.hpp")) as f:
        text = f.read()
    assert "torch" not in text and "hip_runtime" not in text   # plain C ABI consumer


def test_shim_compiles_links_and_fails_loudly_without_a_gpu():
    exe = _build("test_shim")
    with open(os.path.join(ROOT, "shim", "proslam_hip_plugin.h")) as f:
        text = f.read()
    for virtual in ("void initialize(Frame* frame_, const bool& extract_features_ = true) override", "void compute(Frame* frame_) override",
                    "void recoverPoints(Frame* current_frame_, const FramePointPointerVector& lost_points_) const override",
                    "void converge() override", "void linearize(const bool&) override", "void oneRound(const bool&) override"):
        assert virtual in text, virtual
    assert "oracle" not in text.lower().replace("oracle/_ref", "")
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by test_shim_reproduces_fused_path")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fails loudly without a GPU" in out.stdout


def test_device_store_frees_every_allocation_exactly_once():
    """Enable / replace / disable, a failure at every allocation of a store, a double release and destroy with stores live."""
    exe = _build("test_device_store")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "every allocation freed exactly once" in out.stdout


@pytest.mark.gpu
def test_cpp_host_tracker_matches_oracle():
    exe = _build("test_host_tracker")
    out = subprocess.run([exe, "12"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "identical to the oracle" in out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("recovery,orb", [(1, 0), (0, 0), (1, 1)])
def test_shim_reproduces_fused_path(recovery, orb):
    """Both shim classes through the C ABI, driven like PoseTracker3D drives its plug-ins: 16 frames, counters, poses and the
    materialised host objects (points, links, descriptors) equal to the fused device path; with and without recovery (the
    device prune must not depend on recoverPoints being called)."""
    exe = _build("test_shim")
    out = subprocess.run([exe, "16", str(recovery), str(orb)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "identical to the fused device path" in out.stdout and ("descriptor ORB" if orb else "descriptor BRIEF") in out.stdout
