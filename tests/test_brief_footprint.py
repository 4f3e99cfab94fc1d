"""csrc/brief_footprint.h (which box-patch rows, columns and 16-byte chunks a BRIEF pattern samples: what the recovery stages in LDS)
against a brute-force scan of the pattern, for the built-in pattern, the eight extreme taps, one full-width row, one column, rows -24 and
+24 only, uniformly random taps, a single tap and the full rectangle, at every alignment of a projection.  A stand-alone C++ program
(tests/cpp/test_brief_footprint.cpp), host code only, compiled here with plain g++ under AddressSanitizer and UndefinedBehaviorSanitizer
(the flags of tests/cpp's test_device_store) into the test's temporary directory; no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "test_brief_footprint.cpp")
FLAGS = ["-O1", "-g", "-std=c++14", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_footprint_builder_against_brute_force(tmp_path):
    exe = str(tmp_path / "test_brief_footprint")
    cc = subprocess.run([os.environ.get("CXX", "g++")] + FLAGS + ["-o", exe, SOURCE], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "footprint covers every pattern at every alignment" in out.stdout
