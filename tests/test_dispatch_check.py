"""The host-side dispatcher (gm_dispatch.hpp) hands every run-time switch over as the matching
compile-time constant: tools/dispatch_check.cpp walks three flags, every period and a value outside
0-3, and a returned int.  Host-only: the header includes no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_dispatcher_hands_over_constants(tmp_path):
    exe = str(tmp_path / "dispatch_check")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tools", "dispatch_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("bad 0"), out.stdout
