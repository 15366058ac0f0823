"""The polygon index's host build (gm_pip_build_host.hpp over gm_pip_layout.hpp) is plain C++:
tools/pip_host_build_check.cpp runs prepare and classify on tiny sets -- a hole, a shared edge, 513
rings, squares with holes from several chunks, stacked squares, envelopes without height or width, nothing to match -- and checks the arrays'
own invariants.  Built plain and with the host address / undefined-behaviour sanitizers, and run on
four build threads.  Host-only: neither header includes HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_host_build_invariants(tmp_path, sanitize):
    exe = str(tmp_path / "pip_host_build_check")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-pthread"] + sanitize +
                          ["-o", exe, os.path.join(ROOT, "tools", "pip_host_build_check.cpp")])
    env = dict(os.environ, GM_BUILD_THREADS="4")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("bad 0"), out.stdout
    assert "runtime error" not in out.stderr, out.stderr
