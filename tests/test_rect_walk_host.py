"""The implicit-rectangle walk of the lane-group sample loop (csrc/lk_rect_walk.hpp) on the host: tests/host/rect_walk_driver.cpp
runs the loop of evaluate<> for every width 1..70, stride 16 / 32 / 64 / 512 / 4096, first lane below min(stride, 64) (and the
last lane of the wider groups) and sample count 0, 1, rw, rw * rw, 361 and 4999, and compares (row, col) of every visited
sample with the floor division the walk replaces - rw = 1, rw = stride, rw > stride, stride a multiple of rw, lanes without
any sample and the last partial row are all among them.  Built plain and under ASan + UBSan; the program has its own main.
No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_walk_against_the_floor_division(tmp_path, flags):
    exe = tmp_path / "rect_walk_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags
                       + ["-I" + os.path.join(ROOT, "correlation_amd", "csrc"),
                          os.path.join(ROOT, "tests", "host", "rect_walk_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "rect_walk ok" in r.stdout, r.stdout[-1000:] + r.stderr[-4000:]
