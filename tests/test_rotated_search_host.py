"""CPU checks of the rotation-aware automatic guess: the C structs of include/lk_engine.h against their ctypes / numpy
mirrors, lk_rotation_table from plain C and through the binding against numpy, and its refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_c(tmp_path, name, body, link=False):
    src = tmp_path / (name + ".c")
    src.write_text('#include <math.h>\n#include <stddef.h>\n#include <stdio.h>\n#include "lk_engine.h"\n' + body)
    exe = tmp_path / name
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)]
    if link:
        cmd += ["-L" + os.path.join(ROOT, "correlation_amd"), "-llk_engine", "-Wl,-rpath," + os.path.join(ROOT, "correlation_amd"), "-lm"]
    r = subprocess.run(cmd + ["-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()


def test_struct_layouts_match_the_header(tmp_path):
    lines = compile_c(tmp_path, "layout",
                      "#define F(T, m) printf(#T \" \" #m \" %zu\\n\", offsetof(T, m))\n"
                      "int main(void) {\n"
                      '  printf("lk_rotated_search size %zu\\n", sizeof(lk_rotated_search));\n'
                      '  printf("lk_rotated_match size %zu\\n", sizeof(lk_rotated_match));\n'
                      "  F(lk_rotated_search, search); F(lk_rotated_search, angle_center); F(lk_rotated_search, angle_step);\n"
                      "  F(lk_rotated_search, n_half);\n"
                      "  F(lk_rotated_match, center_x); F(lk_rotated_match, center_y); F(lk_rotated_match, shift_x);\n"
                      "  F(lk_rotated_match, shift_y); F(lk_rotated_match, n_samples); F(lk_rotated_match, n_valid);\n"
                      "  F(lk_rotated_match, status); F(lk_rotated_match, angle_index); F(lk_rotated_match, score);\n"
                      "  F(lk_rotated_match, runner_up); F(lk_rotated_match, angle_runner_up); F(lk_rotated_match, angle);\n"
                      "  F(lk_rotated_match, angle_refined);\n"
                      '  printf("max angles %d\\n", LK_RS_MAX_ANGLES);\n'
                      "  return 0; }\n")
    want = [f"lk_rotated_search size {C.sizeof(_ffi.LkRotatedSearch)}", f"lk_rotated_match size {C.sizeof(_ffi.LkRotatedMatch)}"]
    want += [f"lk_rotated_search {f} {getattr(_ffi.LkRotatedSearch, f).offset}" for f, _ in _ffi.LkRotatedSearch._fields_]
    want += [f"lk_rotated_match {f} {getattr(_ffi.LkRotatedMatch, f).offset}" for f, _ in _ffi.LkRotatedMatch._fields_]
    want.append(f"max angles {_ffi.RS_MAX_ANGLES}")
    assert lines == want
    d = ca.ROTATED_MATCH_DTYPE
    assert d.itemsize == C.sizeof(_ffi.LkRotatedMatch) == 64 and d.fields["score"][1] == 32
    assert [d.fields[f][1] for f, _ in _ffi.LkRotatedMatch._fields_] == [getattr(_ffi.LkRotatedMatch, f).offset
                                                                         for f, _ in _ffi.LkRotatedMatch._fields_]
    # no padding: the fields fill the 64 bytes
    assert sum(d.fields[f][0].itemsize for f in d.names) == 64
    assert C.sizeof(_ffi.LkRotatedSearch) == C.sizeof(_ffi.LkGuessSearch) + 12


def ulp_apart(a, b):
    """distance in float32 steps"""
    ia, ib = (np.asarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7fffffff), i) for i in (ia, ib))
    return np.abs(ia - ib)


@pytest.mark.parametrize("step_deg,n_half,center_deg", [(5.0, 6, 0.0), (1.0, 180, 0.0), (0.25, 40, 33.0), (7.5, 0, -20.0), (10.0, 1, 10.0)])
def test_rotation_table_agrees_with_numpy(step_deg, n_half, center_deg):
    step, center = np.float32(np.deg2rad(step_deg)), np.float32(np.deg2rad(center_deg))
    t = ca.rotation_table(step, n_half, center)
    assert t.shape == (2 * n_half + 1, 2) and t.dtype == np.float32
    theta = np.float64(center) + np.arange(-n_half, n_half + 1) * (np.float64(step) if n_half else 0.0)
    assert ulp_apart(t[:, 0], np.cos(theta).astype(np.float32)).max() <= 1
    assert ulp_apart(t[:, 1], np.sin(theta).astype(np.float32)).max() <= 1
    assert np.array_equal(ca.HipCorrelationEngine.rotation_table(step, n_half, center), t)
    if center_deg == 0.0:   # about zero: cos even, sin odd, the middle entry exact
        assert np.array_equal(t[:, 0], t[::-1, 0]) and np.array_equal(t[:, 1], -t[::-1, 1])
        assert t[n_half].tobytes() == np.array([1.0, 0.0], np.float32).tobytes()


def test_rotation_table_rejects_bad_configurations():
    for step, n_half, center in ((0.1, -1, 0.0), (0.1, 181, 0.0), (0.0, 1, 0.0), (-0.1, 1, 0.0), (np.nan, 1, 0.0), (np.inf, 1, 0.0),
                                 (0.1, 1, np.nan), (0.1, 0, np.inf)):
        with pytest.raises(ValueError):
            ca.rotation_table(step, n_half, center)
    assert ca.rotation_table(0.0, 0).tobytes() == np.array([[1.0, 0.0]], np.float32).tobytes()   # one angle: the step is ignored
    assert ca.rotation_table(np.nan, 0, 0.5).shape == (1, 2)
    lib = ca.load_library()
    cfg = _ffi.LkRotatedSearch(_ffi.LkGuessSearch(-1, 0, 0, 0.0, -1), 0.0, 0.1, 1)
    assert lib.lk_rotation_table(None, _ffi.fptr(np.zeros(6, np.float32))) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_rotation_table(C.byref(cfg), None) == ca.ERROR_BAD_DOMAIN


def test_rotation_table_from_plain_c(tmp_path):
    lines = compile_c(tmp_path, "table",
                      "int main(void) {\n"
                      "  lk_rotated_search cfg = {{-1, 6, 0, 0.f, -1}, 0.25f, 0.125f, 3};\n"
                      "  float t[7][2];\n"
                      "  int k, bad = 0;\n"
                      "  if (lk_rotation_table(&cfg, &t[0][0]) != LK_ERROR_NONE) return 1;\n"
                      "  for (k = -3; k <= 3; ++k) {\n"
                      "    double th = (double)cfg.angle_center + k * (double)cfg.angle_step;\n"
                      "    bad += t[k + 3][0] != (float)cos(th) || t[k + 3][1] != (float)sin(th);\n"
                      '    printf("%a %a\\n", t[k + 3][0], t[k + 3][1]);\n'
                      "  }\n"
                      "  cfg.n_half = 181;\n"
                      '  printf("bad %d refused %d\\n", bad, lk_rotation_table(&cfg, &t[0][0]) == LK_ERROR_BAD_DOMAIN);\n'
                      "  return 0; }\n", link=True)
    assert lines[-1] == "bad 0 refused 1"
    got = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines[:-1]], np.float32)
    assert got.tobytes() == ca.rotation_table(0.125, 3, 0.25).tobytes()
