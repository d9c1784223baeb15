"""CPU checks of the automatic initial guess: the C structs of include/lk_engine.h against their ctypes / numpy mirrors, the
tie rules of the numpy reference the GPU tests compare with, and lk_tracker_override_guesses with the frame-0 search hook
of the frame loops in csrc/lk_tracker.cpp under ASan + UBSan (over the CPU mock of the engine)."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np

from correlation_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")


def reference():
    spec = importlib.util.spec_from_file_location("guess_search_reference", os.path.join(ROOT, "tests", "test_guess_search_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lk_engine.h"\n'
                   "#define F(T, m) printf(#T \" \" #m \" %zu\\n\", offsetof(T, m))\n"
                   "int main(void) {\n"
                   '  printf("lk_guess_search size %zu\\n", sizeof(lk_guess_search));\n'
                   '  printf("lk_guess_match size %zu\\n", sizeof(lk_guess_match));\n'
                   "  F(lk_guess_search, level); F(lk_guess_search, radius); F(lk_guess_search, min_samples);\n"
                   "  F(lk_guess_search, min_score); F(lk_guess_search, def_slot);\n"
                   "  F(lk_guess_match, center_x); F(lk_guess_match, center_y); F(lk_guess_match, shift_x);\n"
                   "  F(lk_guess_match, shift_y); F(lk_guess_match, n_samples); F(lk_guess_match, n_valid);\n"
                   "  F(lk_guess_match, status); F(lk_guess_match, score); F(lk_guess_match, runner_up);\n"
                   '  printf("enum %d %d %d %d %d %d %d %d\\n", LK_GS_OK, LK_GS_TEXTURELESS, LK_GS_NO_CANDIDATE, LK_GS_TOO_FEW,\n'
                   "         LK_GS_TOO_LARGE, LK_GS_WEAK, LK_GS_MAX_RADIUS, LK_GS_MAX_SAMPLES);\n"
                   "  return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    want = [f"lk_guess_search size {C.sizeof(_ffi.LkGuessSearch)}", f"lk_guess_match size {C.sizeof(_ffi.LkGuessMatch)}"]
    want += [f"lk_guess_search {f} {getattr(_ffi.LkGuessSearch, f).offset}" for f, _ in _ffi.LkGuessSearch._fields_]
    want += [f"lk_guess_match {f} {getattr(_ffi.LkGuessMatch, f).offset}" for f, _ in _ffi.LkGuessMatch._fields_]
    want.append(f"enum {_ffi.GS_OK} {_ffi.GS_TEXTURELESS} {_ffi.GS_NO_CANDIDATE} {_ffi.GS_TOO_FEW} {_ffi.GS_TOO_LARGE} "
                f"{_ffi.GS_WEAK} {_ffi.GS_MAX_RADIUS} {_ffi.GS_MAX_SAMPLES}")
    assert lines == want
    d = _ffi.GUESS_MATCH_DTYPE
    assert d.itemsize == C.sizeof(_ffi.LkGuessMatch) == 48
    assert [d.fields[f][1] for f, _ in _ffi.LkGuessMatch._fields_] == [getattr(_ffi.LkGuessMatch, f).offset
                                                                       for f, _ in _ffi.LkGuessMatch._fields_]


def template_case(t, dfm_rows):
    """a template `t` (2-D) at the origin of und; the deformed image is built from rows"""
    und = np.zeros((16, 16), np.uint8)
    und[:t.shape[0], :t.shape[1]] = t
    ys, xs = np.mgrid[0:t.shape[0], 0:t.shape[1]]
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    return und, np.asarray(dfm_rows, np.uint8), pts


def test_reference_tie_rules_and_statuses():
    ref = reference()
    t = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 95]], np.uint8)
    # the template appears twice at the same distance, at shifts (+2, 0) and (-2, 0): the smaller i wins
    dfm = np.zeros((16, 16), np.uint8)
    dfm[5:8, 7:10] = t
    dfm[5:8, 3:6] = t
    und, _, pts = template_case(t, dfm)
    g = np.array([5, 5, 0, 0, 0, 0], np.float32)
    r = ref.ref_search(und, dfm, pts, g, 0, 3)
    assert r["status"] == _ffi.GS_OK and r["score"] == 1.0 and (r["shift_x"], r["shift_y"]) == (-2, 0)
    assert r["runner_up"] == 1.0 and {(-2, 0), (2, 0)} <= r["tie_band"]
    # the same score at (3, 0) and (0, -3), equal i^2 + j^2: the smaller j wins
    dfm = np.zeros((16, 16), np.uint8)
    dfm[2:5, 5:8] = t
    dfm[5:8, 8:11] = t
    r = ref.ref_search(und, dfm, pts, g, 0, 3)
    assert (r["shift_x"], r["shift_y"]) == (0, -3)
    # a nearer copy beats a farther one
    dfm = np.zeros((16, 16), np.uint8)
    dfm[5:8, 6:9] = t
    dfm[8:11, 8:11] = t
    r = ref.ref_search(und, dfm, pts, g, 0, 3)
    assert (r["shift_x"], r["shift_y"]) == (1, 0) and r["runner_up"] == 1.0
    # a lone peak: the runner-up ignores its 8 neighbours
    dfm = np.zeros((16, 16), np.uint8)
    dfm[5:8, 5:8] = t
    r = ref.ref_search(und, dfm, pts, g, 0, 1)
    assert (r["shift_x"], r["shift_y"]) == (0, 0) and r["runner_up"] == -2.0
    # level 1: centre = floor(g / 2 + 0.5), the winner goes back to level-0 pixels
    r = ref.ref_search(und, dfm, pts, np.array([9.0, 11.0, 0, 0, 0, 0], np.float32), 1, 2)
    assert (r["center_x"], r["center_y"]) == (5, 6) and r["g"] == (np.float32(2 * (5 + r["shift_x"])),
                                                                 np.float32(2 * (6 + r["shift_y"])))
    # statuses
    assert ref.ref_search(np.full((16, 16), 9, np.uint8), dfm, pts, g, 0, 2)["status"] == _ffi.GS_TEXTURELESS
    assert ref.ref_search(und, np.full((16, 16), 9, np.uint8), pts, g, 0, 2)["status"] == _ffi.GS_NO_CANDIDATE
    assert ref.ref_search(und, dfm, pts, np.array([40, 0, 0, 0, 0, 0], np.float32), 0, 2)["status"] == _ffi.GS_NO_CANDIDATE
    assert ref.ref_search(und, dfm, pts[:8], g, 0, 2)["status"] == _ffi.GS_TOO_FEW
    assert ref.ref_search(und, dfm, pts, g, 0, 1, min_score=1.0)["status"] == _ffi.GS_WEAK
    # FM_U: one row of candidates, the centre's y is 0
    r = ref.ref_search(und, dfm, pts, np.array([4.0, 77.0, 0, 0, 0, 0], np.float32), 0, 3, has_v=False)
    assert r["center_y"] == 0 and r["shift_y"] == 0 and r["n_valid"] <= 7


def test_override_and_frame0_search_hook_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "guess_override_driver"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(HOST, "guess_override_driver.cpp"), os.path.join(HOST, "lk_engine_mock.cpp"),
                        os.path.join(ROOT, "correlation_amd", "csrc", "lk_tracker.cpp"), "-lpthread", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "guess_override_driver ok" in r.stdout, r.stdout[-1000:] + r.stderr[-6000:]
