"""The lane groups walk an implicit rectangle incrementally (csrc/lk_rect_walk.hpp): (row, col) of a lane's first sample by
one division per evaluation, then a constant step with one carry per trip of the sample loop.  The yardstick is the same
sectors given as explicit row-major point lists (set_sector_points with the grid's own centres): that path reads its
coordinates from memory and never touches the walk, and a lane meets the same samples in the same order, so every byte of
every record and of sector_stats() and all 28 sums of evaluate(sector, level, p) at every level have to be equal.  (Checked once with the
library of the commit before the walk, 53d4141, through LK_ENGINE_LIB: the two domains agree byte for byte there too, in
every case and group - profiles/ab_rect_walk.txt.)

192 x 192 speckle pair, a small affine truth, pyramid 0 / 1 / 2, the reference bicubic.  Cases:
  odd     five 19 x 19 sectors in one grid: the odd count leaves the last wavefront of 32-lane groups one idle half, so that
          sector runs 64 lanes wide from its first evaluation
  leaves  two sectors, the first of which leaves the deformed image in its first evaluation (level 2: its last column, x = 184,
          is column 46 of 48, on the bicubic's limit): its wave-mate switches to 64 lanes in mid-solve
  w19     width 19 (19 / 10 / 5 samples wide at the three levels), w33 (wider than a 32-lane group), w16 (the stride of every
          group is a multiple of the width)
each with the lane group the classifier picks and with LK_FORCE_GROUP 16, 32 and 64 (read at commit, one child process each).
No level of any sector is starved (at most 12 samples: those are summed in the reference's order, x outer, which a row-major
list does not have)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import correlation_amd as ca

pytestmark = pytest.mark.gpu

CASES = ("odd", "leaves", "w19", "w33", "w16")

CHILD = r"""
import sys
import numpy as np
import correlation_amd as ca

und, dfm = ca.speckle.speckle_pair(192, 192, p=(0.6, -0.4, 0.001, 0.0, 0.0, -0.0005), seed=7)
P_EVAL = np.float32([0.3, -0.2, 0.001, 0.0005, -0.0004, 0.0008])


def square(x0, y0, w):
    return (x0, y0, x0 + w - 1, y0 + w - 1)


cases = {
    "odd": [square(24 + 19 * i, 24, 19) for i in range(5)],
    "leaves": [square(168, 24, 19), square(24, 24, 19)],
    "w19": [square(24 + 19 * i, 60 + 19 * j, 19) for j in range(2) for i in range(3)],
    "w33": [square(24 + 33 * i, 24 + 33 * j, 33) for j in range(2) for i in range(2)],
    "w16": [square(24 + 16 * i, 100 + 16 * j, 16) for j in range(2) for i in range(2)],
}
out = {}
for name, rects in cases.items():
    centres = None
    for domain in ("rect", "list"):
        e = ca.HipCorrelationEngine(fitting_model=ca.FM_UVUXUYVXVY, interpolation=ca.IM_BICUBIC, py_start=0, py_step=1, py_stop=2)
        e.set_undeformed_image(und)
        e.set_deformed_image(dfm)
        for s, (x0, y0, x1, y1) in enumerate(rects):
            if domain == "rect":
                e.resetPolygon_rect(s, x0, y0, x1, y1)
            else:   # the same samples row by row, the order in which the lane groups walk the rectangle
                ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
                e.set_sector_points(s, np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32), center=centres[s])
        e.commit_sectors()
        S = len(rects)
        if domain == "rect":
            centres = [e.sector_info(s)[1:] for s in range(S)]
        key = name + "_" + domain + "_"
        out[key + "centres"] = np.float32([e.sector_info(s)[1:] for s in range(S)])
        out[key + "counts"] = np.int32([[e.sector_level_count(s, l) for l in range(3)] for s in range(S)])
        out[key + "listed"] = np.int32([[len(e.level_xy(l, s)) for l in range(3)] for s in range(S)])
        out[key + "records"] = e.correlate_all(np.zeros(6, np.float32))
        out[key + "stats"] = e.sector_stats()
        out[key + "groups"] = e.sector_groups()[0]
        sums = np.zeros((S, 3, 44), np.float32)
        for s in range(S):
            for l in range(3):
                A, b, chi, err = e.evaluate(s, l, P_EVAL)
                sums[s, l] = np.concatenate([A.ravel(), b, [chi, err]])
        out[key + "sums"] = sums
        e.close()
np.savez(sys.argv[1], **out)
"""


_solved = {}


def run_child(group, tmp_path_factory):
    """every case in both domains, solved and evaluated by one child process with the given LK_FORCE_GROUP (once per group)"""
    if group not in _solved:
        env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        env.pop("LK_FORCE_GROUP", None)
        if group != "classifier":
            env["LK_FORCE_GROUP"] = group
        out = tmp_path_factory.mktemp("rect_walk") / "solved.npz"
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", CHILD, str(out)]
        done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stdout + done.stderr
        _solved[group] = dict(np.load(out))
    return _solved[group]


@pytest.fixture(scope="module", params=["classifier", "16", "32", "64"])
def solved(request, tmp_path_factory):
    return run_child(request.param, tmp_path_factory)


def test_the_forced_groups_are_three_different_groups(tmp_path_factory):
    """The three children report 16, 32 and 64 lanes for every sector (sector_groups()).  And what shows it in the results: a
    group of another width adds the same products in another order, so the sums and chi of 19 x 19 samples round
    differently.  Were LK_FORCE_GROUP ignored, the three runs would be the classifier's group three times, bit for bit."""
    runs = {g: run_child(g, tmp_path_factory) for g in ("16", "32", "64")}
    for g, d in runs.items():   # the engine's own word (lk_get_sector_groups): every sector of every case in the forced group
        for c in CASES:
            for domain in ("rect", "list"):
                assert (d[f"{c}_{domain}_groups"] == int(g)).all(), (g, c, domain, d[f"{c}_{domain}_groups"])
    bits = {g: b"".join(d[c + "_rect_" + k].tobytes() for c in CASES for k in ("sums", "records")) for g, d in runs.items()}
    assert bits["16"] != bits["32"] and bits["32"] != bits["64"] and bits["16"] != bits["64"]
    for c in CASES:   # and per case at level 0, where a lane of every group has several samples
        lvl0 = {g: d[c + "_rect_sums"][:, 0, :42].tobytes() for g, d in runs.items()}
        assert len(set(lvl0.values())) == 3, c


@pytest.mark.parametrize("case", CASES)
def test_rectangles_against_the_same_samples_as_lists(solved, case):
    r = {k: solved[case + "_rect_" + k] for k in ("centres", "counts", "listed", "records", "stats", "sums")}
    l = {k: solved[case + "_list_" + k] for k in r}
    # the one domain is implicit (no list entry at any level), the other a list of the same samples with the same centres
    assert (r["listed"] == 0).all() and (r["counts"] > 12).all(), (r["listed"], r["counts"])
    assert np.array_equal(l["listed"], r["counts"]) and np.array_equal(l["counts"], r["counts"]), (l["listed"], r["counts"])
    assert r["centres"].tobytes() == l["centres"].tobytes()
    S = len(r["records"])
    a, b = r["records"].view(np.uint8).reshape(S, -1), l["records"].view(np.uint8).reshape(S, -1)
    diff = np.flatnonzero((a != b).any(axis=1))
    assert diff.size == 0, f"{diff.size} records differ, first {diff[:8]}: {r['records'][diff[0]]} vs {l['records'][diff[0]]}"
    assert np.array_equal(r["stats"], l["stats"]), (r["stats"], l["stats"])
    same = r["sums"].view(np.uint32) == l["sums"].view(np.uint32)
    assert same.all(), f"sums differ at (sector, level, sum) {np.argwhere(~same)[:8]}"
    # the cases are what they claim to be
    rec, st = r["records"], r["stats"]
    if case == "leaves":
        assert rec["error_code"][0] == ca.ERROR_INTERPOLATION_OUT_OF_IMAGE and st[0, 0] == 1 and rec["iterations"][0] == 0
        assert rec["error_code"][1] == 0 and st[1, 0] > 1
        assert r["sums"][0, 2, 43] != 0 and r["sums"][1, 2, 43] == 0      # evaluate(): the error flag at level 2
    else:
        assert (rec["error_code"] == 0).all() and (st[:, 0] >= 6).all()   # three levels, two evaluations each at the least
        assert (np.abs(rec["p"][:, 0] - 0.6) < 0.3).all() and (np.abs(rec["p"][:, 1] + 0.4) < 0.3).all()
        assert (r["sums"][:, :, 43] == 0).all() and (r["sums"][:, :, 42] > 0).all()
    widths = {"odd": 19, "leaves": 19, "w19": 19, "w33": 33, "w16": 16}
    assert (r["counts"][:, 0] == widths[case] ** 2).all()
