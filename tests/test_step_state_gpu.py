"""The fast 32-lane solve instance of the six-parameter models keeps the words of a sector's state that every LM step
uses (damping, last good chi, trip count, counters) in registers and touches the slot in LDS only for what a rejection, a
level change, an error, a parked sector or the final record needs.  The earlier form of the step - the whole slot loaded
after every evaluation and stored at the end of the step - stays in the same kernel behind LK_STEP_STATE=0 (read per
solve).  Here both forms solve the same inputs and every byte of every record and of sector_stats must agree, on the
common path and on every rare way out of a step.  Each case also asserts that its sectors really took that way out."""
import os

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd.workload import C2

pytestmark = pytest.mark.gpu

ERR_NONE = 0
SIZE = 512
PITCH = 19   # C2's sectors: 19 x 19 samples, 25 at level 2


def make_engine(monkeypatch, und, dfm, rects, batch_invariant=False, **cfg):
    monkeypatch.setenv("LK_FORCE_GROUP", "32")   # (a few hundred sectors would otherwise be promoted to 64-lane groups)
    e = ca.HipCorrelationEngine(fitting_model=C2.model, **{"py_stop": C2.py_stop, **cfg})
    e.set_batch_invariant(batch_invariant)       # batch-invariant: two sectors per wavefront to the end, no solo
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    for s, (x0, y0) in enumerate(rects):
        e.resetPolygon_rect(s, x0, y0, x0 + PITCH - 1, y0 + PITCH - 1)
    e.commit_sectors()
    return e


def both_forms(monkeypatch, e, guess):
    """(records, sector_stats) of the register form; asserts the slot form gives the same bytes."""
    monkeypatch.delenv("LK_STEP_STATE", raising=False)
    r_new = e.correlate_all(guess)
    s_new = e.sector_stats()
    monkeypatch.setenv("LK_STEP_STATE", "0")
    r_old = e.correlate_all(guess)
    s_old = e.sector_stats()
    monkeypatch.delenv("LK_STEP_STATE")
    assert r_new.dtype.itemsize == 48
    a, b = r_new.view(np.uint8).reshape(len(r_new), 48), r_old.view(np.uint8).reshape(len(r_old), 48)
    diff = np.flatnonzero((a != b).any(axis=1))
    assert diff.size == 0, f"{diff.size} records differ, first {diff[:8]}: {r_new[diff[0]]} vs {r_old[diff[0]]}"
    assert np.array_equal(s_new, s_old), f"sector_stats differ in {np.flatnonzero((s_new != s_old).any(axis=1))[:8]}"
    return r_new, s_new


def grid(nx, ny, x0=24, y0=24):
    return [(x0 + PITCH * i, y0 + PITCH * j) for j in range(ny) for i in range(nx)]


@pytest.fixture(scope="module")
def pair():
    return ca.speckle.speckle_pair(SIZE, SIZE, p=C2.truth, seed=7)


@pytest.mark.parametrize("batch_invariant", [True, False], ids=["two-sectors", "solo"])
def test_common_path(monkeypatch, pair, batch_invariant):
    """A C2-like grid: 24 x 24 sectors, three levels, zero guess.  (solo: that a half-wavefront adopted its partner's sector -
    the copy of the register words in the adoption - has no observable in the records; it is assumed from the sectors'
    differing evaluation counts, asserted below, and from solo being on by default, not asserted itself.)"""
    e = make_engine(monkeypatch, *pair, grid(24, 24), batch_invariant=batch_invariant)
    r, st = both_forms(monkeypatch, e, np.zeros(6, np.float32))
    assert (r["error_code"] == ERR_NONE).all() and (st[:, 3] == 0).all()
    assert (r["iterations"] >= 1).all() and (st[:, 0] >= 6).all()          # three levels, two evaluations each at the least
    assert abs(np.median(r["p"][:, 0]) - C2.truth[0]) < 0.1   # (the truth is affine about the image centre, the grid is centred)
    pairs = st[:, 0].reshape(-1, 2)                            # positional launch: sectors 2 k and 2 k + 1 share a wavefront
    assert (pairs[:, 0] != pairs[:, 1]).any(), "no wavefront whose halves finish at different steps"
    e.close()


def test_odd_sector_count(monkeypatch, pair):
    """The last wavefront has one idle group from the start (by the positional launch's arithmetic: 401 sectors, two per
    wavefront; the records have no observable for it)."""
    e = make_engine(monkeypatch, *pair, grid(24, 24)[:401])
    r, _ = both_forms(monkeypatch, e, np.zeros(6, np.float32))
    assert len(r) == 401 and (r["error_code"] == ERR_NONE).all()
    e.close()


def test_out_of_image_at_evaluation_0_and_later(monkeypatch, pair):
    """One pyramid level (with three, a sector near the border fails the first evaluation of the coarsest level before anything
    else can happen).  The deformed image is the undeformed one moved two pixels to the right, and the sectors' last column
    (x = cols - 4) sits two pixels inside the bicubic's valid region (x < cols - 2): the answer u = 2 lies exactly on the limit.
    Guesses of 0.5 to 1.3 px start inside and the LM steps towards the answer carry the sector out in a tentative evaluation;
    guesses of 2.0 to 2.5 px fail the first evaluation."""
    und = pair[0]
    dfm = und.copy()
    dfm[:, 2:] = und[:, :-2]
    rects, guesses = [], []
    for k in range(41):
        for j in range(3):
            rects += [(SIZE - 3 - PITCH, 100 + 100 * j)] * 2
            guesses += [[0.5 + 0.02 * k, 0, 0, 0, 0, 0], [2.0 + 0.0125 * k, 0, 0, 0, 0, 0]]
    e = make_engine(monkeypatch, und, dfm, rects, py_stop=0)
    r, st = both_forms(monkeypatch, e, np.array(guesses, np.float32))
    out = r["error_code"] == ca.ERROR_INTERPOLATION_OUT_OF_IMAGE
    later, first = np.arange(len(r)) % 2 == 0, np.arange(len(r)) % 2 == 1
    print("out of image:", out.sum(), "of", len(r), "- at the first evaluation", (out & (st[:, 0] == 1)).sum(), ", later", (out & (st[:, 0] > 1)).sum())
    assert out[first].all() and (st[first, 0] == 1).all() and (r["iterations"][first] == 0).all()
    assert out[later].all() and (st[later, 0] > 1).all() and (r["iterations"][later] >= 1).all()
    e.close()


def test_max_iters(monkeypatch, pair):
    e = make_engine(monkeypatch, *pair, grid(16, 16), max_iters=2)
    r, _ = both_forms(monkeypatch, e, np.zeros(6, np.float32))
    hit = r["error_code"] == ca.ERROR_CORRELATION_MAX_ITERS_REACHED
    assert hit.any() and (r["iterations"][hit] == 2).all()
    e.close()


CAP_CHILD = r"""
import os, sys
import numpy as np
import correlation_amd as ca
from correlation_amd.workload import C2
PITCH = 19
und, dfm = ca.speckle.speckle_pair(512, 512, p=C2.truth, seed=7)
e = ca.HipCorrelationEngine(fitting_model=C2.model, py_start=2, py_stop=2, max_iters=50)
e.set_undeformed_image(und)
e.set_deformed_image(dfm)
for s in range(64):
    x0, y0 = 24 + PITCH * (s % 8), 24 + PITCH * (s // 8)
    if s % 3 == 1:
        px, py = x0 // 4 * 4 + 5, y0 // 4 * 4 + 5   # one pixel at 1 mod 4 in both directions: no sample at level 2
        e.resetPolygon_rect(s, px, py, px, py)
    else:
        e.resetPolygon_rect(s, x0, y0, x0 + PITCH - 1, y0 + PITCH - 1)
e.commit_sectors()
out = {}
for form in ("reg", "slot"):
    if form == "slot":
        os.environ["LK_STEP_STATE"] = "0"
    out["r_" + form] = e.correlate_all(np.zeros(6, np.float32))
    out["s_" + form] = e.sector_stats()
np.savez(sys.argv[1], **out)
"""


def test_lambda_at_its_cap(tmp_path):
    """A Gauss-Newton step is a descent direction, so on textured sectors a tentative step is rejected only at the rounding floor
    of chi and the damping never climbs thirteen decades (precision = 0, 3000 trips: every sector of a 16 x 16 grid ran all of
    them).  What is never accepted is a chi that is not a number: a sector without a sample at the level (one pixel at 1 mod 4
    has none at level 2) has the scaling 1 / 0 and chi = 0 * inf, and `chi <= lg_chi` is false.  Such a level is starved, and
    the engine would give it to the one-lane kernel (which keeps the sums of a rejected trip and never re-evaluates) and a bad
    pivot of its system to the SAFE kernel: LK_STARVED_MAX=none and LK_ILL_PASS=0 keep both off, so that the fast 32-lane
    instance itself walks the thirteen rejections.  LK_ILL_PASS is read once per process, hence the child process.  Only
    level 2 is solved, so the level's verdict is the record's: max_iters is reported only for a trip count above max_iters or a
    damping at its cap, and with 14 trips of 50 allowed it is the cap (1e-4 * 10^13).  The lane-group kernel's signature: every
    rejection costs a re-evaluation at the last good parameters (PH_REEVAL, p read back from the slot), 1 + 1 + 2 * 13 = 28
    evaluations at the least, which the one-lane kernel and the finisher (kept sums: 15) never spend.  Ordinary sectors share the wavefronts."""
    import subprocess
    import sys
    env = dict(os.environ, LK_FORCE_GROUP="32", LK_STARVED_MAX="none", LK_ILL_PASS="0", PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    env.pop("LK_STEP_STATE", None)
    out = tmp_path / "cap.npz"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", CAP_CHILD, str(out)]
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    z = np.load(out)
    r, st = z["r_reg"], z["s_reg"]
    assert r.tobytes() == z["r_slot"].tobytes() and np.array_equal(st, z["s_slot"]), "the two forms of the step differ"
    empty = np.arange(64) % 3 == 1
    print("empty-level sectors: errors", np.unique(r["error_code"][empty]), "iterations", np.unique(r["iterations"][empty]), "evaluations", np.unique(st[empty, 0]),
          "sample evaluations", np.unique(st[empty, 1]), "ill", np.unique(st[empty, 3]))
    assert (st[empty, 1] == 0).all(), "these sectors were meant to have no sample at level 2"
    assert (r["error_code"][empty] == ca.ERROR_CORRELATION_MAX_ITERS_REACHED).all()
    assert (r["iterations"][empty] < 50).all() and (r["iterations"][empty] >= 13).all()
    assert (st[empty, 0] >= 28).all(), "no re-evaluation per rejection: this was not the lane-group kernel"
    assert (st[empty, 3] >= 1).all(), "a system of NaNs passed the pivot test"   # (counted in the slot: no SAFE pass to park for)
    assert (r["error_code"][~empty] == ERR_NONE).all()


def test_textureless_sectors_are_parked(monkeypatch, pair):
    """A flat patch in both images: no gradient, every pivot bad - the fast kernel parks those sectors for the SAFE one."""
    und, dfm = pair[0].copy(), pair[1].copy()
    und[:160, :160] = 128
    dfm[:160, :160] = 128
    e = make_engine(monkeypatch, und, dfm, grid(20, 20))
    r, st = both_forms(monkeypatch, e, np.zeros(6, np.float32))
    flat = np.array([x0 + PITCH < 150 and y0 + PITCH < 150 for x0, y0 in grid(20, 20)])
    assert flat.sum() >= 16 and (st[flat, 3] >= 1).all(), "the flat sectors met no bad pivot"
    assert (st[~flat, 3] == 0).sum() > 300
    e.close()
