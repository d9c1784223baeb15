"""Recovery pass (lk_reseed_failed / lk_reseed_plan, include/lk_engine.h): the planning step against a float64 brute force
over all pairs; propagation from one seeded corner over a grid whose every other sector failed; subset launches against
lone lk_correlate calls, byte for byte; that nothing else moves; arguments."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi, speckle

pytestmark = pytest.mark.gpu

SIDE, GRID, X0, Y0 = 19, 8, 8, 40          # 19 x 19 sectors on an 8 x 8 grid of a 256 x 256 pair
TRANSLATION = (37.3, -21.6)                # 9 px at the coarsest of 3 levels: beyond what a zero guess recovers
PRECISION = 1e-3
MODES = ("default", "batch_invariant", "backward")


def grid_rects(n=GRID, side=SIDE, x0=X0, y0=Y0):
    """sector i * n + j = column i, row j (lk_set_rect_grid's numbering)"""
    return [(x0 + side * i, y0 + side * j, x0 + side * i + side - 1, y0 + side * j + side - 1)
            for i in range(n) for j in range(n)]


def make_engine(und, dfm, rects, model=ca.FM_UVUXUYVXVY, mode="default", annular=()):
    e = ca.HipCorrelationEngine(fitting_model=model, precision=PRECISION, py_stop=2)
    if mode == "batch_invariant":
        e.set_batch_invariant(True)
    elif mode == "backward":
        e.set_update(_ffi.UPDATE_BACKWARD)
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    for s, r in enumerate(rects):
        e.resetPolygon_rect(s, *r)
    for k, q in enumerate(annular):
        e.resetPolygon_annular(len(rects) + k, *q)
    e.commit_sectors()
    return e


def centres(e):
    return np.float32([e.sector_info(s)[1:] for s in range(e.n_sectors)])


def is_good(rec, n_params, chi_max):
    ok = (rec["error_code"] == 0) & np.isfinite(rec["chi"]) & np.isfinite(rec["p"][:, :n_params]).all(axis=1)
    if chi_max > 0:
        with np.errstate(invalid="ignore"):
            ok &= rec["chi"] <= np.float32(chi_max)
    return ok


def state(e):
    """everything the header promises to keep for a sector that was not replaced"""
    return dict(last_eval=e.last_evaluated_parameters().copy(), stats=e.sector_stats().copy(), guesses=e.get_guesses().copy())


@pytest.fixture(scope="module")
def small_pair():
    return speckle.speckle_pair(256, 256, p=(1.3, -0.7, 0.002, 0.0, 0.0, -0.001), seed=5)


@pytest.fixture(scope="module")
def shifted_pair(oracle):
    """the translated pair of the propagation test with what the CPU oracle says about it: chi_max = 4 x its largest chi
    from the true guess, E = its largest error there, and how many sectors it loses from a zero guess"""
    und, dfm = speckle.speckle_pair(256, 256, p=TRANSLATION + (0, 0, 0, 0), seed=11)
    rects = grid_rects()
    xy = [oracle.rect_points(*r) for r in rects]
    cen = np.float32([((r[0] + r[2]) // 2, (r[1] + r[3]) // 2) for r in rects])
    o = oracle.Oracle(model=oracle.FM_UVUXUYVXVY, precision=PRECISION, py_stop=2)
    o.set_image(0, und)
    o.set_image(1, dfm)
    true = np.zeros((len(rects), 6), np.float32)
    true[:, :2] = TRANSLATION
    r = o.correlate_sectors(xy, cen, true)
    assert not r["error_code"].any()
    chi_max = 4.0 * float(r["chi"].max())
    err = float(np.abs(r["p"][:, :2].astype(np.float64) - np.float64(TRANSLATION)).max())
    z = o.correlate_sectors(xy, cen, np.zeros((len(rects), 6), np.float32))
    assert (~is_good(z, 6, chi_max)).sum() >= len(rects) // 2     # a condition on the inputs, checked on the oracle too
    return dict(und=und, dfm=dfm, rects=rects, chi_max=chi_max, E=err)


# ---- 1. the plan against a float64 restatement ----------------------------------------------------------------------
def plan_reference(cen, rec, model, radius, chi_max, min_neighbours):
    P = _ffi.N_PARAMS[model]
    good = is_good(rec, P, chi_max)
    c = cen.astype(np.float64)
    p = rec["p"].astype(np.float64)
    S = len(c)
    status = np.zeros(S, np.int32)
    nbrs = np.zeros(S, np.int32)
    guess = np.zeros((S, 6), np.float32)
    r2 = np.float64(np.float32(radius)) ** 2
    for s in range(S):
        if good[s]:
            status[s] = ca.RESEED_GOOD
            continue
        d = c[s] - c
        near = good & (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= r2)
        nbrs[s] = near.sum()
        if nbrs[s] < min_neighbours:
            status[s] = ca.RESEED_NO_NEIGHBOUR
            continue
        status[s] = ca.RESEED_PLANNED
        q, dx, dy = p[near].copy(), d[near, 0], d[near, 1]
        q[:, P:] = 0
        if model == ca.FM_UVUXUYVXVY:
            q[:, 0] = q[:, 0] + (dx * q[:, 2] + dy * q[:, 3])
            q[:, 1] = q[:, 1] + (dx * q[:, 4] + dy * q[:, 5])
        elif model == ca.FM_UVQ:
            q[:, 0] = q[:, 0] + (-dy * q[:, 2])
            q[:, 1] = q[:, 1] + dx * q[:, 2]
        guess[s] = (q.sum(axis=0) / np.float64(nbrs[s])).astype(np.float32)
    return status, nbrs, guess


def synthetic_records(S, rng, chi_max):
    """random parameters; about a third failed: error codes, non-finite parameters or chi, chi above chi_max"""
    rec = np.zeros(S, ca.RESULT_DTYPE)
    rec["p"] = rng.normal(0, 1, (S, 6)) * np.float32([8, 8, 0.05, 0.05, 0.05, 0.05])
    rec["chi"] = rng.uniform(0.1, 0.9 * chi_max, S)
    rec["n_points"] = 361
    rec["iterations"] = rng.integers(1, 20, S)
    bad = rng.permutation(S)[:max(4, S // 3)]
    for k, s in enumerate(bad):
        kind = k % 5
        if kind == 0:
            rec["error_code"][s] = rng.integers(1, 6)
        elif kind == 1:
            rec["p"][s, 0] = np.nan
        elif kind == 2:
            rec["chi"][s] = np.inf
        elif kind == 3:
            rec["chi"][s] = chi_max * 1.5
        else:
            rec["p"][s, 5] = -np.inf     # (a parameter the smaller models do not have: only the six-parameter model minds)
    return rec


ANNULAR = [(20.0, 12.0, 0.3 + 1.1 * k, 0.9, 120.0, 118.0, 6) for k in range(3)]
LAYOUTS = {
    "grid": (grid_rects(), ()),
    "grid_and_annular": (grid_rects(), ANNULAR),           # centres off the lattice (float means)
    "column": (grid_rects()[:GRID], ()),                   # one column: the cell grid is a single cell wide
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("model", [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY])
def test_plan_matches_float64_restatement(small_pair, model, layout):
    rects, annular = LAYOUTS[layout]
    with make_engine(*small_pair, rects, model=model, annular=annular) as e:
        cen = centres(e)
        S = e.n_sectors
        rng = np.random.default_rng(100 * model + len(layout))
        chi_max = 8.0
        rec = synthetic_records(S, rng, chi_max)
        if layout != "column":   # a 3 x 3 block of failed sectors: its middle has no good neighbour at 1.5 pitches
            for i in (3, 4, 5):
                for j in (3, 4, 5):
                    rec["error_code"][i * GRID + j] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        P = _ffi.N_PARAMS[model]
        n_failed = (~is_good(rec, P, chi_max)).sum()
        assert 0 < n_failed < S
        seen = set()
        # (radius, min_neighbours): 19 = the pitch exactly (the test is <=), 1.5 and 2.9 pitches, a radius past everything
        for radius, min_nb in ((float(SIDE), 1), (1.5 * SIDE, 1), (1.5 * SIDE, 4), (2.9 * SIDE, 9), (1000.0, 1), (0.5, 1)):
            guess, info = e.reseed_plan(rec, radius, chi_max=chi_max, min_neighbours=min_nb)
            status, nbrs, want = plan_reference(cen, rec, model, radius, chi_max, min_nb)
            assert np.array_equal(info["status"], status), (radius, min_nb)
            assert np.array_equal(info["neighbours"], nbrs), (radius, min_nb)
            assert (info["round"] == -1).all() and np.array_equal(info["chi_before"], rec["chi"])
            assert np.isfinite(guess).all()
            ulp = np.spacing(np.abs(want))
            assert (np.abs(guess.astype(np.float64) - want.astype(np.float64)) <= ulp).all(), (radius, min_nb)
            assert not guess[status != ca.RESEED_PLANNED].any()
            seen |= set(status.tolist())
            if radius == float(SIDE):   # neighbours AT the radius count: a failed sector beside a good one has one
                at = [s for s in range(S) if status[s] != ca.RESEED_GOOD and nbrs[s] > 0]
                assert at
        assert seen == {ca.RESEED_GOOD, ca.RESEED_PLANNED, ca.RESEED_NO_NEIGHBOUR}


# ---- 2. propagation from a seed -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_recovery_spreads_from_one_seeded_corner(shifted_pair, mode):
    sp = shifted_pair
    S = len(sp["rects"])
    with make_engine(sp["und"], sp["dfm"], sp["rects"], mode=mode) as e:
        g = np.zeros((S, 6), np.float32)
        g[0, :2] = TRANSLATION
        before = e.correlate_all(g)
        failed = ~is_good(before, 6, sp["chi_max"])
        print(f"{mode}: failed before {failed.sum()} of {S}, chi_max {sp['chi_max']:.3f}, E {sp['E']:.4f}")
        assert not failed[0] and failed.sum() >= S // 2
        rec, n = e.reseed_failed(1.5 * SIDE, chi_max=sp["chi_max"], min_neighbours=1, max_rounds=GRID)
        info = e.reseed_info()
        err = np.abs(rec["p"][:, :2].astype(np.float64) - np.float64(TRANSLATION)).max(axis=1)
        print(f"{mode}: recovered {n}, rounds {info['round'].max() + 1}, largest error {err.max():.4f}, "
              f"largest chi {rec['chi'].max():.3f}")
        assert is_good(rec, 6, sp["chi_max"]).all()
        assert n == failed.sum() == (info["status"] == ca.RESEED_RECOVERED).sum()
        assert (info["status"][~failed] == ca.RESEED_GOOD).all() and (info["round"][~failed] == -1).all()
        assert (err <= sp["E"] + 10 * PRECISION).all()
        # the round grows with the grid distance from the seed (radius 1.5 pitches reaches the eight sectors around one)
        dist = np.array([max(s // GRID, s % GRID) for s in range(S)])
        rounds = info["round"]
        assert (rounds[failed] <= dist[failed] - 1).all()
        for d in range(1, GRID - 1):
            a, b = rounds[failed & (dist == d)], rounds[failed & (dist == d + 1)]
            if len(a) and len(b):
                assert a.max() <= b.min(), (d, a, b)
        e.adjust_initial_guess(1, False, np.zeros(6, np.float32), (0.0, 0.0))   # the last parameters are the records'
        assert e.get_guesses().tobytes() == np.ascontiguousarray(rec["p"]).tobytes()
        st = e.stats()
        assert st["sectors"] >= n and st["evaluations"] > 0


# ---- 3. subset launches solve exactly what a lone solve does -----------------------------------------------------------
def two_size_rects():
    small = [(20 + 11 * i, 20 + 11 * j, 30 + 11 * i, 30 + 11 * j) for i in range(6) for j in range(6)]   # 11 x 11: level 2 has 9 samples
    big = [(100 + 27 * i, 100 + 27 * j, 126 + 27 * i, 126 + 27 * j) for i in range(3) for j in range(3)]  # 27 x 27 = 729
    return small + big


@pytest.mark.parametrize("mode", ("batch_invariant", "backward"))
def test_retried_subset_is_byte_identical_to_lone_solves(small_pair, mode):
    rects = two_size_rects()
    S, n_small = len(rects), 36
    spoiled = [7, 14, 22, 29, n_small + 0, n_small + 4]
    with make_engine(*small_pair, rects, mode=mode) as e, make_engine(*small_pair, rects, mode=mode) as lone:
        clean = e.correlate_all(np.zeros((S, 6), np.float32))
        ok = clean["error_code"] == 0
        chi_max = 4.0 * float(clean["chi"][ok].max())
        g = np.zeros((S, 6), np.float32)
        g[spoiled, 0] = 300.0    # beyond the image: these sectors fail by their error code
        before = e.correlate_all(g)
        failed = ~is_good(before, 6, chi_max)
        assert failed[spoiled].all()
        radius = 30.0
        plan, plan_info = e.reseed_plan(before, radius, chi_max=chi_max, min_neighbours=1)
        rec, n = e.reseed_failed(radius, chi_max=chi_max, min_neighbours=1, max_rounds=1)
        info = e.reseed_info()
        recovered = np.flatnonzero(info["status"] == ca.RESEED_RECOVERED)
        print(f"{mode}: failed {np.flatnonzero(failed).tolist()}, recovered {recovered.tolist()}")
        assert n == len(recovered) and (recovered < n_small).any() and (recovered >= n_small).any()
        for s in recovered:
            assert plan_info["status"][s] == ca.RESEED_PLANNED and info["neighbours"][s] == plan_info["neighbours"][s]
            one, _ = lone.correlate(int(s), plan[s])
            assert one.tobytes() == rec[s].tobytes(), (s, one, rec[s])
        untouched = info["status"] != ca.RESEED_RECOVERED
        assert rec[untouched].tobytes() == before[untouched].tobytes()


# ---- 4. nothing else moves ----------------------------------------------------------------------------------------------
def test_all_good_pair_is_left_alone(small_pair):
    rects = grid_rects()
    S = len(rects)
    with make_engine(*small_pair, rects) as e, make_engine(*small_pair, rects) as twin:
        before = e.correlate_all(np.zeros((S, 6), np.float32))
        assert twin.correlate_all(np.zeros((S, 6), np.float32)).tobytes() == before.tobytes()
        assert is_good(before, 6, 0).all()
        kept = state(e)
        rec, n = e.reseed_failed(1.5 * SIDE)
        assert n == 0 and rec.tobytes() == before.tobytes()
        info = e.reseed_info()                      # valid after the early exit
        assert (info["status"] == ca.RESEED_GOOD).all() and (info["round"] == -1).all() and not info["neighbours"].any()
        assert np.array_equal(info["chi_before"], before["chi"])
        after = state(e)
        for k in kept:
            assert kept[k].tobytes() == after[k].tobytes(), k
        assert e.stats()["sectors"] == 0
        for eng in (e, twin):   # the last parameters: the next frame's guess continues from them
            eng.adjust_initial_guess(1, True, np.zeros(6, np.float32), (0.0, 0.0))
        assert e.get_guesses().tobytes() == twin.get_guesses().tobytes()
        assert e.correlate_all().tobytes() == twin.correlate_all().tobytes()


def test_grey_block_stays_as_it_was(small_pair):
    und, dfm = small_pair[0].copy(), small_pair[1].copy()
    rects = grid_rects()
    S = len(rects)
    dead = [3 * GRID + 3, 3 * GRID + 4, 4 * GRID + 3, 4 * GRID + 4]      # a constant block over four interior sectors
    bx0, by0 = X0 + 3 * SIDE - 6, Y0 + 3 * SIDE - 6
    und[by0:by0 + 2 * SIDE + 12, bx0:bx0 + 2 * SIDE + 12] = 100
    dfm[by0:by0 + 2 * SIDE + 12, bx0:bx0 + 2 * SIDE + 12] = 140
    with make_engine(und, dfm, rects) as e:
        before = e.correlate_all(np.zeros((S, 6), np.float32))
        alive = np.ones(S, bool)
        alive[dead] = False
        live_ok = alive & (before["error_code"] == 0)
        chi_max = 4.0 * float(before["chi"][live_ok].max())
        failed = ~is_good(before, 6, chi_max)
        assert failed[dead].all()
        guesses_before = e.get_guesses().copy()
        e.adjust_initial_guess(1, False, np.zeros(6, np.float32), (0.0, 0.0))     # the last parameters, read back as guesses
        last_before = e.get_guesses().copy()
        assert e.correlate_all(guesses_before).tobytes() == before.tobytes()       # (the engine-held guesses are back)
        kept = state(e)
        rec, n = e.reseed_failed(1.5 * SIDE, chi_max=chi_max, min_neighbours=1, max_rounds=4)
        info = e.reseed_info()
        print(f"grey block: failed {np.flatnonzero(failed).tolist()}, statuses {info['status'][failed].tolist()}, recovered {n}")
        assert np.isin(info["status"][dead], (ca.RESEED_NOT_IMPROVED, ca.RESEED_NO_NEIGHBOUR)).all()
        same = info["status"] != ca.RESEED_RECOVERED
        assert rec[same].tobytes() == before[same].tobytes()
        assert (info["status"][~failed] == ca.RESEED_GOOD).all()
        after = state(e)
        for k in ("last_eval", "stats"):
            assert kept[k][same].tobytes() == after[k][same].tobytes(), k
        assert kept["guesses"].tobytes() == after["guesses"].tobytes()
        e.adjust_initial_guess(1, False, np.zeros(6, np.float32), (0.0, 0.0))
        last_after = e.get_guesses()
        assert last_after[same].tobytes() == last_before[same].tobytes()
        changed = ~same
        assert np.array_equal(last_after[changed], rec["p"][changed])


# ---- 5. arguments ---------------------------------------------------------------------------------------------------------
def test_arguments_and_refusals(small_pair):
    rects = grid_rects(n=3)
    e = ca.HipCorrelationEngine(precision=PRECISION, py_stop=2)
    lib, h = e.lib, e._h
    cfg = _ffi.LkReseedConfig(0.0, 30.0, 1, 4)
    n = C.c_int(-1)

    def refused(c=cfg):
        rc = lib.lk_reseed_failed(h, C.byref(c) if c is not None else None, None, C.byref(n))
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and "lk_reseed_failed" in msg, (rc, msg)
        return msg

    assert "no committed sectors" in refused()
    info = np.zeros(9, _ffi.RESEED_INFO_DTYPE)
    assert lib.lk_get_reseed_info(h, info.ctypes.data_as(C.c_void_p)) == ca.ERROR_BAD_DOMAIN
    e.set_undeformed_image(small_pair[0])
    e.set_deformed_image(small_pair[1])
    for s, r in enumerate(rects):
        e.resetPolygon_rect(s, *r)
    e.commit_sectors()
    assert "no solve" in refused()
    e.correlate_all(np.zeros((9, 6), np.float32))
    assert "configuration" in refused(None)
    for bad in ((0.0, 0.0, 1, 4), (0.0, -1.0, 1, 4), (0.0, float("nan"), 1, 4), (0.0, float("inf"), 1, 4),
                (float("nan"), 30.0, 1, 4), (0.0, 30.0, 0, 4), (0.0, 30.0, 1, 0), (0.0, 30.0, 1, 65)):
        refused(_ffi.LkReseedConfig(*bad))
    e.set_reference_order(1)
    assert "reference-order" in refused()
    rec = np.zeros(9, ca.RESULT_DTYPE)
    with pytest.raises(ca.LkError):
        e.reseed_plan(rec, 30.0)
    e.set_reference_order(0)
    e.correlate_all(np.zeros((9, 6), np.float32))
    assert lib.lk_reseed_failed(h, C.byref(cfg), None, None) == 0          # out == NULL, n_recovered == NULL
    assert lib.lk_reseed_failed(h, C.byref(cfg), None, C.byref(n)) == 0 and n.value == 0
    assert lib.lk_get_reseed_info(h, info.ctypes.data_as(C.c_void_p)) == 0   # after an early exit without a plan
    assert (info["status"] == ca.RESEED_GOOD).all()
    e.close()
