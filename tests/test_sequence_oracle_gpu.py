"""Frame-pipelined windows (lk_correlate_sequence_async / lk_wait_sequence) against the CPU oracle, and the bad-pivot paths
of the default mode on textureless sectors.

test_sequence_window_gpu.py compares a window with the HIP one-pair loop; here every frame of a window is put directly
against the oracle running the reference's frame loop (perform_multiframe_correlation, manager_class.cpp:1380-1496): for
each pair k, frames[k + 1] is the oracle's deformed image, every sector's guess is oracle.adjust_initial_guess
(:2602-2707) of that sector's own earlier results, and the pair is one Oracle.correlate_sectors.  Reference-order windows
must give the oracle's bytes (NaN patterns canonical); default-mode windows must stay within the bounds of the one-pair
default-mode tests for the same geometry.

Textureless sectors: speckle frames with one uniform rectangle and one rectangle of stripes that vary in x only (moving with
the sequence), each covering a few 19 x 19-sample sectors.  Their damped systems are singular (A has zero rows), which
the fast flavour meets as a bad pivot: the one-pair launch parks such a sector and hands it to the SAFE pass; a window
raises its flag and is solved again with the SAFE flavour - on the device, before the window's ring slots are released."""
import os

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd.workload import C2, C4
from test_parity_gpu import OraclePair, compare_results
from test_reference_order_gpu import canonical
from test_sequence_window_gpu import ZERO, domain, make_engine, window

pytestmark = pytest.mark.gpu

NT = min(16, os.cpu_count() or 1)          # host threads of the oracle (not its arithmetic: that is n_threads)
CENTER = (223.5, 223.5)
UNIFORM = (96, 96, 176, 176)               # x0, y0, x1, y1 of the uniform rectangle
STRIPES = (256, 256, 336, 336)             # ... and of the rectangle of x-only stripes


@pytest.fixture(scope="module")
def frames9():
    return ca.speckle.speckle_sequence(448, 448, 9, velocity=(0.8, -0.4), dilation=2e-4, seed=5)


def textureless_sequence(n, size=448, velocity=(0.8, -0.4)):
    frames = ca.speckle.speckle_sequence(size, size, n, velocity=velocity, dilation=2e-4, seed=5)
    out = []
    x = np.arange(STRIPES[0], STRIPES[2], dtype=np.float64)
    for f, img in enumerate(frames):
        img = np.array(img, copy=True)
        x0, y0, x1, y1 = UNIFORM
        img[y0:y1, x0:x1] = 131
        x0, y0, x1, y1 = STRIPES
        row = np.rint(128.0 + 70.0 * np.sin(2 * np.pi * (x - velocity[0] * f) / 9.0)).astype(np.uint8)
        img[y0:y1, x0:x1] = row[None, :]
        out.append(img)
    return out


@pytest.fixture(scope="module")
def flat9():
    return textureless_sequence(9)


def oracle_domain(oracle, kind, size=448):
    """the lists and centres of domain(e, kind, size) for the oracle (None: the oracle forms the centres itself)"""
    lo, hi = 24.0, float(size - 25)
    if kind in ("c2like", "c4like"):
        n = int((hi - lo) // (19.7 if kind == "c2like" else 8.95))
        xd, yd, cen = oracle.rect_sector_geometry(lo, lo, hi, hi, n, n)
        return [oracle.rect_points(cx - xd, cy - yd, cx + xd, cy + yd) for cx, cy in cen], cen.astype(np.float32)
    lists, s = [], 0
    for y in range(40, size - 140, 23):
        for x in range(40, size - 140, 23):
            half = (3, 9, 3, 20, 9, 3, 40)[s % 7] if (x + y) % 5 else 3
            lists.append(oracle.rect_points(x, y, x + 2 * half, y + 2 * half))
            s += 1
    return lists, None


def oracle_frames(oracle, o, model, frames, lists, cen, first, n, velocity=True, reference_previous=False, state=None,
                  center=CENTER):
    """The reference's frame loop on the oracle, pairs first .. first+n-1: (records [n][S], state for the next call).
    With reference_previous the undeformed image of pair k is frames[k] (manager_class.cpp:1386-1407)."""
    S = len(lists)
    res, prev = state if state is not None else (np.zeros((S, 6), np.float32), np.zeros((S, 6), np.float32))
    scx = cen[:, 0] if cen is not None else np.zeros(S, np.float32)
    scy = cen[:, 1] if cen is not None else np.zeros(S, np.float32)
    out = []
    for k in range(first, first + n):
        if reference_previous:
            o.set_image(0, frames[k])
        o.set_image(1, frames[k + 1])
        g = np.zeros((S, 6), np.float32)
        for s in range(S):
            g[s], prev[s] = oracle.adjust_initial_guess(model, k, velocity, ZERO, scx[s], scy[s], center[0], center[1],
                                                        res[s], prev[s])
        r = o.correlate_sectors(lists, centers=cen, guesses=g, nthreads=NT)
        res = r["p"].copy()
        out.append(r)
    return np.stack(out), (res, prev)


def oracle_pair_frames(oracle, model, frames, lists, cen, n, **kw):
    """oracle_frames for the parity target oracle(T=1) and the two yardsticks of compare_results (T=8; exact solve)"""
    outs = []
    for T, solver in ((1, 0), (8, 0), (1, 2)):
        o = oracle.Oracle(model=model, n_threads=T, solver=solver)
        o.set_image(0, frames[0])
        outs.append(oracle_frames(oracle, o, model, frames, lists, cen, 0, n, **kw)[0])
        o.close()
    return outs


def assert_same(got, want, label):
    g, w = canonical(got), canonical(want)
    if g.tobytes() != w.tobytes():
        bad = np.flatnonzero([g[i].tobytes() != w[i].tobytes() for i in range(len(g))])
        raise AssertionError(f"{label}: {len(bad)} of {len(g)} records differ; first: sector {bad[0]}\n got  {got[bad[0]]}\n"
                             f" want {want[bad[0]]}")


def _c4_measures(got, want):
    nan_g, nan_w = np.isnan(got["p"]).any(1), np.isnan(want["p"]).any(1)
    both = ~nan_g & ~nan_w & (got["error_code"] == 0) & (want["error_code"] == 0)
    d = np.abs(got["p"][both][:, :2] - want["p"][both][:, :2]).max(1) if both.any() else np.zeros(1)
    return dict(ec=int((got["error_code"] != want["error_code"]).sum()), nan=int((nan_g != nan_w).sum()),
                it=float((got["iterations"] == want["iterations"]).mean()), p50=float(np.percentile(d, 50)),
                p99=float(np.percentile(d, 99)), both=float(both.mean()))


def c4_bounds(got, want, label, yard=None):
    """the bounds of test_full_size_gpu.py::test_config4_default_mode_against_the_oracle_at_full_size (counts per 50 176
    sectors) for sectors with starved levels.  yard: the same frame of the oracle with 8 thread chunks - the reference
    against itself; past the first pair of a sequence the starved sectors' trajectories diverge in the reference itself
    (0 error codes differ between oracle(T=8) and oracle(T=1) at pair 0, 23 of 1936 at pair 7), and, as in compare_results,
    no cap is then tighter than 3x what that yardstick shows (fractions: its value less the same small-sample slack)"""
    S = len(got)
    assert np.array_equal(got["n_points"], want["n_points"]), label
    m = _c4_measures(got, want)
    y = _c4_measures(yard, want) if yard is not None else dict(ec=0, nan=0, it=1.0, p50=0.0, p99=0.0, both=1.0)
    slack = 0.03 + 1.5 / np.sqrt(S)
    assert m["ec"] <= max(int(np.ceil(40 * S / 50176)), 3 * y["ec"]), (label, m, y)
    assert m["nan"] <= max(int(np.ceil(6 * S / 50176)), 3 * y["nan"]), (label, m, y)
    assert m["it"] >= min(0.92, y["it"] - slack), (label, m, y)
    assert m["p50"] < max(1e-5, 3 * y["p50"]), (label, m, y)
    if yard is None or S >= 1000:   # (on a few dozen sectors the 99th percentile is the maximum, which the C4 test leaves free)
        assert m["p99"] < max(0.06, 3 * y["p99"]), (label, m, y)
    assert m["both"] > min(0.995, y["both"] - slack), (label, m, y)


def engine_window(mode, kind, frames, n, model=ca.FM_UVUXUYVXVY, **kw):
    e = make_engine(mode, model)
    e.set_undeformed_image(frames[0])
    domain(e, kind, 448)
    e.sequence_reserve(n)
    _, rec = window(e, frames, 0, n, center=CENTER, **kw)
    return e, rec


# ---- A. reference-order windows: the oracle's bytes ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c2like", "c4like", "mixed"])
@pytest.mark.parametrize("threads", [1, 20])
def test_reference_order_window_is_the_oracles_frame_loop(oracle, frames9, kind, threads):
    """8-frame windows, every frame byte for byte: one 19 x 19 class, 7 x 7 sectors with two starved levels, every group
    width at once; the reference's summation order for one thread and for its default of 20"""
    n = 8
    e, got = engine_window(f"reference_order:{threads}", kind, frames9, n)
    assert e.sequence_is_pipelined
    e.close()
    lists, cen = oracle_domain(oracle, kind)
    o = oracle.Oracle(model=ca.FM_UVUXUYVXVY, n_threads=threads)
    o.set_image(0, frames9[0])
    want, _ = oracle_frames(oracle, o, ca.FM_UVUXUYVXVY, frames9, lists, cen, 0, n)
    assert (want["error_code"][-1] == 0).mean() > 0.7
    for f in range(n):
        assert_same(got[f], want[f], f"{kind} T={threads} frame {f}")


@pytest.mark.parametrize("model", [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY])
def test_reference_order_window_models_and_chained_windows(oracle, frames9, model):
    """all four warp models on c2like, as 3 + 1 + 3 frames in three windows over reused ring slots: the sequence state a
    window leaves (last and previous parameters) is what the oracle's frame loop carries over"""
    e = make_engine("reference_order:1", model)
    e.set_undeformed_image(frames9[0])
    domain(e, "c2like", 448)
    e.sequence_reserve(4)
    got = np.concatenate([window(e, frames9, first, n, center=CENTER, slot0=slot0)[1]
                          for first, n, slot0 in ((0, 3, 0), (3, 1, 3), (4, 3, 0))])
    e.close()
    lists, cen = oracle_domain(oracle, "c2like")
    o = oracle.Oracle(model=model)
    o.set_image(0, frames9[0])
    want, _ = oracle_frames(oracle, o, model, frames9, lists, cen, 0, 7)
    assert (want["error_code"] == 0).mean() > 0.9
    for f in range(7):
        assert_same(got[f], want[f], f"model {model} frame {f}")


def test_reference_order_window_with_the_previous_image_as_reference(oracle, frames9):
    """reference_previous: the undeformed image of frame i is the deformed image of frame i - 1, the guess p(f - 1)"""
    n = 8
    e, got = engine_window("reference_order:1", "c2like", frames9, n)
    e.adjust_initial_guess(0, False, ZERO, CENTER)
    got = e.correlate_sequence(n, reference_previous=True, constant_velocity=False)
    e.close()
    lists, cen = oracle_domain(oracle, "c2like")
    o = oracle.Oracle(model=ca.FM_UVUXUYVXVY)
    o.set_image(0, frames9[0])
    want, _ = oracle_frames(oracle, o, ca.FM_UVUXUYVXVY, frames9, lists, cen, 0, n, velocity=False, reference_previous=True)
    assert np.abs(np.median(want["p"][:, :, 0], axis=1) - 0.8).max() < 0.1
    for f in range(n):
        assert_same(got[f], want[f], f"reference_previous frame {f}")


def _full_size_window(oracle, w, n):
    frames = ca.speckle.speckle_sequence(w.size, w.size, n + 1, velocity=(0.8, -0.4), dilation=1e-4, seed=7, device="cuda")
    frames = [np.ascontiguousarray(f.cpu().numpy() if hasattr(f, "cpu") else f) for f in frames]
    c = (w.size / 2 - 0.5, w.size / 2 - 0.5)
    e = make_engine("reference_order:1", w.model)
    e.set_undeformed_image(frames[0])
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    e.sequence_reserve(n)
    for i in range(n):
        e.sequence_set_frame(i, frames[i + 1])
    e.adjust_initial_guess(0, True, ZERO, c)
    got = e.correlate_sequence(n)
    assert e.sequence_is_pipelined
    e.close()
    xd, yd, cen = oracle.rect_sector_geometry(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    lists = [oracle.rect_points(cx - xd, cy - yd, cx + xd, cy + yd) for cx, cy in cen]
    o = oracle.Oracle(model=w.model, py_stop=w.py_stop)
    o.set_image(0, frames[0])
    want, _ = oracle_frames(oracle, o, w.model, frames, lists, cen.astype(np.float32), 0, n, center=c)
    o.close()
    return got, want


@pytest.mark.parametrize("wl,n", [(C2, 16), (C4, 4)], ids=["C2x16", "C4x4"])
def test_reference_order_window_at_full_size_is_the_oracles(oracle, wl, n):
    """BASELINE config 2 as a 16-frame window (10 000 sectors of 19 x 19), config 4 as a 4-frame one (50 176 of 7 x 7, two
    starved levels): every record of every frame equals the oracle's frame loop, byte for byte"""
    got, want = _full_size_window(oracle, wl, n)
    assert got.shape == want.shape == (n, wl.hs * wl.vs)
    assert (want["error_code"][-1] == 0).mean() > (0.9 if wl is C2 else 0.7)
    for f in range(n):
        assert_same(got[f], want[f], f"{wl.hs} x {wl.vs} sectors, frame {f}")


# ---- A. default-mode windows: the one-pair default-mode bounds --------------------------------------------------------
@pytest.mark.parametrize("kind", ["c2like", "c4like", "mixed"])
def test_default_mode_window_stays_within_the_one_pair_bounds(oracle, frames9, kind):
    """the fast flavour and fixed lane groups inside the window, every frame against the oracle's frame loop: 19 x 19 and the
    mixed domain with compare_results (test_parity_gpu.py), 7 x 7 sectors with the bounds of the config-4 one-pair test"""
    n = 8
    e, got = engine_window("default", kind, frames9, n)
    assert e.sequence_is_pipelined and e.stats()["window_safe_reruns"] == 0
    e.close()
    lists, cen = oracle_domain(oracle, kind)
    want = oracle_pair_frames(oracle, ca.FM_UVUXUYVXVY, frames9, lists, cen, n)
    starved = np.array([len(x) <= 81 for x in lists])     # 9 x 9 / 7 x 7 samples: starved top levels
    for f in range(n):
        # (pair 0 starts every sector from the same guess as a one-pair launch: the one-pair bounds, unrelaxed)
        if starved.any():
            c4_bounds(got[f][starved], want[0][f][starved], f"{kind} starved sectors, frame {f}",
                      yard=want[1][f][starved] if f > 0 else None)
        if (~starved).any():
            compare_results(got[f][~starved], tuple(w[f][~starved] for w in want), f"{kind} frame {f}")


# ---- A. the separable bicubic window against the float64 yardstick ------------------------------------------------------
def test_separable_bicubic_window_against_the_oracle(oracle, frames9):
    """IM_BICUBIC_SEPARABLE in a window (batch-invariant: its frame-pipelined instance): every frame within the bars of
    test_separable_bicubic_extension against the oracle's bicubic frame loop (the separable form is closer to the exact
    Catmull-Rom spline than the reference's monomial evaluation, so not inside the reference's own rounding)"""
    n = 6
    e = ca.HipCorrelationEngine(interpolation=ca.IM_BICUBIC_SEPARABLE)
    e.set_batch_invariant(True)
    e.set_undeformed_image(frames9[0])
    domain(e, "c2like", 448)
    e.sequence_reserve(n)
    _, got = window(e, frames9, 0, n, center=CENTER)
    assert e.sequence_is_pipelined
    e.close()
    lists, cen = oracle_domain(oracle, "c2like")
    o = oracle.Oracle(interp=ca.IM_BICUBIC, model=ca.FM_UVUXUYVXVY)
    o.set_image(0, frames9[0])
    want, _ = oracle_frames(oracle, o, ca.FM_UVUXUYVXVY, frames9, lists, cen, 0, n)
    for f in range(n):
        g, w = got[f], want[f]
        assert np.array_equal(g["error_code"], w["error_code"]), f
        ok = w["error_code"] == 0
        assert (np.abs(g["iterations"] - w["iterations"])[ok] <= 1).mean() >= 0.95, f
        assert np.abs(g["p"] - w["p"])[ok][:, :2].max() < 5e-3, f
        assert np.abs(g["p"] - w["p"])[ok][:, 2:].max() < 1e-4, f
        assert (np.abs(g["chi"] - w["chi"]) / w["chi"])[ok].max() < 5e-3, f


# ---- B. textureless sectors: the bad-pivot paths ---------------------------------------------------------------------
def _flat_sectors(oracle):
    """c2like sectors that lie wholly inside the uniform or the striped rectangle at frame 0, and those that touch one of
    them (within the 8 frames' motion): (lists, centres, flat, touching)"""
    lists, cen = oracle_domain(oracle, "c2like")
    inside, near = np.zeros(len(lists), bool), np.zeros(len(lists), bool)
    for x0, y0, x1, y1 in (UNIFORM, STRIPES):
        inside |= np.array([(l[:, 0].min() >= x0 + 6) & (l[:, 0].max() < x1 - 6) & (l[:, 1].min() >= y0 + 6)
                            & (l[:, 1].max() < y1 - 6) for l in lists])
        near |= np.array([(l[:, 0].max() >= x0 - 12) & (l[:, 0].min() < x1 + 12) & (l[:, 1].max() >= y0 - 12)
                          & (l[:, 1].min() < y1 + 12) for l in lists])
    return lists, cen, inside, near & ~inside


def assert_textureless(got, want, flat, touching, label, first_pair=True):
    """got / want (oracle T=1, T=8, exact solve) of one pair.  Uniform sectors: no gradient at all - NaN parameters and
    an out-of-image error, as in the oracle.  Striped sectors: A has exactly zero rows (v, vx, vy), so the damped system
    is rank-deficient and the undetermined part of the step is whatever the solver's rank decision and rounding make of
    it - the exact-solver yardstick disagrees with the reference on the error code or NaN flag of every such sector.  There
    the engine must disagree no more often than that yardstick, and agree on the determined parameters (u, ux, uy) within
    compare_results' caps where both converge at the first pair.  Sectors wholly in speckle: compare_results.  (Sectors that
    straddle a rectangle's edge are near-singular in one direction: no bound is claimed for them.)"""
    uniform = flat & np.isnan(want[0]["p"]).all(1)
    striped = flat & ~uniform
    assert uniform.sum() >= 6 and striped.sum() >= 6, label
    g, w = got[uniform], want[0][uniform]
    assert np.isnan(g["p"]).all() and np.array_equal(g["chi"], w["chi"]) and np.array_equal(g["error_code"], w["error_code"]), label
    if first_pair:   # (later pairs start from NaN guesses: the default mode reports 0 iterations there, not the stale count)
        assert_same(g, w, label + ", uniform sectors")
    mism = lambda r: int(((r["error_code"] != want[0]["error_code"]) | (np.isnan(r["p"]).any(1) != np.isnan(want[0]["p"]).any(1)))[striped].sum())
    assert mism(got) <= max(mism(want[1]), mism(want[2])), (label, mism(got), mism(want[1]), mism(want[2]))
    if first_pair:
        ok = striped & (got["error_code"] == 0) & (want[0]["error_code"] == 0)
        assert ok.sum() >= 4, label
        dp = np.abs(got["p"] - want[0]["p"])[ok]
        assert dp[:, 0].max() <= 5e-3 and dp[:, 2:4].max() <= 5e-5, (label, dp)
    textured = ~flat & ~touching
    compare_results(got[textured], tuple(w[textured] for w in want), label + ", textured sectors")


def test_one_pair_default_mode_parks_textureless_sectors_for_the_safe_pass(oracle, flat9):
    """One pair, default mode: the bad pivots happen (ill_conditioned_solves > 0) on a non-starved class, and every
    textureless sector is handed to the SAFE pass; against the oracle see assert_textureless.  The SAFE pass's records are
    NOT the reference-order records (its sums are the lane-parallel ones): on the rank-deficient sectors the step's
    undetermined part, and with it the error code, may differ; the reference-order records are the oracle's, bytes and all."""
    und, dfm = flat9[0], flat9[1]
    lists, cen, flat, touching = _flat_sectors(oracle)
    assert flat.sum() >= 6
    e = make_engine("default")
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    domain(e, "c2like", 448)
    got = e.correlate_all(ZERO)
    st, per = e.stats(), e.sector_stats()
    parked = per[:, 3] > 0
    assert st["ill_conditioned_solves"] > 0 and parked[flat].all() and not parked[~flat].any(), (st, np.flatnonzero(parked))
    e.set_reference_order(1)
    exact = e.correlate_all(ZERO)
    e.close()
    os_ = OraclePair(*[oracle.Oracle(n_threads=T, solver=s) for T, s in ((1, 0), (8, 0), (1, 2))])
    os_.set_image(0, und)
    os_.set_image(1, dfm)
    want = os_.correlate_sectors(lists, centers=cen)
    assert_textureless(got, want, flat, touching, "textureless pair")
    assert_same(exact, want[0], "reference-order records of the textureless pair")


def test_one_pair_reference_order_on_textureless_sectors_is_the_oracles(oracle, flat9):
    lists, cen, _, _ = _flat_sectors(oracle)
    for threads in (1, 20):
        e = make_engine(f"reference_order:{threads}")
        e.set_undeformed_image(flat9[0])
        e.set_deformed_image(flat9[2])
        domain(e, "c2like", 448)
        got = e.correlate_all(ZERO)
        e.close()
        o = oracle.Oracle(n_threads=threads)
        o.set_image(0, flat9[0])
        o.set_image(1, flat9[2])
        assert_same(got, o.correlate_sectors(lists, centers=cen, nthreads=NT), f"textureless pair T={threads}")


def _force_safe_window(monkeypatch, frames, n):
    monkeypatch.setenv("LK_FORCE_SAFE", "1")          # read at commit
    e, rec = engine_window("default", "c2like", frames, n)
    monkeypatch.delenv("LK_FORCE_SAFE")
    assert e.stats()["window_safe_reruns"] == 0
    e.close()
    return rec


def test_default_mode_window_on_textureless_sectors_is_solved_again_safe(oracle, flat9, monkeypatch):
    """the window's fast flavour meets the bad pivots and the window is solved again with the SAFE flavour: its records are
    those of an engine committed with LK_FORCE_SAFE=1, byte for byte, and within the default-mode bounds of the oracle"""
    n = 8
    want_safe = _force_safe_window(monkeypatch, flat9, n)
    e, got = engine_window("default", "c2like", flat9, n)
    assert e.stats()["window_safe_reruns"] == 1
    e.close()
    assert got.tobytes() == want_safe.tobytes()
    lists, cen, flat, touching = _flat_sectors(oracle)
    want = oracle_pair_frames(oracle, ca.FM_UVUXUYVXVY, flat9, lists, cen, n)
    for f in range(n):
        assert_textureless(got[f], tuple(w[f] for w in want), flat, touching, f"textureless window, frame {f}",
                           first_pair=f == 0)


def test_a_frame_upload_waits_for_the_safe_rerun_of_the_window(flat9, monkeypatch):
    """A default-mode window over slots 0..n-1 that will be solved again: launched, then slot 0 overwritten from pageable
    memory (the call returns once the copy has landed), then waited for.  A slot that a window still reads is overwritten
    only after that window (lk_engine.h) - SAFE pass included: the records are those of the untouched LK_FORCE_SAFE window."""
    n = 6
    want = _force_safe_window(monkeypatch, flat9, n)
    e = make_engine("default")
    e.set_undeformed_image(flat9[0])
    domain(e, "c2like", 448)
    e.sequence_reserve(n)
    for i in range(n):
        e.sequence_set_frame(i, flat9[i + 1])
    e.adjust_initial_guess(0, True, ZERO, CENTER)
    e.correlate_sequence_async(n)
    e.sequence_set_frame(0, np.ascontiguousarray(flat9[8][::-1]))
    got = e.wait_sequence()
    assert e.stats()["window_safe_reruns"] == 1
    e.close()
    assert got.tobytes() == want.tobytes()


def test_previous_image_frame_loop_keeps_the_undeformed_slot_through_the_rerun(monkeypatch):
    """lk_sequence_run with the previous image as reference, windows of 4: the frames of the next window are uploaded behind
    the running one, the last of them into the current window's undeformed slot.  With textureless sectors every window is
    solved again with the SAFE flavour, and the report must be the text of the same loop on an engine committed with
    LK_FORCE_SAFE=1 (whose windows are never solved again; the one-pair loop of LK_SEQ_SYNC=1 is not byte-comparable in the
    default mode: its lane groups widen by batch composition)"""
    from correlation_amd import tracker as tk
    frames = textureless_sequence(13)        # 12 pairs: three windows, the last two with an undeformed ring slot
    names = [f"f{i}" for i in range(len(frames))]
    monkeypatch.setenv("LK_SEQ_WINDOW", "4")

    def run(force_safe):
        monkeypatch.setenv("LK_FORCE_SAFE", "1" if force_safe else "0")
        e = ca.HipCorrelationEngine(fitting_model=ca.FM_UVUXUYVXVY)
        t = tk.SequenceTracker(ca.FM_UVUXUYVXVY, tk.DOMAIN_RECT, tk.DEF_EULERIAN, tk.REF_PREVIOUS, tk.ERRMODE_CONTINUE, lib=e.lib)
        lo, hi = 24.0, 423.0
        n = int((hi - lo) // 19.7)
        t.set_rect_domain(lo, lo, hi, hi, CENTER[0], CENTER[1], n, n)
        assert tk.run_sequence(e, t, frames, names) == len(frames) - 1
        text, reruns = t.report(), e.stats()["window_safe_reruns"]
        e.close(), t.close()
        return text, reruns

    want, reruns_safe = run(True)
    got, reruns = run(False)
    assert reruns_safe == 0 and reruns == 3
    assert got == want
