"""Lens distortion (lk_lens_fit, lk_lens_correct, include/lk_engine.h) on the GPU: the sums and the fitted lens against the
float64 restatement of tests/lens_ref.py; the true lens recovered from exact, noisy and rotated data; the strain a lens
fakes, before and after the correction; bytes (the host functions, a frame alone, the three sources, repeats, shuffles,
chunks); end to end on rendered frames; that nothing of the engine moves; refusals.

Domain: 12 x 12 sectors of 19 x 19 on 256 x 256 images, as tests/test_strain_gpu.py.  Synthetic data (tests/lens_ref.py): true
lens c = (126, 117), rn = 147.785, k1 = -0.03, k2 = 0.008; five frames t = (+-12, 0), (0, +-9), (8, -6).

Tolerances of the comparisons with the restatement are derived in tests/lens_ref.py's docstring: the sums within
2 (n - 1) 2^-53 sum |term|, the counts exact; the fitted lens within that bound propagated to first order plus rounding."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi
import lens_ref
from lens_ref import PARAMS, SHIFTS, TRUE, make_lens, shifted_records
from test_strain_gpu import SIDE, centres, device_records, grid_rects, make_engine, small_pair, strain_reference  # noqa: F401

pytestmark = pytest.mark.gpu

H = float(SIDE)
NUISANCES = [ca.LENS_TRANSLATION, ca.LENS_SIMILARITY, ca.LENS_AFFINE]
RADIAL = ca.LENS_FREE_K1 | ca.LENS_FREE_K2
FOUR = RADIAL | ca.LENS_FREE_CENTRE
START = make_lens(121.5, 121.5, 147.785)                  # the default start on this domain: the box's centre, half its diagonal
START_REC = lens_ref.as_record(START)                     # (the engine's own default has rn = 147.7853...: the float centres' diagonal)
ROTATIONS = [(k * 2e-4, k * 2e-4) for k in range(-2, 3)]   # frames that also dilate and rotate by k * 2e-4


@pytest.fixture(scope="module")
def engine(small_pair):
    with make_engine(*small_pair, grid_rects()) as e:
        yield e


@pytest.fixture(scope="module")
def cen(engine):
    return centres(engine)


def check_sums(got, ref_sums, ref_abs, what):
    """one frame: counts exact, every entry of the triangle within 2 (n - 1) 2^-53 sum |term|"""
    n = int(ref_sums[0])
    assert got[0] == n and got[-1] == ref_sums[-1], (what, got[0], n, got[-1], ref_sums[-1])
    tol = 2.0 * max(n - 1, 0) * 2.0 ** -53 * ref_abs[1:-1]
    err = np.abs(got[1:-1] - ref_sums[1:-1])
    assert (err <= tol).all(), (what, np.flatnonzero(err > tol), err[err > tol], tol[err > tol])
    return float((err / np.maximum(tol, 1e-300)).max())


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nuisance", NUISANCES)
def test_sums_match_the_restatement(engine, cen, nuisance):
    rec = shifted_records(cen, similarity=ROTATIONS if nuisance != ca.LENS_TRANSLATION else None, noise=0.01, seed=3)
    rec["error_code"][0, [5, 77]] = 2
    rec["chi"][3, 100] = np.nan
    rec["p"][4, 143, 0] = np.inf
    init = make_lens(124.0, 119.0, 147.785, -0.02, 0.004, 1e-3, -5e-4)
    free = RADIAL | ca.LENS_FREE_P1 | ca.LENS_FREE_P2
    out, frames, sums = engine.lens_fit(free, nuisance, init=lens_ref.as_record(init), records=rec, max_iters=1, return_frames=True,
                                        return_sums=True)
    assert sums.shape == (2, 5, ca.lens_sums_len(nuisance)) and out["status"] == ca.LENS_MAX_ITERS and out["iterations"] == 1
    first, first_abs, _ = lens_ref.all_sums(init, nuisance, np.zeros((5, 6)), cen, rec, ca.FM_UVUXUYVXVY)
    # the last evaluation: at the lens and the nuisance the call returns (both non-zero now)
    last, last_abs, _ = lens_ref.all_sums(lens_ref.as_dict(out["lens"]), nuisance, frames["nuisance"], cen, rec, ca.FM_UVUXUYVXVY)
    assert [int(s[0]) for s in first] == [142, 144, 144, 143, 143] and (frames["n"] == [142, 144, 144, 143, 143]).all()
    assert np.abs(frames["nuisance"][:, :2] - SHIFTS).max() < 0.5 and (frames["nuisance"][:, lens_ref.Q_OF[nuisance]:] == 0).all()
    for f in range(5):
        w0 = check_sums(sums[0, f], first[f], first_abs[f], (nuisance, "first", f))
        w1 = check_sums(sums[1, f], last[f], last_abs[f], (nuisance, "last", f))
        print(f"nuisance {nuisance} frame {f}: n {int(first[f][0])}, sums error / bound {w0:.3g} (first) {w1:.3g} (last)")
    assert out["n_records"] == 716 and out["n_frames_used"] == 5 and out["n_outside"] == 0
    assert out["rms"] < out["rms_before"] and abs(out["rms"] - np.sqrt(last[:, -2].sum() / 716)) <= 1e-12


@pytest.mark.parametrize("nuisance,noise", [(ca.LENS_TRANSLATION, 0.0), (ca.LENS_TRANSLATION, 0.01), (ca.LENS_SIMILARITY, 0.01)])
def test_fitted_lens_matches_the_restatement(engine, cen, nuisance, noise):
    rec = shifted_records(cen, similarity=ROTATIONS if nuisance == ca.LENS_SIMILARITY else None, noise=noise, seed=11)
    kw = dict(max_iters=20, tol=1e-12)
    ref = lens_ref.fit(START, FOUR, nuisance, cen, rec, **kw)
    got, frames = engine.lens_fit(FOUR, nuisance, init=START_REC, records=rec, return_frames=True, **kw)
    assert got["status"] == ca.LENS_OK == ref["status"] and got["last_step"] <= 1e-12
    assert got["n_records"] == ref["n_records"] == 720 and got["n_frames_used"] == 5 and got["n_outside"] == 0
    bound = lens_ref.lens_bound(ref, FOUR, nuisance)
    for j, k in enumerate(PARAMS):
        err = abs(float(got["lens"][k]) - ref["lens"][k])
        print(f"nuisance {nuisance} noise {noise} {k}: {float(got['lens'][k]):.12g}, |device - restatement| {err:.3g}, bound {bound[j]:.3g}, "
              f"sigma {got['sigma'][j]:.3g}")
        assert err <= bound[j], (k, err, bound[j])
        assert abs(got["sigma"][j] - ref["sigma"][j]) <= 1e-6 * ref["sigma"][j]
    assert (got["lens"]["p1"], got["lens"]["p2"], got["lens"]["rn"]) == (0.0, 0.0, START["rn"])        # held: init's values
    assert abs(got["rms"] - ref["rms"]) <= 1e-9 * max(ref["rms"], 1e-6) and abs(got["rms_before"] - ref["rms_before"]) <= 1e-9 * ref["rms_before"]
    assert np.abs(frames["nuisance"] - ref["nuisance"]).max() <= 1e-8 and (frames["status"] == ca.LENS_FRAME_OK).all()


# ---- 2. truth ------------------------------------------------------------------------------------------------------------------
def check_truth_exact(lens, what):
    for k in ("k1", "k2"):
        assert abs(float(lens[k]) - TRUE[k]) <= 1e-5 * abs(TRUE[k]), (what, k, float(lens[k]))
    for k in ("cx", "cy"):
        assert abs(float(lens[k]) - TRUE[k]) <= 1e-4, (what, k, float(lens[k]))


def worst_sigmas(lens, sigma):
    return max(abs(float(lens[k]) - TRUE[k]) / sigma[j] for j, k in enumerate(PARAMS) if k not in ("p1", "p2"))


@pytest.mark.parametrize("nuisance", [ca.LENS_TRANSLATION, ca.LENS_SIMILARITY])
def test_the_true_lens_is_recovered(engine, cen, nuisance):
    sim = ROTATIONS if nuisance == ca.LENS_SIMILARITY else None
    exact = shifted_records(cen, similarity=sim)
    got, frames = engine.lens_fit(FOUR, nuisance, init=START_REC, records=exact, return_frames=True)     # from the zero lens
    print(f"nuisance {nuisance} exact: {got['iterations']} iterations, rms {got['rms_before']:.4g} -> {got['rms']:.3g} px, k1 {got['lens']['k1']:.10f}, "
          f"k2 {got['lens']['k2']:.10f}, c ({got['lens']['cx']:.7f}, {got['lens']['cy']:.7f})")
    assert got["status"] == ca.LENS_OK and got["iterations"] <= 8
    check_truth_exact(got["lens"], nuisance)
    assert got["rms_before"] > 0.05 and got["rms"] < 1e-5
    assert np.abs(frames["nuisance"][:, :2] - SHIFTS).max() <= 1e-4
    if sim is not None:
        assert np.abs(frames["nuisance"][:, 2:4] - np.float64(ROTATIONS)).max() <= 1e-7
    # seeded noise of 0.01 px: within 5 of the reported sigma - the restatement first, here on the CPU
    noisy = shifted_records(cen, similarity=sim, noise=0.01, seed=11)
    ref = lens_ref.fit(START, FOUR, nuisance, cen, noisy)
    assert ref["status"] == ca.LENS_OK and worst_sigmas(ref["lens"], ref["sigma"]) <= 5.0
    got = engine.lens_fit(FOUR, nuisance, init=START_REC, records=noisy)
    worst = worst_sigmas(got["lens"], got["sigma"])
    print(f"nuisance {nuisance} noise 0.01 px: {got['iterations']} iterations, rms {got['rms']:.4f} px, worst |error| / sigma {worst:.3g} "
          f"(restatement {worst_sigmas(ref['lens'], ref['sigma']):.3g}); sigma {got['sigma']}")
    assert got["status"] == ca.LENS_OK and got["iterations"] <= 8 and worst <= 5.0
    assert abs(got["rms"] - 0.01 * np.sqrt(2.0)) < 0.002


# ---- 3. the payoff ---------------------------------------------------------------------------------------------------------------
def test_the_strain_a_lens_fakes_is_removed(engine, cen):
    rec = shifted_records(cen)
    radius = 2.5 * H
    default = engine.lens_default()
    assert (default["cx"], default["cy"]) == (121.5, 121.5) and abs(default["rn"] - 147.785) < 1e-3 and not default["k1"]
    lens = engine.lens_fit(FOUR, records=rec)["lens"]                  # the defaults: from lens_default(), a translation per frame
    fixed, new_centres, status = engine.lens_correct(lens, records=rec, return_centres=True, return_status=True)
    assert not status.any() and np.abs(new_centres - lens_ref.undistort(TRUE, cen)[0]).max() <= 1e-3
    worst_before, worst_after = 0.0, 0.0
    for f in range(5):
        want, _, st, _ = strain_reference(cen, rec[f], ca.FM_UVUXUYVXVY, radius, tensor=ca.STRAIN_SMALL)
        predicted = max(np.abs(want[:, 6]).max(), np.abs(want[:, 7]).max())        # exx, eyy of the restatement
        before = engine.strain_field(radius, tensor=ca.STRAIN_SMALL, records=rec[f])
        after = engine.strain_field(radius, tensor=ca.STRAIN_SMALL, records=fixed[f])
        b = max(np.abs(before["exx"]).max(), np.abs(before["eyy"]).max())
        a = max(np.abs(after["exx"]).max(), np.abs(after["eyy"]).max())
        print(f"frame {f} t {SHIFTS[f]}: max |exx|, |eyy| {b:.3e} (restatement {predicted:.3e}) -> {a:.3e} after the correction")
        assert (st == ca.STRAIN_OK).all() and abs(b - predicted) <= 0.05 * predicted
        assert a <= 1e-3 * predicted
        worst_before, worst_after = max(worst_before, b), max(worst_after, a)
    assert 3e-3 < worst_before < 8e-3                       # about 5e-3: what the lens fakes


# ---- 4. bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY])
def test_records_out_are_the_host_function_s_bytes(small_pair, model):
    with make_engine(*small_pair, grid_rects(), model=model) as e:
        c = centres(e)
        rng = np.random.default_rng(40 + model)
        rec = shifted_records(c, noise=0.05, seed=model)
        rec["p"][..., 2:6] = rng.normal(0, 0.01, (5, 144, 4))
        rec["error_code"][1, [3, 50]] = 1
        rec["chi"][2, 7] = 9.0
        lens = lens_ref.as_record(make_lens(126.0, 117.0, 147.785, -0.03, 0.008, 1e-3, -1e-3))
        out, new_centres, status = e.lens_correct(lens, records=rec, chi_max=5.0, return_centres=True, return_status=True)
        for f in range(5):
            good = lens_ref.is_good(rec[f], _ffi.N_PARAMS[model], 5.0)
            want, want_status = ca.lens_correct_records(model, lens, c, rec[f], good=good)
            assert out[f].tobytes() == want.tobytes() and status[f].tobytes() == want_status.tobytes(), (model, f)
        assert (status[1, [3, 50]] == ca.LENS_NOT_GOOD).all() and status[2, 7] == ca.LENS_NOT_GOOD and (status == 0).sum() == 717
        assert new_centres.tobytes() == ca.lens_undistort(lens, c.astype(np.float64)).astype(np.float32).tobytes()
        assert e.lens_correct(lens, records=rec, chi_max=5.0).tobytes() == out.tobytes()
        # a fold: the corner sectors are outside a lens that turns back there - copied, status 2
        fold = lens_ref.as_record(make_lens(121.5, 121.5, 147.785, -0.5))
        out, new_centres, status = e.lens_correct(fold, records=rec[:1], return_centres=True, return_status=True)
        _, outside = lens_ref.undistort(lens_ref.as_dict(fold), c.astype(np.float64))
        assert outside[[0, 11, 132, 143]].all() and not outside[[65, 66, 77, 78]].any()
        assert (status[0][outside] == ca.LENS_OUTSIDE).all() and out[0][outside].tobytes() == rec[0][outside].tobytes()
        assert new_centres[outside].tobytes() == c[outside].tobytes() and np.isfinite(out["p"]).all()
        if model == ca.FM_U:
            assert out["p"][..., 1:].tobytes() == rec[:1]["p"][..., 1:].tobytes()


def test_step_frames_sources_repeats_shuffles_and_chunks(engine, cen, monkeypatch):
    e = engine
    rec = shifted_records(cen, noise=0.01, seed=5)
    rec["error_code"][2, [9, 10]] = 3
    init = lens_ref.as_record(make_lens(123.0, 120.0, 147.785, -0.02, 0.003))
    kw = dict(init=init, records=rec, return_frames=True, return_sums=True)
    for nuisance in NUISANCES:
        free = FOUR if nuisance != ca.LENS_AFFINE else RADIAL
        one = e.lens_fit(free, nuisance, max_iters=1, **kw)
        # the step = lk_lens_step_from_sums of the device's own first sums
        step, dn = ca.lens_step_from_sums(nuisance, free, init["rn"], one[2][0])
        assert step["status"] == ca.LENS_OK
        for j, k in enumerate(PARAMS):
            assert float(one[0]["lens"][k]) == float(init[k]) + step["delta"][j], (nuisance, k)
        assert one[1]["nuisance"].tobytes() == dn.tobytes() and one[0]["last_step"] == step["scaled_step"]
        # the last sums give sigma, rms and the counts
        last, _ = ca.lens_step_from_sums(nuisance, free, init["rn"], one[2][1])
        assert one[0]["sigma"].tobytes() == last["sigma"].tobytes() and one[0]["rms"] == np.sqrt(last["chi2"] / last["n_records"])
        # repeats
        again = e.lens_fit(free, nuisance, max_iters=1, **kw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one, again))
        # frame 3 alone: its first sums (at init, no nuisance yet) are the bytes it has inside the five
        alone = e.lens_fit(free, nuisance, max_iters=1, **dict(kw, records=rec[3:4]))
        assert alone[2][0, 0].tobytes() == one[2][0, 3].tobytes()
    # the whole fit repeats its bytes too
    full = e.lens_fit(FOUR, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(full, e.lens_fit(FOUR, **kw)))
    assert full[0]["status"] == ca.LENS_OK and e.lens_last()[3] == full[0]["iterations"] + 1
    # under a fit_mask, shuffling which sectors outside it are bad changes nothing
    mask = np.arange(144) % 3 != 0
    a, b = rec.copy(), rec.copy()
    a["error_code"][:, [0, 3, 30, 141]] = 1
    b["error_code"][:, [6, 33, 60, 99]] = 4
    fa = e.lens_fit(FOUR, **dict(kw, records=a, fit_mask=mask))
    fb = e.lens_fit(FOUR, **dict(kw, records=b, fit_mask=mask))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(fa, fb)) and fa[0]["n_records"] == 5 * 96 - 1
    # three chunks against one: the sums within the bound, the counts exact
    results = {}
    for chunk in (64, 2048):
        monkeypatch.setenv("LK_LENS_CHUNK", str(chunk))
        results[chunk] = e.lens_fit(FOUR, max_iters=1, **kw)
        _, used, chunks, evaluations, _ = e.lens_last()
        assert used == chunk and chunks == (3 if chunk == 64 else 1) and evaluations == 2      # 144 = 64 + 64 + 16
    monkeypatch.delenv("LK_LENS_CHUNK")
    default = e.lens_fit(FOUR, max_iters=1, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(default, results[2048]))
    ref, ref_abs, _ = lens_ref.all_sums(lens_ref.as_dict(init), ca.LENS_TRANSLATION, np.zeros((5, 6)), cen, rec, ca.FM_UVUXUYVXVY)
    for f in range(5):
        for chunk in (64, 2048):
            check_sums(results[chunk][2][0, f], ref[f], ref_abs[f], (chunk, f))
    # (144 sectors: a chunk of 64 is one wavefront, so here the three chunks even add in the order of the one; the bound is
    # what the interface promises)


def test_the_three_sources_give_the_same_bytes(small_pair):
    with make_engine(*small_pair, grid_rects()) as e:
        lens = lens_ref.as_record(make_lens(126.0, 117.0, 147.785, -0.03, 0.008))
        rec = e.correlate_all(np.zeros((144, 6), np.float32))
        assert lens_ref.is_good(rec, 6, 0.0).sum() >= 140
        kw = dict(free=ca.LENS_FREE_K1, init=lens, return_frames=True, return_sums=True, max_iters=3)
        eng = e.lens_fit(source=ca.TRACK_RECORDS_ENGINE, **kw)
        default = e.lens_fit(**kw)
        caller = e.lens_fit(records=rec, **kw)
        for a, b, c in zip(eng, default, caller):
            assert a.tobytes() == c.tobytes() and b.tobytes() == c.tobytes()
        ckw = dict(return_centres=True, return_status=True)
        for a, b, c in zip(e.lens_correct(lens, source=ca.TRACK_RECORDS_ENGINE, **ckw), e.lens_correct(lens, **ckw),
                           e.lens_correct(lens, records=rec, **ckw)):
            assert a.tobytes() == c.tobytes() and b.tobytes() == c.tobytes()
        # a short window read in place = wait_sequence's host copy passed back in
        e.sequence_reserve(2)
        for i in range(2):
            e.sequence_set_frame(i, small_pair[1])
        e.adjust_initial_guess(0, False, np.zeros(6, np.float32), (128.0, 128.0))
        win = e.correlate_sequence(2, constant_velocity=False)
        assert win.shape == (2, 144)
        inplace = e.lens_fit(source=ca.TRACK_RECORDS_WINDOW, **kw)
        counted = e.lens_fit(n_frames=2, source=ca.TRACK_RECORDS_WINDOW, **kw)
        passed = e.lens_fit(records=win, **kw)
        for a, b, c in zip(inplace, counted, passed):
            assert a.tobytes() == c.tobytes() and b.tobytes() == c.tobytes()
        assert inplace[1].shape == (2,) and inplace[2].shape[1] == 2
        for a, c in zip(e.lens_correct(lens, source=ca.TRACK_RECORDS_WINDOW, **ckw), e.lens_correct(lens, records=win, **ckw)):
            assert a.tobytes() == c.tobytes()


# ---- 5. end to end on rendered frames ---------------------------------------------------------------------------------------------
def test_end_to_end_on_frames_seen_through_a_lens():
    """Measured (profiles/lens_recovery.txt has the CPU oracle's records of the same frames beside the device's)."""
    und, shifted = lens_ref.lens_frames()
    free = ca.LENS_FREE_K1 | ca.LENS_FREE_CENTRE
    with make_engine(und, shifted[0], grid_rects()) as e:
        c = centres(e)
        rec = np.zeros((4, 144), ca.RESULT_DTYPE)
        for f, t in enumerate(lens_ref.IMAGE_SHIFTS):
            e.set_deformed_image(shifted[f])
            g = np.zeros((144, 6), np.float32)
            g[:, :2] = t
            rec[f] = e.correlate_all(g)
        good = lens_ref.is_good(rec, 6, 0.0)
        assert good.sum() >= 4 * 130                       # (the CPU oracle solves 552 of the 576)
        got = e.lens_fit(free, ca.LENS_TRANSLATION, records=rec)
        fixed = e.lens_correct(got["lens"], records=rec)
        before, after = lens_ref.spread_about_frame_mean(rec, good), lens_ref.spread_about_frame_mean(fixed, good)
        k1 = float(got["lens"]["k1"])
        print(f"rendered frames: status {got['status']}, {got['iterations']} iterations, k1 {k1:.5f} +- {got['sigma'][0]:.2g} of "
              f"{lens_ref.IMAGE_LENS['k1']}, c ({got['lens']['cx']:.2f}, {got['lens']['cy']:.2f}) of (126, 117); spread about the frame "
              f"mean {before:.4f} -> {after:.4f} px; rms {got['rms_before']:.4f} -> {got['rms']:.4f} px over {got['n_records']} records")
        assert got["status"] == ca.LENS_OK
        assert abs(k1 - lens_ref.IMAGE_LENS["k1"]) <= 0.1 * abs(lens_ref.IMAGE_LENS["k1"])
        assert after <= before / 3.0


# ---- 6. nothing of the engine moves -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reference_order", [0, 1])
def test_engine_state_is_untouched(small_pair, reference_order):
    rects = grid_rects(n=8)
    S = len(rects)
    with make_engine(*small_pair, rects) as e:
        if reference_order:
            e.set_reference_order(1)
        g = np.zeros((S, 6), np.float32)
        g[[9, 27], 0] = 300.0
        first = e.correlate_all(g)
        if not reference_order:
            e.reseed_failed(1.5 * H)

        def state():
            return dict(records=device_records(e), guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(),
                        stats=e.sector_stats(), reseed=e.reseed_info() if not reference_order else np.zeros(1),
                        counters=np.array(sorted(e.stats().items()), dtype=object))

        def same(a, b):
            for k in a:
                assert (a[k] == b[k]).all() if k == "counters" else a[k].tobytes() == b[k].tobytes(), k

        lens = lens_ref.as_record(make_lens(70.0, 80.0, 100.0, -0.03))
        kept = state()
        a = e.lens_fit(ca.LENS_FREE_K1, init=lens, source=ca.TRACK_RECORDS_ENGINE, max_iters=2, return_frames=True)
        b = e.lens_fit(FOUR, ca.LENS_SIMILARITY, init=lens, records=np.stack([first, first]), chi_max=5.0, fit_mask=np.arange(S) % 2, max_iters=2)
        c = e.lens_correct(lens, return_centres=True, return_status=True)
        d = e.lens_correct(lens, records=np.stack([first, first]), chi_max=5.0)
        assert a[1].shape == (1,) and b["n_frames_used"] == 2 and c[0].shape == (1, S) and d.shape == (2, S)
        assert a[0].tobytes() == e.lens_fit(ca.LENS_FREE_K1, init=lens, records=kept["records"], max_iters=2).tobytes()
        same(kept, state())
        # a rebuild of the lists that waits for the next solve keeps waiting
        e.update_sector(20, 0)
        kept = state()
        assert e.lens_correct(lens)[0].tobytes() == c[0][0].tobytes()
        assert e.lens_fit(ca.LENS_FREE_K1, init=lens, max_iters=2).tobytes() == a[0].tobytes()
        same(kept, state())
        after = e.correlate_all(np.zeros((S, 6), np.float32))
        assert (after["error_code"] == 0).sum() >= S - 2


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_arguments_and_refusals(small_pair):
    rects = grid_rects(n=3)
    e = make_engine(*small_pair, rects, commit=False)
    lib, h = e.lib, e._h
    P = C.c_void_p
    rec = shifted_records(np.float32([(17 + 19 * i, 17 + 19 * j) for i in range(3) for j in range(3)]), L=make_lens(36.0, 36.0, 26.87, -0.02),
                          shifts=SHIFTS[:2])
    out = np.full(1, 7, ca.LENS_RESULT_DTYPE)
    frames = np.full(2, 7, ca.LENS_FRAME_DTYPE)
    rec_out = np.full((2, 9), 7, ca.RESULT_DTYPE)
    good_lens = ca.make_lens(36.0, 36.0, 30.0, -0.01)
    names = ("source", "chi_max", "min_sectors", "free", "nuisance", "max_iters", "tol", "r0", "r1")
    GOOD = (ca.TRACK_RECORDS_CALLER, 0.0, 2, ca.LENS_FREE_K1, ca.LENS_TRANSLATION, 10, 1e-8, 0, 0)

    def config(values):
        v = dict(zip(names, values))
        c = _ffi.LkLensFitConfig(v["source"], v["chi_max"], v["min_sectors"], v["free"], v["nuisance"], v["max_iters"], v["tol"])
        c.reserved[0], c.reserved[1] = v["r0"], v["r1"]
        return c

    def with_(**kw):
        d = dict(zip(names, GOOD))
        d.update(kw)
        return tuple(d.values())

    def lens_with(**kw):
        lens = np.array([good_lens], ca.LENS_DTYPE)
        for k, v in kw.items():
            lens[k] = v
        return lens

    def refused(cfg=GOOD, n_frames=2, records=rec, lens=lens_with(), output=out):
        c = config(cfg) if cfg is not None else None
        rc = lib.lk_lens_fit(h, C.byref(c) if c is not None else None, lens.ctypes.data_as(P) if lens is not None else None, n_frames,
                             records.ctypes.data_as(P) if records is not None else None, None,
                             output.ctypes.data_as(P) if output is not None else None, frames.ctypes.data_as(P), None)
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and "lk_lens_fit" in msg, (rc, msg)
        assert out.tobytes() == np.full(1, 7, ca.LENS_RESULT_DTYPE).tobytes() and frames.tobytes() == np.full(2, 7, ca.LENS_FRAME_DTYPE).tobytes()
        return msg

    def correct_refused(source=ca.TRACK_RECORDS_CALLER, chi_max=0.0, r0=0, r1=0, n_frames=2, records=rec, lens=lens_with(), output=rec_out,
                        no_config=False):
        c = _ffi.LkLensConfig(source, chi_max)
        c.reserved[0], c.reserved[1] = r0, r1
        rc = lib.lk_lens_correct(h, None if no_config else C.byref(c), lens.ctypes.data_as(P) if lens is not None else None, n_frames,
                                 records.ctypes.data_as(P) if records is not None else None,
                                 output.ctypes.data_as(P) if output is not None else None, None, None)
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and "lk_lens_correct" in msg, (rc, msg)
        assert rec_out.tobytes() == np.full((2, 9), 7, ca.RESULT_DTYPE).tobytes()
        return msg

    assert "no committed sectors" in refused() and "no committed sectors" in correct_refused()
    e.commit_sectors()
    assert "configuration" in refused(None) and "configuration" in correct_refused(no_config=True)
    assert "output" in refused(output=None) and "output" in correct_refused(output=None)
    assert "no lens" in refused(lens=None) and "no lens" in correct_refused(lens=None)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "rn" in refused(lens=lens_with(rn=bad)) and "rn" in correct_refused(lens=lens_with(rn=bad))
    for field in ("cx", "cy", "k1", "k2", "p1", "p2"):
        for bad in (float("nan"), float("-inf")):
            assert "finite" in refused(lens=lens_with(**{field: bad})) and "finite" in correct_refused(lens=lens_with(**{field: bad}))
    assert "reserved" in refused(lens=lens_with(reserved=1.0)) and "reserved" in correct_refused(lens=lens_with(reserved=1.0))
    for bad in (0, 32, 64 | ca.LENS_FREE_K1):
        assert "free" in refused(with_(free=bad))
    for bad in (-1, 3):
        assert "nuisance" in refused(with_(nuisance=bad, min_sectors=6))
    assert "LK_LENS_AFFINE" in refused(with_(nuisance=ca.LENS_AFFINE, free=FOUR, min_sectors=6))
    assert "LK_LENS_AFFINE" in refused(with_(nuisance=ca.LENS_AFFINE, free=ca.LENS_FREE_CENTRE, min_sectors=6))
    for bad in (0, -1, 33):
        assert "max_iters" in refused(with_(max_iters=bad))
    for bad in (-1e-9, float("nan"), float("inf")):
        assert "tol" in refused(with_(tol=bad))
    for nuisance, q in ((ca.LENS_TRANSLATION, 2), (ca.LENS_SIMILARITY, 4), (ca.LENS_AFFINE, 6)):
        for bad in (q - 1, -1):
            assert "min_sectors" in refused(with_(nuisance=nuisance, min_sectors=bad))
    assert "reserved" in refused(with_(r0=1)) and "reserved" in refused(with_(r1=-1))
    assert "reserved" in correct_refused(r0=1) and "reserved" in correct_refused(r1=-1)
    for bad in (float("nan"), float("inf")):
        assert "chi_max" in refused(with_(chi_max=bad)) and "chi_max" in correct_refused(chi_max=bad)
    # the sources, as lk_track_points
    for bad in (-1, 3):
        assert "source" in refused(with_(source=bad)) and "source" in correct_refused(source=bad)
    for bad in (0, -1):
        assert "n_frames" in refused(n_frames=bad) and "n_frames" in correct_refused(n_frames=bad)
    assert "records" in refused(records=None) and "records" in correct_refused(records=None)
    for src in (ca.TRACK_RECORDS_ENGINE, ca.TRACK_RECORDS_WINDOW):
        assert "records" in refused(with_(source=src), n_frames=1) and "records" in correct_refused(source=src, n_frames=1)
    assert "n_frames" in refused(with_(source=ca.TRACK_RECORDS_ENGINE), records=None, n_frames=2)
    assert "n_frames" in correct_refused(source=ca.TRACK_RECORDS_ENGINE, records=None, n_frames=2)
    assert "no solve" in refused(with_(source=ca.TRACK_RECORDS_ENGINE), records=None, n_frames=1)
    assert "no solve" in correct_refused(source=ca.TRACK_RECORDS_ENGINE, records=None, n_frames=1)
    assert "no window" in refused(with_(source=ca.TRACK_RECORDS_WINDOW), records=None, n_frames=0)
    assert "no window" in correct_refused(source=ca.TRACK_RECORDS_WINDOW, records=None, n_frames=0)
    assert "n_frames" in refused(with_(source=ca.TRACK_RECORDS_WINDOW), records=None, n_frames=-1)
    assert lib.lk_lens_fit(None, None, None, 2, None, None, None, None, None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_lens_correct(None, None, None, 2, None, None, None, None) == ca.ERROR_BAD_DOMAIN
    with pytest.raises(ValueError):
        e.lens_fit(records=rec, fit_mask=np.ones(5))
    with pytest.raises(ca.LkError, match="no lk_lens_fit"):
        e.lens_last()
    # records passed in need no solve; statuses that are not refusals
    got, fr = e.lens_fit(ca.LENS_FREE_K1, records=rec, return_frames=True)
    assert got["status"] == ca.LENS_OK and got["n_records"] == 18 and (fr["status"] == ca.LENS_FRAME_OK).all()
    few, fr = e.lens_fit(ca.LENS_FREE_K1, records=rec, min_sectors=10, return_frames=True)
    assert few["status"] == ca.LENS_DEGENERATE and few["n_frames_used"] == 0 and (fr["status"] == ca.LENS_FRAME_TOO_FEW).all()
    assert few["lens"].tobytes() == e.lens_default().tobytes() and not few["sigma"].any() and not fr["nuisance"].any()
    still = rec.copy()
    still["p"][:] = 0
    assert e.lens_fit(ca.LENS_FREE_K1, records=still)["status"] == ca.LENS_DEGENERATE                    # no translation at all
    assert e.lens_fit(ca.LENS_FREE_CENTRE, records=rec)["status"] == ca.LENS_DEGENERATE                  # the centre of no lens
    slow = e.lens_fit(ca.LENS_FREE_K1, records=rec, max_iters=1, tol=0.0)
    assert slow["status"] == ca.LENS_MAX_ITERS and slow["iterations"] == 1
    # a solve or a window in flight refuses the engine's records
    e.correlate_all_async()
    assert "waited for" in refused(with_(source=ca.TRACK_RECORDS_ENGINE), records=None, n_frames=1)
    assert "waited for" in correct_refused(source=ca.TRACK_RECORDS_ENGINE, records=None, n_frames=1)
    e.wait_results()
    e.sequence_reserve(2)
    for i in range(2):
        e.sequence_set_frame(i, small_pair[1])
    e.adjust_initial_guess(0, False, np.zeros(6, np.float32), (32.0, 32.0))
    e.correlate_sequence_async(2, constant_velocity=False)
    assert "outstanding" in refused(with_(source=ca.TRACK_RECORDS_WINDOW), records=None, n_frames=0)
    assert "outstanding" in correct_refused(source=ca.TRACK_RECORDS_WINDOW, records=None, n_frames=0)
    e.wait_sequence()
    assert "n_frames" in refused(with_(source=ca.TRACK_RECORDS_WINDOW), records=None, n_frames=3)
    assert "n_frames" in correct_refused(source=ca.TRACK_RECORDS_WINDOW, records=None, n_frames=3)
    e.close()
    # a one-parameter model has no v: no lens can be fitted to it (the correction works: u alone)
    with make_engine(*small_pair, rects, model=ca.FM_U) as e1:
        with pytest.raises(ca.LkError, match="LK_FM_U"):
            e1.lens_fit(records=rec)
        assert e1.lens_correct(good_lens, records=rec).shape == (2, 9)
