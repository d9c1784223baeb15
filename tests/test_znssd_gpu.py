"""The ZNSSD refinement on the GPU (lk_refine_znssd, include/lk_engine.h): the sums of the seed evaluation against the
oracle's per-sample floats and the info against the host function, the fixed point of the converged sectors, the accuracy
against the analytic map, the lighting identity and the failure of the plain solve on the darker frame, the pipeline from
lk_search_guesses, batch independence and the modes, the statuses, that nothing of the engine moves, and the arguments.

Geometry and bounds: znssd_ref.py - a 256 x 256 pair with a known affine map; an 8 x 8 grid of 19 x 19 rectangles (16-lane
rows), a 24 x 24 rectangle (a wavefront), a 96 x 96 rectangle (the 512-lane group) and an annular list sector.

Sums: per sum |device - float64 sum of the restated terms| <= 64 n 2^-53 sum|terms|, the bound of test_uncertainty_gpu.py
and test_residual_gpu.py - device and restatement differ only in the order of double additions.  For
LK_IM_BICUBIC_SEPARABLE, which the oracle has no sampler for, value and gradient come from lk_sample."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import residual_ref as rr
import znssd_ref as zr

pytestmark = pytest.mark.gpu

MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
NEAR = np.float32([1.25, -0.65, 0.001, 0.0005, -0.0005, -0.001])
S = zr.N_SECTORS
BIG, WAVE, RING = len(zr.GRID) + 1, len(zr.GRID), len(zr.RECTS)   # the 96 x 96, the 24 x 24 and the annular sector


@pytest.fixture(scope="module")
def pair():
    return zr.pair()


def make_engine(und, dfm, rects=zr.RECTS, model=ca.FM_UVUXUYVXVY, annular=zr.ANNULAR, interp=ca.IM_BICUBIC, commit=True):
    e = ca.HipCorrelationEngine(interpolation=interp, fitting_model=model, precision=zr.PRECISION, py_start=0, py_stop=2)
    if und is not None:
        e.set_undeformed_image(und)
        e.set_deformed_image(dfm)
    for s, r in enumerate(rects):
        e.resetPolygon_rect(s, *r)
    for k, q in enumerate(annular):
        e.resetPolygon_annular(len(rects) + k, *q)
    if commit:
        e.commit_sectors()
    return e


def geometry(e, rects=zr.RECTS):
    """the samples of every sector in the pass's order and the committed centres"""
    lists = [zr.rect_rows(*rects[s]) if s < len(rects) else e.level_xy(0, s) for s in range(e.n_sectors)]
    centres = [e.sector_info(s)[1:3] for s in range(e.n_sectors)]
    return lists, centres


def near_guesses(n=S):
    return np.tile(NEAR, (n, 1))


def errors_against_the_map(rec, centres):
    want = np.array([zr.analytic_uv(float(cx), float(cy)) for cx, cy in centres])
    return np.hypot(rec["p"][:, 0].astype(np.float64) - want[:, 0], rec["p"][:, 1].astype(np.float64) - want[:, 1])


# ---- 1. the sums of the seed evaluation ---------------------------------------------------------------------------------------
CASES = [(m, ca.IM_BICUBIC) for m in MODELS] + [(ca.FM_UVUXUYVXVY, ca.IM_BILINEAR), (ca.FM_UVUXUYVXVY, ca.IM_BICUBIC_SEPARABLE)]


def check_seed_evaluation(oracle, e, und, dfm, model, interp, lists, centres, g, sampler=None, ratios=None, refine=None, allow_refused=False):
    """refine_znssd with max_iters = 0 from the seeds g: per sector the sums against the oracle's per-sample floats within
    64 n 2^-53 sum|terms|, the info the host function of the device's sums bit for bit, the record; the same call again gives
    the same bytes -> (worst sum error / bound, the records).  refine: the pass (default e.refine_znssd; lk_refine_spline has the
    same contract under its own sampler).  allow_refused: a sector may be one the criterion refuses or whose step is singular (a
    starved sector of test_pass_instances_gpu.py); without it every sector must evaluate and step, as ever."""
    P = _ffi.N_PARAMS[model]
    used = zr.layout(P)[4]
    n0 = [e.sector_info(s)[0] for s in range(e.n_sectors)]
    refine = refine or e.refine_znssd
    rec, info, sums = refine(guesses=g, max_iters=0, return_sums=True)
    worst = 0.0
    for s in range(e.n_sectors):
        xy, (cx, cy) = lists[s], centres[s]
        n = len(xy)
        f, gg, H, bad = zr.sample_floats(oracle, interp, model, und, dfm, xy, cx, cy, g[s], sampler)
        assert not bad.any()
        terms = zr.sum_terms(f, gg, H)
        bound = 64.0 * n * 2.0 ** -53 * np.abs(terms).sum(axis=0)
        err = np.abs(sums[s][:used] - terms.sum(axis=0))
        ratio = float((err[bound > 0] / bound[bound > 0]).max())
        assert (err <= bound).all(), (s, err, bound)
        assert not sums[s][used:].any(), (s, sums[s][used:])
        worst = max(worst, ratio)
        if ratios is not None:
            ratios.append((s, ratio))
        # the info is the host function of the device's sums, bit for bit
        status, delta, crit, gain, offset = ca.znssd_step_from_sums(model, n, sums[s], zr.LAMBDA0)
        refused, _, _, _, zncc = zr.criterion(model, n, sums[s])
        i = info[s]
        if allow_refused:   # (the step's status is the restatement's: a starved sector's matrix may be singular)
            assert status == zr.step(model, n, sums[s], zr.LAMBDA0)[0] and (status == 0 or n < 16), (s, status)
            assert i["status"] == (refused if refused else ca.ZN_MAX_ITERS) and i["n_points"] == n, (s, status, i)
        else:
            assert status == 0 and not refused and i["status"] == ca.ZN_MAX_ITERS and i["n_points"] == n, (s, status, i)
        assert (i["iterations"], i["evaluations"]) == (0, 1) and i["shift"] == 0 and i["last_step"] == 0 and not i["reserved"].any()
        if not refused:
            for name, want in (("gain", gain), ("offset", offset), ("znssd", crit), ("zncc", zncc), ("zncc_seed", zncc)):
                assert i[name].tobytes() == np.float32(want).tobytes(), (s, name, i[name], want)
            assert i["lambda"] == np.float32(zr.LAMBDA0)
        # the record: the seed, the forward evaluation's chi, the committed centre and the level-0 count
        r = rec[s]
        assert r["p"][:P].tobytes() == g[s][:P].tobytes() and not r["p"][P:].any(), (s, r)
        V = (f - gg).astype(np.float64)
        assert abs(float(r["chi"]) - (V * V).mean()) <= 1e-6 * (V * V).mean(), (s, r["chi"], (V * V).mean())
        if not refused:
            assert r["error_code"] == ca.ERROR_CORRELATION_MAX_ITERS_REACHED and r["iterations"] == 0
        assert r["n_points"] == n0[s] and (r["und_cx"], r["und_cy"]) == (np.float32(cx), np.float32(cy)), (s, r)
    print(f"model {model} interp {interp}: worst sum error / bound {worst:.3g}")
    # the same call again: the same bytes
    again = refine(guesses=g, max_iters=0, return_sums=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (rec, info, sums)))
    return worst, rec


@pytest.mark.parametrize("model,interp", CASES)
def test_sums_and_info_of_the_seed_evaluation(oracle, pair, model, interp):
    """(all sixteen (model, interpolator) pairs run on the geometry of test_pass_instances_gpu.py; this one keeps the grid
    sectors and the 24 x 24 wavefront sector)"""
    und, dfm = pair
    # a quarter of the grid, and the three sectors of the other kinds
    rects = zr.GRID[::4] + zr.RECTS[len(zr.GRID):]
    with make_engine(und, dfm, rects, model=model, interp=interp) as e:
        n0 = [e.sector_info(s)[0] for s in range(e.n_sectors)]
        assert n0[:len(rects)] == [361] * 16 + [576, 9216] and 0 < n0[-1] <= 512 and n0[-1] % 16
        lists, centres = geometry(e, rects)
        sampler = (lambda pts: e.sample(ca.IMG_DEF, 0, pts)) if interp == ca.IM_BICUBIC_SEPARABLE else None
        _, rec = check_seed_evaluation(oracle, e, und, dfm, model, interp, lists, centres, near_guesses(e.n_sectors), sampler)
        # the forward evaluation's chi (lk_evaluate, scaled by 1 / n as the solve scales it) at the same parameters
        chi = e.evaluate(0, 0, NEAR)[2] / n0[0]
        assert abs(float(rec["chi"][0]) - chi) <= n0[0] * 2.0 ** -23 * chi, (rec["chi"][0], chi)   # (its float summation)


# ---- 2, 3. fixed point and accuracy on the clean pair ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean_run(pair):
    with make_engine(*pair) as e:
        rec, info, sums = e.refine_znssd(guesses=zr.zero_gradient_seeds(S), return_sums=True)
        lists, centres = geometry(e)
    return dict(rec=rec, info=info, sums=sums, lists=lists, centres=centres)


def check_fixed_point(oracle, und, dfm, model, interp, lists, centres, rec, info, sums, sampler=None):
    """every ZN_CONVERGED sector: the restatement evaluated at the returned parameters gives a step below 4 x precision at the
    returned lambda, and the kept sums are those of the returned parameters; every sector with sums: the info is the host
    function of them, bit for bit -> the largest weighted step"""
    used = zr.layout(_ffi.N_PARAMS[model])[4]
    worst = 0.0
    for s in range(len(lists)):
        xy, (cx, cy) = lists[s], centres[s]
        n = len(xy)
        if sums[s].any() and info["evaluations"][s] > 0 and info["status"][s] not in (ca.ZN_TOO_FEW, ca.ZN_FLAT, ca.ZN_OUT_OF_IMAGE, ca.ZN_NEGATIVE,
                                                                                           ca.ZN_BAD_SEED):
            _, _, crit, gain, offset = ca.znssd_step_from_sums(model, n, sums[s], float(info["lambda"][s]))
            zncc = zr.criterion(model, n, sums[s])[4]
            for name, want in (("gain", gain), ("offset", offset), ("znssd", crit), ("zncc", zncc)):
                assert info[name][s].tobytes() == np.float32(want).tobytes(), (s, name, info[name][s], want)
        if info["status"][s] != ca.ZN_CONVERGED:
            continue
        f, g, H, bad = zr.sample_floats(oracle, interp, model, und, dfm, xy, cx, cy, rec["p"][s], sampler)
        ref = zr.sums_of(f, g, H, bad)
        st, delta = zr.step(model, n, ref, float(info["lambda"][s]))[:2]
        w = zr.weighted_step(model, n, delta)
        worst = max(worst, w)
        assert st == 0 and w < 4.0 * zr.PRECISION, (s, st, w, info[s])
        # the kept sums are those of the returned parameters
        bound = 64.0 * n * 2.0 ** -53 * np.abs(zr.sum_terms(f, g, H)).sum(axis=0)
        assert (np.abs(sums[s][:used] - ref[:used]) <= bound).all() and sums[s][used] == 0, s
    return worst


def test_fixed_point_of_the_converged_sectors(oracle, pair, clean_run):
    """the restatement evaluated at the returned parameters gives a step below 4 x precision at the returned lambda"""
    und, dfm = pair
    rec, info = clean_run["rec"], clean_run["info"]
    print("status histogram", np.bincount(info["status"], minlength=9), "trips", info["iterations"].min(), "..", info["iterations"].max(),
          "evaluations", info["evaluations"].min(), "..", info["evaluations"].max())
    assert not np.isin(info["status"], (ca.ZN_MAX_ITERS, ca.ZN_STALLED)).any(), info["status"]
    assert (info["status"] == ca.ZN_CONVERGED).all(), info["status"]
    assert (rec["error_code"] == 0).all() and (rec["iterations"] == info["iterations"]).all()
    worst = check_fixed_point(oracle, und, dfm, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, clean_run["lists"], clean_run["centres"], rec, info,
                              clean_run["sums"])
    print(f"largest weighted step of the restatement at the returned state: {worst:.3g} (allowed {4.0 * zr.PRECISION:.3g})")


def test_accuracy_against_the_analytic_map(clean_run):
    err = errors_against_the_map(clean_run["rec"], clean_run["centres"])
    comp = np.abs(np.stack([clean_run["rec"]["p"][:, k].astype(np.float64) - np.array([zr.analytic_uv(float(cx), float(cy))[k]
                                                                                        for cx, cy in clean_run["centres"]]) for k in (0, 1)]))
    print(f"largest |(u, v) - analytic| = {comp.max():.6f} px (allowed {1.5 * zr.ACCURACY:.6f}); largest distance {err.max():.6f}")
    assert comp.max() <= 1.5 * zr.ACCURACY, (comp.max(), zr.ACCURACY)


# ---- 4. lighting ----------------------------------------------------------------------------------------------------------------
def test_lighting(pair):
    und, dfm = pair
    d, d2 = zr.lighting_frames(dfm)
    seeds = zr.zero_gradient_seeds(S)
    with make_engine(und, d) as e:
        centres = [e.sector_info(s)[1:3] for s in range(S)]
        a, ia = e.refine_znssd(guesses=seeds)
        e.set_deformed_image(d2)
        b, ib = e.refine_znssd(guesses=seeds)
        plain = e.correlate_all(seeds)
        # the refinement from the engine-held records of that solve: the repair the pass is for
        c, ic = e.refine_znssd()
    assert (ia["status"] == ca.ZN_CONVERGED).all() and (ib["status"] == ca.ZN_CONVERGED).all(), (ia["status"], ib["status"])
    diff = np.abs(a["p"][:, :2].astype(np.float64) - b["p"][:, :2].astype(np.float64)).max()
    print(f"largest |(u, v) on D - (u, v) on D'| = {diff:.6f} px (allowed {2.0 * zr.D_LIGHT:.6f})")
    assert diff <= 2.0 * zr.D_LIGHT, diff
    for s in range(S):
        dz, tol = abs(float(ia["zncc"][s]) - float(ib["zncc"][s])), rr.lighting_tol("zncc", ia["zncc"][s])
        assert dz <= tol, (s, ia["zncc"][s], ib["zncc"][s], dz, tol)
    assert np.abs(ib["gain"] - 2.0 * ia["gain"]).max() < 1e-3 and np.abs(ib["offset"] - (ia["offset"] - 64.0 * ia["gain"])).max() < 0.1
    e_zn, e_ls = errors_against_the_map(b, centres), errors_against_the_map(plain, centres)
    worse = (e_ls > e_zn) | ~np.isfinite(e_ls)
    print(f"on D': the engine's solve is worse than the refinement on {int(worse.sum())} of {S} sectors; median error "
          f"{np.median(e_ls):.4f} against {np.median(e_zn):.4f} px; solve error codes {np.bincount(plain['error_code'], minlength=6)}")
    assert worse.sum() >= 0.9 * S
    good = plain["error_code"] == 0
    assert (ic["status"][~good] == ca.ZN_BAD_SEED).all() and c[~good].tobytes() == plain[~good].tobytes()
    # (the solve's records on D' are most of a pixel off with gradient terms to match: seeds this pass, which works at one
    # level, is not meant for - whatever it makes of them, it says so)
    print("refined from the solve's records: status histogram", np.bincount(ic["status"], minlength=9))
    assert np.isin(ic["status"][good], (ca.ZN_CONVERGED, ca.ZN_MAX_ITERS, ca.ZN_STALLED)).all(), ic["status"]
    assert (c["error_code"][good] == np.where(ic["status"][good] == ca.ZN_CONVERGED, 0, ca.ERROR_CORRELATION_MAX_ITERS_REACHED)).all()


# ---- 5. the pipeline --------------------------------------------------------------------------------------------------------------
def test_pipeline_from_the_guess_search(pair):
    und, dfm = pair
    _, d2 = zr.lighting_frames(dfm)
    with make_engine(und, d2) as e:
        centres = [e.sector_info(s)[1:3] for s in range(S)]
        g = e.search_guesses(4, level=0, guesses=np.zeros((S, 6), np.float32))
        assert (np.abs(g[:, :2] - np.float32([1.0, -1.0])) <= 1.0).all(), g[:, :2]
        rec, info = e.refine_znssd(guesses=g)
    print("status histogram", np.bincount(info["status"], minlength=9), "largest shift", info["shift"].max())
    assert (info["status"] == ca.ZN_CONVERGED).all(), info["status"]
    want = np.array([zr.analytic_uv(float(cx), float(cy)) for cx, cy in centres])
    comp = np.abs(rec["p"][:, :2].astype(np.float64) - want).max()
    print(f"largest |(u, v) - analytic| = {comp:.6f} px (allowed {1.5 * zr.ACCURACY + 2.0 * zr.D_LIGHT:.6f})")
    assert comp <= 1.5 * zr.ACCURACY + 2.0 * zr.D_LIGHT


# ---- 6. a sector alone is the sector in the grid ------------------------------------------------------------------------------------
def test_a_sector_alone_modes_and_the_ring_slot_give_the_same_bytes(pair, clean_run):
    rec, info, sums = clean_run["rec"], clean_run["info"], clean_run["sums"]
    seeds = zr.zero_gradient_seeds(S)
    for k in (0, 37, WAVE, BIG):
        with make_engine(*pair, [zr.RECTS[k]], annular=()) as e:
            r, i, q = e.refine_znssd(guesses=seeds[:1], return_sums=True)
            assert r[0].tobytes() == rec[k].tobytes() and i[0].tobytes() == info[k].tobytes() and q[0].tobytes() == sums[k].tobytes(), k
    with make_engine(*pair, [], annular=zr.ANNULAR) as e:
        r, i = e.refine_znssd(guesses=seeds[:1])
        assert r[0].tobytes() == rec[RING].tobytes() and i[0].tobytes() == info[RING].tobytes()
    with make_engine(*pair) as e:
        def same():
            r, i, q = e.refine_znssd(guesses=seeds, return_sums=True)
            assert r.tobytes() == rec.tobytes() and i.tobytes() == info.tobytes() and q.tobytes() == sums.tobytes()

        same()
        e.set_batch_invariant(True)
        same()
        e.set_batch_invariant(False)
        e.set_update(ca.UPDATE_BACKWARD)
        same()
        e.set_update(ca.UPDATE_FORWARD)
        e.set_reference_order(1)
        same()
        # records as seeds: those given and those held give the same bytes
        held = e.correlate_all(seeds)
        a, b = e.refine_znssd(), e.refine_znssd(records=held)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert (a[1]["status"] == ca.ZN_CONVERGED).all()
        e.set_reference_order(0)
        e.sequence_reserve(2)
        e.sequence_set_frame(0, pair[1])
        e.sequence_set_frame(1, pair[0])
        r, i = e.refine_znssd(guesses=seeds, def_slot=0)
        assert r.tobytes() == rec.tobytes() and i.tobytes() == info.tobytes()
        assert e.refine_znssd(guesses=seeds, def_slot=1)[0].tobytes() != rec.tobytes()


# ---- 7. statuses --------------------------------------------------------------------------------------------------------------------
def test_statuses(pair):
    und, dfm = (a.copy() for a in pair)
    und[100:140, 100:140] = 128            # a constant patch of the undeformed image only
    dfm[150:200, 20:70] = 90               # a constant patch of the deformed image only
    rects = [(8, 8, 26, 26), (110, 110, 128, 128), (30, 160, 48, 178), (52, 8, 70, 26), (74, 8, 92, 26), (96, 8, 114, 26), (200, 8, 202, 9)]
    n = len(rects)
    with make_engine(und, dfm, rects, annular=()) as e:
        g = near_guesses(n)
        g[3, 0] = 1000.0                   # leaves the image
        g[4, 4] = np.nan
        rec, info, sums = e.refine_znssd(guesses=g, return_sums=True)
        assert info["status"].tolist() == [ca.ZN_CONVERGED, ca.ZN_FLAT, ca.ZN_FLAT, ca.ZN_OUT_OF_IMAGE, ca.ZN_BAD_SEED, ca.ZN_CONVERGED,
                                           ca.ZN_TOO_FEW], info["status"]
        assert rec["error_code"].tolist() == [0, _ffi.ERROR_SOLVER, _ffi.ERROR_SOLVER, ca.ERROR_INTERPOLATION_OUT_OF_IMAGE, ca.ERROR_BAD_DOMAIN,
                                              0, _ffi.ERROR_SOLVER]
        assert info["n_points"].tolist() == [361] * 6 + [6] and not info["reserved"].any()
        floats = ("zncc", "gain", "offset", "znssd", "zncc_seed", "shift", "last_step")
        for s in (1, 2, 3, 4, 6):
            assert not any(info[k][s] for k in floats) and info["iterations"][s] == 0, (s, info[s])
            assert rec["p"][s].tobytes() == g[s].tobytes() and rec["iterations"][s] == 0, (s, rec[s])
        assert not sums[3].any() and not sums[4].any() and info["evaluations"].tolist() == [info["evaluations"][0], 1, 1, 1, 0,
                                                                                             info["evaluations"][5], 1]
        assert sums[1][0] == 128.0 * 361 and abs(sums[2][1] - 90.0 * 361) < 0.01 and sums[6][0] > 0   # the seed's sums of the refused
        # records as seeds: a bad record passes through, byte for byte
        seeds = np.zeros(n, ca.RESULT_DTYPE)
        seeds["p"][:] = NEAR
        seeds["chi"] = 1.0
        seeds["error_code"][0] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        seeds["iterations"][0] = 50
        seeds["p"][5, 1] = np.inf
        seeds["chi"][3] = 5.0
        out, oi = e.refine_znssd(records=seeds, chi_max=2.0)
        assert oi["status"].tolist() == [ca.ZN_BAD_SEED, ca.ZN_FLAT, ca.ZN_FLAT, ca.ZN_BAD_SEED, ca.ZN_CONVERGED, ca.ZN_BAD_SEED, ca.ZN_TOO_FEW]
        for s in (0, 3, 5):
            assert out[s].tobytes() == seeds[s].tobytes() and not any(oi[k][s] for k in floats) and oi["evaluations"][s] == 0, s
        assert e.refine_znssd(records=seeds)[1]["status"][3] == ca.ZN_CONVERGED    # chi_max <= 0: the error code alone
        assert out[4]["error_code"] == 0
        # the inverted deformed frame: anti-correlated patches
        e.set_deformed_image((255 - pair[1]).astype(np.uint8))
        neg, ni = e.refine_znssd(guesses=near_guesses(n))
        assert (ni["status"][[0, 2, 3, 4, 5]] == ca.ZN_NEGATIVE).all() and (ni["zncc"][[0, 5]] < -0.9).all(), (ni["status"], ni["zncc"])
        assert (neg["error_code"][[0, 5]] == _ffi.ERROR_SOLVER).all() and (ni["evaluations"][[0, 5]] == 1).all()
        # one trip from a seed 2 px off: MAX_ITERS, and the record is the better of the two states
        e.set_deformed_image(pair[1])
        g = near_guesses(n)
        g[:, 0] += 2.0
        one, oi = e.refine_znssd(guesses=g, max_iters=1)
        zero, zi = e.refine_znssd(guesses=g, max_iters=0)
        for s in (0, 5):
            assert oi["status"][s] == ca.ZN_MAX_ITERS and one["error_code"][s] == ca.ERROR_CORRELATION_MAX_ITERS_REACHED
            assert (oi["iterations"][s], oi["evaluations"][s], one["iterations"][s]) == (1, 2, 1)
            assert oi["zncc_seed"][s] == zi["zncc"][s]
            if oi["shift"][s] > 0:           # the trial state was accepted: it is the better one
                assert oi["znssd"][s] < zi["znssd"][s] and one["p"][s].tobytes() != g[s].tobytes()
            else:
                assert oi["znssd"][s] == zi["znssd"][s] and one["p"][s].tobytes() == g[s].tobytes()
        assert (oi["shift"][[0, 5]] > 0).any()


# ---- 8. engine state untouched ----------------------------------------------------------------------------------------------------
def hip_runtime():
    hip = C.CDLL("libamdhip64.so")   # the runtime the engine library itself is linked to
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def device_records(e):
    d = C.c_void_p()
    assert e.lib.lk_get_results_device(e._h, C.byref(d)) == 0
    out = np.zeros(e.n_sectors, ca.RESULT_DTYPE)
    assert e.lib.lk_synchronize(e._h) == 0
    assert hip_runtime().hipMemcpy(out.ctypes.data_as(C.c_void_p), d, out.nbytes, 2) == 0
    return out


def test_engine_state_is_untouched(pair):
    seeds = zr.zero_gradient_seeds(S)
    seeds[[9, 27], 0] = 300.0
    with make_engine(*pair) as e, make_engine(*pair) as plain:
        first = e.correlate_all(seeds)
        plain.correlate_all(seeds)

        def state():
            return dict(records=device_records(e), guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(),
                        stats=e.sector_stats(), strain=e.strain_field(2.5 * zr.SIDE), uncertainty=e.parameter_uncertainty(),
                        counters=np.array(sorted(e.stats().items()), dtype=object))

        kept = state()
        a = e.refine_znssd()
        b = e.refine_znssd(records=first)
        c = e.refine_znssd(guesses=zr.zero_gradient_seeds(S))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert (a[1]["status"][[9, 27]] == ca.ZN_BAD_SEED).all() and (c[1]["status"] == ca.ZN_CONVERGED).all()
        after = state()
        for k in kept:
            if k == "counters":
                assert (kept[k] == after[k]).all()
            else:
                assert kept[k].tobytes() == after[k].tobytes(), k
        # the next solve is the one an engine gives that never made the calls
        assert e.correlate_all(zr.zero_gradient_seeds(S)).tobytes() == plain.correlate_all(zr.zero_gradient_seeds(S)).tobytes()
        assert e.last_evaluated_parameters().tobytes() == plain.last_evaluated_parameters().tobytes()


# ---- 9. arguments and refusals ------------------------------------------------------------------------------------------------------
def test_arguments_and_refusals(pair):
    rects = zr.GRID[:9]
    e = make_engine(*pair, rects, annular=(), commit=False)
    lib, h = e.lib, e._h
    seeds = np.zeros(9, ca.RESULT_DTYPE)
    seeds["p"][:] = NEAR
    g = near_guesses(9)
    rec = np.full(9, 7, np.uint8).repeat(48).view(ca.RESULT_DTYPE)
    info = np.full(9, 7, np.uint8).repeat(64).view(ca.ZNSSD_DTYPE)
    sums = np.full((9, ca.ZN_SUMS), 7.0)
    kept = [rec.tobytes(), info.tobytes(), sums.tobytes()]

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def config(**kw):
        fields = dict(def_slot=-1, chi_max=0.0, max_iters=-1, precision=0.0, lambda0=0.0)
        fields.update(kw)
        return _ffi.LkZnssdConfig(**fields)

    def refused(cfg="default", records=None, guesses=None, outputs=(rec, info), word=None, **kw):
        if cfg == "default":
            cfg = config(**kw)
        if word is not None:
            cfg.reserved[word] = 1
        rc = lib.lk_refine_znssd(h, C.byref(cfg) if cfg is not None else None, ptr(records), _ffi.fptr(guesses) if guesses is not None else None,
                                 ptr(outputs[0]), ptr(outputs[1]), ptr(sums))
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and msg.startswith("lk_refine_znssd: "), (rc, msg)   # names the function called
        return msg

    assert "no committed sectors" in refused(guesses=g) and "no committed sectors" in refused(records=seeds)
    e.commit_sectors()
    assert "no solve" in refused()                                       # neither records nor guesses before any batch solve
    assert "no configuration" in refused(None, guesses=g)
    assert "no output" in refused(guesses=g, outputs=(None, None))
    for word in range(3):
        assert "reserved" in refused(guesses=g, word=word)
    assert "both given" in refused(records=seeds, guesses=g)
    assert "chi_max" in refused(records=seeds, chi_max=np.nan) and "chi_max" in refused(guesses=g, chi_max=np.inf)
    assert "precision" in refused(guesses=g, precision=np.nan) and "lambda0" in refused(guesses=g, lambda0=np.inf)
    assert "ring slot" in refused(guesses=g, def_slot=0) and "def_slot" in refused(guesses=g, def_slot=-2)
    assert lib.lk_refine_znssd(None, C.byref(config()), None, _ffi.fptr(g), ptr(rec), ptr(info), None) == ca.ERROR_BAD_DOMAIN
    assert [rec.tobytes(), info.tobytes(), sums.tobytes()] == kept       # every refusal left the outputs as they were
    # either output alone; guesses and records need no solve; the defaults of the C configuration are lk_config's
    cfg = config()
    assert lib.lk_refine_znssd(h, C.byref(cfg), None, _ffi.fptr(g), ptr(rec), None, None) == 0
    assert lib.lk_refine_znssd(h, C.byref(cfg), ptr(seeds), None, None, ptr(info), None) == 0
    both = e.refine_znssd(guesses=g, max_iters=50, precision=1e-3, lambda0=1e-3)
    assert rec.tobytes() == both[0].tobytes() and info.tobytes() == both[1].tobytes() and (info["status"] == ca.ZN_CONVERGED).all()
    # a solve in flight refuses the engine-held records and finishes normally afterwards
    e.correlate_all_async()
    assert "waited for" in refused()
    solved = e.wait_results()
    assert e.refine_znssd()[0].tobytes() == e.refine_znssd(records=solved)[0].tobytes()
    e.close()
    bare = make_engine(None, None, rects, annular=())
    rc = bare.lib.lk_refine_znssd(bare._h, C.byref(config()), None, _ffi.fptr(g), ptr(rec), ptr(info), None)
    msg = bare.lib.lk_last_error_string(bare._h).decode()
    assert rc == ca.ERROR_BAD_DOMAIN and "image" in msg and msg.startswith("lk_refine_znssd: "), (rc, msg)
    bare.close()
