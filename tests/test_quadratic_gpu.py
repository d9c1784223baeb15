"""The second-order refinement on the GPU (lk_refine_quadratic, include/lk_engine.h): the 87 sums of the seed evaluation
against the restated per-sample terms and the info against the host function, the accuracy against the exactly quadratic
field next to lk_refine_znssd's affine bias, the fixed point, batch independence and the modes, the engine models, the
statuses, that nothing of the engine moves, and the arguments.

Geometry, pair and bounds: quadratic_ref.py - a 256 x 256 pair U(X) = D(X + w(X)) with a quadratic w; 25 squares each of
sides 21 (16-lane rows), 31 and 49 (wavefronts), a 96 x 96 square (the 512-lane group) and an annular list sector.

Sums: per sum |device - float64 sum of the restated terms| <= 64 n 2^-53 sum|terms|, the bound of test_znssd_gpu.py -
device and restatement differ only in the order of double additions.  For LK_IM_BICUBIC_SEPARABLE, which the oracle has no
sampler for, value and gradient come from lk_sample."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import quadratic_ref as qr

pytestmark = pytest.mark.gpu

S = qr.N_SECTORS
NEAR = np.float32([1.25, -0.65, 0.001, 0.0005, -0.0005, -0.001, 2e-4, -1e-4, 1e-4, -2e-4, 1e-4, 3e-4])
OFF = np.array([-0.05, 0.05, 0.001, 0.0005, -0.0005, -0.001, 1e-4, -1e-4, 1e-4, -1e-4, 1e-4, 1e-4])
FLOATS = ("zncc", "gain", "offset", "znssd", "zncc_seed", "shift", "last_step", "bend")
# one sector of every kind: a 16-lane row, two wavefronts, the 512-lane group; the annular list is appended by make_engine
KINDS = [3, 25 + 12, 50 + 21, qr.BIG]


@pytest.fixture(scope="module")
def pair():
    return qr.pair()


def make_engine(und, dfm, rects=qr.RECTS, model=ca.FM_UVUXUYVXVY, annular=qr.ANNULAR, interp=ca.IM_BICUBIC, commit=True, points=()):
    e = ca.HipCorrelationEngine(interpolation=interp, fitting_model=model, precision=qr.PRECISION, py_start=0, py_stop=2)
    if und is not None:
        e.set_undeformed_image(und)
        e.set_deformed_image(dfm)
    for s, r in enumerate(rects):
        e.resetPolygon_rect(s, *r)
    for k, q in enumerate(annular):
        e.resetPolygon_annular(len(rects) + k, *q)
    for k, xy in enumerate(points):
        e.set_sector_points(len(rects) + len(annular) + k, xy)
    if commit:
        e.commit_sectors()
    return e


def geometry(e, rects):
    """the samples of every sector in the pass's order and the committed centres"""
    lists = [qr.rect_rows(*rects[s]) if s < len(rects) else e.level_xy(0, s) for s in range(e.n_sectors)]
    centres = [e.sector_info(s)[1:3] for s in range(e.n_sectors)]
    return lists, centres


# ---- 1. the seed evaluation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [ca.IM_NEAREST, ca.IM_BILINEAR, ca.IM_BICUBIC, ca.IM_BICUBIC_SEPARABLE])
def test_sums_and_info_of_the_seed_evaluation(oracle, pair, interp):
    und, dfm = pair
    rects = [qr.RECTS[k] for k in KINDS]
    with make_engine(und, dfm, rects, interp=interp) as e:
        n0 = [e.sector_info(s)[0] for s in range(e.n_sectors)]
        assert n0[:4] == [441, 961, 2401, 9216] and 0 < n0[4] <= 512 and n0[4] % 16
        lists, centres = geometry(e, rects)
        sampler = (lambda pts: e.sample(ca.IMG_DEF, 0, pts)) if interp == ca.IM_BICUBIC_SEPARABLE else None
        # seeds near the field: its twelve parameters at the centre, moved by OFF
        seeds = (qr.true_translation_seeds(centres)[1] + OFF).astype(np.float32)
        g, g2 = np.ascontiguousarray(seeds[:, :6]), np.ascontiguousarray(seeds[:, 6:])
        rec, info, sums = e.refine_quadratic(guesses=g, second=g2, max_iters=0, return_sums=True)
        worst = 0.0
        for s in range(e.n_sectors):
            xy, (cx, cy) = lists[s], centres[s]
            n = len(xy)
            fl = qr.sample_floats(oracle, interp, und, dfm, xy, cx, cy, seeds[s], sampler)
            assert not fl[6].any()
            terms = qr.sum_terms(*fl[:6])
            bound = 64.0 * n * 2.0 ** -53 * np.abs(terms).sum(axis=0)
            err = np.abs(sums[s][:qr.FLAGGED] - terms.sum(axis=0))
            assert (err <= bound).all(), (s, np.nonzero(err > bound), err, bound)
            assert sums[s][qr.SPARE] == 0 and sums[s][qr.FLAGGED] == 0, (s, sums[s][qr.SPARE:])
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
            # the info is the host function of the device's sums, bit for bit
            status, delta, crit, gain, offset = ca.quadratic_step_from_sums(n, sums[s], qr.LAMBDA0)
            zncc = qr.criterion(n, sums[s])[4]
            i = info[s]
            assert status == 0 and i["status"] == ca.ZN_MAX_ITERS and i["n_points"] == n, (s, status, i)
            assert (i["iterations"], i["evaluations"]) == (0, 1) and i["shift"] == 0 and i["last_step"] == 0 and not i["reserved"].any()
            for name, want in (("gain", gain), ("offset", offset), ("znssd", crit), ("zncc", zncc), ("zncc_seed", zncc),
                               ("bend", qr.bend(seeds[s], n0[s]))):
                assert i[name].tobytes() == np.float32(want).tobytes(), (s, name, i[name], want)
            assert i["lambda"] == np.float32(qr.LAMBDA0) and i["p"].tobytes() == seeds[s].tobytes()
            # the record: the first-order seed, the forward evaluation's chi, the committed centre and the level-0 count
            r = rec[s]
            assert r["p"].tobytes() == seeds[s][:6].tobytes(), (s, r)
            V = (fl[0] - fl[1]).astype(np.float64)
            assert abs(float(r["chi"]) - (V * V).mean()) <= 1e-6 * (V * V).mean(), (s, r["chi"], (V * V).mean())
            assert r["error_code"] == ca.ERROR_CORRELATION_MAX_ITERS_REACHED and r["iterations"] == 0
            assert r["n_points"] == n0[s] and (r["und_cx"], r["und_cy"]) == (np.float32(cx), np.float32(cy)), (s, r)
        print(f"interp {interp}: worst sum error / bound {worst:.3g}")
        # the same call again: the same bytes
        again = e.refine_quadratic(guesses=g, second=g2, max_iters=0, return_sums=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (rec, info, sums)))
        # zero second-order seeds on the affine engine: the warp's bits are the affine warp's, so the grey-value sums, the
        # seed's zncc and the record's chi are lk_refine_znssd's at the same seed
        for second in (None, np.zeros_like(g2)):
            qrec, qinfo, qsums = e.refine_quadratic(guesses=g, second=second, max_iters=0, return_sums=True)
            zrec, zinfo, zsums = e.refine_znssd(guesses=g, max_iters=0, return_sums=True)
            assert qsums[:, :5].tobytes() == zsums[:, :5].tobytes()
            assert qinfo["zncc_seed"].tobytes() == zinfo["zncc_seed"].tobytes() and qrec["chi"].tobytes() == zrec["chi"].tobytes()
            assert not qinfo["p"][:, 6:].any() and not qinfo["bend"].any()


# ---- 2. accuracy: the test that needs the second-order terms ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean_run(pair):
    with make_engine(*pair) as e:
        centres = [e.sector_info(s)[1:3] for s in range(S)]
        n0 = [e.sector_info(s)[0] for s in range(S)]
        seeds, truth = qr.true_translation_seeds(centres)
        rec, info, sums = e.refine_quadratic(guesses=seeds, return_sums=True)
        affine, ainfo = e.refine_znssd(guesses=seeds)
    return dict(rec=rec, info=info, sums=sums, affine=affine, ainfo=ainfo, centres=centres, seeds=seeds, truth=truth, n0=n0)


def test_accuracy_against_the_quadratic_field(clean_run):
    rec, info, truth = clean_run["rec"], clean_run["info"], clean_run["truth"]
    print("status histogram", np.bincount(info["status"], minlength=9), "trips", info["iterations"].min(), "..", info["iterations"].max(),
          "evaluations", info["evaluations"].min(), "..", info["evaluations"].max())
    side = np.array(qr.SIDE_OF + [0])
    for sd in (31, 49):
        assert (info["status"][side == sd] == ca.ZN_CONVERGED).all(), (sd, info["status"][side == sd])
    assert (rec["error_code"] == np.where(info["status"] == ca.ZN_CONVERGED, 0, rec["error_code"])).all()
    assert rec["p"].tobytes() == np.ascontiguousarray(info["p"][:, :6]).tobytes() and (rec["iterations"] == info["iterations"]).all()
    failures = []
    for sd in qr.SIDES:
        idx = np.nonzero((side == sd) & (info["status"] == ca.ZN_CONVERGED))[0]
        assert len(idx) >= 20, (sd, info["status"][side == sd])
        p = info["p"][idx].astype(np.float64)
        err = np.abs(p[:, :2] - truth[idx, :2]).max(axis=1)
        err2 = np.abs(p[:, 6:] - truth[idx, 6:]).max(axis=1)
        aff = np.abs(clean_run["affine"]["p"][idx, :2].astype(np.float64) - truth[idx, :2]).max(axis=1)
        bend = np.array([qr.bend(truth[s], clean_run["n0"][s]) for s in idx])
        print(f"side {sd}: {len(idx)} converged; twelve parameters max / mean |(u, v) - truth| {err.max():.6f} / {err.mean():.6f} px (allowed "
              f"{1.5 * qr.ACCURACY_Q[sd]:.6f}); second-order max {err2.max():.3g} (allowed {1.5 * qr.SECOND_Q[sd]:.3g}); lk_refine_znssd "
              f"max / mean {aff.max():.6f} / {aff.mean():.6f} px (at least {qr.AFFINE_BIAS[sd] / 2:.6f} on average); bend "
              f"{info['bend'][idx].min():.4f}..{info['bend'][idx].max():.4f} px (truth {bend[0]:.4f})")
        if not err.max() <= 1.5 * qr.ACCURACY_Q[sd]:
            failures.append(("accuracy", sd, err.max()))
        if not err2.max() <= 1.5 * qr.SECOND_Q[sd]:
            failures.append(("second order", sd, err2.max()))
        if not aff.mean() >= qr.AFFINE_BIAS[sd] / 2.0:
            failures.append(("affine bias", sd, aff.mean()))
    assert not failures, failures
    # the 512-lane group and the list sector converge to the same field
    for s, allowed in ((qr.BIG, 1.5 * qr.ACCURACY_BIG), (qr.RING, 1.5 * qr.ACCURACY_RING)):
        err = np.abs(info["p"][s][:2].astype(np.float64) - truth[s][:2]).max()
        print(f"sector {s} ({info['n_points'][s]} samples): |(u, v) - truth| {err:.6f} px (allowed {allowed:.6f})")
        assert info["status"][s] == ca.ZN_CONVERGED and err <= allowed, info[s]


# ---- 3. the fixed point --------------------------------------------------------------------------------------------------------
def test_fixed_point(pair, clean_run):
    rec, info = clean_run["rec"], clean_run["info"]
    with make_engine(*pair) as e:
        again, ainfo = e.refine_quadratic(records=rec, second=info["p"][:, 6:])
    done = info["status"] == ca.ZN_CONVERGED
    print("second run: status histogram", np.bincount(ainfo["status"][done], minlength=9), "trips", np.bincount(ainfo["iterations"][done]))
    assert (ainfo["status"][done] == ca.ZN_CONVERGED).all() and (ainfo["iterations"][done] <= 1).all(), (ainfo["status"], ainfo["iterations"])
    worst = 0.0
    for s in np.nonzero(done)[0]:
        # an accepted step has max_k w_k |delta_k| < precision; the parameters are floats, so half a step of each on top
        a, b = info["p"][s], ainfo["p"][s]
        bound = qr.PRECISION / qr.weights(int(info["n_points"][s])) + np.spacing(np.abs(a))
        move = np.abs(b.astype(np.float64) - a.astype(np.float64))
        assert (move < bound).all(), (s, move, bound)
        worst = max(worst, float((move / bound).max()))
    print(f"largest move / bound {worst:.3g}")


# ---- 4. a sector alone is the sector in the full set ---------------------------------------------------------------------------
def test_batch_independence_and_modes(pair, clean_run):
    rec, info, sums, seeds = clean_run["rec"], clean_run["info"], clean_run["sums"], clean_run["seeds"]
    idx = KINDS + [qr.RING]
    with make_engine(*pair, [qr.RECTS[k] for k in KINDS]) as e:
        r, i, q = e.refine_quadratic(guesses=seeds[idx], return_sums=True)
        for k, s in enumerate(idx):
            assert r[k].tobytes() == rec[s].tobytes() and i[k].tobytes() == info[s].tobytes() and q[k].tobytes() == sums[s].tobytes(), s
    with make_engine(*pair) as e:
        def same():
            r, i, q = e.refine_quadratic(guesses=seeds, return_sums=True)
            assert r.tobytes() == rec.tobytes() and i.tobytes() == info.tobytes() and q.tobytes() == sums.tobytes()

        same()
        e.set_reference_order(1)
        same()
        held = e.correlate_all(seeds)
        same()
        # records as seeds: those given and those held give the same bytes
        a, b = e.refine_quadratic(), e.refine_quadratic(records=held)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        e.set_reference_order(0)
        same()


# ---- 5. the engine's model says how seeds are read and records written -------------------------------------------------------------
@pytest.mark.parametrize("model", [ca.FM_U, ca.FM_UV, ca.FM_UVQ])
def test_engine_models(pair, model):
    P = _ffi.N_PARAMS[model]
    rects = [qr.RECTS[k] for k in (25 + 12, 50 + 12)]      # the centre squares of sides 31 and 49
    with make_engine(*pair, rects, model=model, annular=()) as e:
        n = e.n_sectors
        g = np.tile(np.float32([1.25, -0.65, 0.004, 7.0, np.nan, np.inf]), (n, 1))   # (behind P: not read)
        want = np.zeros(12, np.float32)
        want[:min(P, 2)] = g[0, :min(P, 2)]
        if model == ca.FM_UVQ:
            want[3], want[4] = -g[0, 2], g[0, 2]
        rec, info = e.refine_quadratic(guesses=g, max_iters=0)
        for s in range(n):
            assert info["status"][s] == ca.ZN_MAX_ITERS and info["p"][s].tobytes() == want.tobytes(), (s, info[s])
            assert rec["p"][s][:P].tobytes() == g[s][:P].tobytes() and not rec["p"][s][P:].any(), (s, rec[s])
        # the same seed through an affine engine: the same twelve parameters, so the same sums
        with make_engine(*pair, rects, annular=()) as full:
            ga = np.tile(want[:6], (n, 1))
            sums_a = full.refine_quadratic(guesses=ga, max_iters=0, return_sums=True)[2]
        assert e.refine_quadratic(guesses=g, max_iters=0, return_sums=True)[2].tobytes() == sums_a.tobytes()
        # refined: the record carries the model's own parameters of the twelve in the info
        g[:, :2] = qr.true_translation_seeds([e.sector_info(s)[1:3] for s in range(n)])[0][:, :2]
        g[:, 2] = 0.0
        rec, info = e.refine_quadratic(guesses=g)
        assert (info["status"] == ca.ZN_CONVERGED).all(), info["status"]
        p = info["p"]
        layout = {ca.FM_U: [p[:, 0]], ca.FM_UV: [p[:, 0], p[:, 1]], ca.FM_UVQ: [p[:, 0], p[:, 1], (p[:, 4] - p[:, 3]) * np.float32(0.5)]}[model]
        for k in range(6):
            want_k = layout[k] if k < P else np.zeros(n, np.float32)
            assert rec["p"][:, k].tobytes() == np.ascontiguousarray(want_k, np.float32).tobytes(), (k, rec["p"], p)
        assert np.abs(p[:, 6:]).max() > 1e-4        # (whatever the engine's model, all twelve parameters are refined)
        # records as seeds read the same layout
        back, binfo = e.refine_quadratic(records=rec, second=p[:, 6:], max_iters=0)
        assert back["p"].tobytes() == rec["p"].tobytes() or model == ca.FM_UVQ
        if model == ca.FM_UVQ:
            q = rec["p"][:, 2]
            assert binfo["p"][:, 3].tobytes() == (-q).tobytes() and binfo["p"][:, 4].tobytes() == q.tobytes()
        assert binfo["p"][:, 6:].tobytes() == np.ascontiguousarray(p[:, 6:]).tobytes()


# ---- 6. statuses; nothing of the engine moves --------------------------------------------------------------------------------------
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


def test_statuses_and_engine_state(pair):
    und, dfm = (a.copy() for a in pair)
    und[100:140, 100:140] = 128            # a constant patch of the undeformed image only
    dfm[150:200, 20:70] = 90               # a constant patch of the deformed image only
    rects = [(8, 8, 28, 28), (108, 108, 128, 128), (30, 160, 50, 180), (52, 8, 72, 28), (74, 8, 94, 28), (96, 8, 116, 28), (118, 8, 138, 28)]
    thirteen = np.float32([(200 + k % 5, 20 + k // 5) for k in range(13)])
    n = len(rects) + 1
    with make_engine(und, dfm, rects, annular=(), points=[thirteen]) as e:
        centres = [e.sector_info(s)[1:3] for s in range(n)]
        assert [e.sector_info(s)[0] for s in range(n)] == [441] * 7 + [13]
        g = qr.true_translation_seeds(centres)[0]
        g2 = np.zeros((n, 6), np.float32)
        g[3, 0] = 1000.0                   # leaves the image
        g[4, 4] = np.nan
        g2[5, 2] = np.inf                  # a second-order seed that is not finite
        rec, info, sums = e.refine_quadratic(guesses=g, second=g2, return_sums=True)
        assert info["status"].tolist() == [ca.ZN_CONVERGED, ca.ZN_FLAT, ca.ZN_FLAT, ca.ZN_OUT_OF_IMAGE, ca.ZN_BAD_SEED, ca.ZN_BAD_SEED,
                                           ca.ZN_CONVERGED, ca.ZN_TOO_FEW], info["status"]
        assert rec["error_code"].tolist() == [0, _ffi.ERROR_SOLVER, _ffi.ERROR_SOLVER, ca.ERROR_INTERPOLATION_OUT_OF_IMAGE, ca.ERROR_BAD_DOMAIN,
                                              ca.ERROR_BAD_DOMAIN, 0, _ffi.ERROR_SOLVER]
        assert info["n_points"].tolist() == [441] * 7 + [13] and not info["reserved"].any()
        for s in (1, 2, 3, 4, 5, 7):
            assert not any(info[k][s] for k in FLOATS) and info["iterations"][s] == 0, (s, info[s])
            assert rec["p"][s].tobytes() == g[s].tobytes() and rec["iterations"][s] == 0, (s, rec[s])
        for s in (3, 4, 5):
            assert not info["p"][s].any() and not sums[s].any(), (s, info[s])
        assert info["evaluations"].tolist() == [info["evaluations"][0], 1, 1, 1, 0, 0, info["evaluations"][6], 1]
        assert sums[1][0] == 128.0 * 441 and abs(sums[2][1] - 90.0 * 441) < 0.01 and sums[7][0] > 0   # the seed's sums of the refused
        # records as seeds: a bad record passes through, byte for byte
        seeds = np.zeros(n, ca.RESULT_DTYPE)
        seeds["p"][:] = g
        seeds["p"][3:5] = seeds["p"][0]
        seeds["chi"] = 1.0
        seeds["error_code"][0] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        seeds["iterations"][0] = 50
        seeds["p"][6, 1] = np.inf
        seeds["chi"][3] = 5.0
        out, oi = e.refine_quadratic(records=seeds, second=g2, chi_max=2.0)
        assert oi["status"][[0, 3, 5, 6]].tolist() == [ca.ZN_BAD_SEED] * 4 and oi["status"][[1, 2, 7]].tolist() == [ca.ZN_FLAT, ca.ZN_FLAT, ca.ZN_TOO_FEW]
        for s in (0, 3, 6):
            assert out[s].tobytes() == seeds[s].tobytes() and not any(oi[k][s] for k in FLOATS) and oi["evaluations"][s] == 0, s
        assert out[5]["error_code"] == ca.ERROR_BAD_DOMAIN and out[5]["p"].tobytes() == seeds[5]["p"].tobytes()   # the second-order seed
        assert e.refine_quadratic(records=seeds)[1]["status"][3] != ca.ZN_BAD_SEED    # chi_max <= 0: the error code alone
        # one trip from a seed 2 px off: MAX_ITERS, and the record is the better of the two states
        g = qr.true_translation_seeds(centres)[0]
        g[:, 0] += 2.0
        one, oi = e.refine_quadratic(guesses=g, max_iters=1)
        zero, zi = e.refine_quadratic(guesses=g, max_iters=0)
        for s in (0, 6):
            assert oi["status"][s] == ca.ZN_MAX_ITERS and one["error_code"][s] == ca.ERROR_CORRELATION_MAX_ITERS_REACHED
            assert (oi["iterations"][s], oi["evaluations"][s], one["iterations"][s]) == (1, 2, 1)
            assert oi["zncc_seed"][s] == zi["zncc"][s]
            if oi["shift"][s] > 0:           # the trial state was accepted: it is the better one
                assert oi["znssd"][s] < zi["znssd"][s] and one["p"][s].tobytes() != g[s].tobytes()
            else:
                assert oi["znssd"][s] == zi["znssd"][s] and one["p"][s].tobytes() == g[s].tobytes()
        assert (oi["shift"][[0, 6]] > 0).any()
    # nothing of the engine moves: the held records and guesses, and the next solve
    with make_engine(*pair) as e, make_engine(*pair) as plain:
        seeds = clean_seeds = qr.true_translation_seeds([e.sector_info(s)[1:3] for s in range(S)])[0]
        first = e.correlate_all(seeds)
        plain.correlate_all(seeds)
        e.synchronize()
        e.stats()   # (the solve's event times are read when the counters are: read them once before they are compared)
        kept = dict(records=device_records(e), guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(),
                    counters=np.array(sorted(e.stats().items()), dtype=object))
        a = e.refine_quadratic()
        b = e.refine_quadratic(records=first)
        e.refine_quadratic(guesses=clean_seeds)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        after = dict(records=device_records(e), guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(),
                     counters=np.array(sorted(e.stats().items()), dtype=object))
        for k in kept:
            if k == "counters":
                assert kept[k].tolist() == after[k].tolist(), [(a, b) for a, b in zip(kept[k].tolist(), after[k].tolist()) if a != b]
            else:
                assert kept[k].tobytes() == after[k].tobytes(), k
        assert e.correlate_all(seeds).tobytes() == plain.correlate_all(seeds).tobytes()


# ---- 7. arguments and refusals -------------------------------------------------------------------------------------------------------
def test_arguments_and_refusals(pair):
    rects = qr.RECTS[:9]
    e = make_engine(*pair, rects, annular=(), commit=False)
    lib, h = e.lib, e._h
    seeds = np.zeros(9, ca.RESULT_DTYPE)
    g = np.tile(NEAR[:6], (9, 1))
    seeds["p"][:] = g
    rec = np.full(9, 7, np.uint8).repeat(48).view(ca.RESULT_DTYPE)
    info = np.full(9, 7, np.uint8).repeat(128).view(ca.QUADRATIC_DTYPE)
    sums = np.full((9, ca.QD_SUMS), 7.0)
    kept = [rec.tobytes(), info.tobytes(), sums.tobytes()]

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def config(**kw):
        fields = dict(def_slot=-1, chi_max=0.0, max_iters=-1, precision=0.0, lambda0=0.0)
        fields.update(kw)
        return _ffi.LkQuadraticConfig(**fields)

    def refused(cfg="default", records=None, guesses=None, outputs=(rec, info), word=None, **kw):
        if cfg == "default":
            cfg = config(**kw)
        if word is not None:
            cfg.reserved[word] = 1
        rc = lib.lk_refine_quadratic(h, C.byref(cfg) if cfg is not None else None, ptr(records), _ffi.fptr(guesses) if guesses is not None else None,
                                     None, ptr(outputs[0]), ptr(outputs[1]), ptr(sums))
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and msg.startswith("lk_refine_quadratic: "), (rc, msg)   # names the function called
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
    assert lib.lk_refine_quadratic(None, C.byref(config()), None, _ffi.fptr(g), None, ptr(rec), ptr(info), None) == ca.ERROR_BAD_DOMAIN
    assert [rec.tobytes(), info.tobytes(), sums.tobytes()] == kept       # every refusal left the outputs as they were
    # either output alone; guesses and records need no solve; the defaults of the C configuration are lk_config's
    cfg = config()
    assert lib.lk_refine_quadratic(h, C.byref(cfg), None, _ffi.fptr(g), None, ptr(rec), None, None) == 0
    assert lib.lk_refine_quadratic(h, C.byref(cfg), ptr(seeds), None, None, None, ptr(info), None) == 0
    both = e.refine_quadratic(guesses=g, max_iters=50, precision=1e-3, lambda0=1e-3)
    assert rec.tobytes() == both[0].tobytes() and info.tobytes() == both[1].tobytes()
    # a solve in flight refuses the engine-held records and finishes normally afterwards
    e.correlate_all_async()
    assert "waited for" in refused()
    solved = e.wait_results()
    assert e.refine_quadratic()[0].tobytes() == e.refine_quadratic(records=solved)[0].tobytes()
    e.close()
    bare = make_engine(None, None, rects, annular=())
    rc = bare.lib.lk_refine_quadratic(bare._h, C.byref(config()), None, _ffi.fptr(g), None, ptr(rec), ptr(info), None)
    msg = bare.lib.lk_last_error_string(bare._h).decode()
    assert rc == ca.ERROR_BAD_DOMAIN and "image" in msg and msg.startswith("lk_refine_quadratic: "), (rc, msg)
    bare.close()
