"""Per-sector uncertainty on the GPU (lk_parameter_uncertainty, include/lk_engine.h): the 28 sums of a solved batch against
the oracle's per-sample values, the records against the host function and the numpy restatement, batch independence, the
status cases, the consistency experiment, the modes, that nothing of the engine moves, and the arguments.

Sums: per entry |device - float64 sum of the restated products| <= 64 n 2^-53 sum|terms| - the device and the restatement
differ only in the order of double sums.  The per-sample floats are the oracle's (model_point, interpolate_many; float32
products and sum for J); for LK_IM_BICUBIC_SEPARABLE, which the oracle has no sampler for, the value and gradient come
from lk_sample - the forward solve's own sampler in its stand-alone kernel - and everything else from the oracle.

Consistency: R_gpu = std(u) / mean(sigma_u) of the experiment of test_uncertainty_host.py solved by the engine, within
5 % of the oracle's recorded R = 1.3388 (uncertainty_ref.R_ORACLE)."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi, speckle

import uncertainty_ref as ur

pytestmark = pytest.mark.gpu

TRUTH = (1.3, -0.7, 0.002, 0.0, 0.0, -0.001)
MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
# every lane group and both list kinds: 16 lanes (n <= 512), a wavefront (<= 8192), a 512-thread workgroup (above); no n is
# a multiple of its group (361 = 22 * 16 + 9, 49, 899 = 14 * 64 + 3, 10000 = 19 * 512 + 272)
RECTS = [(8, 8, 26, 26), (40, 8, 46, 14), (8, 60, 38, 88), (140, 140, 239, 239)]
ANNULAR = [(20.0, 12.0, 0.3, 0.9, 70.0, 190.0, 6)]
GROUPS = [16, 16, 64, 512]


@pytest.fixture(scope="module")
def pair():
    return speckle.speckle_pair(256, 256, p=TRUTH, seed=5)


def make_engine(und, dfm, rects, model=ca.FM_UVUXUYVXVY, annular=(), interp=ca.IM_BICUBIC, py_start=0, commit=True):
    e = ca.HipCorrelationEngine(interpolation=interp, fitting_model=model, precision=ur.EXP_PRECISION, py_start=py_start, py_stop=2)
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


def start_guesses(S):
    g = np.zeros((S, 6), np.float32)
    g[:, :2] = TRUTH[:2]
    return g


def good_record(rec, P):
    return rec["error_code"] == 0 and np.isfinite(rec["chi"]) and np.isfinite(rec["p"][:P]).all()


def check_against_oracle(oracle, e, model, interp, rec, out, sums, level, rects, n_annular, cond_max=1e4, ratios=None):
    """every sector of the engine: status, sums within the bound, the record byte for byte the host function of the device's
    sums and within the restatement's tolerance -> (worst sum error / bound, statuses)"""
    P = _ffi.N_PARAMS[model]
    und, dfm = e.get_pyramid_level(ca.IMG_UND, level), e.get_pyramid_level(ca.IMG_DEF, level)
    sampler = None
    if interp == ca.IM_BICUBIC_SEPARABLE:
        def sampler(pts):
            return e.sample(ca.IMG_DEF, level, pts)
    worst = 0.0
    for s in range(e.n_sectors):
        is_rect = s < len(rects) and rects[s] is not None     # (None in rects: a list sector among the rectangles)
        xy = ur.rect_rows(*ur.rect_level(rects[s], level)) if is_rect else e.level_xy(level, s)
        n = len(xy)
        assert out["n_points"][s] == n and out["reserved"][s] == 0
        if not good_record(rec[s], P):
            want = ca.UNC_BAD_RECORD
        else:
            _, cx, cy = e.sector_info(s)
            scale = np.float32(1.0 / (1 << level))
            p = rec["p"][s].copy()
            p[:2] *= scale
            terms, bad = ur.sample_terms(oracle, interp, model, und, dfm, xy, np.float32(cx) * scale if level else cx,
                                         np.float32(cy) * scale if level else cy, p[:P], sampler)
            want = ca.UNC_OUT_OF_IMAGE if bad else None
        if want is not None:
            assert out["status"][s] == want and not sums[s].any() and not out["sigma"][s].any(), (s, out[s])
            continue
        bound = 64.0 * n * 2.0 ** -53 * np.abs(terms).sum(axis=0)
        err = np.abs(sums[s] - terms.sum(axis=0))
        ratio = float((err[bound > 0] / bound[bound > 0]).max())
        print(f"model {model} interp {interp} level {level} sector {s} (n = {n}): worst sum error / bound {ratio:.3g}")
        assert (err <= bound).all(), (s, err, bound)
        worst = max(worst, ratio)
        if ratios is not None:
            ratios.append((s, ratio))
        assert ca.uncertainty_from_sums(model, n, sums[s], level).tobytes() == out[s].tobytes(), s
        ur.check_record(out[s], model, n, sums[s], level, (model, interp, s), cond_max.get(s, 1e4) if isinstance(cond_max, dict) else cond_max)
    return worst


CASES = [(m, ca.IM_BICUBIC) for m in MODELS] + [(ca.FM_UVUXUYVXVY, ca.IM_BILINEAR), (ca.FM_UVQ, ca.IM_BICUBIC_SEPARABLE)]


@pytest.mark.parametrize("model,interp", CASES)
def test_sums_and_records_of_a_solved_batch(oracle, pair, model, interp):
    with make_engine(*pair, RECTS, model=model, annular=ANNULAR, interp=interp) as e:
        S = e.n_sectors
        assert S == len(RECTS) + len(ANNULAR)
        n0 = [e.sector_info(s)[0] for s in range(S)]
        assert n0[:4] == [361, 49, 899, 10000] and 0 < n0[4] <= 512
        assert all(n % g for n, g in zip(n0, GROUPS))
        rec = e.correlate_all(start_guesses(S))
        out, sums = e.parameter_uncertainty(return_sums=True)
        worst = check_against_oracle(oracle, e, model, interp, rec, out, sums, 0, RECTS, len(ANNULAR))
        print(f"model {model} interp {interp}: worst sum error / bound {worst:.3g}; status {out['status']}, sigma_u {out['sigma'][:, 0]}, "
              f"noise {out['noise']}")
        # records a solve might have given, passed in: every sector is evaluated whatever the solve above made of it
        near = np.zeros(S, ca.RESULT_DTYPE)
        near["p"][:] = np.float32([1.25, -0.65, 0.001, 0.0005, -0.0005, -0.001])
        near["chi"] = 1.0
        out2, sums2 = e.parameter_uncertainty(records=near, return_sums=True)
        assert (out2["status"] == ca.UNC_OK).all(), out2["status"]
        check_against_oracle(oracle, e, model, interp, near, out2, sums2, 0, RECTS, len(ANNULAR))
        # the same call again, and with the records passed in: the same bytes
        again, sums2 = e.parameter_uncertainty(records=rec, return_sums=True)
        assert again.tobytes() == out.tobytes() and sums2.tobytes() == sums.tobytes()
        assert e.parameter_uncertainty().tobytes() == out.tobytes()


@pytest.fixture(scope="module")
def grid_solution(pair):
    """the 12 x 12 grid of 19 x 19 sectors, six parameters, solved once in the default mode"""
    rects = ur.experiment_rects()
    with make_engine(*pair, rects) as e:
        rec = e.correlate_all(start_guesses(len(rects)))
        out, sums = e.parameter_uncertainty(return_sums=True)
    assert (rec["error_code"] == 0).all() and (out["status"] == ca.UNC_OK).all()
    return rects, rec, out, sums


def test_a_sector_alone_is_the_sector_in_the_grid(pair, grid_solution):
    rects, rec, out, sums = grid_solution
    for k in (0, 77, 143):
        with make_engine(*pair, [rects[k]]) as e:
            e.correlate_all(start_guesses(1))
            alone, alone_sums = e.parameter_uncertainty(records=rec[k:k + 1], return_sums=True)
            assert alone[0].tobytes() == out[k].tobytes() and alone_sums[0].tobytes() == sums[k].tobytes(), k


def test_status_cases(pair):
    und, dfm = (a.copy() for a in pair)
    und[100:140, 100:140] = 128            # a textureless patch in both images
    dfm[100:140, 100:140] = 128
    rects = [(8, 8, 26, 26), (60, 60, 61, 61), (110, 110, 128, 128), (30, 8, 48, 26), (52, 8, 70, 26), (74, 8, 92, 26)]
    with make_engine(und, dfm, rects) as e:
        rec = np.zeros(len(rects), ca.RESULT_DTYPE)
        rec["p"][:] = np.float32(TRUTH)
        rec["chi"] = 1.0
        rec["p"][3, 0] = 1000.0
        rec["error_code"][4] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        rec["p"][5, 4] = np.nan
        out, sums = e.parameter_uncertainty(records=rec, return_sums=True)
        assert out["status"].tolist() == [ca.UNC_OK, ca.UNC_TOO_FEW, ca.UNC_SINGULAR, ca.UNC_OUT_OF_IMAGE, ca.UNC_BAD_RECORD,
                                          ca.UNC_BAD_RECORD]
        assert out["n_points"].tolist() == [361, 4, 361, 361, 361, 361]
        for s in range(1, 6):
            assert not out["sigma"][s].any() and not any(out[k][s] for k in ur.FLOATS), (s, out[s])
        assert not sums[3:].any() and sums[1].any()
        A, _, chi = ur.unpack(ca.FM_UVUXUYVXVY, sums[2])
        assert not A.any() and chi == 0    # no gradient anywhere, and equal grey levels
        rec["chi"][0] = np.inf
        assert e.parameter_uncertainty(records=rec)["status"][0] == ca.UNC_BAD_RECORD


def test_one_directional_texture(pair):
    und = np.repeat(pair[0][128:129], 256, axis=0)      # the pair's row 128 in every row: varies in x only
    dfm = np.repeat(pair[1][128:129], 256, axis=0)
    rects = [(30, 30, 48, 48), (100, 60, 130, 88)]
    rec = np.zeros(2, ca.RESULT_DTYPE)
    rec["p"][:, 0] = 1.25
    rec["chi"] = 1.0
    with make_engine(und, dfm, rects, model=ca.FM_UV) as e:
        out, sums = e.parameter_uncertainty(records=rec, return_sums=True)
        assert (out["status"] == ca.UNC_SINGULAR).all() and not out["sigma"].any()
        assert (sums[:, 0] > 0).all() and not sums[:, 1:3].any()         # A00 > 0, A01 = A11 = 0 exactly
    with make_engine(und, dfm, rects, model=ca.FM_U) as e:
        as_u, sums_u = e.parameter_uncertainty(records=rec, return_sums=True)
        assert (as_u["status"] == ca.UNC_OK).all() and (as_u["sigma"][:, 0] > 0).all()
        assert (as_u["sigma_major"] == as_u["sigma"][:, 0]).all() and not as_u["rho_uv"].any() and not as_u["sigma_minor"].any()
        assert np.array_equal(sums_u[:, 0], sums[:, 0]) and np.array_equal(sums_u[:, 2], sums[:, 5])   # A00 and chi: the same samples
        for s in range(2):
            ur.check_record(as_u[s], ca.FM_U, int(as_u["n_points"][s]), sums_u[s], 0, ("x only", s))


def test_predicted_sigma_matches_the_oracles_experiment():
    und, dfm = ur.experiment_pair()
    rects = ur.experiment_rects()
    with make_engine(und, dfm, rects, model=ca.FM_UV) as e:
        rec = e.correlate_all(np.zeros((len(rects), 6), np.float32))
        out = e.parameter_uncertainty()
    assert (rec["error_code"] == 0).all() and (out["status"] == ca.UNC_OK).all()
    R = float(np.std(rec["p"][:, 0].astype(np.float64)) / np.mean(out["sigma"][:, 0].astype(np.float64)))
    print(f"R_gpu = {R:.4f} (oracle {ur.R_ORACLE}); std(u) = {rec['p'][:, 0].std():.5f} px, mean sigma_u = {out['sigma'][:, 0].mean():.5f} px, "
          f"noise {out['noise'].mean():.3f} grey levels (two images of {ur.EXP_NOISE}: {ur.EXP_NOISE * 2 ** 0.5:.3f})")
    assert abs(R - ur.R_ORACLE) <= 0.05 * ur.R_ORACLE, (R, ur.R_ORACLE)


def test_modes_and_the_ring_slot_give_the_same_bytes(pair, grid_solution):
    rects, rec, out, sums = grid_solution
    with make_engine(*pair, rects) as e:
        assert e.parameter_uncertainty(records=rec).tobytes() == out.tobytes()
        e.set_batch_invariant(True)
        assert e.parameter_uncertainty(records=rec).tobytes() == out.tobytes()
        e.set_batch_invariant(False)
        e.set_update(ca.UPDATE_BACKWARD)
        assert e.parameter_uncertainty(records=rec).tobytes() == out.tobytes()
        e.correlate_all(start_guesses(len(rects)))      # (the pass evaluates forward behind a backward solve as well)
        got, got_sums = e.parameter_uncertainty(records=rec, return_sums=True)
        assert got.tobytes() == out.tobytes() and got_sums.tobytes() == sums.tobytes()
        e.set_update(ca.UPDATE_FORWARD)
        e.set_reference_order(1)
        assert e.parameter_uncertainty(records=rec).tobytes() == out.tobytes()
        held = e.correlate_all(start_guesses(len(rects)))
        assert e.parameter_uncertainty().tobytes() == e.parameter_uncertainty(records=held).tobytes()
        e.set_reference_order(0)
        e.sequence_reserve(2)
        e.sequence_set_frame(0, pair[1])
        e.sequence_set_frame(1, pair[0])
        assert e.parameter_uncertainty(records=rec, def_slot=0).tobytes() == out.tobytes()
        assert e.parameter_uncertainty(records=rec, def_slot=1).tobytes() != out.tobytes()


def test_py_start_one_is_evaluated_at_level_one(oracle, pair):
    rects = [RECTS[0], RECTS[2]]
    with make_engine(*pair, rects, model=ca.FM_UVUXUYVXVY, py_start=1) as e:
        rec = e.correlate_all(start_guesses(2))
        assert (rec["error_code"] == 0).all()
        out, sums = e.parameter_uncertainty(return_sums=True)
        assert (out["status"] == ca.UNC_OK).all() and out["n_points"].tolist() == [10 * 10, 16 * 15]
        check_against_oracle(oracle, e, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, rec, out, sums, 1, rects, 0)


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
    rects = ur.experiment_rects()[:64]
    S = len(rects)
    g = start_guesses(S)
    g[[9, 27], 0] = 300.0

    def solve_and_repair(e):
        first = e.correlate_all(g)
        e.reseed_failed(1.5 * ur.EXP_SIDE)
        return first

    with make_engine(*pair, rects) as e, make_engine(*pair, rects) as plain:
        first = solve_and_repair(e)
        solve_and_repair(plain)

        def state():
            return dict(records=device_records(e), guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(),
                        stats=e.sector_stats(), reseed=e.reseed_info(), strain=e.strain_field(2.5 * ur.EXP_SIDE),
                        counters=np.array(sorted(e.stats().items()), dtype=object))

        kept = state()
        a = e.parameter_uncertainty()
        b, _ = e.parameter_uncertainty(records=first, return_sums=True)
        c = e.parameter_uncertainty()
        assert a.tobytes() == c.tobytes()
        assert (b["status"][[9, 27]] == ca.UNC_BAD_RECORD).all()
        after = state()
        for k in kept:
            if k == "counters":
                assert (kept[k] == after[k]).all()
            else:
                assert kept[k].tobytes() == after[k].tobytes(), k
        # the next solve is the one an engine gives that never made the call
        assert e.correlate_all(start_guesses(S)).tobytes() == plain.correlate_all(start_guesses(S)).tobytes()
        assert e.last_evaluated_parameters().tobytes() == plain.last_evaluated_parameters().tobytes()


def test_arguments_and_refusals(pair):
    rects = ur.experiment_rects()[:9]
    e = make_engine(*pair, rects, commit=False)
    lib, h = e.lib, e._h
    cfg = _ffi.LkUncertaintyConfig(-1, 0)
    out = np.zeros(9, ca.UNCERTAINTY_DTYPE)
    rec = np.zeros(9, ca.RESULT_DTYPE)
    rec["chi"] = 1.0

    def refused(c=cfg, records=None, output=out, engine=None):
        rc = lib.lk_parameter_uncertainty(engine or h, C.byref(c) if c is not None else None,
                                          records.ctypes.data_as(C.c_void_p) if records is not None else None,
                                          output.ctypes.data_as(C.c_void_p) if output is not None else None, None)
        msg = lib.lk_last_error_string(engine or h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and "lk_parameter_uncertainty" in msg, (rc, msg)
        return msg

    assert "no committed sectors" in refused()
    assert "no committed sectors" in refused(records=rec)
    e.commit_sectors()
    assert "no solve" in refused()                            # records == NULL before any batch solve
    assert "configuration" in refused(None, records=rec)
    assert "output" in refused(records=rec, output=None)
    assert "ring slot" in refused(_ffi.LkUncertaintyConfig(0, 0), records=rec)     # no ring reserved
    assert "def_slot" in refused(_ffi.LkUncertaintyConfig(-2, 0), records=rec)
    assert lib.lk_parameter_uncertainty(None, C.byref(cfg), None, out.ctypes.data_as(C.c_void_p), None) == ca.ERROR_BAD_DOMAIN
    e.sequence_reserve(1)
    assert "image" in refused(_ffi.LkUncertaintyConfig(0, 0), records=rec)         # a slot that holds no frame
    # records passed in need no solve; a solve in flight refuses records == NULL and finishes normally afterwards
    got = e.parameter_uncertainty(records=rec)
    assert (got["status"] == ca.UNC_OK).all()
    e.correlate_all_async()
    assert "waited for" in refused()
    solved = e.wait_results()
    assert e.parameter_uncertainty().tobytes() == e.parameter_uncertainty(records=solved).tobytes()
    e.close()
    bare = make_engine(None, None, rects)
    assert "image" in refused(records=rec, engine=bare._h)
    bare.close()
