"""Photometry and the back-warped residual map on the GPU (lk_photometry, lk_residual_map, include/lk_engine.h): the eight
sums of a batch against the oracle's per-sample floats, the records against the host function and the numpy restatement,
batch independence, the modes, the statuses, the lighting identities; the maps of several windows against the oracle bit for
bit, the agreement of map and photometry, the owner rule with bad records and on a dense domain that overflows the LDS
staging, the output pointers, that nothing of the engine moves, and the arguments.

Sums: per sum |device - float64 sum of the restated terms| <= 64 n 2^-53 sum|terms| - device and restatement differ only in
the order of double additions.  The per-sample floats are the oracle's (model_point, interpolate_many); for
LK_IM_BICUBIC_SEPARABLE, which the oracle has no sampler for, the value comes from lk_sample - the solve's own sampler in its
stand-alone kernel - and everything else from the oracle."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi, speckle

import residual_ref as rr
import uncertainty_ref as ur

pytestmark = pytest.mark.gpu

TRUTH = (1.3, -0.7, 0.002, 0.0, 0.0, -0.001)
MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
# the sectors of test_uncertainty_gpu.py: every lane group and both list kinds, no n a multiple of its group
RECTS = [(8, 8, 26, 26), (40, 8, 46, 14), (8, 60, 38, 88), (140, 140, 239, 239)]
ANNULAR = [(20.0, 12.0, 0.3, 0.9, 70.0, 190.0, 6)]
GROUPS = [16, 16, 64, 512]
NEAR = np.float32([1.25, -0.65, 0.001, 0.0005, -0.0005, -0.001])
RADIUS = 15.0


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


def near_records(S):
    rec = np.zeros(S, ca.RESULT_DTYPE)
    rec["p"][:] = NEAR
    rec["chi"] = 1.0
    return rec


def centres(e):
    return np.float32([e.sector_info(s)[1:3] for s in range(e.n_sectors)])


def sampler_of(e, interp, level):
    if interp != ca.IM_BICUBIC_SEPARABLE:
        return None
    return lambda pts: e.sample(ca.IMG_DEF, level, pts) if len(pts) else np.zeros((0, 4), np.float32)


def check_photometry(oracle, e, model, interp, rec, out, sums, level, rects, chi_max=0.0, ratios=None):
    """every sector of the engine: status, the six sums within the bound, the flagged count, max |V| exactly, the record byte
    for byte the host function of the device's sums and within the restatement's tolerance -> worst sum error / bound"""
    P = _ffi.N_PARAMS[model]
    und, dfm = e.get_pyramid_level(ca.IMG_UND, level), e.get_pyramid_level(ca.IMG_DEF, level)
    good = rr.good_records(rec, model, chi_max)
    worst = 0.0
    for s in range(e.n_sectors):
        is_rect = s < len(rects) and rects[s] is not None     # (None in rects: a list sector among the rectangles)
        xy = ur.rect_rows(*ur.rect_level(rects[s], level)) if is_rect else e.level_xy(level, s)
        n = len(xy)
        assert out["n_points"][s] == n and not out["reserved"][s].any()
        want = None
        if not good[s]:
            want = ca.PHOTO_BAD_RECORD
        else:
            _, cx, cy = e.sector_info(s)
            scale = np.float32(1.0 / (1 << level))
            p = rec["p"][s].copy()
            p[:2] *= scale
            f, g, V, bad = rr.sample_values(oracle, interp, model, und, dfm, xy, np.float32(cx) * scale if level else cx,
                                            np.float32(cy) * scale if level else cy, p[:P], sampler_of(e, interp, level))
            if bad:
                want = ca.PHOTO_OUT_OF_IMAGE
        if want is not None:
            assert out["status"][s] == want and not sums[s].any() and not any(out[k][s] for k in rr.FLOATS), (s, out[s])
            continue
        terms = rr.sum_terms(f, g, V)
        bound = 64.0 * n * 2.0 ** -53 * np.abs(terms).sum(axis=0)
        err = np.abs(sums[s][:6] - terms.sum(axis=0))
        ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        print(f"model {model} interp {interp} level {level} sector {s} (n = {n}): worst sum error / bound {ratio:.3g}; "
              f"zncc {out['zncc'][s]:.6f} gain {out['gain'][s]:.5f} offset {out['offset'][s]:.4f} rms {out['rms'][s]:.4f} "
              f"rms_zn {out['rms_zn'][s]:.4f}")
        assert (err <= bound).all(), (s, err, bound)
        assert sums[s][6] == 0.0 and sums[s][7] == float(np.abs(V).max()), (s, sums[s][6:], np.abs(V).max())
        worst = max(worst, ratio)
        if ratios is not None:
            ratios.append((s, ratio))
        assert ca.photometry_from_sums(n, sums[s]).tobytes() == out[s].tobytes(), s
        rr.check_record(out[s], f, g, V, sums[s], (model, interp, s))
    return worst


CASES = [(m, ca.IM_BICUBIC) for m in MODELS] + [(ca.FM_UVUXUYVXVY, ca.IM_BILINEAR), (ca.FM_UVQ, ca.IM_BICUBIC_SEPARABLE)]


@pytest.mark.parametrize("model,interp", CASES)
def test_photometry_sums_and_records(oracle, pair, model, interp):
    with make_engine(*pair, RECTS, model=model, annular=ANNULAR, interp=interp) as e:
        S = e.n_sectors
        n0 = [e.sector_info(s)[0] for s in range(S)]
        assert n0[:4] == [361, 49, 899, 10000] and 0 < n0[4] <= 512
        assert all(n % g for n, g in zip(n0, GROUPS))
        rec = e.correlate_all(start_guesses(S))
        out, sums = e.photometry(return_sums=True)
        worst = check_photometry(oracle, e, model, interp, rec, out, sums, 0, RECTS)
        print(f"model {model} interp {interp}: worst sum error / bound {worst:.3g}; status {out['status']}")
        # records a solve might have given, passed in: every sector is evaluated whatever the solve above made of it
        near = near_records(S)
        out2, sums2 = e.photometry(records=near, return_sums=True)
        assert (out2["status"] == ca.PHOTO_OK).all(), out2["status"]
        check_photometry(oracle, e, model, interp, near, out2, sums2, 0, RECTS)
        # the same call again, and with the records passed in: the same bytes
        again, sums3 = e.photometry(records=rec, return_sums=True)
        assert again.tobytes() == out.tobytes() and sums3.tobytes() == sums.tobytes()
        assert e.photometry().tobytes() == out.tobytes()


@pytest.fixture(scope="module")
def grid(pair):
    """the 12 x 12 grid of 19 x 19 sectors, six parameters, solved once in the default mode, with its photometry and its
    whole-image maps at radius 15"""
    rects = ur.experiment_rects()
    with make_engine(*pair, rects) as e:
        rec = e.correlate_all(start_guesses(len(rects)))
        out, sums = e.photometry(return_sums=True)
        maps = e.residual_map(RADIUS)
        last = e.residual_last()
        cen = centres(e)
    assert (rec["error_code"] == 0).all() and (out["status"] == ca.PHOTO_OK).all()
    return dict(rects=rects, rec=rec, out=out, sums=sums, maps=maps, last=last, centres=cen)


def test_a_sector_alone_is_the_sector_in_the_grid(pair, grid):
    for k in (0, 77, 143):
        with make_engine(*pair, [grid["rects"][k]]) as e:
            alone, alone_sums = e.photometry(records=grid["rec"][k:k + 1], return_sums=True)
            assert alone[0].tobytes() == grid["out"][k].tobytes() and alone_sums[0].tobytes() == grid["sums"][k].tobytes(), k


def test_modes_and_the_ring_slot_give_the_same_bytes(pair, grid):
    rects, rec, out, sums = grid["rects"], grid["rec"], grid["out"], grid["sums"]
    window = (30, 40, 67, 21)
    with make_engine(*pair, rects) as e:
        maps = e.residual_map(RADIUS, window, records=rec)

        def same():
            got, got_sums = e.photometry(records=rec, return_sums=True)
            assert got.tobytes() == out.tobytes() and got_sums.tobytes() == sums.tobytes()
            for a, b in zip(e.residual_map(RADIUS, window, records=rec), maps):
                assert a.tobytes() == b.tobytes()

        same()
        e.set_batch_invariant(True)
        same()
        e.set_batch_invariant(False)
        e.set_update(ca.UPDATE_BACKWARD)
        same()
        e.correlate_all(start_guesses(len(rects)))
        same()
        e.set_update(ca.UPDATE_FORWARD)
        e.set_reference_order(1)
        same()
        held = e.correlate_all(start_guesses(len(rects)))
        assert e.photometry().tobytes() == e.photometry(records=held).tobytes()
        for a, b in zip(e.residual_map(RADIUS, window), e.residual_map(RADIUS, window, records=held)):
            assert a.tobytes() == b.tobytes()
        e.set_reference_order(0)
        e.sequence_reserve(2)
        e.sequence_set_frame(0, pair[1])
        e.sequence_set_frame(1, pair[0])
        assert e.photometry(records=rec, def_slot=0).tobytes() == out.tobytes()
        assert e.photometry(records=rec, def_slot=1).tobytes() != out.tobytes()
        for a, b in zip(e.residual_map(RADIUS, window, records=rec, def_slot=0), maps):
            assert a.tobytes() == b.tobytes()
        assert e.residual_map(RADIUS, window, records=rec, def_slot=1)[0].tobytes() != maps[0].tobytes()
    # the whole-image maps of the fixture hold the window
    x0, y0, w, h = window
    for a, b in zip(grid["maps"], maps):
        assert a[y0:y0 + h, x0:x0 + w].tobytes() == b.tobytes()


def test_statuses(pair):
    und, dfm = (a.copy() for a in pair)
    und[100:140, 100:140] = 128            # a constant patch of the undeformed image only
    rects = [(8, 8, 26, 26), (110, 110, 128, 128), (30, 8, 48, 26), (52, 8, 70, 26), (74, 8, 92, 26), (96, 8, 114, 26)]
    with make_engine(und, dfm, rects) as e:
        rec = near_records(len(rects))
        rec["p"][2, 0] = 1000.0
        rec["error_code"][3] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        rec["p"][4, 4] = np.nan
        rec["chi"][5] = 5.0
        out, sums = e.photometry(records=rec, return_sums=True)
        assert out["status"].tolist() == [ca.PHOTO_OK, ca.PHOTO_FLAT, ca.PHOTO_OUT_OF_IMAGE, ca.PHOTO_BAD_RECORD, ca.PHOTO_BAD_RECORD,
                                          ca.PHOTO_OK]
        assert (out["n_points"] == 361).all() and not out["reserved"].any()
        for s in (2, 3, 4):
            assert not sums[s].any() and not any(out[k][s] for k in rr.FLOATS), (s, out[s])
        flat = out[1]
        assert flat["mean_f"] == 128.0 and flat["std_f"] == 0.0 and flat["std_g"] > 0 and flat["rms"] > 0 and flat["max_abs"] > 0
        assert not any(flat[k] for k in ("zncc", "gain", "offset", "rms_zn", "znssd"))
        assert ca.photometry_from_sums(361, sums[1]).tobytes() == flat.tobytes()
        # the shared good rule's chi_max
        out = e.photometry(records=rec, chi_max=2.0)
        assert out["status"].tolist()[5] == ca.PHOTO_BAD_RECORD and out["status"][0] == ca.PHOTO_OK
        rec["chi"][0] = np.inf
        assert e.photometry(records=rec)["status"][0] == ca.PHOTO_BAD_RECORD


def test_lighting_changes_rms_but_not_zncc(pair):
    und, dfm = pair
    d, d2 = rr.lighting_frames(dfm)
    rec = near_records(len(RECTS))
    with make_engine(und, d, RECTS) as e:
        a = e.photometry(records=rec)
        e.set_deformed_image(d2)
        b = e.photometry(records=rec)
    assert (a["status"] == ca.PHOTO_OK).all() and (b["status"] == ca.PHOTO_OK).all()
    for s in range(len(RECTS)):
        for k, (left, right) in rr.lighting_sides(a[s], b[s]).items():
            diff, tol = abs(float(left) - float(right)), rr.lighting_tol(k, right)
            print(f"sector {s} {k}: {float(left):.8g} against {float(right):.8g}, difference {diff:.3g} (allowed {tol:.3g})")
            assert diff <= tol, (s, k, left, right, diff, tol)
        print(f"sector {s}: rms {a['rms'][s]:.4f} -> {b['rms'][s]:.4f}, rms_zn {a['rms_zn'][s]:.4f} -> {b['rms_zn'][s]:.4f}")
        assert b["rms"][s] > a["rms"][s] and b["rms"][s] > b["rms_zn"][s]


# ---- the map ---------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_map(oracle, e, model, interp, rec, window, level=0, radius=RADIUS, chi_max=0.0):
    """the three maps of a window against the oracle: owner exactly (the flagged pixels included), warped and residual bit
    for bit where a value is specified, NaN exactly elsewhere -> the device's maps"""
    und, dfm = e.get_pyramid_level(ca.IMG_UND, level), e.get_pyramid_level(ca.IMG_DEF, level)
    good = rr.good_records(rec, model, chi_max)
    want_w, want_r, want_o = rr.oracle_map(oracle, interp, model, und, dfm, centres(e), rec, good, radius, window, level,
                                           sampler_of(e, interp, level))
    got_w, got_r, got_o = e.residual_map(radius, window, records=rec, chi_max=chi_max)
    assert got_o.shape == (window[3], window[2])
    assert np.array_equal(got_o, want_o), np.argwhere(got_o != want_o)[:8]
    m = want_o >= 0
    assert np.array_equal(np.isnan(got_w), ~m) and np.array_equal(np.isnan(got_r), ~m)
    assert np.array_equal(bits(got_w)[m], bits(want_w)[m])
    assert np.array_equal(bits(got_r)[m], bits(want_r)[m])
    print(f"model {model} interp {interp} level {level} window {window}: {int(m.sum())} owned, {int((want_o == -1).sum())} ownerless, "
          f"{int((want_o < -1).sum())} outside the deformed image; tiles, fall-back tiles {e.residual_last()[1:]}")
    return got_w, got_r, got_o


def test_map_windows_against_the_oracle(oracle, pair, grid):
    rects, rec = grid["rects"], grid["rec"]
    with make_engine(*pair, rects) as e:
        _, _, o = check_map(oracle, e, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, rec, (30, 40, 67, 21))
        assert (o >= 0).all() and e.residual_last()[1:] == (3 * 3, 0)
        check_map(oracle, e, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, rec, (100, 100, 1, 1))
        # the image corner, with parameters that carry part of it out of the deformed image
        out = rec.copy()
        out["p"][:, 0] = -20.0
        _, _, o = check_map(oracle, e, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, out, (0, 0, 40, 24))
        assert (o < -1).any() and (o >= 0).any() and (o == -1).any()
        # a band that reaches past the grid into ownerless pixels
        _, _, o = check_map(oracle, e, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, rec, (200, 100, 56, 9))
        assert (o == -1).any() and (o >= 0).any()
        # the engine-held records are the fixture's: the same maps without passing them
        e.correlate_all(start_guesses(len(rects)))
        for a, b in zip(e.residual_map(RADIUS, (30, 40, 67, 21)), e.residual_map(RADIUS, (30, 40, 67, 21), records=rec)):
            assert a.tobytes() == b.tobytes()


def test_map_at_py_start_one(oracle, pair):
    rects = ur.experiment_rects()
    with make_engine(*pair, rects, py_start=1) as e:
        rec = e.correlate_all(start_guesses(len(rects)))
        _, _, o = check_map(oracle, e, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, rec, (5, 7, 33, 17), level=1)
        assert (o >= 0).any()
        whole = e.residual_map(RADIUS)
        assert whole[0].shape == (128, 128) and whole[2][7:24, 5:38].tobytes() == o.tobytes()


@pytest.mark.parametrize("model,interp", [(ca.FM_U, ca.IM_BICUBIC), (ca.FM_UVQ, ca.IM_BICUBIC), (ca.FM_UVQ, ca.IM_BICUBIC_SEPARABLE),
                                          (ca.FM_UV, ca.IM_BILINEAR)])
def test_map_of_the_other_models(oracle, pair, model, interp):
    rects = ur.experiment_rects()
    with make_engine(*pair, rects, model=model, interp=interp) as e:
        rec = near_records(len(rects))     # (whatever a one-parameter solve makes of this pair: every sector takes part)
        _, _, o = check_map(oracle, e, model, interp, rec, (195, 60, 45, 13))
        assert (o >= 0).any() and (o == -1).any()


def test_map_and_photometry_agree(grid):
    warped, residual, owner = grid["maps"]
    assert grid["last"][2] == 0 and grid["last"][1] == 8 * 32
    for s, (x0, y0, x1, y1) in enumerate(grid["rects"]):
        assert (owner[y0:y1 + 1, x0:x1 + 1] == s).all(), s         # every sample of the sector is owned by it
        r = residual[y0:y1 + 1, x0:x1 + 1].astype(np.float64).ravel()
        n = r.size
        total = float((r * r).sum())
        assert abs(total - grid["sums"][s][5]) <= 64.0 * n * 2.0 ** -53 * total, (s, total, grid["sums"][s][5])
        assert np.float32(np.abs(r).max()) == grid["out"]["max_abs"][s], s


def decode(owner):
    return np.where(owner < -1, -2 - owner, owner)


def test_owner_rule_with_bad_records_and_on_a_dense_domain(pair, grid):
    rec = grid["rec"].copy()
    rec["error_code"][::3] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
    good = rr.good_records(rec, ca.FM_UVUXUYVXVY)
    with make_engine(*pair, grid["rects"]) as e:
        owner = e.residual_map(RADIUS, (0, 0, 256, 80), records=rec, want=("owner",))[2]
        ms, tiles, fallback = e.residual_last()
        assert (tiles, fallback) == (8 * 10, 0)
        want = rr.brute_owner(grid["centres"], good, RADIUS, 0, 0, 256, 80)
        assert np.array_equal(decode(owner), want)
        assert not np.isin(owner[owner >= 0], np.arange(0, 144, 3)).any()       # a bad sector owns nothing
        assert (want[17, 8:27] != 0).all() and (want[17:27, 8:27] > 0).any()     # sector 0's pixels: a neighbour's, or nobody's
    # 24 x 24 sectors of 7 x 7 at a pitch of one pixel: the cells a tile reaches hold all 576, more than the LDS staging takes
    rects = [(100 + i, 100 + j, 106 + i, 106 + j) for i in range(24) for j in range(24)]
    rec = near_records(len(rects))
    rec["error_code"][::3] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
    good = rr.good_records(rec, ca.FM_UVUXUYVXVY)
    with make_engine(*pair, rects) as e:
        window = (80, 80, 140, 70)
        owner = e.residual_map(12.0, window, records=rec, want=("owner",))[2]
        ms, tiles, fallback = e.residual_last()
        print(f"dense domain: {tiles} tiles, {fallback} took the fall-back")
        assert tiles == 5 * 9 and 0 < fallback < tiles
        want = rr.brute_owner(centres(e), good, 12.0, *window)
        assert np.array_equal(decode(owner), want)
        assert (want == -1).any() and (want >= 0).any()


def test_omitted_outputs_leave_the_others_unchanged(pair, grid):
    window = (30, 40, 67, 21)
    names = ("warped", "residual", "owner")
    with make_engine(*pair, grid["rects"]) as e:
        full = e.residual_map(RADIUS, window, records=grid["rec"])
        for skip in range(3):
            got = e.residual_map(RADIUS, window, records=grid["rec"], want=tuple(n for i, n in enumerate(names) if i != skip))
            assert got[skip] is None
            for i in range(3):
                if i != skip:
                    assert got[i].tobytes() == full[i].tobytes(), (skip, i)
        only = e.residual_map(RADIUS, window, records=grid["rec"], want=("residual",))
        assert only[0] is None and only[2] is None and only[1].tobytes() == full[1].tobytes()


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
                        uncertainty=e.parameter_uncertainty(), counters=np.array(sorted(e.stats().items()), dtype=object))

        kept = state()
        a = e.photometry()
        b = e.photometry(records=first)
        m1 = e.residual_map(RADIUS, (0, 60, 100, 140))
        m2 = e.residual_map(RADIUS, (0, 60, 100, 140), records=first)
        assert e.photometry().tobytes() == a.tobytes() and e.residual_map(RADIUS, (0, 60, 100, 140))[1].tobytes() == m1[1].tobytes()
        assert (b["status"][[9, 27]] == ca.PHOTO_BAD_RECORD).all()
        assert not np.isin(m2[2], [9, 27]).any()
        after = state()
        for k in kept:
            if k == "counters":
                assert (kept[k] == after[k]).all()
            else:
                assert kept[k].tobytes() == after[k].tobytes(), k
        # the next solve is the one an engine gives that never made the calls
        assert e.correlate_all(start_guesses(S)).tobytes() == plain.correlate_all(start_guesses(S)).tobytes()
        assert e.last_evaluated_parameters().tobytes() == plain.last_evaluated_parameters().tobytes()


def test_arguments_and_refusals(pair):
    rects = ur.experiment_rects()[:9]
    e = make_engine(*pair, rects, commit=False)
    lib, h = e.lib, e._h
    rec = near_records(9)
    out = np.full(9, 7, np.uint8).repeat(64).view(ca.PHOTOMETRY_DTYPE)
    maps = [np.full((4, 4), 7.0, np.float32), np.full((4, 4), 7.0, np.float32), np.full((4, 4), 7, np.int32)]
    kept = [out.tobytes()] + [m.tobytes() for m in maps]

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def photo(cfg=_ffi.LkPhotometryConfig(-1, 0.0), records=None, output=out, word=None):
        if word is not None:
            cfg = _ffi.LkPhotometryConfig(-1, 0.0)
            cfg.reserved[word] = 1
        rc = lib.lk_photometry(h, C.byref(cfg) if cfg is not None else None, ptr(records), ptr(output), None)
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and msg.startswith("lk_photometry: "), (rc, msg)   # names the function called
        return msg

    def mapped(cfg=None, records=None, outputs=maps, **kw):
        if cfg is None:
            fields = dict(def_slot=-1, chi_max=0.0, radius=15.0, x0=2, y0=3, w=4, h=4, reserved=0)
            fields.update(kw)
            cfg = _ffi.LkResidualMapConfig(**fields)
        rc = lib.lk_residual_map(h, C.byref(cfg) if cfg != "none" else None, ptr(records), *[ptr(o) for o in outputs])
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and msg.startswith("lk_residual_map: "), (rc, msg)   # names the function called
        return msg

    assert "no committed sectors" in photo(records=rec) and "no committed sectors" in mapped(records=rec)
    e.commit_sectors()
    assert "no solve" in photo() and "no solve" in mapped()             # records == NULL before any batch solve
    assert "lk_photometry: no configuration" in photo(None, records=rec)
    assert "lk_photometry: no output" in photo(records=rec, output=None)
    assert "reserved" in photo(records=rec, word=0) and "reserved" in photo(records=rec, word=1)
    assert "chi_max" in photo(_ffi.LkPhotometryConfig(-1, np.inf), records=rec)
    assert "ring slot" in photo(_ffi.LkPhotometryConfig(0, 0.0), records=rec)
    assert "def_slot" in photo(_ffi.LkPhotometryConfig(-2, 0.0), records=rec)
    assert "lk_residual_map: no configuration" in mapped("none", records=rec)
    assert "lk_residual_map: no output" in mapped(records=rec, outputs=[None, None, None])
    assert "reserved" in mapped(records=rec, reserved=1)
    for radius in (0.0, -1.0, np.inf, np.nan):
        assert "radius" in mapped(records=rec, radius=radius)
    assert "chi_max" in mapped(records=rec, chi_max=np.nan)
    for window in ((-1, 0, 4, 4), (0, -1, 4, 4), (253, 0, 4, 4), (0, 253, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, 4, -4),
                   (1, 0, 0, 0), (0, 0, 257, 1), (2 ** 31 - 2, 0, 4, 4)):
        assert "window" in mapped(records=rec, **dict(zip(("x0", "y0", "w", "h"), window))), window
    assert "ring slot" in mapped(records=rec, def_slot=0) and "def_slot" in mapped(records=rec, def_slot=-2)
    assert lib.lk_photometry(None, C.byref(_ffi.LkPhotometryConfig(-1, 0.0)), None, ptr(out), None) == ca.ERROR_BAD_DOMAIN
    assert [out.tobytes()] + [m.tobytes() for m in maps] == kept        # every refusal left the outputs as they were
    # records passed in need no solve; a solve in flight refuses records == NULL and finishes normally afterwards
    assert (e.photometry(records=rec)["status"] == ca.PHOTO_OK).all()
    assert e.residual_map(15.0, (2, 3, 4, 4), records=rec)[2].shape == (4, 4)
    e.correlate_all_async()
    assert "waited for" in photo() and "waited for" in mapped()
    solved = e.wait_results()
    assert e.photometry().tobytes() == e.photometry(records=solved).tobytes()
    e.close()
    bare = make_engine(None, None, rects)
    rc = bare.lib.lk_photometry(bare._h, C.byref(_ffi.LkPhotometryConfig(-1, 0.0)), ptr(rec), ptr(out), None)
    msg = bare.lib.lk_last_error_string(bare._h).decode()
    assert rc == ca.ERROR_BAD_DOMAIN and "image" in msg and msg.startswith("lk_photometry: "), (rc, msg)
    bare.close()
