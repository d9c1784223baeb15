"""Every compiled (model, interpolator, lane group) instance of the kernels a lane group runs per sector - the backward solve
and its evaluation (lk_backward.hip), uncertainty, photometry, the ZNSSD, the weighted, the spline and the composed
refinement - against its reference, on one geometry (pass_instances_ref.py) that puts a sector on either side of both thresholds of lk_bw_group, gives
every group an implicit rectangle and a list, and holds a sector smaller than a row of lanes.

Which instance ran is asserted, not assumed: the backward launches through lk_get_launch_report (roles LK_LAUNCH_BACKWARD and
LK_LAUNCH_BACKWARD_EVAL), the passes through the level-0 counts of the sectors and the (16, 64, 512) split of the *_last()
hooks.  The references: backward_ref.py (the oracle alone; the engine's lk_sample for the separable bicubic, which the oracle
lacks), and the checkers of test_uncertainty_gpu.py, test_residual_gpu.py, test_znssd_gpu.py, test_weighted_gpu.py and
test_composed_gpu.py with their bounds as they are.  profiles/pass_instances.txt (tests/tools/pass_instances_report.py) has the measured figures."""
import numpy as np
import pytest

import correlation_amd as ca

import backward_ref as br
import frame_shapes_ref as fs
import composed_ref as cr
import pass_instances_ref as pi
import weighted_ref as wr
import znssd_ref as zr

pytestmark = pytest.mark.gpu

UNCERTAINTY = fs.module("test_uncertainty_gpu")   # check_against_oracle
RESIDUAL = fs.module("test_residual_gpu")         # check_photometry
ZNSSD = fs.module("test_znssd_gpu")               # check_seed_evaluation, check_fixed_point
WEIGHTED = fs.module("test_weighted_gpu")         # check_seed_evaluation, check_fixed_point
COMPOSED = fs.module("test_composed_gpu")         # device_sampler, check_seed_evaluation, check_fixed_point
S = pi.N_SECTORS
F32 = np.float32
THREADS = {16: 256, 64: 256, 512: 512}            # sector_group_threads<G>()
PER_BLOCK = {16: 16, 64: 4, 512: 1}
cases = pytest.mark.parametrize("case", pi.CASES, ids=pi.case_id)


@pytest.fixture(scope="module")
def pair():
    return zr.pair()


def engine_sampler(e, interp):
    if interp != ca.IM_BICUBIC_SEPARABLE:
        return None
    return lambda slot, level, pts: e.sample(slot, level, pts)


def level_sampler(e, interp, level=0):
    """the `sampler` of znssd_ref.sample_floats: the deformed image of one level"""
    if interp != ca.IM_BICUBIC_SEPARABLE:
        return None
    return lambda pts: e.sample(ca.IMG_DEF, level, pts)


def backward_record(model, interp, group, role, threads, sectors, grid):
    return dict(model=model, interp=interp, group=group, threads=threads, flavour=ca.FLAVOUR_SAFE, seq=0, role=role, sectors=sectors,
                team_w=0, persistent=0, grid=grid)


def near_records():
    rec = np.zeros(S, ca.RESULT_DTYPE)
    rec["p"][:] = pi.NEAR
    rec["chi"] = 1.0
    return rec


# ---- a. the backward evaluation ------------------------------------------------------------------------------------------------
@cases
def test_backward_evaluation(oracle, pair, case):
    """lk_evaluate_backward of every sector at the levels 0, 1 and 2 against backward_ref within close()'s bounds (rtol 2e-5,
    atol 1e-3; atol 1e-2 for chi: test_one_evaluation_against_numpy's); the error code is the restatement's; no NaN, the
    3 x 3 sector (4 samples at level 1, one at level 2) included; every call reports its one instance"""
    model, interp = case
    n = br.P[model]
    groups = pi.groups()
    with pi.make_engine(*pair, model, interp) as e:
        centres = pi.check_engine_geometry(e)
        problems = pi.backward_problems(oracle, model, interp, *pair, sampler=engine_sampler(e, interp), centres_=centres)
        worst = {g: 0.0 for g in (16, 64, 512)}
        for s in range(S):
            for level in (0, 1, 2):
                ref = problems[s].sector(level)
                pl = pi.NEAR.copy()
                pl[n:] = 0
                pl[:min(n, 2)] *= F32(1.0 / (1 << level))
                H, b, chi, err = e.evaluate_backward(s, level, pl[:n])
                report = e.launch_report()
                assert report == [backward_record(model, interp, groups[s], ca.LAUNCH_BACKWARD_EVAL, groups[s], 1, 1)], (s, level, report)
                pi.SEEN.add(("backward eval", model, interp, report[0]["group"]))
                b_ref, chi_ref, bad = ref.evaluate(pl)
                assert err == (ca.ERROR_INTERPOLATION_OUT_OF_IMAGE if (bad or ref.tbad) else ca.ERROR_NONE), (s, level, err)
                assert err == ca.ERROR_NONE, (s, level)      # (the geometry keeps every sample inside at every level)
                assert np.isfinite(H).all() and np.isfinite(b).all() and np.isfinite(chi), (s, level, H, b, chi)
                assert not H[n:].any() and not H[:, n:].any() and not b[n:].any(), (s, level)
                assert br.close(H[:n, :n], ref.H), (s, level, H[:n, :n], ref.H)
                assert br.close(b[:n], b_ref), (s, level, b[:n], b_ref)
                assert br.close(chi, chi_ref, atol=1e-2), (s, level, chi, chi_ref)
                for got, want, atol in ((H[:n, :n], ref.H, 1e-3), (b[:n], b_ref, 1e-3), (chi, chi_ref, 1e-2)):
                    want = np.asarray(want, np.float64)
                    dev = np.abs(np.asarray(got, np.float64) - want).max() / (2e-5 * max(np.abs(want).max(), 1.0) + atol)
                    worst[groups[s]] = max(worst[groups[s]], float(dev))
        print(f"{pi.case_id(case)}: worst deviation / bound per group {worst}")
        for G, w in worst.items():
            pi.MEASURED["backward eval", model, interp, G] = w


# ---- b. backward whole solves --------------------------------------------------------------------------------------------------
@cases
def test_backward_whole_solves(oracle, pair, case):
    """correlate_all in backward mode against backward_ref's loop with test_whole_solves_against_restatement's bounds, on the
    sectors the restatement's float64 and float32 runs settle (backward_ref.settled); an unsettled sector is held to the
    restatement evaluated at the kernel's own parameters.  pass_instances_ref.BW_PY and backward_guesses say why the solves
    start near the answer and run two levels.  One LK_LAUNCH_BACKWARD record per group, in the order 16, 64, 512; a sector
    alone gives the batch's bytes.

    The 3 x 3 sector is starved at both levels under six parameters (9 and 4 samples for 2 P = 12): the kernel takes the
    reference's float32 QR there, and so does the restatement (backward_ref.solve_ref's step).  With a float64 solve in its
    place the restatement is 1.4e-5 px and 1.1e-5 (gradient terms, allowed 1e-6) from the kernel on that sector with the
    bicubic sampler - the first run of this test found that."""
    model, interp = case
    n = br.P[model]
    groups = pi.groups()
    g = pi.backward_guesses(interp)
    with pi.make_engine(*pair, model, interp, py_stop=pi.BW_PY[2]) as e:
        centres = pi.check_engine_geometry(e)
        e.set_update(ca.UPDATE_BACKWARD)
        got = e.correlate_all(g)
        report = e.launch_report()
        want_report = [backward_record(model, interp, G, ca.LAUNCH_BACKWARD, THREADS[G], k, -(-k // PER_BLOCK[G]))
                       for G, k in zip((16, 64, 512), pi.count3())]
        assert report == want_report, report
        assert pi.count3() == (4, 2, 2)
        pi.SEEN.update(("backward solve", model, interp, r["group"]) for r in report)
        missed = []
        measured = {G: dict(duv=0.0, rest=0.0, chi=0.0, settled=0, sectors=0, it_diff=0) for G in (16, 64, 512)}
        problems = pi.backward_problems(oracle, model, interp, *pair, sampler=engine_sampler(e, interp), centres_=centres)
        r64, r32, settled = pi.backward_runs(problems, model, interp)
        unsettled = [s for s in range(S) if not settled[s]]
        print(f"{pi.case_id(case)}: unsettled sectors {unsettled}; iterations kernel {got['iterations'].tolist()} restatement "
              f"{[r[2] for r in r64]}")
        assert len(unsettled) <= pi.UNSETTLED_CAP[interp], unsettled
        for s in range(S):
            p, chi, it, err = r64[s]
            r = got[s]
            m = measured[groups[s]]
            m["sectors"] += 1
            m["settled"] += int(settled[s])
            m["it_diff"] += int(r["iterations"] != it)
            if settled[s]:
                assert r["error_code"] == err, (s, r, err)
                assert abs(int(r["iterations"]) - it) <= 1, (s, r["iterations"], it)
                if err == ca.ERROR_NONE:
                    duv = np.abs(r["p"][:min(n, 2)] - p[:min(n, 2)]).max()
                    drest = np.abs(r["p"][2:n] - p[2:n]).max() if n > 2 else 0.0
                    dchi = abs(r["chi"] - chi) / (5e-5 * abs(chi) + 1e-6)
                    print(f"   sector {s} (group {groups[s]}): |d(u, v)| {duv:.2e} of 1e-4, rest {drest:.2e} of 1e-6, chi {dchi:.3f} of its bound")
                    m.update(duv=max(m["duv"], float(duv)), rest=max(m["rest"], float(drest)), chi=max(m["chi"], float(dchi)))
                    if not (duv < br.BOUND_UV and drest < br.BOUND_REST and abs(r["chi"] - chi) <= 5e-5 * abs(chi) + 1e-6):
                        missed.append((s, float(duv), float(drest), float(dchi), r["p"], p))    # (asserted below, behind the figures)
            else:
                assert r["error_code"] in (err, r32[s][3]), (s, r, err, r32[s][3])
                if r["error_code"] == ca.ERROR_NONE:
                    # the record's chi against the restatement evaluated at the returned parameters, within (a)'s bound for chi
                    ref = problems[s].sector(0)
                    chi_ref = ref.evaluate(r["p"])[1]
                    assert br.close(float(r["chi"]) * ref.n, chi_ref, atol=1e-2), (s, r, chi_ref / ref.n)
        for G in measured:
            pi.MEASURED["backward solve", model, interp, G] = measured[G]
        # the sectors one at a time: the batch's bytes, and each call reports its own group
        for s in range(S):
            one, _ = e.correlate(s, g[s])
            assert one.tobytes() == got[s].tobytes(), s
            assert e.launch_report() == [backward_record(model, interp, groups[s], ca.LAUNCH_BACKWARD, THREADS[groups[s]], 1, 1)], s
        assert not missed, missed     # |d(u, v)| < 1e-4, the other parameters within 1e-6, chi within 5e-5 relative + 1e-6


@cases
def test_backward_three_levels_from_zero(oracle, pair, case):
    """The issue's own input - a zero guess, the levels 2, 1 and 0 - on the sectors the restatement settles from it (no cap
    here: the run above carries it): the same bounds.  This is the run that takes every group through level 2 and the
    hand-over from level to level.

    A sector enters when it settles and every level of it holds at least as many samples as the model has parameters.  The
    3 x 3 sector has one sample at level 2: with two or more parameters its system there has rank one, and what a pivoted QR
    returns for it is decided by the rounding of the pivot search, not by the data - the kernel's QR and the oracle's agree on
    the iteration counts there and leave 4.5e-6 px and 2.0e-6 (rotation, three parameters, bicubic; bound 1e-6) of difference
    in the record.  The two-level run above keeps that sector, at levels of nine and four samples."""
    model, interp = case
    n = br.P[model]
    zero = np.zeros((S, 6), F32)
    with pi.make_engine(*pair, model, interp) as e:
        centres = pi.check_engine_geometry(e)
        e.set_update(ca.UPDATE_BACKWARD)
        got = e.correlate_all(zero)
        problems = pi.backward_problems(oracle, model, interp, *pair, sampler=engine_sampler(e, interp), centres_=centres)
        r64, _, settled = pi.backward_runs(problems, model, interp, guesses=zero, py=(0, 1, 2))
        print(f"{pi.case_id(case)}: settled from zero over three levels {[s for s in range(S) if settled[s]]}; iterations kernel "
              f"{got['iterations'].tolist()} restatement {[r[2] for r in r64]}")
        full_rank = [all(len(l) >= n for l in pb.lists) for pb in problems]
        compared = [s for s in range(S) if settled[s] and full_rank[s]]
        pi.MEASURED["three levels settled", model, interp, 0] = compared
        assert {pi.groups()[s] for s in compared} == {16, 64, 512}, compared     # (every lane group is still compared)
        for s in compared:
            p, chi, it, err = r64[s]
            r = got[s]
            assert r["error_code"] == err, (s, r, err)
            assert abs(int(r["iterations"]) - it) <= 1, (s, r["iterations"], it)
            if err == ca.ERROR_NONE:
                assert np.abs(r["p"][:min(n, 2)] - p[:min(n, 2)]).max() < br.BOUND_UV, (s, r["p"], p)
                assert n <= 2 or np.abs(r["p"][2:n] - p[2:n]).max() < br.BOUND_REST, (s, r["p"], p)
                assert abs(r["chi"] - chi) <= 5e-5 * abs(chi) + 1e-6, (s, r["chi"], chi)


# ---- c. uncertainty and photometry ---------------------------------------------------------------------------------------------
@cases
def test_uncertainty_and_photometry(oracle, pair, case):
    """check_against_oracle and check_photometry, with their bounds (64 n 2^-53 sum|terms| on the double sums; the record
    byte for byte the host function of the device's sums), at records near the truth: every sector is evaluated"""
    model, interp = case
    with pi.make_engine(*pair, model, interp) as e:
        pi.check_engine_geometry(e)
        e.correlate_all(pi.truth_seeds())
        near, ratios = near_records(), []
        out, sums = e.parameter_uncertainty(records=near, return_sums=True)
        # (the 3 x 3 sector has 9 samples for up to 6 parameters: its matrix may be as badly conditioned as it likes - the
        # tolerance of uncertainty_ref.check_record grows with the condition number)
        worst = UNCERTAINTY.check_against_oracle(oracle, e, model, interp, near, out, sums, 0, pi.RECTS, 0, cond_max={pi.TINY: 1e12},
                                                  ratios=ratios)
        pi.note("uncertainty", case, ratios)
        photo, psums = e.photometry(records=near, return_sums=True)
        assert (photo["status"] == ca.PHOTO_OK).all(), photo["status"]
        ratios = []
        pworst = RESIDUAL.check_photometry(oracle, e, model, interp, near, photo, psums, 0, pi.RECTS, ratios=ratios)
        pi.note("photometry", case, ratios)
        print(f"{pi.case_id(case)}: uncertainty worst sum error / bound {worst:.3g}, status {out['status']}; photometry {pworst:.3g}")


# ---- d. the ZNSSD and the weighted refinement ------------------------------------------------------------------------------------
def converged_as_demanded(interp, info, tiny_status):
    """bilinear, bicubic and separable: every sector but the 3 x 3 one converges, and that one carries `tiny_status` where the
    restatement's criterion refuses it; nearest: no status is demanded"""
    if interp == ca.IM_NEAREST:
        return
    rest = [s for s in range(S) if s != pi.TINY]
    assert (info["status"][rest] == ca.ZN_CONVERGED).all(), info["status"]
    if tiny_status:
        assert info["status"][pi.TINY] == tiny_status, info["status"]


def tiny_refusal(model, lists, centres, info, sums, sigma, mask, order=1):
    """the status weighted_ref's (order 2: composed_ref's) criterion gives the 3 x 3 sector at its returned sums, or 0"""
    xy, (cx, cy) = lists[pi.TINY], centres[pi.TINY]
    w = wr.sample_weights(xy, cx, cy, wr.inv_of(sigma) if sigma > 0 else 0.0, mask)
    n_valid, N = int(info["n_valid"][pi.TINY]), wr.device_sum(w.astype(np.float64), wr.group_of(len(xy)))
    assert n_valid == int((w > 0).sum())
    return cr.criterion(n_valid, N, sums[pi.TINY])[0] if order == 2 else wr.criterion(model, n_valid, N, sums[pi.TINY])[0]


@cases
def test_znssd(oracle, pair, case):
    model, interp = case
    und, dfm = pair
    lists = pi.lists()
    with pi.make_engine(und, dfm, model, interp) as e:
        centres = pi.check_engine_geometry(e)
        sampler = level_sampler(e, interp)
        g = np.tile(pi.NEAR, (S, 1))
        ratios = []
        ZNSSD.check_seed_evaluation(oracle, e, und, dfm, model, interp, lists, centres, g, sampler, ratios, allow_refused=True)
        pi.note("znssd sums", case, ratios)
        assert e.znssd_last()[1] == pi.count3() == (4, 2, 2)
        rec, info, sums = e.refine_znssd(guesses=pi.truth_seeds(), return_sums=True)
        assert e.znssd_last()[1] == pi.count3()
        print(f"{pi.case_id(case)}: status {info['status'].tolist()} trips {info['iterations'].tolist()}")
        tiny = zr.criterion(model, len(lists[pi.TINY]), sums[pi.TINY])[0]
        converged_as_demanded(interp, info, tiny)
        worst = ZNSSD.check_fixed_point(oracle, und, dfm, model, interp, lists, centres, rec, info, sums, sampler)
        print(f"   largest weighted step of the restatement at the returned state {worst:.3g} (allowed {4.0 * zr.PRECISION:.3g})")
        pi.MEASURED["znssd fixed point", model, interp, 0] = worst / (4.0 * zr.PRECISION)


@cases
def test_weighted(oracle, pair, case):
    model, interp = case
    und, dfm = pair
    lists = pi.lists()
    mask = pi.weighted_mask()
    with pi.make_engine(und, dfm, model, interp) as e:
        centres = pi.check_engine_geometry(e)
        sampler = level_sampler(e, interp)
        g, ratios = np.tile(pi.NEAR, (S, 1)), []
        cut = WEIGHTED.check_seed_evaluation(oracle, e, und, dfm, model, interp, lists, centres, g, pi.SIGMA, mask, sampler, ratios,
                                              allow_refused=True)
        pi.note("weighted sums", case, ratios)
        assert cut >= 2 * 10 * 64 + 10 * 96       # the band of the 8192- and the 8193-sample sector, and that of the 9216-sample one
        assert e.weighted_last()[1] == pi.count3() == (4, 2, 2)
        rec, info, sums = e.refine_weighted(guesses=pi.truth_seeds(), sigma=pi.SIGMA, mask=mask, return_sums=True)
        assert e.weighted_last()[1] == pi.count3()
        print(f"{pi.case_id(case)}: status {info['status'].tolist()} trips {info['iterations'].tolist()}")
        converged_as_demanded(interp, info, tiny_refusal(model, lists, centres, info, sums, pi.SIGMA, mask))
        worst = WEIGHTED.check_fixed_point(oracle, und, dfm, model, interp, lists, centres, rec, info, sums, pi.SIGMA, mask, sampler)
        print(f"   largest weighted step of the restatement at the returned state {worst:.3g} (allowed {4.0 * zr.PRECISION:.3g})")
        pi.MEASURED["weighted fixed point", model, interp, 0] = worst / (4.0 * zr.PRECISION)


# ---- e. the spline and the composed refinement ---------------------------------------------------------------------------------------
SPLINE_CASES = [(m, order) for m in pi.MODELS for order in (3, 5)]            # x 3 groups: the 24 instances of lk_spline_kernel
SECOND_CASES = [(i, 0) for i in pi.INTERPS] + [(ca.IM_BICUBIC, 3), (ca.IM_BICUBIC, 5)]   # x 3 groups: lk_composed_second_kernel's 18


@pytest.mark.parametrize("model,order", SPLINE_CASES, ids=lambda v: str(v))
def test_spline(oracle, pair, model, order):
    """lk_refine_spline: test_znssd's content with the per-sample floats taken through the pass's own sampler (lk_spline_sample,
    pinned against spline_ref by test_spline_gpu.py) - the engine's interpolator plays no part, so the models cross the orders"""
    und, dfm = pair
    lists = pi.lists()
    with pi.make_engine(und, dfm, model, ca.IM_BICUBIC) as e:
        centres = pi.check_engine_geometry(e)
        sampler = COMPOSED.device_sampler(e, order)
        g, ratios = np.tile(pi.NEAR, (S, 1)), []
        ZNSSD.check_seed_evaluation(oracle, e, und, dfm, model, ca.IM_BICUBIC, lists, centres, g, sampler, ratios,
                                    refine=lambda **kw: e.refine_spline(order=order, **kw), allow_refused=True)
        pi.note("spline sums", (model, order), ratios)
        assert e.spline_last()[1] == pi.count3() == (4, 2, 2)
        rec, info, sums = e.refine_spline(guesses=pi.truth_seeds(), order=order, return_sums=True)
        assert e.spline_last()[1] == pi.count3()
        print(f"{pi.MODEL_NAME[model]} order {order}: status {info['status'].tolist()} trips {info['iterations'].tolist()}")
        converged_as_demanded(ca.IM_BICUBIC, info, zr.criterion(model, len(lists[pi.TINY]), sums[pi.TINY])[0])
        worst = ZNSSD.check_fixed_point(oracle, und, dfm, model, ca.IM_BICUBIC, lists, centres, rec, info, sums, sampler)
        pi.MEASURED["spline fixed point", model, order, 0] = worst / (4.0 * zr.PRECISION)


def composed_case(oracle, pair, model, interp, order, sampler, what):
    """test_weighted's content for lk_refine_composed under (order, sampler), the mask and the Gaussian window"""
    und, dfm = pair
    lists, mask = pi.lists(), pi.weighted_mask()
    with pi.make_engine(und, dfm, model, interp) as e:
        centres = pi.check_engine_geometry(e)
        g, ratios = np.tile(pi.NEAR, (S, 1)), []
        second = np.tile(COMPOSED.SECOND, (S, 1)) if order == 2 else None
        cut = COMPOSED.check_seed_evaluation(oracle, e, und, dfm, model, interp, order, sampler, lists, centres, g, second, pi.SIGMA, mask,
                                             ratios, allow_refused=True)
        pi.note(what + " sums", (model if order == 1 else interp, sampler), ratios)
        assert cut >= 2 * 10 * 64 + 10 * 96
        assert e.composed_last()[1] == pi.count3() == (4, 2, 2)
        rec, info, sums = e.refine_composed(guesses=pi.truth_seeds(), order=order, sampler=sampler, sigma=pi.SIGMA, mask=mask, return_sums=True)
        assert e.composed_last()[1] == pi.count3()
        print(f"{what} {pi.MODEL_NAME[model]} {pi.INTERP_NAME[interp]} sampler {sampler}: status {info['status'].tolist()} trips "
              f"{info['iterations'].tolist()}")
        converged_as_demanded(interp if not sampler else ca.IM_BICUBIC, info, tiny_refusal(model, lists, centres, info, sums, pi.SIGMA, mask, order))
        worst = COMPOSED.check_fixed_point(oracle, e, und, dfm, model, interp, order, sampler, lists, centres, rec, info, sums, pi.SIGMA, mask)
        pi.MEASURED[what + " fixed point", model if order == 1 else interp, sampler, 0] = worst / (4.0 * zr.PRECISION)


@pytest.mark.parametrize("model,sampler", SPLINE_CASES, ids=lambda v: str(v))
def test_composed_first(oracle, pair, model, sampler):
    """lk_composed_first_kernel: the engine's model under a spline sampler - 4 models x samplers {3, 5} x 3 groups = 24"""
    composed_case(oracle, pair, model, ca.IM_BICUBIC, 1, sampler, "composed first")


@pytest.mark.parametrize("interp,sampler", SECOND_CASES, ids=lambda v: str(v))
def test_composed_second(oracle, pair, interp, sampler):
    """lk_composed_second_kernel: twelve parameters under the four interpolators and the two splines x 3 groups = 18 (the
    kernel has no model template: the six-parameter engine seeds it)"""
    composed_case(oracle, pair, ca.FM_UVUXUYVXVY, interp, 2, sampler, "composed second")
