"""Backward update (lk_set_update(LK_UPDATE_BACKWARD), the inverse-compositional LM solve): one evaluation against numpy
float64 sums built from the oracle's levels, decimated lists and sampler (backward_ref.py); whole solves against its numpy
restatement of the loop in include/lk_engine.h; accuracy on a full-size speckle pair against the analytic map and the
forward mode; byte equality of records across batches, single-sector calls, modes and sequence windows; mode rules;
edges."""
import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import backward_ref as br
from backward_ref import P, F32, close  # noqa: F401  (the restatement lives in backward_ref.py, on the oracle alone)

pytestmark = pytest.mark.gpu


def decimate(lib, pts):
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    out = np.zeros_like(pts)
    k = lib.lk_roi_decimate(_ffi.fptr(pts), len(pts), 1, _ffi.fptr(out))
    return out[:k]


def sampler_of(e, interp):
    """the `sampler` of backward_ref.Frames: None where the oracle has the sampler, the engine's lk_sample for the separable
    bicubic extension (test_separable_bicubic_extension pins it)"""
    if interp != ca.IM_BICUBIC_SEPARABLE:
        return None
    return lambda slot, level, pts: e.sample(slot, level, pts)


def rows_sorted(xy):
    xy = np.asarray(xy, F32).reshape(-1, 2)
    return xy[np.lexsort((xy[:, 0], xy[:, 1]))]


def oracle_lists(oracle, domain):
    """the level-0 sample lists of build()'s sectors by the oracle: rect_sector_geometry and rect_points, annular_points,
    blob_points, the registered point lists as they are"""
    if domain == "rect":
        xdim, ydim, cen = oracle.rect_sector_geometry(60.0, 60.0, 451.0, 451.0, 6, 6)
        return [oracle.rect_points(cx - xdim, cy - ydim, cx + xdim, cy + ydim) for cx, cy in cen]
    out = [oracle.annular_points(r0, dr, 0.2 + k * 1.05, 0.9, 256.0, 250.0, 6) for r0, dr in ((45.0, 30.0), (80.0, 35.0)) for k in range(6)]
    ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
    out += [oracle.blob_points(np.stack([c[0] + 40 * np.cos(ang), c[1] + 35 * np.sin(ang)], 1).astype(F32))
            for c in ((100.3, 400.7), (410.2, 405.1), (400.6, 100.4))]
    rng = np.random.default_rng(3)
    out += [(np.array(c) + rng.uniform(-25, 25, (300, 2))).astype(F32)
            for c in ((380.0, 120.0), (120.0, 130.0), (150.0, 60.0), (330.0, 60.0), (460.0, 250.0), (60.0, 250.0))]
    out += [oracle.rect_points(x0, y0, x0 + 50, y0 + 42) for x0, y0 in ((330, 330), (160, 320), (250, 440))]
    return out


def problems_of(oracle, e, pair, model, interp, domain):
    """backward_ref's problem of every sector of build(): the level-0 lists are the oracle's (oracle_lists; the engine's own are
    the same samples), the centres the committed ones; everything an evaluation computes - pyramids, decimated lists, level
    centres, template and samples - is the oracle's.  The engine's own level lists and its host decimation (lk_roi_decimate)
    are cross-checked against the oracle's here."""
    frames = br.Frames(oracle, interp, pair[0], pair[1], sampler=sampler_of(e, interp))
    lists = oracle_lists(oracle, domain)
    assert len(lists) == e.n_sectors
    out = []
    for s in range(e.n_sectors):
        assert np.array_equal(rows_sorted(lists[s]), rows_sorted(e.getUndXY0ToCPU(s))), s
        pb = br.Problem(frames, model, lists[s], e.sector_info(s)[1:3])
        for level in (1, 2):
            assert np.array_equal(decimate(e.lib, pb.lists[level - 1]), pb.lists[level]), (s, level)
            xy = e.level_xy(level, s)
            if len(xy):   # (an implicit rectangle has no list on the device)
                assert np.array_equal(rows_sorted(xy), rows_sorted(pb.lists[level])), (s, level)
        out.append(pb)
    return out


def pair512():
    return ca.speckle.speckle_pair(512, 512, p=(1.3, -0.7, 0.002, 0.001, -0.001, -0.001), seed=5)


def build(pair, model=ca.FM_UVUXUYVXVY, interp=ca.IM_BICUBIC, domain="rect", **cfg):
    e = ca.HipCorrelationEngine(interpolation=interp, fitting_model=model, **cfg)
    e.set_undeformed_image(pair[0])
    e.set_deformed_image(pair[1])
    if domain == "rect":
        e.set_rect_grid(60.0, 60.0, 451.0, 451.0, 6, 6)
    else:  # annular sectors, a blob, point lists, rectangles
        s = 0
        for ring, (r0, dr) in enumerate(((45.0, 30.0), (80.0, 35.0))):
            for k in range(6):
                e.resetPolygon_annular(s, r0, dr, 0.2 + k * 1.05, 0.9, 256.0, 250.0, 6)
                s += 1
        ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
        for c in ((100.3, 400.7), (410.2, 405.1), (400.6, 100.4)):
            e.resetPolygon_blob(s, np.stack([c[0] + 40 * np.cos(ang), c[1] + 35 * np.sin(ang)], 1).astype(F32))
            s += 1
        rng = np.random.default_rng(3)
        for c in ((380.0, 120.0), (120.0, 130.0), (150.0, 60.0), (330.0, 60.0), (460.0, 250.0), (60.0, 250.0)):
            e.set_sector_points(s, (np.array(c) + rng.uniform(-25, 25, (300, 2))).astype(F32))
            s += 1
        for x0, y0 in ((330, 330), (160, 320), (250, 440)):
            e.resetPolygon_rect(s, x0, y0, x0 + 50, y0 + 42)
            s += 1
    e.commit_sectors()
    return e


@pytest.mark.parametrize("domain", ["rect", "mixed"])
@pytest.mark.parametrize("model,interp", [(ca.FM_UVUXUYVXVY, ca.IM_BICUBIC), (ca.FM_UVQ, ca.IM_BICUBIC_SEPARABLE),
                                          (ca.FM_UV, ca.IM_BILINEAR), (ca.FM_U, ca.IM_NEAREST),
                                          (ca.FM_UVUXUYVXVY, ca.IM_BILINEAR)])
def test_one_evaluation_against_numpy(oracle, domain, model, interp):
    pair = pair512()
    e = build(pair, model, interp, domain)
    problems = problems_of(oracle, e, pair, model, interp, domain)
    n = P[model]
    p = np.array([1.1, -0.6, 0.0015, 0.0008, -0.0007, -0.0012], F32)[:n]
    if model == ca.FM_UVQ:
        p[2] = 0.001
    for s in range(e.n_sectors):
        for level in (0, 1, 2):
            ref = problems[s].sector(level)
            scale = F32(1.0 / (1 << level))
            pl = p.copy()
            pl[:min(n, 2)] *= scale
            H, b, chi, err = e.evaluate_backward(s, level, pl)
            b_ref, chi_ref, bad = ref.evaluate(pl)
            assert err == (ca.ERROR_INTERPOLATION_OUT_OF_IMAGE if (bad or ref.tbad) else ca.ERROR_NONE)
            if err:
                continue
            assert close(H[:n, :n], ref.H), (s, level, H[:n, :n], ref.H)
            assert close(b[:n], b_ref), (s, level, b[:n], b_ref)
            assert close(chi, chi_ref, atol=1e-2), (s, level, chi, chi_ref)
            # the forward evaluation's chi at the same parameters: same residuals, another summation order
            _, _, chi_fwd, err_fwd = e.evaluate(s, level, pl)
            assert err_fwd == ca.ERROR_NONE
            assert abs(chi - chi_fwd) <= 2e-5 * abs(chi_fwd) + 1e-3
    e.close()


@pytest.mark.parametrize("domain", ["rect", "mixed"])
@pytest.mark.parametrize("model", [ca.FM_UVUXUYVXVY, ca.FM_UV, ca.FM_UVQ])
def test_whole_solves_against_restatement(oracle, domain, model):
    pair = pair512()
    e = build(pair, model, ca.IM_BICUBIC, domain)
    problems = problems_of(oracle, e, pair, model, ca.IM_BICUBIC, domain)
    e.set_update(ca.UPDATE_BACKWARD)
    S = e.n_sectors
    got = e.correlate_all(np.zeros(6, F32))
    n = P[model]
    it_diff, chi_loose = 0, 0
    for s in range(S):
        p, chi, it, err = br.solve_ref(problems[s], np.zeros(6, F32))
        r = got[s]
        assert r["error_code"] == err, (s, r, err)
        it_diff += int(r["iterations"] != it)
        assert abs(int(r["iterations"]) - it) <= 1, (s, r["iterations"], it)
        if err == ca.ERROR_NONE:
            assert np.abs(r["p"][:2] - p[:2]).max() < 1e-4, (s, r["p"], p)
            if n > 2:
                assert np.abs(r["p"][2:n] - p[2:n]).max() < 1e-6, (s, r["p"], p)
            # (the kernel's chi is a float32 sum over each lane's share of the samples: a few 1e-6 relative from the
            # float64 one, up to ~1e-5 on 4000-sample sectors - the default-mode parity bound, held on most sectors)
            assert abs(r["chi"] - chi) <= 5e-5 * abs(chi) + 1e-6, (s, r["chi"], chi)
            chi_loose += int(abs(r["chi"] - chi) > 1e-5 * abs(chi) + 1e-6)
    assert it_diff <= max(1, S // 100)
    assert chi_loose <= max(2, S // 10), chi_loose
    e.close()


def grid_engine(und, dfm, model=ca.FM_UVUXUYVXVY, grid=(24.0, 24.0, 2023.0, 2023.0, 100, 100), **cfg):
    e = ca.HipCorrelationEngine(fitting_model=model, **cfg)
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    e.set_rect_grid(*grid)
    e.commit_sectors()
    return e


def test_accuracy_full_size_pair():
    truth = (1.3, -0.7, 0.002, 0.0, 0.0, -0.001)
    und, dfm = ca.speckle.speckle_pair(2048, 2048, p=truth, device="cuda")
    e = grid_engine(und, dfm)
    fwd = e.correlate_all(np.zeros(6, F32))
    e.set_update(ca.UPDATE_BACKWARD)
    bwd = e.correlate_all(np.zeros(6, F32))
    st = e.stats()
    assert st["evaluations"] > 0 and st["algorithmic_bytes"] == 40 * st["sample_evaluations"] + 196 * st["evaluations"]
    e.close()
    assert len(bwd) == 10000
    cx, cy = bwd["und_cx"] - 1024.0, bwd["und_cy"] - 1024.0
    u = truth[0] + truth[2] * cx + truth[3] * cy
    v = truth[1] + truth[4] * cx + truth[5] * cy

    def duv(r):
        return np.maximum(np.abs(r["p"][:, 0] - u), np.abs(r["p"][:, 1] - v))

    assert (fwd["error_code"] == 0).all() and (bwd["error_code"] == 0).all()
    # (the forward mode's own distance to the analytic map on these 19 x 19-sample sectors: max 0.059 px, measured)
    assert duv(fwd).max() < 0.1
    # Level 0 alone, from a zero guess: the backward solve recovers every sector (measured max 0.063 px).
    e0 = grid_engine(und, dfm, py_stop=0)
    e0.set_update(ca.UPDATE_BACKWARD)
    b0 = e0.correlate_all(np.zeros(6, F32))
    e0.close()
    assert (b0["error_code"] == 0).all() and duv(b0).max() < 0.1, duv(b0).max()
    # With the pyramid, a few sectors go wrong at the coarsest level: 25 samples for 6 parameters,
    # where the inverse-compositional step - a Jacobian fixed at the template - runs the gradient terms away (0.3 - 1.1
    # against the true 0.002) into a chi minimum of that level, from which the finer levels do not return.  Every sector
    # the full solve gets wrong by more than 0.1 px is such a sector: level 2 alone already leaves it with a gradient
    # term beyond 0.05.
    e2 = grid_engine(und, dfm, py_start=2, py_stop=2)
    e2.set_update(ca.UPDATE_BACKWARD)
    b2 = e2.correlate_all(np.zeros(6, F32))
    e2.close()
    runaway = np.abs(b2["p"][:, 2:]).max(1) > 0.05
    bad = duv(bwd) > 0.1
    assert (runaway[bad]).all(), np.nonzero(bad & ~runaway)
    assert bad.sum() <= 20, bad.sum()   # (measured: 10 of 10 000)
    # elsewhere backward agrees with forward: the two schemes' stationary points on quantised images (measured p99
    # 0.0094 px (u, v), 0.002 (gradient terms))
    keep = ~runaway
    d = np.abs(fwd["p"][keep] - bwd["p"][keep])
    assert duv(bwd)[keep].max() < 0.1
    assert np.quantile(d[:, :2].max(1), 0.99) < 0.015, np.quantile(d[:, :2].max(1), 0.99)
    assert np.quantile(d[:, 2:].max(1), 0.99) < 5e-3, np.quantile(d[:, 2:].max(1), 0.99)


def test_last_evaluated_parameters_follow_the_forward_rule():
    """lk_get_last_evaluated_parameters (the strict-Lagrangian rewarp's input): the last evaluation's parameters in the
    level-0 scale - also for a sector whose first evaluation fails at a coarse level, and one whose template fails below
    py_stop"""
    und, dfm = pair512()
    out = {}
    for mode in (ca.UPDATE_FORWARD, ca.UPDATE_BACKWARD):
        e = ca.HipCorrelationEngine()
        e.set_undeformed_image(und)
        e.set_deformed_image(dfm)
        e.resetPolygon_rect(0, 420, 200, 470, 250)   # guess u = 60: level 2 samples leave the deformed image at once
        e.resetPolygon_rect(1, 200, 200, 250, 250)   # converges
        e.commit_sectors()
        e.set_update(mode)
        g = np.zeros((2, 6), F32)
        g[0, :2] = (60.0, 8.0)
        r = e.correlate_all(g)
        out[mode] = (r, e.last_evaluated_parameters(), e.sector_stats())
        e.close()
    (rf, lf, sf), (rb, lb, sb) = out[ca.UPDATE_FORWARD], out[ca.UPDATE_BACKWARD]
    assert rf[0]["error_code"] == rb[0]["error_code"] == ca.ERROR_INTERPOLATION_OUT_OF_IMAGE
    assert lb[0, :2].tolist() == [60.0, 8.0] and lf[0].tobytes() == lb[0].tobytes()
    assert sb[0].tolist()[:3] == sf[0].tolist()[:3]          # one evaluation, its samples, one point iteration
    assert rb[1]["error_code"] == 0 and np.abs(lb[1] - rb[1]["p"])[:2].max() < 0.05
    # a template that fails below py_stop: a column of level-0 nodes on x = 1 (out of the bicubic's image), which the
    # decimation drops from the coarser levels (odd x)
    e = ca.HipCorrelationEngine()
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    xx, yy = np.meshgrid(np.r_[1.0, np.arange(8.0, 61.0)], np.arange(200.0, 251.0))
    e.set_sector_points(0, np.stack([xx.ravel(), yy.ravel()], 1).astype(F32))
    e.commit_sectors()
    e.set_update(ca.UPDATE_BACKWARD)
    r = e.correlate_all(np.zeros(6, F32))
    last = e.last_evaluated_parameters()
    st = e.sector_stats()
    e.close()
    assert r[0]["error_code"] == ca.ERROR_INTERPOLATION_OUT_OF_IMAGE
    assert st[0][0] > 0   # the coarser levels ran
    # the last evaluation ran at level 1: its (u, v) rescaled to level 0 are the returned ones (the template failure at
    # level 0 returns the level-1 parameters translated the same way)
    assert np.abs(last[0, :2] - r[0]["p"][:2]).max() < 0.5


def test_group_of_three_ranks_equals_the_engine():
    und, dfm = pair512()
    grid = (24.0, 24.0, 487.0, 487.0, 13, 11)
    e = ca.HipCorrelationEngine()
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    e.set_rect_grid(*grid)
    e.commit_sectors()
    e.set_update(ca.UPDATE_BACKWARD)
    rng = np.random.default_rng(4)
    guesses = (rng.standard_normal((143, 6)) * [0.3, 0.3, 1e-3, 1e-3, 1e-3, 1e-3]).astype(F32)
    want = e.correlate_all(guesses)
    e.close()
    g = ca.HipCorrelationGroup([0, 0, 0])
    g.for_each_engine("lk_set_update", ca.UPDATE_BACKWARD)
    g.set_image(ca.IMG_UND, und)
    g.set_image(ca.IMG_DEF, dfm)
    g.set_rect_grid(*grid)
    g.commit_sectors()
    assert g.correlate_all(guesses).tobytes() == want.tobytes()
    g.close()


@pytest.mark.parametrize("deformation", ["eulerian", "strict_lagrangian"])
def test_sequence_run_against_frame_loop(deformation):
    """lk_sequence_run against the lk_sequence_frame loop in backward mode: the same frame_results and report text.  The
    strict Lagrangian description rewarps every frame's sample lists from the backward solve's last evaluated parameters."""
    from correlation_amd import tracker as tk
    frames = ca.speckle.speckle_sequence(256, 256, 5, velocity=(0.9, -0.5), dilation=4e-4, seed=3)
    dm, ref = ((tk.DEF_EULERIAN, tk.REF_FIRST) if deformation == "eulerian"
               else (tk.DEF_STRICT_LAGRANGIAN, tk.REF_PREVIOUS))

    def make():
        e = ca.HipCorrelationEngine()
        e.set_update(ca.UPDATE_BACKWARD)
        t = tk.SequenceTracker(ca.FM_UVUXUYVXVY, tk.DOMAIN_RECT, dm, ref, lib=e.lib)
        t.set_rect_domain(40.0, 44.0, 215.0, 211.0, 127.5, 127.5, 3, 3)
        return e, t

    e, t = make()
    assert tk.run_sequence(e, t, frames) == 4
    want_res, want_rep = t.results(), t.report()
    e.close(), t.close()
    e, t = make()
    e.set_undeformed_image(frames[0])
    for k in range(4):
        if k > 0 and ref == tk.REF_PREVIOUS:
            e.makeUndPyramidFromDef()
        e.set_deformed_image(frames[k + 1])
        tk.sequence_frame(e, t, k, "frame0" if ref == tk.REF_FIRST else f"frame{k}", f"frame{k + 1}")
    got_res, got_rep = t.results(), t.report()
    e.close(), t.close()
    assert got_res.tobytes() == want_res.tobytes()
    assert got_rep == want_rep
    assert (want_res["error_code"] == ca.ERROR_NONE).mean() > 0.9
    assert np.isfinite(want_res["resulting_parameters"]).all()


def test_invariance_of_records():
    pair = pair512()
    e = build(pair, domain="mixed")
    e.set_update(ca.UPDATE_BACKWARD)
    g = np.zeros(6, F32)
    full = e.correlate_all(g)
    # single sectors
    for s in range(e.n_sectors):
        r, _ = e.correlate(s, g)
        assert r.tobytes() == full[s].tobytes(), s
    # batch invariant on / off, several pairs in flight
    e.set_batch_invariant(1)
    assert e.correlate_all(g).tobytes() == full.tobytes()
    e.set_batch_invariant(0)
    e.set_pairs_in_flight(3)
    assert e.correlate_all(g).tobytes() == full.tobytes()
    e.close()
    # a subset of the sectors: the same sectors alone in another engine
    f = build(pair, domain="mixed")
    f.set_update(ca.UPDATE_BACKWARD)
    f.clear_sectors()
    f.resetPolygon_rect(0, 250, 440, 300, 482)
    f.commit_sectors()
    sub = f.correlate_all(g)
    assert sub[0].tobytes() == full[-1].tobytes()
    f.close()


def test_mode_rules_and_switch_back():
    pair = pair512()
    e = build(pair)
    e.set_update(ca.UPDATE_BACKWARD)
    with pytest.raises(ca.LkError) as ex:
        e.set_reference_order(1)
    assert ex.value.code == ca.ERROR_BAD_DOMAIN
    e.set_update(ca.UPDATE_FORWARD)
    e.set_reference_order(1)
    with pytest.raises(ca.LkError) as ex:
        e.set_update(ca.UPDATE_BACKWARD)
    assert ex.value.code == ca.ERROR_BAD_DOMAIN
    with pytest.raises(ca.LkError):
        e.set_update(2)
    e.set_reference_order(0)
    g = np.zeros(6, F32)
    e.set_update(ca.UPDATE_BACKWARD)
    bwd = e.correlate_all(g)
    e.set_update(ca.UPDATE_FORWARD)
    again = e.correlate_all(g)
    fresh = build(pair)
    assert again.tobytes() == fresh.correlate_all(g).tobytes()
    assert bwd.tobytes() != again.tobytes()
    e.close()
    fresh.close()


def test_sequence_window_against_pair_loop():
    frames = ca.speckle.speckle_sequence(256, 256, 9, velocity=(0.7, -0.4), dilation=3e-4, seed=3)
    grid = (24.0, 24.0, 231.0, 231.0, 4, 4)
    e = grid_engine(frames[0], frames[1], grid=grid)
    e.set_update(ca.UPDATE_BACKWARD)
    e.sequence_reserve(8)
    for i in range(8):
        e.sequence_set_frame(i, frames[i + 1])
    e.adjust_initial_guess(0, True, np.zeros(6, F32), (127.5, 127.5))
    win = e.correlate_sequence(8)
    assert not e.sequence_is_pipelined
    f = grid_engine(frames[0], frames[1], grid=grid)
    f.set_update(ca.UPDATE_BACKWARD)
    for k in range(8):
        f.set_deformed_image(frames[k + 1])
        f.adjust_initial_guess(k, True, np.zeros(6, F32), (127.5, 127.5))
        r = f.correlate_all()
        assert r.tobytes() == win[k].tobytes(), k
    e.close()
    f.close()


def test_edges_border_and_textureless():
    und, dfm = pair512()
    e = ca.HipCorrelationEngine()
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    e.resetPolygon_rect(0, 0, 100, 30, 140)        # touches the left border: the template's nodes leave the image
    e.resetPolygon_rect(1, 200, 200, 250, 250)
    e.commit_sectors()
    e.set_update(ca.UPDATE_BACKWARD)
    r = e.correlate_all(np.zeros(6, F32))
    assert r[0]["error_code"] == ca.ERROR_INTERPOLATION_OUT_OF_IMAGE
    assert r[1]["error_code"] == ca.ERROR_NONE
    e.close()
    flat = np.full((256, 256), 120, np.uint8)
    stripes = np.tile(((np.arange(256) // 3) % 2 * 80 + 60).astype(np.uint8)[None, :], (256, 1))
    for img in (flat, stripes):
        outs = []
        for mode in (ca.UPDATE_FORWARD, ca.UPDATE_BACKWARD):
            e = ca.HipCorrelationEngine()
            e.set_undeformed_image(img)
            e.set_deformed_image(img)
            e.resetPolygon_rect(0, 100, 100, 140, 140)
            e.commit_sectors()
            e.set_update(mode)
            outs.append(e.correlate_all(np.zeros(6, F32)))
            e.close()
        fwd, bwd = outs
        assert bwd["error_code"][0] == fwd["error_code"][0], (fwd, bwd)
        assert np.array_equal(np.isfinite(bwd["p"]), np.isfinite(fwd["p"])), (fwd, bwd)
