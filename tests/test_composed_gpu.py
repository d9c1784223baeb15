"""The composed refinement on the GPU (lk_refine_composed, include/lk_engine.h): it reduces to each of the four passes it
combines, byte for byte; the seed evaluation of the new combinations against the restatement; byte independence of batch,
mode and ring slot; the rim of a hole, where the mask and the model that bends are needed together; the S-curve under the
bending model; the rescue of a sector at the image border; the statuses; the refusals; and that nothing of the engine moves.

Geometries and pinned figures: quadratic_ref.py, weighted_ref.py and composed_ref.py.  All pairs are 256 x 256 (the shifted
pairs 192 x 192); the batch is quadratic_ref.RECTS and its annular list sector: 16-, 64- and 512-lane groups and the list
walk.  Sums: per sum |device - float64 sum of the restated weighted terms| <= 64 n 2^-53 sum|w term|, the bound of
test_weighted_gpu.py - device and restatement differ only in the order of double additions."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import composed_ref as cr
import quadratic_ref as qr
import weighted_ref as wr
import znssd_ref as zr

pytestmark = pytest.mark.gpu

MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
NEAR = np.float32([1.25, -0.65, 0.001, 0.0005, -0.0005, -0.001])
SECOND = np.float32([1e-4, -1e-4, 5e-5, -5e-5, 1e-4, -1e-4])
S, BIG, RING = qr.N_SECTORS, qr.BIG, qr.RING
SIGMA = 31 / 6
ZN_FIELDS = ca.ZNSSD_DTYPE.names[:-1]        # what struct lk_composed shares with struct lk_znssd
QD_FIELDS = ca.QUADRATIC_DTYPE.names[:-1]    # ... with struct lk_quadratic: everything up to and including bend
WT_FIELDS = ("n_valid", "weight_sum", "n_eff", "centroid_dx", "centroid_dy")
FLOATS = ("zncc", "gain", "offset", "znssd", "zncc_seed", "shift", "last_step", "bend")


def make_engine(und, dfm, rects=qr.RECTS, model=ca.FM_UVUXUYVXVY, annular=qr.ANNULAR, interp=ca.IM_BICUBIC, commit=True, py_start=0):
    e = ca.HipCorrelationEngine(interpolation=interp, fitting_model=model, precision=zr.PRECISION, py_start=py_start, py_stop=2)
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


def geometry(e, rects):
    lists = [qr.rect_rows(*rects[s]) if s < len(rects) else e.level_xy(0, s) for s in range(e.n_sectors)]
    centres = [e.sector_info(s)[1:3] for s in range(e.n_sectors)]
    return lists, centres


def the_mask():
    """a mask that cuts through squares of every side, the 96 x 96 square and the annular sector, with scattered single pixels"""
    m = np.ones((256, 256), np.uint8)
    m[:, 98:106] = 0
    m[150:160, 150:170] = 0
    m[200:203, 60:80] = 0
    rng = np.random.default_rng(17)
    m[rng.integers(0, 256, 600), rng.integers(0, 256, 600)] = 0
    return m


def same(a, b, fields):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in fields)


@pytest.fixture(scope="module")
def pair():
    return qr.pair()


def seeds_for(e):
    centres = [e.sector_info(s)[1:3] for s in range(e.n_sectors)]
    return qr.true_translation_seeds(centres)[0]


# ---- 1. the composed pass reduces to each of the four ------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_reduces_to_the_four_passes(pair, model):
    P = _ffi.N_PARAMS[model]
    mask = the_mask()
    with make_engine(*pair, model=model) as e:
        n0 = [e.sector_info(s)[0] for s in range(S)]
        assert n0[0] == 441 and n0[25] == 961 and n0[50] == 2401 and n0[BIG] == 9216 and 0 < n0[RING] <= 512   # 16, 64, 512 lanes
        g = seeds_for(e)

        def first_order(got, want, fields):
            (r, i, q), (wr_, wi, wq) = got, want
            assert r.tobytes() == wr_.tobytes() and q.tobytes() == wq.tobytes() and q.shape == (S, ca.ZN_SUMS)
            assert same(i, wi, fields)
            ran = ~np.isin(i["status"], (ca.ZN_BAD_SEED, ca.ZN_OUT_OF_IMAGE))
            assert i["p"][ran, :P].tobytes() == r["p"][ran, :P].tobytes() and not i["p"][:, P:].any() and not i["p"][~ran].any()
            assert not i["bend"].any() and not i["reserved"].any()

        # (order 1, sampler 0, no mask, sigma 0) = lk_refine_znssd
        want = e.refine_znssd(guesses=g, return_sums=True)
        got = e.refine_composed(guesses=g, order=1, sampler=0, return_sums=True)
        first_order(got, want, ZN_FIELDS)
        assert (got[1]["n_valid"] == got[1]["n_points"]).all() and (got[1]["weight_sum"] == got[1]["n_points"]).all()
        print("model", model, "znssd statuses", np.bincount(want[1]["status"], minlength=9))
        # the same with a mask and a window = lk_refine_weighted, the weights' words included
        want = e.refine_weighted(guesses=g, sigma=SIGMA, mask=mask, min_fraction=0.25, return_sums=True)
        got = e.refine_composed(guesses=g, order=1, sampler=0, sigma=SIGMA, mask=mask, min_fraction=0.25, return_sums=True)
        first_order(got, want, ZN_FIELDS + WT_FIELDS)
        assert (want[1]["n_valid"] < want[1]["n_points"]).sum() >= 10
        # (order 1, sampler 3 / 5, unit weights) = lk_refine_spline
        for order in (3, 5):
            want = e.refine_spline(guesses=g, order=order, return_sums=True)
            first_order(e.refine_composed(guesses=g, order=1, sampler=order, return_sums=True), want, ZN_FIELDS)
            first_order(e.refine_composed(guesses=g, order=1, sampler=order, mask=np.ones((256, 256), np.uint8), return_sums=True),
                        want, ZN_FIELDS)
        # (order 2, sampler 0, unit weights) = lk_refine_quadratic, with and without second-order seeds
        for second in (None, np.tile(SECOND, (S, 1))):
            wr_, wi, wq = e.refine_quadratic(guesses=g, second=second, return_sums=True)
            r, i, q = e.refine_composed(guesses=g, second=second, order=2, sampler=0, return_sums=True)
            assert r.tobytes() == wr_.tobytes() and q.tobytes() == wq.tobytes() and q.shape == (S, ca.QD_SUMS)
            assert same(i, wi, QD_FIELDS) and (i["n_valid"] == i["n_points"]).all() and (i["weight_sum"] == i["n_points"]).all()
            assert (i["n_eff"] == i["n_points"]).all() and not i["reserved"].any() and not i["centroid_dx"][:RING].any()
        # records as seeds take the same way
        rec = e.refine_znssd(guesses=g)[0]
        a, b = e.refine_quadratic(records=rec), e.refine_composed(records=rec, order=2)
        assert a[0].tobytes() == b[0].tobytes() and same(a[1], b[1], QD_FIELDS)


# ---- 2. the seed evaluation of the new combinations against the restatement ---------------------------------------------------------
def device_sampler(e, order):
    """points -> [n][4] = W, Wx, Wy, flag from the pass's own sampler (lk_spline_sample of the deformed image)"""
    def sampler(pts):
        out = e.spline_sample(ca.IMG_DEF, np.asarray(pts, np.float32), order).copy()
        out[:, 3] = 1.0 - out[:, 3]
        return out
    return sampler


def check_seed_evaluation(oracle, e, und, dfm, model, interp, order, sampler, lists, centres, g, second, sigma, mask, ratios=None,
                          allow_refused=False):
    """refine_composed with max_iters = 0 under (order, sampler, sigma, mask) from the seeds g (and `second`, order 2): per
    sector the weighted sums against the per-sample floats within 64 n 2^-53 sum|terms|, the prologue, the info the host
    function of the device's own sums and N bit for bit, the record -> the samples of weight 0.  sampler 3 or 5: the floats
    come from the pass's own sampler (device_sampler).  allow_refused: a sector may have fewer valid samples than the model
    needs (a starved sector of test_pass_instances_gpu.py: ZN_TOO_FEW from the prologue, nothing evaluated) or a singular step."""
    Pm = _ffi.N_PARAMS[model]
    inv = wr.inv_of(sigma)
    used = qr.FLAGGED if order == 2 else zr.layout(Pm)[4]
    n_sums = ca.QD_SUMS if order == 2 else ca.ZN_SUMS
    n0 = [e.sector_info(s)[0] for s in range(e.n_sectors)]
    fn = device_sampler(e, sampler) if sampler else ((lambda pts: e.sample(ca.IMG_DEF, 0, pts)) if interp == ca.IM_BICUBIC_SEPARABLE else None)
    rec, info, sums = e.refine_composed(guesses=g, second=second, order=order, sampler=sampler, sigma=sigma, mask=mask, max_iters=0,
                                        return_sums=True)
    assert sums.shape == (e.n_sectors, n_sums)
    worst, cut = 0.0, 0
    for s in range(e.n_sectors):
        xy, (cx, cy) = lists[s], centres[s]
        n = len(xy)
        w = wr.sample_weights(xy, cx, cy, inv, mask)
        live = w > 0
        cut += int(n - live.sum())
        i = info[s]
        pro = wr.prologue(xy, cx, cy, w)
        N = wr.device_sum(w.astype(np.float64), wr.group_of(n0[s]))
        assert i["n_points"] == n and i["n_valid"] == pro["n_valid"] == int(live.sum()) <= n, (s, i)
        if allow_refused and pro["n_valid"] < (qr.P if order == 2 else Pm) + 2:
            assert i["status"] == ca.ZN_TOO_FEW and i["evaluations"] == 0 and not sums[s].any(), (s, i)
            continue
        p12 = np.concatenate([g[s], second[s] if order == 2 else np.zeros(6, np.float32)])
        if order == 2:
            f, gg, gx, gy, dx, dy, bad = qr.sample_floats(oracle, interp, und, dfm, xy, cx, cy, p12, fn)
            terms = cr.weighted_terms(f[live], gg[live], gx[live], gy[live], dx[live], dy[live], w[live])
        else:
            f, gg, H, bad = zr.sample_floats(oracle, interp, model, und, dfm, xy, cx, cy, g[s], fn)
            terms = wr.weighted_terms(f[live], gg[live], H[live], w[live])
        assert not bad[live].any()
        bound = 64.0 * n * 2.0 ** -53 * np.abs(terms).sum(axis=0)
        err = np.abs(sums[s][:used] - terms.sum(axis=0))
        assert (err <= bound).all(), (s, err, bound)
        assert not sums[s][used:].any(), (s, sums[s][used:])
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        if ratios is not None:
            ratios.append((s, float((err[bound > 0] / bound[bound > 0]).max())))
        # the prologue: N in the device's order of additions, bit for bit
        assert i["weight_sum"].tobytes() == np.float32(N).tobytes(), (s, i, N)
        assert abs(float(i["n_eff"]) - pro["n_eff"]) <= 4 * 2.0 ** -24 * pro["n_eff"], (s, i, pro)
        # the info is the host function of the device's own sums and N, bit for bit
        status, delta, crit, gain, offset = ca.composed_step_from_sums(order, model, pro["n_valid"], N, sums[s], zr.LAMBDA0)
        refused, _, _, _, zncc = cr.criterion(pro["n_valid"], N, sums[s]) if order == 2 else wr.criterion(model, pro["n_valid"], N, sums[s])
        if allow_refused:
            assert (status == 0 or n < 16) and i["status"] == (refused if refused else ca.ZN_MAX_ITERS), (s, status, i)
        else:
            assert status == 0 and not refused and i["status"] == ca.ZN_MAX_ITERS, (s, status, i)
        assert (i["iterations"], i["evaluations"]) == (0, 1) and i["shift"] == 0 and i["last_step"] == 0 and not i["reserved"].any()
        if not refused:
            for name, want in (("gain", gain), ("offset", offset), ("znssd", crit), ("zncc", zncc), ("zncc_seed", zncc)):
                assert i[name].tobytes() == np.float32(want).tobytes(), (s, name, i[name], want)
        if order == 2:
            assert i["p"].tobytes() == p12.tobytes() and i["bend"].tobytes() == np.float32(qr.bend(p12, n0[s])).tobytes(), (s, i)
        else:
            assert i["p"][:Pm].tobytes() == g[s][:Pm].tobytes() and not i["p"][Pm:].any() and i["bend"] == 0, (s, i)
        r = rec[s]
        V = (f[live] - gg[live]).astype(np.float64)
        chi = (w[live].astype(np.float64) * V * V).sum() / pro["sw"]
        assert r["p"][:Pm].tobytes() == g[s][:Pm].tobytes() and not r["p"][Pm:].any() and abs(float(r["chi"]) - chi) <= 1e-6 * chi, (s, r, chi)
        if not refused:
            assert r["error_code"] == ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        assert r["n_points"] == n0[s]
    print(f"order {order} sampler {sampler}: worst sum error / bound {worst:.3g}; {cut} samples of weight 0")
    return cut


def check_fixed_point(oracle, e, und, dfm, model, interp, order, sampler, lists, centres, rec, info, sums, sigma, mask):
    """every ZN_CONVERGED sector of a refine_composed run: the restatement evaluated at the returned parameters gives a step
    below 4 x precision at the returned lambda; every sector that kept sums carries the host function of them, bit for bit
    -> the largest restated step"""
    Pm = _ffi.N_PARAMS[model]
    inv = wr.inv_of(sigma) if sigma > 0 else 0.0
    fn = device_sampler(e, sampler) if sampler else ((lambda pts: e.sample(ca.IMG_DEF, 0, pts)) if interp == ca.IM_BICUBIC_SEPARABLE else None)
    worst = 0.0
    for s in range(len(lists)):
        xy, (cx, cy) = lists[s], centres[s]
        n = len(xy)
        w = wr.sample_weights(xy, cx, cy, inv, mask)
        i = info[s]
        if sums[s].any() and i["evaluations"] > 0 and i["status"] not in (ca.ZN_TOO_FEW, ca.ZN_FLAT, ca.ZN_OUT_OF_IMAGE, ca.ZN_NEGATIVE,
                                                                          ca.ZN_BAD_SEED):
            N = wr.device_sum(w.astype(np.float64), wr.group_of(n))
            _, _, crit, gain, offset = ca.composed_step_from_sums(order, model, int(i["n_valid"]), N, sums[s], float(i["lambda"]))
            zncc = (cr.criterion(int(i["n_valid"]), N, sums[s]) if order == 2 else wr.criterion(model, int(i["n_valid"]), N, sums[s]))[4]
            for name, want in (("gain", gain), ("offset", offset), ("znssd", crit), ("zncc", zncc)):
                assert i[name].tobytes() == np.float32(want).tobytes(), (s, name, i[name], want)
        if i["status"] != ca.ZN_CONVERGED:
            continue
        pro = wr.prologue(xy, cx, cy, w)
        if order == 2:
            ref = cr.sums_of(*qr.sample_floats(oracle, interp, und, dfm, xy, cx, cy, i["p"], fn), w)
            st, delta = cr.step(pro["n_valid"], pro["sw"], ref, float(i["lambda"]))[:2]
            step = qr.weighted_step(n, delta)
        else:
            f, g, H, bad = zr.sample_floats(oracle, interp, model, und, dfm, xy, cx, cy, rec["p"][s], fn)
            st, delta = wr.step(model, pro["n_valid"], pro["sw"], wr.sums_of(f, g, H, bad, w), float(i["lambda"]))[:2]
            step = zr.weighted_step(model, n, delta)
        worst = max(worst, step)
        assert st == 0 and step < 4.0 * zr.PRECISION, (s, st, step, i)
    return worst


@pytest.mark.parametrize("order,sampler", [(2, 0), (2, 5), (1, 5)])
def test_sums_and_info_of_the_seed_evaluation(oracle, pair, order, sampler):
    """(test_pass_instances_gpu.py crosses the models, the samplers and the interpolators on its own geometry; this one keeps
    quadratic_ref's squares of three sides and the narrow window)"""
    und, dfm = pair
    model, interp = ca.FM_UVUXUYVXVY, ca.IM_BICUBIC
    rects = qr.RECTS[::8] + [qr.RECTS[BIG]]     # squares of the three sides, the 96 x 96 square; then the annular sector
    with make_engine(und, dfm, rects) as e:
        n0 = [e.sector_info(s)[0] for s in range(e.n_sectors)]
        assert {wr.group_of(n) for n in n0} == {16, 64, 512}
        lists, centres = geometry(e, rects)
        g = seeds_for(e)            # the true translation, and gradients that are not the answer
        g[:, 2:] = NEAR[2:]
        second = np.tile(SECOND, (e.n_sectors, 1)) if order == 2 else None
        cut = check_seed_evaluation(oracle, e, und, dfm, model, interp, order, sampler, lists, centres, g, second, SIGMA, the_mask())
        assert cut > 100


# ---- 3. byte independence ------------------------------------------------------------------------------------------------------------
COMBOS = [dict(order=2, sampler=0), dict(order=2, sampler=5), dict(order=1, sampler=5)]


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "order%d_sampler%d" % (c["order"], c["sampler"]))
def test_a_sector_alone_modes_and_the_ring_slot_give_the_same_bytes(pair, combo):
    kw = dict(sigma=SIGMA, mask=the_mask(), return_sums=True, **combo)
    with make_engine(*pair) as e:
        g = seeds_for(e)
        rec, info, sums = e.refine_composed(guesses=g, **kw)
        print(combo, "status histogram", np.bincount(info["status"], minlength=9))
        assert np.isin(info["status"], (ca.ZN_CONVERGED, ca.ZN_MAX_ITERS, ca.ZN_STALLED)).all() and (info["status"] == ca.ZN_CONVERGED).sum() >= S // 2
        assert (info["n_valid"] < info["n_points"]).sum() >= 10 and (info["n_eff"] < info["n_valid"]).all()

        def again(**more):
            r, i, q = e.refine_composed(guesses=g, **dict(kw, **more))
            assert r.tobytes() == rec.tobytes() and i.tobytes() == info.tobytes() and q.tobytes() == sums.tobytes()

        again()
        e.set_batch_invariant(True)
        again()
        e.set_batch_invariant(False)
        e.set_update(ca.UPDATE_BACKWARD)
        again()
        e.set_update(ca.UPDATE_FORWARD)
        e.set_reference_order(1)
        again()
        held = e.correlate_all(g)
        a, b = e.refine_composed(**kw), e.refine_composed(records=held, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        e.set_reference_order(0)
        e.sequence_reserve(2)
        e.sequence_set_frame(0, pair[1])
        e.sequence_set_frame(1, pair[0])
        again(def_slot=0)
        assert e.refine_composed(guesses=g, def_slot=1, **kw)[0].tobytes() != rec.tobytes()
    for k in (0, 30, 60, BIG):
        with make_engine(*pair, [qr.RECTS[k]], annular=()) as e:
            r, i, q = e.refine_composed(guesses=g[k:k + 1], **kw)
            assert r[0].tobytes() == rec[k].tobytes() and i[0].tobytes() == info[k].tobytes() and q[0].tobytes() == sums[k].tobytes(), k
    with make_engine(*pair, [], annular=qr.ANNULAR) as e:
        r, i, q = e.refine_composed(guesses=g[RING:], **kw)
        assert r[0].tobytes() == rec[RING].tobytes() and i[0].tobytes() == info[RING].tobytes() and q[0].tobytes() == sums[RING].tobytes()


# ---- 4. the rim of a hole ------------------------------------------------------------------------------------------------------------
def test_rim_of_a_hole():
    """Side 49 (composed_ref.RIM_SIDE): in the restatement all eight sectors are CONVERGED under (order 2, mask) there.
    Figures of one run on the MI355X: see DESIGN.md section 27."""
    und, dfm = cr.rim_pair()
    rects = cr.rim_rects(cr.RIM_SIDE)
    mask = cr.rim_mask()
    with make_engine(und, dfm, rects, annular=()) as e:
        centres = [e.sector_info(s)[1:3] for s in range(e.n_sectors)]
        assert [(float(cx), float(cy)) for cx, cy in centres] == [(float(x), float(y)) for x, y in cr.RIM_CENTRES]
        g, truth = qr.true_translation_seeds(centres)
        runs = {"composed": e.refine_composed(guesses=g, order=2, sampler=0, mask=mask),
                "quadratic": e.refine_quadratic(guesses=g),
                "weighted": e.refine_weighted(guesses=g, mask=mask)}
    err = {k: cr.uv_error(r["p"], truth) for k, (r, _) in runs.items()}
    for k in runs:
        print(f"rim, side {cr.RIM_SIDE}, {k}: largest |(u, v) - truth| = {err[k].max():.6f} px (allowed {1.5 * cr.RIM[k][0]:.6f}), "
              f"mean {err[k].mean():.6f} px (allowed {1.5 * cr.RIM[k][1]:.6f}); statuses {runs[k][1]['status']}")
    print(f"mean ratios: quadratic / composed {err['quadratic'].mean() / err['composed'].mean():.2f}, "
          f"weighted / composed {err['weighted'].mean() / err['composed'].mean():.2f}")
    ci = runs["composed"][1]
    assert (ci["status"] == ca.ZN_CONVERGED).all() and (runs["composed"][0]["error_code"] == 0).all(), ci["status"]
    h = cr.RIM_SIDE // 2
    assert (ci["n_valid"] == (h + 5) * cr.RIM_SIDE).all() and (ci["centroid_dx"] == np.float32((4 - h) / 2)).all() and not ci["centroid_dy"].any()
    for k in runs:
        assert err[k].max() <= 1.5 * cr.RIM[k][0] and err[k].mean() <= 1.5 * cr.RIM[k][1], (k, err[k], cr.RIM[k])
    assert err["composed"].mean() < err["quadratic"].mean() and err["composed"].mean() < err["weighted"].mean()


# ---- 5. the S-curve under the bending model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", cr.CURVE_SHIFTS)
def test_s_curve_under_the_bending_model(shift):
    """Figures of one run on the MI355X: see DESIGN.md section 27."""
    und, dfm = cr.shifted_pair(shift)
    with make_engine(und, dfm, cr.CURVE_RECTS, model=ca.FM_UV, annular=()) as e:
        g = cr.curve_seeds(shift)
        bias = {}
        for sampler in (0, 5):
            rec, info = e.refine_composed(guesses=g, order=2, sampler=sampler)
            assert (info["status"] == ca.ZN_CONVERGED).all(), (sampler, info["status"])
            bias[sampler] = float((info["p"][:, 0].astype(np.float64) - shift).mean())
            print(f"shift {shift}, (2, {sampler}): mean u - s = {bias[sampler]:+.6f} px (restated {cr.CURVE[shift][sampler]:+.6f}, "
                  f"allowed |.| <= {1.5 * abs(cr.CURVE[shift][sampler]):.6f})")
    for sampler in (0, 5):
        assert abs(bias[sampler]) <= 1.5 * abs(cr.CURVE[shift][sampler]), (shift, sampler, bias, cr.CURVE[shift])
    assert abs(bias[5]) < abs(bias[0]), (shift, bias)


# ---- 6. the border -------------------------------------------------------------------------------------------------------------------
def test_a_mask_rescues_a_second_order_sector_at_the_image_border():
    und, dfm = zr.pair()
    seeds = zr.zero_gradient_seeds(1)
    with make_engine(und, dfm, [wr.BORDER_RECT], annular=()) as e:
        cx, cy = e.sector_info(0)[1:3]
        plain, pi = e.refine_quadratic(guesses=seeds)
        unit, ui = e.refine_composed(guesses=seeds, order=2, sampler=0)
        r, i = e.refine_composed(guesses=seeds, order=2, sampler=0, mask=wr.column_mask(wr.BORDER_CUT))
    assert pi["status"][0] == ca.ZN_OUT_OF_IMAGE == ui["status"][0] and plain.tobytes() == unit.tobytes()
    assert plain["error_code"][0] == ca.ERROR_INTERPOLATION_OUT_OF_IMAGE
    u, v = zr.analytic_uv(float(cx), float(cy))
    err = max(abs(float(r["p"][0, 0]) - u), abs(float(r["p"][0, 1]) - v))
    print(f"border: (2, 0, mask): |(u, v) - analytic| = {err:.6f} px; status {i['status'][0]}, bend {i['bend'][0]:.4f}")
    assert i["status"][0] == ca.ZN_CONVERGED and r["error_code"][0] == 0 and i["n_valid"][0] == 27 * 31 and i["centroid_dx"][0] == -2.0


# ---- 7. statuses ---------------------------------------------------------------------------------------------------------------------
SY = 118
STATUS_RECTS = [(x, SY, x + 20, SY + 20) for x in (60, 84, 108, 132, 156, 180)]   # 21 x 21, across the middle of the pair


def test_statuses(pair):
    n = len(STATUS_RECTS)
    mask = np.ones((256, 256), np.uint8)
    mask[SY:SY + 21, 84:105] = 0       # all of sector 1
    mask[SY:SY + 21, 108:113] = 0      # five of the 21 columns of sector 2: 336 of 441 samples stay
    mask[SY:SY + 21, 156:177] = 0      # sector 4 keeps thirteen samples: one fewer than 12 + 2
    mask[SY, 156:169] = 1
    with make_engine(*pair, STATUS_RECTS, annular=()) as e:
        g = seeds_for(e)
        second = np.zeros((n, 6), np.float32)
        second[5, 2] = np.inf
        kw = dict(order=2, sampler=0, return_sums=True)
        base, bi, bs = e.refine_composed(guesses=g, second=np.zeros_like(second), **kw)
        rec, info, sums = e.refine_composed(guesses=g, second=second, mask=mask, **kw)
        assert info["status"].tolist() == [ca.ZN_CONVERGED, ca.ZN_TOO_FEW, ca.ZN_CONVERGED, ca.ZN_CONVERGED, ca.ZN_TOO_FEW, ca.ZN_BAD_SEED]
        assert rec["error_code"].tolist() == [0, _ffi.ERROR_SOLVER, 0, 0, _ffi.ERROR_SOLVER, ca.ERROR_BAD_DOMAIN]
        assert info["n_valid"].tolist() == [441, 0, 336, 441, 13, 0] and info["weight_sum"].tolist() == [441, 0, 336, 441, 13, 0]
        assert (info["n_points"] == 441).all()
        for s in (1, 4, 5):            # nothing was evaluated: floats and sums 0, the seed as the parameters, no NaN in any byte
            assert not any(info[k][s] for k in FLOATS) and info["iterations"][s] == 0 and info["evaluations"][s] == 0, (s, info[s])
            assert not sums[s].any() and rec["chi"][s] == 0 and rec["iterations"][s] == 0
            assert rec["p"][s].tobytes() == g[s].tobytes()
        assert info["p"][1, :6].tobytes() == g[1].tobytes() and info["p"][4, :6].tobytes() == g[4].tobytes() and not info["p"][5].any()
        assert all(np.isfinite(info[k]).all() for k in info.dtype.names) and np.isfinite(sums).all() and np.isfinite(rec["chi"]).all()
        assert np.isfinite(np.frombuffer(info[1].tobytes(), np.float32)).all()     # every byte of the all-zero sector's info
        for s in (0, 3):               # the neighbours are untouched by a mask elsewhere
            assert rec[s].tobytes() == base[s].tobytes() and info[s].tobytes() == bi[s].tobytes() and sums[s].tobytes() == bs[s].tobytes()
        assert rec[2].tobytes() != base[2].tobytes()
        # the same thirteen samples are enough for the six parameters of order 1
        one = e.refine_composed(guesses=g, mask=mask, order=1, sampler=0)[1]
        assert one["n_valid"][4] == 13 and one["status"][4] != ca.ZN_TOO_FEW and one["evaluations"][4] >= 1 and one["status"][1] == ca.ZN_TOO_FEW
        # min_fraction on both sides of 336 / 441 = 0.7619
        lo = e.refine_composed(guesses=g, second=second, mask=mask, min_fraction=0.76, **kw)
        hi = e.refine_composed(guesses=g, second=second, mask=mask, min_fraction=0.77, **kw)
        assert lo[0].tobytes() == rec.tobytes() and lo[1].tobytes() == info.tobytes()
        assert hi[1]["status"].tolist() == [ca.ZN_CONVERGED, ca.ZN_TOO_FEW, ca.ZN_TOO_FEW, ca.ZN_CONVERGED, ca.ZN_TOO_FEW, ca.ZN_BAD_SEED]
        assert hi[1]["n_valid"][2] == 336 and hi[1]["evaluations"][2] == 0 and hi[0][0].tobytes() == rec[0].tobytes()
        # records as seeds: a bad record passes through, byte for byte
        seeds = np.zeros(n, ca.RESULT_DTYPE)
        seeds["p"][:] = g
        seeds["chi"] = 1.0
        seeds["error_code"][0] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        seeds["iterations"][0] = 50
        seeds["p"][3, 1] = np.inf
        seeds["chi"][2] = 5.0
        for combo in COMBOS:
            out, oi = e.refine_composed(records=seeds, mask=mask, chi_max=2.0, **combo)
            assert oi["status"][[0, 2, 3]].tolist() == [ca.ZN_BAD_SEED] * 3 and oi["status"][1] == ca.ZN_TOO_FEW, (combo, oi["status"])
            for s in (0, 2, 3):
                assert out[s].tobytes() == seeds[s].tobytes() and not any(oi[k][s] for k in FLOATS) and oi["evaluations"][s] == 0, s
                assert oi["n_valid"][s] == 0 and oi["weight_sum"][s] == 0 and not oi["p"][s].any()


# ---- 8. engine state untouched, arguments and refusals ---------------------------------------------------------------------------------
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
    with make_engine(*pair) as e, make_engine(*pair) as plain:
        seeds = seeds_for(e)
        seeds[[9, 27], 0] = 300.0
        good = seeds_for(e)
        first = e.correlate_all(seeds)
        plain.correlate_all(seeds)

        def state():
            return dict(records=device_records(e), guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(),
                        stats=e.sector_stats(), uncertainty=e.parameter_uncertainty(),
                        counters=np.array(sorted(e.stats().items()), dtype=object))

        kept = state()
        for combo in COMBOS:
            kw = dict(sigma=SIGMA, mask=the_mask(), **combo)
            a = e.refine_composed(**kw)
            b = e.refine_composed(records=first, **kw)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            assert (a[1]["status"][[9, 27]] == ca.ZN_BAD_SEED).all()
            ms, count = e.composed_last()
            assert ms > 0 and count == (26, 50, 1), count       # 25 squares of 441 and the list; 961 and 2401 samples; 9216
        after = state()
        for k in kept:
            if k == "counters":
                assert (kept[k] == after[k]).all()
            else:
                assert kept[k].tobytes() == after[k].tobytes(), k
        assert e.correlate_all(good).tobytes() == plain.correlate_all(good).tobytes()
        assert e.last_evaluated_parameters().tobytes() == plain.last_evaluated_parameters().tobytes()


def test_arguments_and_refusals(pair):
    rects = qr.RECTS[:9]
    e = make_engine(*pair, rects, annular=(), commit=False)
    lib, h = e.lib, e._h
    seeds = np.zeros(9, ca.RESULT_DTYPE)
    seeds["p"][:] = NEAR
    g = np.tile(NEAR, (9, 1))
    g2 = np.tile(SECOND, (9, 1))
    rec = np.full(9, 7, np.uint8).repeat(48).view(ca.RESULT_DTYPE)
    info = np.full(9, 7, np.uint8).repeat(128).view(ca.COMPOSED_DTYPE)
    sums = np.full((9, ca.QD_SUMS), 7.0)
    kept = [rec.tobytes(), info.tobytes(), sums.tobytes()]
    ones = np.ones((256, 256), np.uint8)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def config(**kw):
        fields = dict(def_slot=-1, chi_max=0.0, max_iters=-1, precision=0.0, lambda0=0.0, order=2, sampler=0, sigma=0.0, min_fraction=0.0,
                      mask_rows=0, mask_cols=0)
        fields.update(kw)
        return _ffi.LkComposedConfig(**fields)

    def refused(cfg="default", mask=None, records=None, guesses=None, second=None, outputs=(rec, info), word=None, **kw):
        if cfg == "default":
            cfg = config(**kw)
        if word is not None:
            cfg.reserved[word] = 1
        rc = lib.lk_refine_composed(h, C.byref(cfg) if cfg is not None else None, ptr(mask), ptr(records),
                                    _ffi.fptr(guesses) if guesses is not None else None, _ffi.fptr(second) if second is not None else None,
                                    ptr(outputs[0]), ptr(outputs[1]), ptr(sums))
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and msg.startswith("lk_refine_composed: "), (rc, msg)   # names the function called
        return msg

    assert "no committed sectors" in refused(guesses=g) and "no committed sectors" in refused(records=seeds)
    e.commit_sectors()
    g[:] = seeds_for(e)
    seeds["p"][:] = g
    assert "no solve" in refused()
    assert "no configuration" in refused(None, guesses=g)
    assert "no output" in refused(guesses=g, outputs=(None, None))
    for word in range(5):
        assert "reserved" in refused(guesses=g, word=word)
    assert "both given" in refused(records=seeds, guesses=g)
    assert "chi_max" in refused(records=seeds, chi_max=np.nan) and "chi_max" in refused(guesses=g, chi_max=np.inf)
    assert "precision" in refused(guesses=g, precision=np.nan) and "lambda0" in refused(guesses=g, lambda0=np.inf)
    assert "ring slot" in refused(guesses=g, def_slot=0) and "def_slot" in refused(guesses=g, def_slot=-2)
    for bad in (-1.0, np.nan, np.inf, 1e-30):
        assert "sigma" in refused(guesses=g, sigma=bad)
    for bad in (-0.1, 1.5, np.nan):
        assert "min_fraction" in refused(guesses=g, min_fraction=bad)
    assert "without dimensions" in refused(guesses=g, mask=ones) and "without dimensions" in refused(guesses=g, mask=ones, mask_rows=256)
    assert "without a mask" in refused(guesses=g, mask_rows=256, mask_cols=256)
    for rows, cols in ((255, 256), (256, 255), (128, 128), (512, 512)):
        assert "mask dimensions" in refused(guesses=g, mask=ones, mask_rows=rows, mask_cols=cols)
    # this pass's own
    for bad in (0, 3, -1):
        assert "order" in refused(guesses=g, order=bad)
    for bad in (1, 2, 4, -3, 7):
        assert "sampler" in refused(guesses=g, sampler=bad)
    assert "second" in refused(guesses=g, second=g2, order=1) and "second" in refused(records=seeds, second=g2, order=1, sampler=5)
    assert lib.lk_refine_composed(None, C.byref(config()), None, None, _ffi.fptr(g), None, ptr(rec), ptr(info), None) == ca.ERROR_BAD_DOMAIN
    assert [rec.tobytes(), info.tobytes(), sums.tobytes()] == kept       # every refusal left the outputs as they were
    with pytest.raises(ValueError):
        e.refine_composed(guesses=g, mask=np.ones(256, np.uint8))
    with pytest.raises(ca.LkError):
        e.refine_composed(guesses=g, mask=np.ones((128, 128), np.uint8))
    with pytest.raises(ca.LkError):
        e.refine_composed(guesses=g, second=g2, order=1)
    # either output alone; the defaults of the C configuration are lk_config's; a bool mask is a mask
    cfg = config(mask_rows=256, mask_cols=256, sampler=5)
    assert lib.lk_refine_composed(h, C.byref(cfg), ptr(ones), None, _ffi.fptr(g), None, ptr(rec), None, None) == 0
    assert lib.lk_refine_composed(h, C.byref(cfg), ptr(ones), ptr(seeds), None, None, None, ptr(info), None) == 0
    both = e.refine_composed(guesses=g, sampler=5, mask=np.ones((256, 256), bool), max_iters=50, precision=1e-3, lambda0=1e-3)
    assert rec.tobytes() == both[0].tobytes() and info.tobytes() == both[1].tobytes() and (info["status"] == ca.ZN_CONVERGED).all()
    # a solve in flight refuses the engine-held records and finishes normally afterwards
    e.correlate_all_async()
    assert "waited for" in refused()
    solved = e.wait_results()
    assert e.refine_composed(sigma=SIGMA)[0].tobytes() == e.refine_composed(records=solved, sigma=SIGMA)[0].tobytes()
    e.close()
    # level 1: the mask and the coefficient image are the level image's; sigma, the centroid and p are level-0 pixels
    with make_engine(*pair, [(40, 40, 78, 78)], annular=(), py_start=1) as e1:
        g1, truth = qr.true_translation_seeds([e1.sector_info(0)[1:3]])
        with pytest.raises(ca.LkError):
            e1.refine_composed(guesses=g1, mask=ones)
        half = np.ones((128, 128), np.uint8)
        half[:, :25] = 0
        for combo in COMBOS:
            r1, i1 = e1.refine_composed(guesses=g1, sigma=12.0, mask=half, **combo)
            assert i1["status"][0] in (ca.ZN_CONVERGED, ca.ZN_MAX_ITERS, ca.ZN_STALLED) and i1["evaluations"][0] > 1, (combo, i1)
            xy = qr.rect_rows(20, 20, 39, 39)    # the rectangle at level 1
            cx, cy = (np.float32(t) * np.float32(0.5) for t in e1.sector_info(0)[1:3])
            pro = wr.prologue(xy, cx, cy, wr.sample_weights(xy, cx, cy, wr.inv_of(12.0, level=1), half), level=1)
            assert i1["n_points"][0] == len(xy) and 0 < i1["n_valid"][0] == pro["n_valid"] < len(xy)
            assert abs(float(i1["weight_sum"][0]) - pro["sw"]) <= 4 * 2.0 ** -24 * pro["sw"]
            assert abs(float(i1["centroid_dx"][0]) - pro["centroid"][0]) <= 1e-5 and pro["centroid"][0] > 0.5
            assert np.abs(i1["p"][0, :2] - truth[0, :2]).max() < 0.25 and i1["p"][0, :6].tobytes() == r1["p"][0].tobytes()
    bare = make_engine(None, None, rects, annular=())
    rc = bare.lib.lk_refine_composed(bare._h, C.byref(config()), None, None, _ffi.fptr(g), None, ptr(rec), ptr(info), None)
    msg = bare.lib.lk_last_error_string(bare._h).decode()
    assert rc == ca.ERROR_BAD_DOMAIN and "image" in msg and msg.startswith("lk_refine_composed: "), (rc, msg)
    bare.close()
