"""The weighted refinement on the GPU (lk_refine_weighted, include/lk_engine.h): unit weights give lk_refine_znssd's bytes; the
seed evaluation under a window and a mask against the restatement; byte independence of batch, mode and ring slot; the edge
sectors with and without the mask; the rescue of a sector at the image border; the Gaussian window on a curved field; the
statuses; the refusals; and that nothing of the engine moves.

Geometries and bounds: znssd_ref.py, quadratic_ref.py and weighted_ref.py (the edge pair, the pinned figures of the
restatement).  Sums: per sum |device - float64 sum of the restated weighted terms| <= 64 n 2^-53 sum|w term|, the bound of
test_znssd_gpu.py - device and restatement differ only in the order of double additions."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import quadratic_ref as qr
import weighted_ref as wr
import znssd_ref as zr

pytestmark = pytest.mark.gpu

MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
NEAR = np.float32([1.25, -0.65, 0.001, 0.0005, -0.0005, -0.001])
S = zr.N_SECTORS
BIG, WAVE, RING = len(zr.GRID) + 1, len(zr.GRID), len(zr.RECTS)   # the 96 x 96, the 24 x 24 and the annular sector
SIGMA = 19 / 6
ZN_FIELDS = ca.ZNSSD_DTYPE.names[:-1]     # the first 48 bytes of both info records
FLOATS = ("zncc", "gain", "offset", "znssd", "zncc_seed", "shift", "last_step")


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
    lists = [zr.rect_rows(*rects[s]) if s < len(rects) else e.level_xy(0, s) for s in range(e.n_sectors)]
    centres = [e.sector_info(s)[1:3] for s in range(e.n_sectors)]
    return lists, centres


def the_mask():
    """a mask that cuts through grid sectors, the 96 x 96 square and the annular sector, with scattered single pixels"""
    m = np.ones((256, 256), np.uint8)
    m[:, 98:106] = 0
    m[150:160, 150:170] = 0
    m[200:203, 60:80] = 0
    rng = np.random.default_rng(17)
    m[rng.integers(0, 256, 600), rng.integers(0, 256, 600)] = 0
    return m


@pytest.fixture(scope="module")
def pair():
    return zr.pair()


def first48(info):
    return b"".join(np.ascontiguousarray(info[k]).tobytes() for k in ZN_FIELDS)


# ---- 1. unit weights are lk_refine_znssd's bytes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_unit_weights_give_the_znssd_bytes(pair, model):
    seeds = zr.zero_gradient_seeds(S)
    with make_engine(*pair, model=model) as e:
        n0 = [e.sector_info(s)[0] for s in range(S)]
        assert n0[0] == 361 and n0[WAVE] == 576 and n0[BIG] == 9216 and 0 < n0[RING] <= 512
        rec, info, sums = e.refine_znssd(guesses=seeds, return_sums=True)
        assert (info["status"] == ca.ZN_CONVERGED).all(), info["status"]
        for kw in (dict(), dict(mask=np.ones((256, 256), np.uint8)), dict(mask=np.full((256, 256), 200, np.uint8), min_fraction=1.0)):
            r, i, q = e.refine_weighted(guesses=seeds, return_sums=True, **kw)
            assert r.tobytes() == rec.tobytes(), kw.keys()
            assert first48(i) == first48(info), kw.keys()
            assert q.tobytes() == sums.tobytes(), kw.keys()
            assert (i["n_valid"] == info["n_points"]).all() and (i["weight_sum"] == info["n_points"]).all()
            assert (i["n_eff"] == info["n_points"]).all() and not i["reserved"].any()
            # the centroid of a rectangle is its committed centre exactly; the committed centre of the sample list is the
            # float32 nearest its mean, so there the offset is that rounding: below one step of the centre's float32
            assert not i["centroid_dx"][:RING].any() and not i["centroid_dy"][:RING].any()
            assert abs(i["centroid_dx"][RING]) <= np.spacing(r["und_cx"][RING]) and abs(i["centroid_dy"][RING]) <= np.spacing(r["und_cy"][RING])
        # records as seeds take the same way
        a, b = e.refine_znssd(records=rec), e.refine_weighted(records=rec)
        assert a[0].tobytes() == b[0].tobytes() and first48(a[1]) == first48(b[1])


# ---- 2. the seed evaluation against the restatement ------------------------------------------------------------------------------
CASES = [(m, ca.IM_BICUBIC) for m in MODELS] + [(ca.FM_UVUXUYVXVY, ca.IM_BILINEAR)]


def check_seed_evaluation(oracle, e, und, dfm, model, interp, lists, centres, g, sigma, mask, sampler=None, ratios=None, allow_refused=False):
    """refine_weighted with max_iters = 0 from the seeds g under `mask` and the window of `sigma`: per sector the weighted sums
    against the oracle's per-sample floats within 64 n 2^-53 sum|terms|, the prologue, the info the host function of the
    device's sums and N bit for bit, the record; the same call again gives the same bytes -> the samples of weight 0.  allow_refused: as
    test_znssd_gpu.check_seed_evaluation's."""
    P = _ffi.N_PARAMS[model]
    used = zr.layout(P)[4]
    inv = wr.inv_of(sigma)
    n0 = [e.sector_info(s)[0] for s in range(e.n_sectors)]
    rec, info, sums = e.refine_weighted(guesses=g, sigma=sigma, mask=mask, max_iters=0, return_sums=True)
    worst = 0.0
    cut = 0
    for s in range(e.n_sectors):
        xy, (cx, cy) = lists[s], centres[s]
        n = len(xy)
        w = wr.sample_weights(xy, cx, cy, inv, mask)
        live = w > 0
        cut += int(n - live.sum())
        f, gg, H, bad = zr.sample_floats(oracle, interp, model, und, dfm, xy, cx, cy, g[s], sampler)
        assert not bad[live].any()
        terms = wr.weighted_terms(f[live], gg[live], H[live], w[live])
        bound = 64.0 * n * 2.0 ** -53 * np.abs(terms).sum(axis=0)
        err = np.abs(sums[s][:used] - terms.sum(axis=0))
        assert (err <= bound).all(), (s, err, bound)
        assert not sums[s][used:].any(), (s, sums[s][used:])
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        if ratios is not None:
            ratios.append((s, float((err[bound > 0] / bound[bound > 0]).max())))
        # the prologue: the counts and the weight sums against numpy; N itself in the device's order of additions
        i = info[s]
        pro = wr.prologue(xy, cx, cy, w)
        wd = w.astype(np.float64)
        N = wr.device_sum(wd, wr.group_of(n0[s]))
        assert i["n_points"] == n and i["n_valid"] == pro["n_valid"] == int(live.sum()) <= n, (s, i)
        assert i["weight_sum"].tobytes() == np.float32(N).tobytes() and abs(N - pro["sw"]) <= n * 2.0 ** -53 * pro["sw"], (s, i, N)
        assert abs(float(i["n_eff"]) - pro["n_eff"]) <= 4 * 2.0 ** -24 * pro["n_eff"], (s, i, pro)
        half = np.abs(xy - np.float32([cx, cy])).max()
        for got, want in ((i["centroid_dx"], pro["centroid"][0]), (i["centroid_dy"], pro["centroid"][1])):
            assert abs(float(got) - want) <= 4 * 2.0 ** -24 * half, (s, got, want)
        # the info is the host function of the device's own sums and N, bit for bit
        status, delta, crit, gain, offset = ca.weighted_step_from_sums(model, pro["n_valid"], N, sums[s], zr.LAMBDA0)
        refused, _, _, _, zncc = wr.criterion(model, pro["n_valid"], N, sums[s])
        if allow_refused:   # (the step's status is the restatement's: a starved sector's matrix may be singular)
            assert status == wr.step(model, pro["n_valid"], N, sums[s], zr.LAMBDA0)[0] and (status == 0 or n < 16), (s, status)
            assert i["status"] == (refused if refused else ca.ZN_MAX_ITERS), (s, status, i)
        else:
            assert status == 0 and not refused and i["status"] == ca.ZN_MAX_ITERS, (s, status, i)
        assert (i["iterations"], i["evaluations"]) == (0, 1) and i["shift"] == 0 and i["last_step"] == 0 and not i["reserved"].any()
        if not refused:
            for name, want in (("gain", gain), ("offset", offset), ("znssd", crit), ("zncc", zncc), ("zncc_seed", zncc)):
                assert i[name].tobytes() == np.float32(want).tobytes(), (s, name, i[name], want)
            assert i["lambda"] == np.float32(zr.LAMBDA0)
        # the record: the seed, chi = sum w (f - g)^2 / sum w, the committed centre and the level-0 count
        r = rec[s]
        assert r["p"][:P].tobytes() == g[s][:P].tobytes() and not r["p"][P:].any(), (s, r)
        V = (f[live] - gg[live]).astype(np.float64)
        chi = (wd[live] * V * V).sum() / pro["sw"]
        assert abs(float(r["chi"]) - chi) <= 1e-6 * chi, (s, r["chi"], chi)
        if not refused:
            assert r["error_code"] == ca.ERROR_CORRELATION_MAX_ITERS_REACHED and r["iterations"] == 0
        assert r["n_points"] == n0[s] and (r["und_cx"], r["und_cy"]) == (np.float32(cx), np.float32(cy)), (s, r)
    print(f"model {model} interp {interp}: worst sum error / bound {worst:.3g}; {cut} samples of weight 0")
    again = e.refine_weighted(guesses=g, sigma=sigma, mask=mask, max_iters=0, return_sums=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (rec, info, sums)))
    return cut


def check_fixed_point(oracle, und, dfm, model, interp, lists, centres, rec, info, sums, sigma, mask, sampler=None):
    """test_znssd_gpu.check_fixed_point with the weights: every ZN_CONVERGED sector has a restated step below 4 x precision at
    the returned parameters and lambda; every sector with sums carries the host function of them, bit for bit"""
    inv = wr.inv_of(sigma)
    worst = 0.0
    for s in range(len(lists)):
        xy, (cx, cy) = lists[s], centres[s]
        n = len(xy)
        w = wr.sample_weights(xy, cx, cy, inv, mask)
        i = info[s]
        if sums[s].any() and i["evaluations"] > 0 and i["status"] not in (ca.ZN_TOO_FEW, ca.ZN_FLAT, ca.ZN_OUT_OF_IMAGE, ca.ZN_NEGATIVE,
                                                                          ca.ZN_BAD_SEED):
            N = wr.device_sum(w.astype(np.float64), wr.group_of(n))
            _, _, crit, gain, offset = ca.weighted_step_from_sums(model, int(i["n_valid"]), N, sums[s], float(i["lambda"]))
            zncc = wr.criterion(model, int(i["n_valid"]), N, sums[s])[4]
            for name, want in (("gain", gain), ("offset", offset), ("znssd", crit), ("zncc", zncc)):
                assert i[name].tobytes() == np.float32(want).tobytes(), (s, name, i[name], want)
        if i["status"] != ca.ZN_CONVERGED:
            continue
        pro = wr.prologue(xy, cx, cy, w)
        f, g, H, bad = zr.sample_floats(oracle, interp, model, und, dfm, xy, cx, cy, rec["p"][s], sampler)
        st, delta = wr.step(model, pro["n_valid"], pro["sw"], wr.sums_of(f, g, H, bad, w), float(i["lambda"]))[:2]
        step = zr.weighted_step(model, n, delta)
        worst = max(worst, step)
        assert st == 0 and step < 4.0 * zr.PRECISION, (s, st, step, i)
    return worst


@pytest.mark.parametrize("model,interp", CASES)
def test_sums_and_info_of_the_seed_evaluation(oracle, pair, model, interp):
    """(all sixteen (model, interpolator) pairs run on the geometry of test_pass_instances_gpu.py; this one keeps the grid
    sectors, the 24 x 24 wavefront sector and the narrow window)"""
    und, dfm = pair
    rects = zr.GRID[::8] + zr.RECTS[len(zr.GRID):]     # eight of the grid, and the three sectors of the other kinds
    with make_engine(und, dfm, rects, model=model, interp=interp) as e:
        assert e.n_sectors == 11
        lists, centres = geometry(e, rects)
        cut = check_seed_evaluation(oracle, e, und, dfm, model, interp, lists, centres, np.tile(NEAR, (e.n_sectors, 1)), SIGMA, the_mask())
        assert cut > 100


# ---- 3. byte independence ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weighted_run(pair):
    with make_engine(*pair) as e:
        rec, info, sums = e.refine_weighted(guesses=zr.zero_gradient_seeds(S), sigma=SIGMA, mask=the_mask(), return_sums=True)
    return dict(rec=rec, info=info, sums=sums)


def test_a_sector_alone_modes_and_the_ring_slot_give_the_same_bytes(pair, weighted_run):
    rec, info, sums = weighted_run["rec"], weighted_run["info"], weighted_run["sums"]
    print("status histogram", np.bincount(info["status"], minlength=9), "n_eff", info["n_eff"].min(), "..", info["n_eff"].max())
    assert (info["status"] == ca.ZN_CONVERGED).all(), info["status"]
    assert (info["n_valid"] < info["n_points"]).sum() >= 10 and (info["n_eff"] < info["n_valid"]).all()
    seeds = zr.zero_gradient_seeds(S)
    kw = dict(sigma=SIGMA, mask=the_mask())
    for k in (0, 37, WAVE, BIG):
        with make_engine(*pair, [zr.RECTS[k]], annular=()) as e:
            r, i, q = e.refine_weighted(guesses=seeds[:1], return_sums=True, **kw)
            assert r[0].tobytes() == rec[k].tobytes() and i[0].tobytes() == info[k].tobytes() and q[0].tobytes() == sums[k].tobytes(), k
    with make_engine(*pair, [], annular=zr.ANNULAR) as e:
        r, i = e.refine_weighted(guesses=seeds[:1], **kw)
        assert r[0].tobytes() == rec[RING].tobytes() and i[0].tobytes() == info[RING].tobytes()
    with make_engine(*pair) as e:
        def same():
            r, i, q = e.refine_weighted(guesses=seeds, return_sums=True, **kw)
            assert r.tobytes() == rec.tobytes() and i.tobytes() == info.tobytes() and q.tobytes() == sums.tobytes()

        same()
        same()
        e.set_batch_invariant(True)
        same()
        e.set_batch_invariant(False)
        e.set_update(ca.UPDATE_BACKWARD)
        same()
        e.set_update(ca.UPDATE_FORWARD)
        e.set_reference_order(1)
        same()
        held = e.correlate_all(seeds)
        a, b = e.refine_weighted(**kw), e.refine_weighted(records=held, **kw)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        e.set_reference_order(0)
        e.sequence_reserve(2)
        e.sequence_set_frame(0, pair[1])
        e.sequence_set_frame(1, pair[0])
        r, i = e.refine_weighted(guesses=seeds, def_slot=0, **kw)
        assert r.tobytes() == rec.tobytes() and i.tobytes() == info.tobytes()
        assert e.refine_weighted(guesses=seeds, def_slot=1, **kw)[0].tobytes() != rec.tobytes()


# ---- 4. the edge -----------------------------------------------------------------------------------------------------------------------
def test_edge_sectors_with_and_without_the_mask():
    """Figures of one run on the MI355X: see DESIGN.md section 26."""
    und, dfm = wr.edge_pair()
    n = len(wr.EDGE_RECTS)
    seeds = zr.zero_gradient_seeds(n)
    with make_engine(und, dfm, wr.EDGE_RECTS, annular=()) as e:
        centres = [e.sector_info(s)[1:3] for s in range(n)]
        assert [(float(cx), float(cy)) for cx, cy in centres] == [(float(x), float(y)) for x, y in wr.EDGE_CENTRES]
        masked, mi = e.refine_weighted(guesses=seeds, mask=wr.column_mask(wr.EDGE_KEEP + 1))
        plain, pi = e.refine_znssd(guesses=seeds)
    want = np.array([zr.analytic_uv(float(cx), float(cy)) for cx, cy in centres])
    em = np.abs(masked["p"][:, :2].astype(np.float64) - want).max(axis=1)
    ep = np.abs(plain["p"][:, :2].astype(np.float64) - want).max(axis=1)
    print(f"edge: masked largest |(u, v) - analytic| = {em.max():.6f} px (allowed {1.5 * wr.EDGE_MASKED:.6f}), mean {em.mean():.6f}; "
          f"lk_refine_znssd mean {ep.mean():.6f} px (at least {4.0 * wr.EDGE_MASKED:.6f}); statuses {mi['status']} {pi['status']}")
    assert (mi["status"] == ca.ZN_CONVERGED).all() and (masked["error_code"] == 0).all(), mi["status"]
    assert (mi["n_valid"] == 20 * 31).all() and (mi["centroid_dx"] == -5.5).all() and not mi["centroid_dy"].any()
    assert em.max() <= 1.5 * wr.EDGE_MASKED, (em, wr.EDGE_MASKED)
    assert ep.mean() >= 4.0 * wr.EDGE_MASKED, (ep, wr.EDGE_MASKED)


# ---- 5. the border ---------------------------------------------------------------------------------------------------------------------
def test_a_mask_rescues_a_sector_at_the_image_border(pair):
    seeds = zr.zero_gradient_seeds(1)
    with make_engine(*pair, [wr.BORDER_RECT], annular=()) as e:
        cx, cy = e.sector_info(0)[1:3]
        plain, pi = e.refine_znssd(guesses=seeds)
        same, si = e.refine_weighted(guesses=seeds)
        r, i = e.refine_weighted(guesses=seeds, mask=wr.column_mask(wr.BORDER_CUT))
    assert pi["status"][0] == ca.ZN_OUT_OF_IMAGE == si["status"][0] and plain.tobytes() == same.tobytes()
    assert plain["error_code"][0] == ca.ERROR_INTERPOLATION_OUT_OF_IMAGE
    u, v = zr.analytic_uv(float(cx), float(cy))
    err = max(abs(float(r["p"][0, 0]) - u), abs(float(r["p"][0, 1]) - v))
    print(f"border: |(u, v) - analytic| = {err:.6f} px (allowed {1.5 * zr.ACCURACY:.6f}; the restatement: {wr.BORDER})")
    assert i["status"][0] == ca.ZN_CONVERGED and r["error_code"][0] == 0 and i["n_valid"][0] == 27 * 31 and i["centroid_dx"][0] == -2.0
    assert err <= 1.5 * zr.ACCURACY


# ---- 6. the Gaussian window ------------------------------------------------------------------------------------------------------------
def test_gaussian_window_on_a_curved_field():
    """Figures of one run on the MI355X: see DESIGN.md section 26."""
    und, dfm = qr.pair()
    sides = (31, 49)
    rects = [qr.square(x, y, side) for side in sides for (x, y) in qr.CENTRES]
    with make_engine(und, dfm, rects, annular=()) as e:
        centres = [e.sector_info(s)[1:3] for s in range(e.n_sectors)]
        g, truth = qr.true_translation_seeds(centres)
        unit = e.refine_znssd(guesses=g)[0]
        for k, side in enumerate(sides):
            rec, info = e.refine_weighted(guesses=g, sigma=side / 6)
            mine = slice(k * len(qr.CENTRES), (k + 1) * len(qr.CENTRES))
            assert (info["status"][mine] == ca.ZN_CONVERGED).all(), info["status"][mine]
            err = np.abs(rec["p"][mine, :2].astype(np.float64) - truth[mine, :2]).max(axis=1)
            plain = np.abs(unit["p"][mine, :2].astype(np.float64) - truth[mine, :2]).max(axis=1)
            print(f"side {side}, sigma {side / 6:.3f}: mean |(u, v) - truth| = {err.mean():.6f} px (allowed {1.5 * wr.GAUSS[side]:.6f}); "
                  f"lk_refine_znssd {plain.mean():.6f} px; n_eff {info['n_eff'][mine].mean():.1f} of {side * side}")
            assert err.mean() <= 1.5 * wr.GAUSS[side], (side, err.mean(), wr.GAUSS[side])
            assert (info["n_eff"][mine] < 0.4 * side * side).all() and (info["n_valid"][mine] == side * side).all()


# ---- 7. statuses -----------------------------------------------------------------------------------------------------------------------
STATUS_RECTS = [(8, 8, 26, 26), (30, 8, 48, 26), (52, 8, 70, 26), (74, 8, 92, 26), (96, 8, 114, 26), (118, 8, 136, 26)]


def test_statuses(pair):
    n = len(STATUS_RECTS)
    mask = np.ones((256, 256), np.uint8)
    mask[8:27, 30:49] = 0          # all of sector 1
    mask[8:27, 52:57] = 0          # five of the nineteen columns of sector 2: 266 of 361 samples stay
    mask[8:27, 96:115] = 0         # sector 4 keeps seven samples: one fewer than P + 2
    mask[8, 96:103] = 1
    with make_engine(*pair, STATUS_RECTS, annular=()) as e:
        g = np.tile(NEAR, (n, 1))
        g[5, 4] = np.nan
        base, bi, bs = e.refine_weighted(guesses=g, return_sums=True)
        rec, info, sums = e.refine_weighted(guesses=g, mask=mask, return_sums=True)
        assert info["status"].tolist() == [ca.ZN_CONVERGED, ca.ZN_TOO_FEW, ca.ZN_CONVERGED, ca.ZN_CONVERGED, ca.ZN_TOO_FEW, ca.ZN_BAD_SEED]
        assert rec["error_code"].tolist() == [0, _ffi.ERROR_SOLVER, 0, 0, _ffi.ERROR_SOLVER, ca.ERROR_BAD_DOMAIN]
        assert info["n_valid"].tolist() == [361, 0, 266, 361, 7, 0] and info["weight_sum"].tolist() == [361, 0, 266, 361, 7, 0]
        assert info["n_eff"].tolist() == [361, 0, 266, 361, 7, 0] and (info["n_points"] == 361).all()
        for s in (1, 4, 5):            # nothing was evaluated: floats and sums 0, the seed as the parameters, no NaN in any byte
            assert not any(info[k][s] for k in FLOATS) and info["iterations"][s] == 0 and info["evaluations"][s] == 0, (s, info[s])
            assert not sums[s].any() and rec["chi"][s] == 0 and rec["iterations"][s] == 0
            assert rec["p"][s].tobytes() == g[s].tobytes()
        assert all(np.isfinite(info[k]).all() for k in info.dtype.names) and np.isfinite(sums).all()
        assert np.isfinite(rec["chi"]).all() and np.isfinite(rec["p"][:5]).all()   # (sector 5 returns its seed, a NaN included)
        assert info["centroid_dx"][1] == 0 and info["centroid_dy"][1] == 0 and info["centroid_dx"][4] == -6.0 and info["centroid_dy"][4] == -9.0
        # the neighbours are untouched by a mask elsewhere
        for s in (0, 3):
            assert rec[s].tobytes() == base[s].tobytes() and info[s].tobytes() == bi[s].tobytes() and sums[s].tobytes() == bs[s].tobytes()
        assert rec[2].tobytes() != base[2].tobytes()
        # min_fraction on both sides of 266 / 361 = 0.7368
        lo = e.refine_weighted(guesses=g, mask=mask, min_fraction=0.73)
        hi = e.refine_weighted(guesses=g, mask=mask, min_fraction=0.74)
        assert lo[0].tobytes() == rec.tobytes() and lo[1].tobytes() == info.tobytes()
        assert hi[1]["status"].tolist() == [ca.ZN_CONVERGED, ca.ZN_TOO_FEW, ca.ZN_TOO_FEW, ca.ZN_CONVERGED, ca.ZN_TOO_FEW, ca.ZN_BAD_SEED]
        assert hi[1]["n_valid"][2] == 266 and hi[1]["evaluations"][2] == 0 and hi[0]["error_code"][2] == _ffi.ERROR_SOLVER
        assert hi[0][0].tobytes() == rec[0].tobytes()
        exact = e.refine_weighted(guesses=g, mask=mask, min_fraction=float(np.float32(266.0 / 361.0)))   # (the float below 266 / 361)
        assert np.float32(266.0 / 361.0) * 361.0 <= 266.0 and exact[1]["status"][2] == ca.ZN_CONVERGED
        # a window so narrow that it dies inside the subset: the samples with t >= 126 have weight 0 and take no part
        narrow = e.refine_weighted(guesses=g, sigma=0.5)[1]
        assert (narrow["n_valid"][:5] < 361).all() and (narrow["n_valid"][:5] >= 9).all() and (narrow["n_eff"][:5] < 4).all()
        assert np.isin(narrow["status"][:5], (ca.ZN_CONVERGED, ca.ZN_MAX_ITERS, ca.ZN_STALLED, ca.ZN_FLAT, ca.ZN_SINGULAR, ca.ZN_NEGATIVE)).all()
        # records as seeds: a bad record passes through, byte for byte
        seeds = np.zeros(n, ca.RESULT_DTYPE)
        seeds["p"][:] = NEAR
        seeds["chi"] = 1.0
        seeds["error_code"][0] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        seeds["iterations"][0] = 50
        seeds["p"][3, 1] = np.inf
        seeds["chi"][2] = 5.0
        out, oi = e.refine_weighted(records=seeds, mask=mask, chi_max=2.0)
        assert oi["status"].tolist() == [ca.ZN_BAD_SEED, ca.ZN_TOO_FEW, ca.ZN_BAD_SEED, ca.ZN_BAD_SEED, ca.ZN_TOO_FEW, ca.ZN_CONVERGED]
        for s in (0, 2, 3):
            assert out[s].tobytes() == seeds[s].tobytes() and not any(oi[k][s] for k in FLOATS) and oi["evaluations"][s] == 0, s
            assert oi["n_valid"][s] == 0 and oi["weight_sum"][s] == 0
        assert e.refine_weighted(records=seeds, mask=mask)[1]["status"][2] == ca.ZN_CONVERGED    # chi_max <= 0: the error code alone


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
        kw = dict(sigma=SIGMA, mask=the_mask())
        a = e.refine_weighted(**kw)
        b = e.refine_weighted(records=first, **kw)
        c = e.refine_weighted(guesses=zr.zero_gradient_seeds(S), **kw)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert (a[1]["status"][[9, 27]] == ca.ZN_BAD_SEED).all() and (c[1]["status"] == ca.ZN_CONVERGED).all()
        ms, count = e.weighted_last()
        assert ms > 0 and sum(count) == S and count == (S - 2, 1, 1)
        after = state()
        for k in kept:
            if k == "counters":
                assert (kept[k] == after[k]).all()
            else:
                assert kept[k].tobytes() == after[k].tobytes(), k
        assert e.correlate_all(zr.zero_gradient_seeds(S)).tobytes() == plain.correlate_all(zr.zero_gradient_seeds(S)).tobytes()
        assert e.last_evaluated_parameters().tobytes() == plain.last_evaluated_parameters().tobytes()


def test_arguments_and_refusals(pair):
    rects = zr.GRID[:9]
    e = make_engine(*pair, rects, annular=(), commit=False)
    lib, h = e.lib, e._h
    seeds = np.zeros(9, ca.RESULT_DTYPE)
    seeds["p"][:] = NEAR
    g = np.tile(NEAR, (9, 1))
    rec = np.full(9, 7, np.uint8).repeat(48).view(ca.RESULT_DTYPE)
    info = np.full(9, 7, np.uint8).repeat(80).view(ca.WEIGHTED_DTYPE)
    sums = np.full((9, ca.ZN_SUMS), 7.0)
    kept = [rec.tobytes(), info.tobytes(), sums.tobytes()]
    ones = np.ones((256, 256), np.uint8)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def config(**kw):
        fields = dict(def_slot=-1, chi_max=0.0, max_iters=-1, precision=0.0, lambda0=0.0, sigma=0.0, min_fraction=0.0, mask_rows=0,
                      mask_cols=0)
        fields.update(kw)
        return _ffi.LkWeightedConfig(**fields)

    def refused(cfg="default", mask=None, records=None, guesses=None, outputs=(rec, info), word=None, **kw):
        if cfg == "default":
            cfg = config(**kw)
        if word is not None:
            cfg.reserved[word] = 1
        rc = lib.lk_refine_weighted(h, C.byref(cfg) if cfg is not None else None, ptr(mask), ptr(records),
                                    _ffi.fptr(guesses) if guesses is not None else None, ptr(outputs[0]), ptr(outputs[1]), ptr(sums))
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and msg.startswith("lk_refine_weighted: "), (rc, msg)   # names the function called
        return msg

    assert "no committed sectors" in refused(guesses=g) and "no committed sectors" in refused(records=seeds)
    e.commit_sectors()
    assert "no solve" in refused()
    assert "no configuration" in refused(None, guesses=g)
    assert "no output" in refused(guesses=g, outputs=(None, None))
    for word in range(3):
        assert "reserved" in refused(guesses=g, word=word)
    assert "both given" in refused(records=seeds, guesses=g)
    assert "chi_max" in refused(records=seeds, chi_max=np.nan) and "chi_max" in refused(guesses=g, chi_max=np.inf)
    assert "precision" in refused(guesses=g, precision=np.nan) and "lambda0" in refused(guesses=g, lambda0=np.inf)
    assert "ring slot" in refused(guesses=g, def_slot=0) and "def_slot" in refused(guesses=g, def_slot=-2)
    # this pass's own
    for bad in (-1.0, np.nan, np.inf):
        assert "sigma" in refused(guesses=g, sigma=bad)
    assert "sigma" in refused(guesses=g, sigma=1e-30)
    for bad in (-0.1, 1.5, np.nan):
        assert "min_fraction" in refused(guesses=g, min_fraction=bad)
    assert "without dimensions" in refused(guesses=g, mask=ones) and "without dimensions" in refused(guesses=g, mask=ones, mask_rows=256)
    assert "without a mask" in refused(guesses=g, mask_rows=256, mask_cols=256)
    for rows, cols in ((255, 256), (256, 255), (128, 128), (512, 512)):
        assert "mask dimensions" in refused(guesses=g, mask=ones, mask_rows=rows, mask_cols=cols)
    assert lib.lk_refine_weighted(None, C.byref(config()), None, None, _ffi.fptr(g), ptr(rec), ptr(info), None) == ca.ERROR_BAD_DOMAIN
    assert [rec.tobytes(), info.tobytes(), sums.tobytes()] == kept       # every refusal left the outputs as they were
    with pytest.raises(ValueError):
        e.refine_weighted(guesses=g, mask=np.ones(256, np.uint8))
    with pytest.raises(ca.LkError):
        e.refine_weighted(guesses=g, mask=np.ones((128, 128), np.uint8))
    # either output alone; the defaults of the C configuration are lk_config's; a bool mask is a mask
    cfg = config(mask_rows=256, mask_cols=256)
    assert lib.lk_refine_weighted(h, C.byref(cfg), ptr(ones), None, _ffi.fptr(g), ptr(rec), None, None) == 0
    assert lib.lk_refine_weighted(h, C.byref(cfg), ptr(ones), ptr(seeds), None, None, ptr(info), None) == 0
    both = e.refine_weighted(guesses=g, mask=np.ones((256, 256), bool), max_iters=50, precision=1e-3, lambda0=1e-3)
    assert rec.tobytes() == both[0].tobytes() and info.tobytes() == both[1].tobytes() and (info["status"] == ca.ZN_CONVERGED).all()
    # a solve in flight refuses the engine-held records and finishes normally afterwards
    e.correlate_all_async()
    assert "waited for" in refused()
    solved = e.wait_results()
    assert e.refine_weighted(sigma=SIGMA)[0].tobytes() == e.refine_weighted(records=solved, sigma=SIGMA)[0].tobytes()
    # level 1: the mask is the level image's, sigma and the centroid are level-0 pixels
    e.close()
    with ca.HipCorrelationEngine(fitting_model=ca.FM_UVUXUYVXVY, precision=zr.PRECISION, py_start=1, py_stop=2) as e1:
        e1.set_undeformed_image(pair[0])
        e1.set_deformed_image(pair[1])
        e1.resetPolygon_rect(0, 40, 40, 78, 78)
        e1.commit_sectors()
        g1 = zr.zero_gradient_seeds(1)
        with pytest.raises(ca.LkError):
            e1.refine_weighted(guesses=g1, mask=ones)
        half = np.ones((128, 128), np.uint8)
        half[:, :25] = 0
        r1, i1 = e1.refine_weighted(guesses=g1, sigma=6.0, mask=half)
        assert i1["status"][0] == ca.ZN_CONVERGED and r1["error_code"][0] == 0
        xy = zr.rect_rows(20, 20, 39, 39)    # the rectangle at level 1
        cx, cy = (np.float32(t) * np.float32(0.5) for t in e1.sector_info(0)[1:3])
        pro = wr.prologue(xy, cx, cy, wr.sample_weights(xy, cx, cy, wr.inv_of(6.0, level=1), half), level=1)
        assert i1["n_points"][0] == len(xy) and 0 < i1["n_valid"][0] == pro["n_valid"] < len(xy)
        assert abs(float(i1["weight_sum"][0]) - pro["sw"]) <= 4 * 2.0 ** -24 * pro["sw"]
        assert abs(float(i1["n_eff"][0]) - pro["n_eff"]) <= 4 * 2.0 ** -24 * pro["n_eff"] and pro["n_eff"] < pro["n_valid"]
        assert abs(float(i1["centroid_dx"][0]) - pro["centroid"][0]) <= 1e-5 and abs(float(i1["centroid_dy"][0]) - pro["centroid"][1]) <= 1e-5
        assert pro["centroid"][0] > 0.5      # in level-0 pixels: the mask cut the left columns
    bare = make_engine(None, None, rects, annular=())
    rc = bare.lib.lk_refine_weighted(bare._h, C.byref(config()), None, None, _ffi.fptr(g), ptr(rec), ptr(info), None)
    msg = bare.lib.lk_last_error_string(bare._h).decode()
    assert rc == ca.ERROR_BAD_DOMAIN and "image" in msg and msg.startswith("lk_refine_weighted: "), (rc, msg)
    bare.close()
