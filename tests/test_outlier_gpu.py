"""Outlier flags (lk_flag_outliers, include/lk_engine.h) against the numpy restatement of the header (outlier_ref.py) on
synthetic records; known answers (planted outliers on an affine field); both lane groups and both storage paths; that
nothing of the engine moves but the marked error codes; end to end on a pair with a patch that moved on its own; arguments.

Plain mode is compared byte for byte: a median does not depend on the visiting order and the ratio is correctly rounded
double arithmetic.  Detrended mode: the device and the restatement differ only in the order of the plane's double sums of
at most a few hundred terms (as in test_strain_gpu.py), so an e-valued field (med, mad) agrees within
tol_e = 2^-22 |ref| + 1e-9 max(U, 1), U the largest |displacement| of the good records; a perturbation d of e_s, med and
mad moves the ratio by at most (2 + ratio) d / eps, so the ratios agree within (2 + ratio) tol_e / eps + 2^-22 ratio
(tol_e there: the larger of med's and mad's).  Flags must be equal; the inputs are seeded so that no reference ratio lies
within that bound of the threshold, which each comparison asserts of the reference first."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi, speckle

import outlier_ref as oref
from test_strain_gpu import (LAYOUTS, centres, device_records, grid_rects, make_engine, strain_reference, synthetic_records,
                             check_against_reference as check_strain)

pytestmark = pytest.mark.gpu

SIDE = 19
MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
EPS, THRESHOLD = 0.02, 3.0


@pytest.fixture(scope="module")
def small_pair():
    return speckle.speckle_pair(256, 256, p=(1.3, -0.7, 0.002, 0.0, 0.0, -0.001), seed=5)


def scale_of(rec, model, chi_max):
    good = oref.is_good(rec, _ffi.N_PARAMS[model], chi_max)
    return float(np.abs(rec["p"][good][:, :1 if model == ca.FM_U else 2]).max()) if good.any() else 1.0


def check(got, n_got, ref, U, detrend, what, eps=EPS, threshold=THRESHOLD):
    want, ratio, history = ref
    assert np.array_equal(want["status"] == ca.OUTLIER_FLAGGED, history[-1])
    tol = oref.tolerances(want, U, eps)
    if detrend:   # a condition on the inputs: no reference ratio so near the threshold that the two could differ
        live = np.isin(want["status"], (ca.OUTLIER_OK, ca.OUTLIER_FLAGGED))
        for k, name in enumerate(("ratio_u", "ratio_v")):
            assert (np.abs(ratio[live, k] - threshold) > tol[name][live]).all(), (what, "a ratio at the threshold")
    assert np.array_equal(got["status"], want["status"]), (what, np.flatnonzero(got["status"] != want["status"]))
    assert np.array_equal(got["neighbours"], want["neighbours"]), what
    assert n_got == int(history[-1].sum()), what
    worst = 0.0
    if not detrend:
        assert got.tobytes() == want.tobytes(), what
    else:
        for name in oref.FLOATS:
            err = np.abs(got[name].astype(np.float64) - want[name].astype(np.float64))
            worst = max(worst, float((err / tol[name]).max()))
            assert (err <= tol[name]).all(), (what, name, int(np.argmax(err / tol[name])), float(err.max()))
    dead = np.isin(want["status"], (ca.OUTLIER_TOO_FEW, ca.OUTLIER_DEGENERATE))
    for name in oref.FLOATS:
        assert not got[name][dead].any(), (what, name)
    bad = want["status"] == ca.OUTLIER_NOT_GOOD
    assert not got["ratio_u"][bad].any() and not got["ratio_v"][bad].any()
    return worst


# ---- 1. against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("model", MODELS)
def test_flags_match_the_restatement(small_pair, model, layout):
    rects, annular = LAYOUTS[layout]
    chi_max = 8.0
    with make_engine(*small_pair, rects, model=model, annular=annular) as e:
        cen = centres(e)
        S = e.n_sectors
        rng = np.random.default_rng(200 * model + len(layout))
        rec = synthetic_records(S, rng, chi_max, 0.2)       # 20 % bad in each of the three ways
        rec["p"][rng.permutation(S)[:5], :2] *= -0.0        # some zeros of either sign among the displacements
        U = scale_of(rec, model, chi_max)
        seen = set()
        for detrend in (0, 1):
            for radius, min_nb, passes in ((1.0 * SIDE, 4 if detrend else 3, 1), (1.5 * SIDE, 4, 1), (2.5 * SIDE, 5, 1),
                                           (2.5 * SIDE, 4, 2)):
                assert radius == np.float32(radius)
                ref = oref.flag_reference(cen, rec, model, radius, chi_max, EPS, THRESHOLD, min_nb, bool(detrend), passes)
                got, n = e.flag_outliers(radius, chi_max=chi_max, eps=EPS, threshold=THRESHOLD, min_neighbours=min_nb,
                                         detrend=detrend, passes=passes, records=rec)
                worst = check(got, n, ref, U, detrend, (layout, model, detrend, radius, passes))
                print(f"{layout} model {model} detrend {detrend} radius {radius} passes {passes}: worst error / tolerance "
                      f"{worst:.3g}, statuses {np.bincount(ref[0]['status'], minlength=5).tolist()}, neighbours "
                      f"{ref[0]['neighbours'].min()}..{ref[0]['neighbours'].max()}")
                seen |= set(ref[0]["status"].tolist())
                if layout == "column" and detrend:
                    assert np.isin(ref[0]["status"], (ca.OUTLIER_DEGENERATE, ca.OUTLIER_TOO_FEW)).all()
                elif layout == "grid" and radius == 1.0 * SIDE:
                    # the four neighbours at exactly one pitch count; the sector itself does not; a corner has two
                    assert ref[0]["neighbours"].max() <= 4
                    assert (ref[0]["status"][[0, 11, 132, 143]] == ca.OUTLIER_TOO_FEW).all()
        if layout == "column":   # all twelve good: every detrended window is two to four centres on a line
            clean = synthetic_records(S, rng, chi_max, 0.0)
            clean["error_code"], clean["chi"] = 0, 1.0
            clean["p"] = np.nan_to_num(clean["p"])
            got, n = e.flag_outliers(2.5 * SIDE, chi_max=chi_max, records=clean)
            check(got, n, oref.flag_reference(cen, clean, model, 2.5 * SIDE, chi_max), scale_of(clean, model, chi_max), 1, "clean column")
            assert (got["status"][2:10] == ca.OUTLIER_DEGENERATE).all() and got["neighbours"].tolist() == [2, 3] + [4] * 8 + [3, 2]
            assert n == 0
        else:
            assert {ca.OUTLIER_OK, ca.OUTLIER_FLAGGED, ca.OUTLIER_TOO_FEW, ca.OUTLIER_NOT_GOOD} <= seen


# ---- 2. known answers ----------------------------------------------------------------------------------------------------
def planted_records(cen, seed):
    """an exact affine field of gradient 0.02 with six sectors moved by +-0.5 px in one component"""
    rng = np.random.default_rng(seed)
    c = cen.astype(np.float64)
    rec = np.zeros(len(cen), ca.RESULT_DTYPE)
    rec["p"][:, 0] = 1.0 + 0.02 * c[:, 0] - 0.004 * c[:, 1]
    rec["p"][:, 1] = -2.0 + 0.006 * c[:, 0] + 0.02 * c[:, 1]
    rec["chi"], rec["n_points"] = 1.0, 361
    idx = rng.choice(len(cen), 6, replace=False)
    sign = rng.choice([-1.0, 1.0], (6, 2))
    comp = rng.integers(0, 2, 6)
    for k, s in enumerate(idx):
        rec["p"][s, comp[k]] += np.float32(0.5 * sign[k, comp[k]])
    return rec, np.sort(idx)


def test_planted_outliers_on_an_affine_field(small_pair):
    """Seed 7 (chosen with the restatement on the CPU): the planted sectors are 82, 87, 96, 111, 127, 131; pass 1 of the
    detrended test at 2.5 pitches finds all six and also flags 143, the corner whose plane sector 131 bends; pass 2, with
    the flagged seven out of every window, leaves exactly the six.  The plain test finds one of the six and flags a healthy
    edge sector - whatever the restatement says, the device says."""
    with make_engine(*small_pair, grid_rects(), model=ca.FM_UV) as e:
        cen = centres(e)
        rec, idx = planted_records(cen, 7)
        assert idx.tolist() == [82, 87, 96, 111, 127, 131]
        U = scale_of(rec, ca.FM_UV, 0)
        radius = 2.5 * SIDE
        flagged = {}
        for passes in (1, 2):
            ref = oref.flag_reference(cen, rec, ca.FM_UV, radius, passes=passes)
            got, n = e.flag_outliers(radius, passes=passes, records=rec)
            check(got, n, ref, U, 1, ("planted", passes))
            flagged[passes] = np.flatnonzero(got["status"] == ca.OUTLIER_FLAGGED).tolist()
        assert flagged[1] == idx.tolist()[:-1] + [131, 143] and flagged[2] == idx.tolist()
        ref = oref.flag_reference(cen, rec, ca.FM_UV, radius, min_neighbours=3, detrend=False)
        got, n = e.flag_outliers(radius, detrend=0, records=rec)
        check(got, n, ref, U, 0, "planted, plain")
        plain = set(np.flatnonzero(got["status"] == ca.OUTLIER_FLAGGED).tolist())
        assert len(plain & set(idx.tolist())) == 1 and len(plain - set(idx.tolist())) == 1
        # a sector that is not good reports its neighbours' median and is never flagged - here a planted one
        spoiled = rec.copy()
        spoiled["error_code"][96] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        ref = oref.flag_reference(cen, spoiled, ca.FM_UV, radius)
        got, n = e.flag_outliers(radius, records=spoiled)
        check(got, n, ref, U, 1, "not good")
        assert got["status"][96] == ca.OUTLIER_NOT_GOOD and ref[0]["status"][96] == ca.OUTLIER_NOT_GOOD
        assert got["ratio_u"][96] == 0 and got["ratio_v"][96] == 0
        assert got["med_u"][96] == ref[0]["med_u"][96] != 0 or got["med_v"][96] == ref[0]["med_v"][96] != 0
        # marking: the records come back with the new code in the flagged sectors and not a byte moved elsewhere
        got, n, marked = e.flag_outliers(radius, passes=2, mark=1, records=rec, return_records=True)
        assert np.flatnonzero(marked["error_code"] == ca.ERROR_OUTLIER).tolist() == idx.tolist()
        marked["error_code"][idx] = 0
        assert marked.tobytes() == rec.tobytes()
        _, _, plain_copy = e.flag_outliers(radius, passes=2, mark=0, records=rec, return_records=True)
        assert plain_copy.tobytes() == rec.tobytes()


# ---- 3. both widths, both storage paths -----------------------------------------------------------------------------------
COMBOS = ((None, None), ("16", None), ("64", None), ("16", "0"), ("64", "0"), ("16", "32"), ("64", "64"))


def set_hooks(monkeypatch, group, cap):
    for key, val in (("LK_OUTLIER_GROUP", group), ("LK_OUTLIER_LDS_CAP", cap)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, val)


def test_both_lane_groups_and_both_storage_paths(small_pair, monkeypatch):
    """LK_OUTLIER_GROUP forces the lane group, LK_OUTLIER_LDS_CAP the members a group may keep in LDS: 0 re-walks every
    window from global memory in every counting round, 32 / 64 leave a lane two rows / one row (windows of 20 members fit,
    those of 56 at an off-lattice centre may not).  Plain mode: the same bytes from all of them."""
    rects, annular = LAYOUTS["grid_and_annular"]
    chi_max = 8.0
    with make_engine(*small_pair, rects, annular=annular) as e:
        cen = centres(e)
        rec = synthetic_records(e.n_sectors, np.random.default_rng(17), chi_max, 0.07)
        U = scale_of(rec, ca.FM_UVUXUYVXVY, chi_max)
        for radius in (2.5 * SIDE, 1000.0):
            for detrend in (0, 1):
                ref = oref.flag_reference(cen, rec, ca.FM_UVUXUYVXVY, radius, chi_max, min_neighbours=4, detrend=bool(detrend), passes=2)
                first = None
                for group, cap in COMBOS:
                    set_hooks(monkeypatch, group, cap)
                    got, n = e.flag_outliers(radius, chi_max=chi_max, min_neighbours=4, detrend=detrend, passes=2, records=rec)
                    check(got, n, ref, U, detrend, (radius, detrend, group, cap))
                    assert got.tobytes() == e.flag_outliers(radius, chi_max=chi_max, min_neighbours=4, detrend=detrend, passes=2, records=rec)[0].tobytes()
                    first = got if first is None else first
                    if not detrend:
                        assert got.tobytes() == first.tobytes()


def test_a_window_of_more_than_500_members(small_pair, monkeypatch):
    """32 x 32 sectors of 8 x 8, radius 13 pitches: an interior window has 528 members, more than 16 lanes can keep (16 x 16),
    so the 16-lane kernel re-walks by itself where the 64-lane one (the default here: all 1024 sectors are candidates)
    keeps them in LDS."""
    rects = grid_rects(n=32, side=8, x0=0, y0=0)
    with make_engine(*small_pair, rects, model=ca.FM_UV) as e:
        cen = centres(e)
        rec = synthetic_records(e.n_sectors, np.random.default_rng(23), 8.0, 0.02)
        U = scale_of(rec, ca.FM_UV, 8.0)
        radius = 13.0 * 8
        for detrend in (0, 1):
            ref = oref.flag_reference(cen, rec, ca.FM_UV, radius, 8.0, min_neighbours=4, detrend=bool(detrend))
            assert ref[0]["neighbours"].max() > 500
            first = None
            for group, cap in COMBOS[:5]:
                set_hooks(monkeypatch, group, cap)
                got, n = e.flag_outliers(radius, chi_max=8.0, min_neighbours=4, detrend=detrend, records=rec)
                check(got, n, ref, U, detrend, ("wide", detrend, group, cap))
                first = got if first is None else first
                if not detrend:
                    assert got.tobytes() == first.tobytes()


# ---- 4. engine state ------------------------------------------------------------------------------------------------------
def test_engine_state_moves_only_by_the_marks(small_pair):
    rects = grid_rects(n=8)
    S = len(rects)
    with make_engine(*small_pair, rects) as e:
        g = np.zeros((S, 6), np.float32)
        g[[9, 27], 0] = 300.0
        e.correlate_all(g)
        e.reseed_failed(1.5 * SIDE)

        def state():
            return dict(records=device_records(e), guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(),
                        stats=e.sector_stats(), reseed=e.reseed_info(), strain=e.strain_field(2.5 * SIDE),
                        counters=np.array(sorted(e.stats().items()), dtype=object))

        def same(kept, after, but=()):
            for k in kept:
                if k in but:
                    continue
                if k == "counters":
                    assert (kept[k] == after[k]).all()
                else:
                    assert kept[k].tobytes() == after[k].tobytes(), k

        kept = state()
        # a real solve's noise is thousandths of a pixel: a threshold this low flags some sectors
        kw = dict(eps=1e-4, threshold=2.0, passes=2)
        a, n_a = e.flag_outliers(2.5 * SIDE, **kw)
        b, n_b = e.flag_outliers(2.5 * SIDE, **kw)
        assert a.tobytes() == b.tobytes() and n_a == n_b and 1 <= n_a < S
        assert a.tobytes() == e.flag_outliers(2.5 * SIDE, records=kept["records"], **kw)[0].tobytes()
        same(kept, state())
        # a rebuild of the lists that waits for the next solve (here: after a change of mode) keeps waiting
        e.set_reference_order(1)
        assert e.flag_outliers(2.5 * SIDE, **kw)[0].tobytes() == a.tobytes()
        same(kept, state(), but=("counters",))
        # mark = 1 on the engine-held records is refused in that mode - and has written nothing
        with pytest.raises(ca.LkError, match="reference-order"):
            e.flag_outliers(2.5 * SIDE, mark=1, **kw)
        same(kept, state(), but=("counters",))
        e.set_reference_order(0)
        # mark = 1: exactly the flagged sectors' error codes change
        c, n_c, returned = e.flag_outliers(2.5 * SIDE, mark=1, return_records=True, **kw)
        assert c.tobytes() == a.tobytes() and n_c == n_a
        after = state()
        same(kept, after, but=("records", "strain"))
        flagged = a["status"] == ca.OUTLIER_FLAGGED
        assert returned.tobytes() == after["records"].tobytes()
        assert (after["records"]["error_code"][flagged] == ca.ERROR_OUTLIER).all()
        restored = after["records"].copy()
        restored["error_code"][flagged] = kept["records"]["error_code"][flagged]
        assert restored.tobytes() == kept["records"].tobytes()
        assert (after["strain"]["status"][flagged] != ca.STRAIN_OK).all()


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------
MID = 5 * 12 + 6
PATCH_OFFSET, PATCH_MARGIN, E2E_CHI_MAX = (4, 3), 2, 100.0


def patched_pair():
    """a global translation of (1.3, -0.7); the speckles that sector MID's pixels move onto (and two pixels around) carry
    (5.3, 2.3) instead"""
    und, dfm = speckle.speckle_pair(256, 256, p=(1.3, -0.7, 0, 0, 0, 0), seed=5)
    und2, dfm2 = speckle.speckle_pair(256, 256, p=(1.3 + PATCH_OFFSET[0], -0.7 + PATCH_OFFSET[1], 0, 0, 0, 0), seed=5)
    assert (und == und2).all()
    x0, y0, x1, y1 = grid_rects()[MID]
    sx, sy, m = 1 + PATCH_OFFSET[0], -1 + PATCH_OFFSET[1], PATCH_MARGIN
    out = dfm.copy()
    out[y0 + sy - m:y1 + sy + m + 1, x0 + sx - m:x1 + sx + m + 1] = dfm2[y0 + sy - m:y1 + sy + m + 1, x0 + sx - m:x1 + sx + m + 1]
    return und, out


def test_end_to_end_a_patch_that_moved_on_its_own(oracle):
    und, dfm = patched_pair()
    rects = grid_rects()
    S = len(rects)
    radius = 2.5 * SIDE
    with make_engine(und, dfm, rects, model=ca.FM_UV) as e:
        cen = centres(e)
        # the construction, by the CPU oracle: the sector converges cleanly, 4 and 3 pixels away from its neighbours; the
        # three neighbours the patch spills into end with chi in the thousands and fail the good rule at chi_max = 100
        o = oracle.Oracle(model=oracle.FM_UV, precision=1e-3, py_stop=2)
        o.set_image(0, und)
        o.set_image(1, dfm)
        want = o.correlate_sectors([oracle.rect_points(*r) for r in rects], cen, np.zeros((S, 6), np.float32))
        assert want["error_code"][MID] == 0 and want["chi"][MID] < 10
        others = oref.is_good(want, 2, E2E_CHI_MAX)
        others[MID] = False
        assert others.sum() >= S - 4
        assert (np.abs(want["p"][MID, :2] - want["p"][others][:, :2]) > 1.0).all()
        ref = oref.flag_reference(cen, want, ca.FM_UV, radius, E2E_CHI_MAX)
        assert np.flatnonzero(ref[2][0]).tolist() == [MID]
        # the device, default mode
        rec = e.correlate_all(np.zeros((S, 6), np.float32))
        assert rec["error_code"][MID] == 0 and rec["chi"][MID] < 10
        got, n = e.flag_outliers(radius, chi_max=E2E_CHI_MAX)
        check(got, n, oref.flag_reference(cen, rec, ca.FM_UV, radius, E2E_CHI_MAX), scale_of(rec, ca.FM_UV, E2E_CHI_MAX), 1, "end to end")
        assert np.flatnonzero(got["status"] == ca.OUTLIER_FLAGGED).tolist() == [MID] and n == 1
        print(f"end to end: ratios of the patch sector {got['ratio_u'][MID]:.1f}, {got['ratio_v'][MID]:.1f}; largest other "
              f"{max(np.delete(got['ratio_u'], MID).max(), np.delete(got['ratio_v'], MID).max()):.2f}")
        got, n, marked = e.flag_outliers(radius, chi_max=E2E_CHI_MAX, mark=1, return_records=True)
        assert marked["error_code"][MID] == ca.ERROR_OUTLIER and n == 1
        assert device_records(e).tobytes() == marked.tobytes()
        # the strain field fills the sector from its neighbours, and is the restatement's field of the marked records
        strain = e.strain_field(radius, chi_max=E2E_CHI_MAX)
        assert strain["status"][MID] == ca.STRAIN_FILLED
        check_strain(strain, strain_reference(cen, marked, ca.FM_UV, radius, E2E_CHI_MAX), scale_of(marked, ca.FM_UV, E2E_CHI_MAX), "marked")
        near = [s for s in range(S) if s != MID and (s // 12 - 5) ** 2 + (s % 12 - 6) ** 2 <= 6]
        assert len(near) == 20 and (strain["neighbours"][near] <= 20).all()   # the sector has left its neighbours' windows
        # the recovery pass retries the marked sector; every sector it did not retry stays byte for byte
        after, _ = e.reseed_failed(1.5 * SIDE)
        info = e.reseed_info()
        assert info["status"][MID] in (ca.RESEED_RECOVERED, ca.RESEED_NOT_IMPROVED)
        keep = np.ones(S, bool)
        keep[MID] = False
        assert after[keep].tobytes() == marked[keep].tobytes()
        assert (info["status"][keep] == ca.RESEED_GOOD).all()


# ---- 6. arguments -----------------------------------------------------------------------------------------------------------
def test_arguments_and_refusals(small_pair):
    rects = grid_rects(n=3)
    e = make_engine(*small_pair, rects, commit=False)
    lib, h = e.lib, e._h
    good_cfg = (47.5, 0.0, 0.02, 3.0, 4, 1, 1, 0)
    out = np.zeros(9, ca.OUTLIER_DTYPE)
    rec = np.zeros(9, ca.RESULT_DTYPE)
    rec["p"][:, 0] = np.arange(9)

    def cfg_with(**kw):
        names = [f for f, _ in _ffi.LkOutlierConfig._fields_]
        vals = list(good_cfg)
        for k, v in kw.items():
            vals[names.index(k)] = v
        return _ffi.LkOutlierConfig(*vals)

    def refused(c=cfg_with(), records=None, output=out):
        rc = lib.lk_flag_outliers(h, C.byref(c) if c is not None else None,
                                  records.ctypes.data_as(C.c_void_p) if records is not None else None,
                                  output.ctypes.data_as(C.c_void_p) if output is not None else None, None, None)
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and "lk_flag_outliers" in msg, (rc, msg)
        return msg

    assert "no committed sectors" in refused()
    assert "no committed sectors" in refused(records=rec)
    e.commit_sectors()
    assert "no solve" in refused()                            # records == NULL before any batch solve
    assert "configuration" in refused(None)
    assert "output" in refused(output=None)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "radius" in refused(cfg_with(radius=bad), records=rec)
        assert "eps" in refused(cfg_with(eps=bad), records=rec)
        assert "threshold" in refused(cfg_with(threshold=bad), records=rec)
    for bad in (float("nan"), float("inf")):
        assert "chi_max" in refused(cfg_with(chi_max=bad), records=rec)
    for bad in (3, 0, -1):
        assert "min_neighbours" in refused(cfg_with(min_neighbours=bad), records=rec)
    assert "min_neighbours" in refused(cfg_with(min_neighbours=2, detrend=0), records=rec)
    for bad in (0, 5, -1):
        assert "passes" in refused(cfg_with(passes=bad), records=rec)
    for bad in (-1, 2):
        assert "detrend" in refused(cfg_with(detrend=bad), records=rec)
        assert "mark" in refused(cfg_with(mark=bad), records=rec)
    assert lib.lk_flag_outliers(None, C.byref(cfg_with()), None, out.ctypes.data_as(C.c_void_p), None, None) == ca.ERROR_BAD_DOMAIN
    # records passed in need no solve; min_neighbours = 3 is allowed without the plane
    got, n = e.flag_outliers(47.5, records=rec)
    assert got["neighbours"].tolist() == [7, 8, 7, 8, 8, 8, 7, 8, 7] and n == 0   # (opposite corners are 2.83 pitches apart)
    got, n = e.flag_outliers(19.0, min_neighbours=3, detrend=0, records=rec)
    assert got["neighbours"].tolist() == [2, 3, 2, 3, 4, 3, 2, 3, 2]
    assert (got["status"] == ca.OUTLIER_TOO_FEW).tolist() == [True, False, True, False, False, False, True, False, True]
    # mark = 1 on records passed in is allowed in reference-order mode: nothing of the engine is written
    e.set_reference_order(1)
    _, _, back = e.flag_outliers(47.5, mark=1, records=rec, return_records=True)
    assert back.tobytes() == rec.tobytes()
    e.set_reference_order(0)
    e.correlate_all_async()
    assert "waited for" in refused()
    solved = e.wait_results()
    assert (solved["error_code"] == 0).all()
    assert e.flag_outliers(47.5)[0].tobytes() == e.flag_outliers(47.5, records=solved)[0].tobytes()
    e.close()
