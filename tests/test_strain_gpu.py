"""Strain field (lk_strain_field, include/lk_engine.h): the windowed plane fit against a float64 brute force over all pairs
on synthetic records; known answers (an affine field, a quadratic one, a failed sector filled from its neighbours); end to
end behind a reference-order solve and behind the recovery pass; that nothing of the engine moves; arguments.

Tolerance of the comparisons with the restatement (every float field): 2^-22 |ref| + 1e-9 U / h, with U the largest
|displacement| of the good records and h the grid pitch.  The device and the restatement differ only in the order of
double sums of at most 200 terms (about 1e-13 relative on moments whose condition number, in units of h, stays below about
100 for the half windows at an edge), so 1e-9 leaves more than three decades; the first term is the float rounding of the
outputs.  A note on the radius: 2.5 pitches is exactly 47.5, but no two centres of an integer lattice are 2.5 pitches apart
(i^2 + j^2 = 6.25 has no solution); the pairs AT the radius, which must be counted, are those of the 1.0-pitch case."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi, speckle
from records_ref import synthetic_records  # noqa: F401  (other test modules import it from here)

pytestmark = pytest.mark.gpu

SIDE, X0, Y0 = 19, 8, 8                     # 19 x 19 sectors; 12 x 12 of them fit a 256 x 256 pair
PRECISION = 1e-3
MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
FLOATS = ("u", "v", "ux", "uy", "vx", "vy", "exx", "eyy", "exy", "e1", "e2", "theta", "residual")


def grid_rects(n=12, side=SIDE, x0=X0, y0=Y0, columns=None):
    """sector i * n + j = column i, row j (lk_set_rect_grid's numbering)"""
    return [(x0 + side * i, y0 + side * j, x0 + side * i + side - 1, y0 + side * j + side - 1)
            for i in range(n if columns is None else columns) for j in range(n)]


def make_engine(und, dfm, rects, model=ca.FM_UVUXUYVXVY, annular=(), commit=True):
    e = ca.HipCorrelationEngine(fitting_model=model, precision=PRECISION, py_stop=2)
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    for s, r in enumerate(rects):
        e.resetPolygon_rect(s, *r)
    for k, q in enumerate(annular):
        e.resetPolygon_annular(len(rects) + k, *q)
    if commit:
        e.commit_sectors()
    return e


def centres(e):
    return np.float32([e.sector_info(s)[1:] for s in range(e.n_sectors)])


def is_good(rec, n_params, chi_max):
    ok = (rec["error_code"] == 0) & np.isfinite(rec["chi"]) & np.isfinite(rec["p"][:, :n_params]).all(axis=1)
    if chi_max > 0:
        with np.errstate(invalid="ignore"):
            ok &= rec["chi"] <= np.float32(chi_max)
    return ok


@pytest.fixture(scope="module")
def small_pair():
    return speckle.speckle_pair(256, 256, p=(1.3, -0.7, 0.002, 0.0, 0.0, -0.001), seed=5)


# ---- the float64 restatement of the header ----------------------------------------------------------------------------
def tensor_reference(tensor, g32):
    g = np.asarray(g32, np.float32).astype(np.float64)
    ux, uy, vx, vy = g
    if tensor == ca.STRAIN_GREEN_LAGRANGE:
        exx = ux + 0.5 * (ux * ux + vx * vx)
        eyy = vy + 0.5 * (uy * uy + vy * vy)
        exy = 0.5 * (uy + vx) + 0.5 * (ux * uy + vx * vy)
    else:
        exx, eyy, exy = ux, vy, 0.5 * (uy + vx)
    rad = np.sqrt(((exx - eyy) / 2) ** 2 + exy ** 2)
    return [exx, eyy, exy, (exx + eyy) / 2 + rad, (exx + eyy) / 2 - rad, 0.5 * np.arctan2(2 * exy, exx - eyy)]


def strain_reference(cen, rec, model, radius, chi_max=0.0, min_neighbours=3, tensor=ca.STRAIN_GREEN_LAGRANGE):
    """-> (STRAIN_DTYPE-like float64 table [S][13], neighbours, status, D / (Cxx Cyy) or nan)"""
    good = is_good(rec, _ffi.N_PARAMS[model], chi_max)
    c = cen.astype(np.float64)
    with np.errstate(invalid="ignore"):
        u = rec["p"][:, 0].astype(np.float64)
        v = rec["p"][:, 1].astype(np.float64) if model != ca.FM_U else np.zeros(len(c))
    S = len(c)
    vals, nbrs, status, ratio = np.zeros((S, 13)), np.zeros(S, np.int32), np.zeros(S, np.int32), np.full(S, np.nan)
    r2 = np.float64(np.float32(radius)) ** 2
    for s in range(S):
        d = c - c[s]
        near = good & (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= r2)
        n = int(near.sum())
        nbrs[s] = n
        if n < min_neighbours:
            status[s] = ca.STRAIN_TOO_FEW
            continue
        x, y, uu, vv = d[near, 0], d[near, 1], u[near], v[near]
        Sx, Sy, Su, Sv = x.sum(), y.sum(), uu.sum(), vv.sum()
        Cxx, Cxy, Cyy = (x * x).sum() - Sx * Sx / n, (x * y).sum() - Sx * Sy / n, (y * y).sum() - Sy * Sy / n
        Cxu, Cyu = (x * uu).sum() - Sx * Su / n, (y * uu).sum() - Sy * Su / n
        Cxv, Cyv = (x * vv).sum() - Sx * Sv / n, (y * vv).sum() - Sy * Sv / n
        D = Cxx * Cyy - Cxy * Cxy
        if Cxx * Cyy != 0:
            ratio[s] = D / (Cxx * Cyy)
        if Cxx * Cyy == 0 or D <= 1e-6 * Cxx * Cyy:
            status[s] = ca.STRAIN_DEGENERATE
            continue
        status[s] = ca.STRAIN_OK if good[s] else ca.STRAIN_FILLED
        ux, uy = (Cyy * Cxu - Cxy * Cyu) / D, (Cxx * Cyu - Cxy * Cxu) / D
        vx, vy = (Cyy * Cxv - Cxy * Cyv) / D, (Cxx * Cyv - Cxy * Cxv) / D
        u0, v0 = Su / n - ux * Sx / n - uy * Sy / n, Sv / n - vx * Sx / n - vy * Sy / n
        ru, rv = uu - (u0 + ux * x + uy * y), vv - (v0 + vx * x + vy * y)
        res = np.sqrt((ru * ru + rv * rv).sum() / n)
        vals[s] = [u0, v0, ux, uy, vx, vy] + tensor_reference(tensor, [ux, uy, vx, vy]) + [res]
    return vals, nbrs, status, ratio


def scale_of(rec, model, chi_max):
    good = is_good(rec, _ffi.N_PARAMS[model], chi_max)
    return float(np.abs(rec["p"][good][:, :1 if model == ca.FM_U else 2]).max())


def check_against_reference(got, ref, U, what, pitch=SIDE):
    """pitch: the h of the tolerance (the docstring above) - this file's lattice, or the nominal pitch of another layout
    (tests/test_cell_grid_gpu.py)"""
    vals, nbrs, status, _ = ref
    assert np.array_equal(got["status"], status), what
    assert np.array_equal(got["neighbours"], nbrs), what
    assert not got["reserved"].any()
    worst = 0.0
    for k, name in enumerate(FLOATS):
        tol = 2.0 ** -22 * np.abs(vals[:, k]) + 1e-9 * U / pitch
        err = np.abs(got[name].astype(np.float64) - vals[:, k])
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (what, name, int(np.argmax(err / tol)), float(err.max()))
    dead = np.isin(status, (ca.STRAIN_TOO_FEW, ca.STRAIN_DEGENERATE))
    for name in FLOATS:
        assert not got[name][dead].any(), (what, name)
    return worst


# ---- 1. against the float64 brute force over all pairs ------------------------------------------------------------------
ANNULAR = [(20.0, 12.0, 0.3 + 1.1 * k, 0.9, 120.0 + 7.0 * k, 118.0 - 5.0 * k, 6) for k in range(4)]
LAYOUTS = {
    "grid": (grid_rects(), ()),
    "grid_and_annular": (grid_rects(), ANNULAR),           # four centres off the lattice (float means)
    "column": (grid_rects(columns=1), ()),                 # one column of 12: every window lies on a line
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("model", MODELS)
def test_field_matches_float64_brute_force(small_pair, model, layout):
    rects, annular = LAYOUTS[layout]
    chi_max = 8.0
    with make_engine(*small_pair, rects, model=model, annular=annular) as e:
        cen = centres(e)
        S = e.n_sectors
        assert S == len(rects) + len(annular)
        rng = np.random.default_rng(100 * model + len(layout))
        seen = set()
        # 20 % bad in each of the three ways, and a lighter field (7 % each, 20 % in all) whose windows are mostly whole
        for share in (0.2, 0.07):
            rec = synthetic_records(S, rng, chi_max, share)
            U = scale_of(rec, model, chi_max)
            tensors = (ca.STRAIN_GREEN_LAGRANGE, ca.STRAIN_SMALL) if model == ca.FM_UVUXUYVXVY else (ca.STRAIN_GREEN_LAGRANGE,)
            for radius, min_nb in ((2.5 * SIDE, 3), (1.0 * SIDE, 5)):
                assert radius == np.float32(radius)
                for tensor in tensors:
                    ref = strain_reference(cen, rec, model, radius, chi_max, min_nb, tensor)
                    ratio = ref[3][np.isfinite(ref[3])]
                    # a condition on the inputs: no window sits near the DEGENERATE threshold, where the two could differ
                    assert not ((ratio > 1e-9) & (ratio < 1e-3)).any(), (layout, radius, ratio)
                    got = e.strain_field(radius, chi_max=chi_max, min_neighbours=min_nb, tensor=tensor, records=rec)
                    worst = check_against_reference(got, ref, U, (layout, model, share, radius, tensor))
                    print(f"{layout} model {model} share {share} radius {radius} tensor {tensor}: worst error / tolerance {worst:.3g}, "
                          f"statuses {np.bincount(ref[2], minlength=4).tolist()}, neighbours {ref[1].min()}..{ref[1].max()}")
                    seen |= set(ref[2].tolist())
                    if layout == "column":
                        assert np.isin(ref[2], (ca.STRAIN_DEGENERATE, ca.STRAIN_TOO_FEW)).all()
                    elif radius == 1.0 * SIDE:
                        # the four neighbours at exactly one pitch count: an interior sector of a clean patch has five
                        if layout == "grid":
                            assert ref[1].max() == 5 if share < 0.1 else ref[1].max() <= 5
                        corners = [0, 11, 132, 143]
                        assert (ref[2][corners] == ca.STRAIN_TOO_FEW).all()
        if layout == "column":   # all twelve good: every window is three to five centres on a line
            rec = synthetic_records(S, rng, chi_max, 0.0)
            rec["error_code"], rec["chi"] = 0, 1.0
            rec["p"] = np.nan_to_num(rec["p"])
            got = e.strain_field(2.5 * SIDE, chi_max=chi_max, records=rec)
            ref = strain_reference(cen, rec, model, 2.5 * SIDE, chi_max)
            check_against_reference(got, ref, scale_of(rec, model, chi_max), (layout, model, "clean"))
            assert (got["status"] == ca.STRAIN_DEGENERATE).all() and got["neighbours"].tolist() == [3, 4] + [5] * 8 + [4, 3]
        else:
            assert {ca.STRAIN_OK, ca.STRAIN_FILLED, ca.STRAIN_TOO_FEW} <= seen


def test_both_lane_groups_and_the_unpacked_walk(small_pair, monkeypatch):
    """The library picks 16 lanes per sector up to 1024 expected members of the 3 x 3 cells (9 S / cells) and 64 above: a
    radius past the whole domain puts all 148 sectors into one cell (1332 members) and takes the 64-lane kernel, 2.5 pitches
    takes the 16-lane one.  LK_STRAIN_GROUP / LK_STRAIN_PACKED force each of the four kernels on both."""
    rects, annular = LAYOUTS["grid_and_annular"]
    chi_max = 8.0
    with make_engine(*small_pair, rects, annular=annular) as e:
        cen = centres(e)
        rec = synthetic_records(e.n_sectors, np.random.default_rng(17), chi_max, 0.07)
        U = scale_of(rec, ca.FM_UVUXUYVXVY, chi_max)
        for radius in (2.5 * SIDE, 1000.0):
            ref = strain_reference(cen, rec, ca.FM_UVUXUYVXVY, radius, chi_max)
            if radius == 1000.0:
                assert (ref[1] == is_good(rec, 6, chi_max).sum()).all()
            for group, packed in ((None, None), ("16", "1"), ("64", "1"), ("16", "0"), ("64", "0")):
                for key, val in (("LK_STRAIN_GROUP", group), ("LK_STRAIN_PACKED", packed)):
                    if val is None:
                        monkeypatch.delenv(key, raising=False)
                    else:
                        monkeypatch.setenv(key, val)
                got = e.strain_field(radius, chi_max=chi_max, records=rec)
                check_against_reference(got, ref, U, (radius, group, packed))
                assert got.tobytes() == e.strain_field(radius, chi_max=chi_max, records=rec).tobytes()


def test_model_without_v_has_no_v_gradient(small_pair):
    with make_engine(*small_pair, grid_rects(), model=ca.FM_U) as e:
        rec = synthetic_records(e.n_sectors, np.random.default_rng(3), 8.0, 0.05)
        got = e.strain_field(2.5 * SIDE, chi_max=8.0, records=rec)
        ok = got["status"] == ca.STRAIN_OK
        assert ok.sum() > 100 and not got["v"].any() and not got["vx"].any() and not got["vy"].any()
        assert got["ux"][ok].any()


# ---- 2. known answers ---------------------------------------------------------------------------------------------------
A0 = np.float64([3.0, -2.0])
B = np.float64([[0.01, -0.004], [0.006, 0.02]])


def field_records(cen, fn):
    rec = np.zeros(len(cen), ca.RESULT_DTYPE)
    uv = fn(cen.astype(np.float64))
    rec["p"][:, 0], rec["p"][:, 1] = uv[0], uv[1]
    rec["chi"] = 1.0
    rec["n_points"] = 361
    return rec


def test_exact_affine_field_and_a_filled_sector(small_pair):
    with make_engine(*small_pair, grid_rects(), model=ca.FM_UV) as e:
        cen = centres(e)
        c = cen.astype(np.float64)
        rec = field_records(cen, lambda c: (A0[0] + c @ B[0], A0[1] + c @ B[1]))
        U = float(np.abs(rec["p"][:, :2]).max())
        # the inputs are the field rounded to float (at most 2^-24 U each); over a lever arm of at least one pitch a
        # gradient moves by less than 2^-22 U / h, the plane's value and the rms residual by less than 2^-22 U
        tol_g, tol_u = 2.0 ** -22 * U / SIDE, 2.0 ** -22 * U
        want_e = tensor_reference(ca.STRAIN_GREEN_LAGRANGE, B.reshape(4))
        # d exx = (1 + ux) d ux + vx d vx and alike: the tensor moves by less than 2 tol_g for gradients this small
        # (the principal values by the same bound); + the float rounding of B fed to the analytic formula and of the result
        tol_e = 2.0 * tol_g + 2.0 ** -22 * np.abs(B).max()

        def check(got, sel):
            for k, name in enumerate(("ux", "uy", "vx", "vy")):
                assert (np.abs(got[name][sel] - B.reshape(4)[k]) <= tol_g).all(), name
            assert (np.abs(got["u"][sel] - (A0[0] + c[sel] @ B[0])) <= tol_u).all()
            assert (np.abs(got["v"][sel] - (A0[1] + c[sel] @ B[1])) <= tol_u).all()
            assert (got["residual"][sel] <= tol_u).all()
            for k, name in enumerate(("exx", "eyy", "exy", "e1", "e2")):
                assert (np.abs(got[name][sel] - want_e[k]) <= tol_e).all(), name
            assert (got["e1"][sel] >= got["e2"][sel]).all()

        got = e.strain_field(2.5 * SIDE, records=rec)
        assert (got["status"] == ca.STRAIN_OK).all()
        assert got["neighbours"].max() == 21 and got["neighbours"][0] == 8     # interior: 21 lattice points; a corner: 8
        check(got, np.ones(len(cen), bool))
        # (c) a failed sector in the middle: filled from its neighbours, with the values they give
        mid = 5 * 12 + 6
        spoiled = rec.copy()
        spoiled["error_code"][mid] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        spoiled["p"][mid] = 777.0
        filled = e.strain_field(2.5 * SIDE, records=spoiled)
        assert filled["status"][mid] == ca.STRAIN_FILLED and filled["neighbours"][mid] == 20
        assert (np.delete(filled["status"], mid) == ca.STRAIN_OK).all()
        check(filled, np.ones(len(cen), bool))
        ref = strain_reference(cen, spoiled, ca.FM_UV, 2.5 * SIDE)
        check_against_reference(filled, ref, U, "filled")
        far = filled["neighbours"] == got["neighbours"]                        # windows the spoiled sector is not in
        assert far.sum() == len(cen) - 21 and filled[far].tobytes() == got[far].tobytes()


def test_quadratic_field_returns_the_centre_gradient(small_pair):
    with make_engine(*small_pair, grid_rects(), model=ca.FM_UV) as e:
        cen = centres(e)
        c = cen.astype(np.float64)
        rec = field_records(cen, lambda c: (1e-4 * c[:, 0] ** 2, 1e-4 * c[:, 0] * c[:, 1]))
        U = float(np.abs(rec["p"][:, :2]).max())
        got = e.strain_field(2.5 * SIDE, tensor=ca.STRAIN_SMALL, records=rec)
        whole = got["neighbours"] == 21          # complete windows are point-symmetric: the quadratic part drops out
        i, j = np.divmod(np.arange(144), 12)
        assert np.array_equal(whole, (i >= 2) & (i <= 9) & (j >= 2) & (j <= 9))
        tol_g = 2.0 ** -22 * U / SIDE
        want = np.stack([2e-4 * c[:, 0], np.zeros(144), 1e-4 * c[:, 1], 1e-4 * c[:, 0]], 1)
        for k, name in enumerate(("ux", "uy", "vx", "vy")):
            assert (np.abs(got[name][whole] - want[whole, k]) <= tol_g).all(), name
        assert (got["residual"][whole] > 1e-3).all()      # 1e-4 dx^2 over +-2 pitches: hundredths of a pixel
        assert (got["exx"][whole] == got["ux"][whole]).all() and (got["eyy"][whole] == got["vy"][whole]).all()
        # an incomplete window is not symmetric: the corner's gradient is the window's mean, not the centre's
        assert abs(got["ux"][0] - want[0, 0]) > 100 * tol_g


# ---- 3. end to end ------------------------------------------------------------------------------------------------------
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


def test_end_to_end_behind_a_reference_order_solve_and_the_recovery_pass(oracle, small_pair):
    rects = grid_rects(n=8)
    S = len(rects)
    radius = 2.5 * SIDE
    with make_engine(*small_pair, rects) as e:
        cen = centres(e)
        o = oracle.Oracle(model=oracle.FM_UVUXUYVXVY, precision=PRECISION, py_stop=2)
        o.set_image(0, small_pair[0])
        o.set_image(1, small_pair[1])
        want = o.correlate_sectors([oracle.rect_points(*r) for r in rects], cen, np.zeros((S, 6), np.float32))
        e.set_reference_order(1)
        rec = e.correlate_all(np.zeros((S, 6), np.float32))
        assert rec.tobytes() == want.tobytes()
        assert is_good(want, 6, 0).all()
        U = scale_of(want, ca.FM_UVUXUYVXVY, 0)
        held = e.strain_field(radius)
        worst = check_against_reference(held, strain_reference(cen, want, ca.FM_UVUXUYVXVY, radius), U, "reference order")
        assert (held["status"] == ca.STRAIN_OK).all()
        print(f"reference order: worst error / tolerance {worst:.3g}; ux {held['ux'].mean():.5f} +- {held['ux'].std():.5f}, "
              f"vy {held['vy'].mean():.5f} +- {held['vy'].std():.5f} (truth 0.002, -0.001); per-sector parameters "
              f"{rec['p'][:, 2].mean():.5f} +- {rec['p'][:, 2].std():.5f}, {rec['p'][:, 5].mean():.5f} +- {rec['p'][:, 5].std():.5f}")
        assert held.tobytes() == e.strain_field(radius, records=rec).tobytes()
        # default mode, some sectors sent off the image: the recovery pass repairs them, the strain field reads the repaired records
        e.set_reference_order(0)
        g = np.zeros((S, 6), np.float32)
        spoiled = [9, 27, 28, 50]
        g[spoiled, 0] = 300.0
        before = e.correlate_all(g)
        assert (before["error_code"][spoiled] != 0).all()
        repaired, n = e.reseed_failed(1.5 * SIDE)
        assert n >= 1
        after = e.strain_field(radius)
        check_against_reference(after, strain_reference(cen, repaired, ca.FM_UVUXUYVXVY, radius),
                                scale_of(repaired, ca.FM_UVUXUYVXVY, 0), "after the recovery pass")
        assert (after["status"] == ca.STRAIN_OK).sum() >= S - len(spoiled) + n


# ---- 4. nothing else moves ----------------------------------------------------------------------------------------------
def test_engine_state_is_untouched_and_the_result_repeats(small_pair):
    rects = grid_rects(n=8)
    S = len(rects)
    with make_engine(*small_pair, rects) as e:
        g = np.zeros((S, 6), np.float32)
        g[[9, 27], 0] = 300.0
        first = e.correlate_all(g)
        e.reseed_failed(1.5 * SIDE)

        def state():
            return dict(records=device_records(e), guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(),
                        stats=e.sector_stats(), reseed=e.reseed_info(), counters=np.array(sorted(e.stats().items()), dtype=object))

        kept = state()
        a = e.strain_field(2.5 * SIDE)
        b = e.strain_field(2.5 * SIDE)
        other = e.strain_field(1.0 * SIDE, chi_max=5.0, min_neighbours=4, tensor=ca.STRAIN_SMALL, records=first)
        c = e.strain_field(2.5 * SIDE)
        assert a.tobytes() == b.tobytes() == c.tobytes() and other.tobytes() != a.tobytes()
        after = state()
        for k in kept:
            if k == "counters":
                assert (kept[k] == after[k]).all()
            else:
                assert kept[k].tobytes() == after[k].tobytes(), k
        # a rebuild of the lists that waits for the next solve (here: after a change of mode) keeps waiting
        e.set_reference_order(1)
        assert e.strain_field(2.5 * SIDE).tobytes() == a.tobytes()
        after = state()
        for k in kept:
            if k != "counters":
                assert kept[k].tobytes() == after[k].tobytes(), k
        e.set_reference_order(0)
        # an asynchronous solve and its wait see the same engine
        e.correlate_all_async()
        rec = e.wait_results()
        assert e.strain_field(2.5 * SIDE).tobytes() == e.strain_field(2.5 * SIDE, records=rec).tobytes()


# ---- 5. arguments -------------------------------------------------------------------------------------------------------
def test_arguments_and_refusals(small_pair):
    rects = grid_rects(n=3)
    e = make_engine(*small_pair, rects, commit=False)
    lib, h = e.lib, e._h
    cfg = _ffi.LkStrainConfig(47.5, 0.0, 3, ca.STRAIN_GREEN_LAGRANGE)
    out = np.zeros(9, ca.STRAIN_DTYPE)
    rec = np.zeros(9, ca.RESULT_DTYPE)
    rec["p"][:, 0] = np.arange(9)

    def refused(c=cfg, records=None, output=out):
        rc = lib.lk_strain_field(h, C.byref(c) if c is not None else None,
                                 records.ctypes.data_as(C.c_void_p) if records is not None else None,
                                 output.ctypes.data_as(C.c_void_p) if output is not None else None)
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and "lk_strain_field" in msg, (rc, msg)
        return msg

    assert "no committed sectors" in refused()
    assert "no committed sectors" in refused(records=rec)
    e.commit_sectors()
    assert "no solve" in refused()                            # records == NULL before any batch solve
    assert "configuration" in refused(None)
    assert "output" in refused(output=None)
    for bad in ((0.0, 0.0, 3, 0), (-1.0, 0.0, 3, 0), (float("nan"), 0.0, 3, 0), (float("inf"), 0.0, 3, 0)):
        assert "radius" in refused(_ffi.LkStrainConfig(*bad), records=rec)
    for bad in (float("nan"), float("inf")):
        assert "chi_max" in refused(_ffi.LkStrainConfig(47.5, bad, 3, 0), records=rec)
    for bad in (2, 0, -1):
        assert "min_neighbours" in refused(_ffi.LkStrainConfig(47.5, 0.0, bad, 0), records=rec)
    for bad in (-1, 2):
        assert "tensor" in refused(_ffi.LkStrainConfig(47.5, 0.0, 3, bad), records=rec)
    assert lib.lk_strain_field(None, C.byref(cfg), None, out.ctypes.data_as(C.c_void_p)) == ca.ERROR_BAD_DOMAIN
    # records passed in need no solve; a solve in flight refuses records == NULL and finishes normally afterwards
    got = e.strain_field(47.5, records=rec)
    assert (got["status"] == ca.STRAIN_OK).all()
    assert got["neighbours"].tolist() == [8, 9, 8, 9, 9, 9, 8, 9, 8]     # (opposite corners are 2.83 pitches apart)
    e.correlate_all_async()
    assert "waited for" in refused()
    solved = e.wait_results()
    assert (solved["error_code"] == 0).all() and np.abs(solved["p"][:, :2] - np.float32([1.3, -0.7])).max() < 0.5
    assert e.strain_field(47.5).tobytes() == e.strain_field(47.5, records=solved).tobytes()
    e.close()
