"""Lens distortion, the host side (include/lk_engine.h: lk_lens_distort, lk_lens_undistort, lk_lens_correct_record,
lk_lens_step_from_sums): the kernels' own functions compiled for the host, against the float64 restatement of
tests/lens_ref.py; the restatement's rows against its own central differences; every status; every refusal.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi
import lens_ref
from lens_ref import SHIFTS, TRUE, make_lens

P = C.c_void_p
NUISANCES = [ca.LENS_TRANSLATION, ca.LENS_SIMILARITY, ca.LENS_AFFINE]
MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
ALL_FREE = ca.LENS_FREE_K1 | ca.LENS_FREE_K2 | ca.LENS_FREE_P1 | ca.LENS_FREE_P2 | ca.LENS_FREE_CENTRE


def lattice(n=12, pitch=19.0, first=17.0):
    """the centres of tests/test_strain_gpu.py's domain: 12 x 12 sectors of 19 x 19 from (8, 8)"""
    g = first + pitch * np.arange(n)
    return np.float32([(x, y) for x in g for y in g])


def test_layout_and_symbols(engine_lib):
    assert ca.LENS_DTYPE.itemsize == 64 and ca.LENS_RESULT_DTYPE.itemsize == 160 and ca.LENS_FRAME_DTYPE.itemsize == 64
    assert ca.LENS_STEP_DTYPE.itemsize == 136 and C.sizeof(_ffi.LkLensConfig) == 16 and C.sizeof(_ffi.LkLensFitConfig) == 40
    assert [ca.LENS_DTYPE.fields[k][1] for k in ("cx", "cy", "rn", "k1", "k2", "p1", "p2", "reserved")] == list(range(0, 64, 8))
    assert [ca.LENS_RESULT_DTYPE.fields[k][1] for k in ("lens", "sigma", "rms_before", "rms", "last_step", "status", "iterations",
                                                        "n_records", "n_frames_used", "n_outside")] == [0, 64, 112, 120, 128, 136, 140, 144, 148, 152]
    assert [ca.LENS_FRAME_DTYPE.fields[k][1] for k in ("nuisance", "rms", "n", "status")] == [0, 48, 56, 60]
    assert [ca.LENS_STEP_DTYPE.fields[k][1] for k in ("delta", "sigma", "chi2", "chi2_profiled", "scaled_step", "status", "n_outside")] == \
        [0, 48, 96, 104, 112, 120, 132]
    assert [_ffi.LkLensFitConfig.tol.offset, _ffi.LkLensFitConfig.reserved.offset] == [24, 32]
    for name in ("lk_lens_fit", "lk_lens_correct", "lk_lens_distort", "lk_lens_undistort", "lk_lens_correct_record", "lk_lens_step_from_sums"):
        assert hasattr(engine_lib, name) and name in _ffi.SYMBOLS
    assert hasattr(engine_lib, "lk_internal_lens_last")
    assert (ca.LENS_TRANSLATION, ca.LENS_SIMILARITY, ca.LENS_AFFINE) == (0, 1, 2) and (ca.LENS_OK, ca.LENS_MAX_ITERS, ca.LENS_DEGENERATE) == (0, 1, 2)
    assert [ca.lens_sums_len(k) - 2 for k in NUISANCES] == [45, 66, 91]


def test_model_and_inverse_over_the_domain(engine_lib):
    """U(D(x)) = x within 1e-9 px over the domain at 5 % rim distortion (rho = 1: |k1| = 0.05), with both signs, a second
    radial term and both tangential ones; the library's D and U against the restatement's"""
    g = np.arange(8.0, 236.5, 4.0)
    xy = np.float64([(x, y) for x in g for y in g])
    for k1, k2, p1, p2 in ((-0.05, 0.0, 0.0, 0.0), (0.05, 0.0, 0.0, 0.0), (-0.03, 0.008, 0.0, 0.0), (-0.04, 0.01, 2e-3, -3e-3)):
        L = make_lens(126.0, 117.0, 147.785, k1, k2, p1, p2)
        rec = lens_ref.as_record(L)
        d = ca.lens_distort(rec, xy)
        assert np.abs(d - lens_ref.distort(L, xy)).max() <= 1e-12
        back, status = ca.lens_undistort(rec, d, return_status=True)
        ref, outside = lens_ref.undistort(L, d)
        err = np.abs(back - xy).max()
        print(f"k1 {k1} k2 {k2} p1 {p1} p2 {p2}: |D - x| up to {np.abs(d - xy).max():.3f} px, |U(D(x)) - x| {err:.3g} px")
        assert not status.any() and not outside.any() and err <= 1e-9 and np.abs(back - ref).max() <= 1e-11
        # one step fewer already reaches it: six leave room
        assert np.abs(lens_ref.undistort(L, d, steps=5)[0] - xy).max() <= 1e-9


def test_a_fold_is_a_status_not_a_nan(engine_lib):
    L = make_lens(126.0, 117.0, 147.785, k1=-0.5)          # d(rho) turns back at rho = sqrt(1 / 1.5) = 0.816
    xy = np.float64([(126.0, 117.0), (140.0, 120.0), (126.0 + 0.6 * 147.785, 117.0), (250.0, 240.0), (126.0 + 147.785, 117.0)])
    out, status = ca.lens_undistort(lens_ref.as_record(L), xy, return_status=True)
    ref, outside = lens_ref.undistort(L, xy)
    print("fold: status", status, "restatement", outside)
    assert np.isfinite(out).all() and (status == np.where(outside, 2, 0)).all() and status[-2:].all() and not status[:2].any()
    assert (out[status == 2] == xy[status == 2]).all()
    rec = np.zeros(1, ca.RESULT_DTYPE)
    rec["p"][0, :2] = (1.0, 2.0)
    got, st = ca.lens_correct_records(ca.FM_UV, lens_ref.as_record(L), np.float32([[250.0, 240.0]]), rec)
    assert st[0] == ca.LENS_OUTSIDE and got.tobytes() == rec.tobytes()
    # the centre inside, the displaced point outside
    rec["p"][0, :2] = (120.0, 0.0)
    got, st = ca.lens_correct_records(ca.FM_UV, lens_ref.as_record(L), np.float32([[130.0, 117.0]]), rec)
    assert st[0] == ca.LENS_OUTSIDE and got.tobytes() == rec.tobytes()


@pytest.mark.parametrize("nuisance", NUISANCES)
def test_rows_match_central_differences(nuisance):
    rng = np.random.default_rng(nuisance)
    X = lattice().astype(np.float64)
    o = lens_ref.origin_of(lattice())
    L = make_lens(126.0, 117.0, 147.785, -0.03, 0.008, 1.5e-3, -2e-3)
    nu = np.float64([3.0, -2.0, 2e-3, -1e-3, 1.5e-3, 5e-4])
    uv = np.float64([8.0, -6.0]) + rng.normal(0, 0.3, X.shape)
    Q = lens_ref.Q_OF[nuisance]
    ax, ay, outside = lens_ref.rows(L, nuisance, nu, o, X, uv)
    assert not outside.any()
    r0, _ = lens_ref.residuals(L, nuisance, nu, o, X, uv)
    assert np.abs(ax[:, 6 + Q] - r0[:, 0]).max() <= 1e-12 and np.abs(ay[:, 6 + Q] - r0[:, 1]).max() <= 1e-12
    for j in range(6 + Q):
        # a step that moves a position by about 1e-4 px: the truncation (h^2) and the rounding (2^-53 * 256 / h) both stay
        # below 1e-7 of the column
        lens_col = j < 6
        scale = float(np.abs(np.concatenate([ax[:, j], ay[:, j]])).max())
        h = 1e-4 / scale
        Lp, Lm, nup, num = dict(L), dict(L), nu.copy(), nu.copy()
        if lens_col:
            Lp[lens_ref.PARAMS[j]] += h
            Lm[lens_ref.PARAMS[j]] -= h
        else:
            nup[j - 6] += h
            num[j - 6] -= h
        rp, _ = lens_ref.residuals(Lp, nuisance, nup, o, X, uv)
        rm, _ = lens_ref.residuals(Lm, nuisance, num, o, X, uv)
        fd = (rp - rm) / (2 * h)
        err = max(np.abs(fd[:, 0] - ax[:, j]).max(), np.abs(fd[:, 1] - ay[:, j]).max())
        print(f"nuisance {nuisance} column {j}: largest |entry| {scale:.4g}, |analytic - central difference| {err:.3g}")
        assert err <= 1e-6 * scale


@pytest.mark.parametrize("model", MODELS)
def test_correct_record_matches_the_restatement(engine_lib, model):
    rng = np.random.default_rng(20 + model)
    cen = lattice()
    L = make_lens(126.0, 117.0, 147.785, -0.03, 0.008, 1e-3, -1e-3)
    rec = np.zeros(len(cen), ca.RESULT_DTYPE)
    rec["p"][:, :2] = np.float64([8.0, -6.0]) + rng.normal(0, 0.5, (len(cen), 2))
    rec["p"][:, 2:6] = rng.normal(0, 0.01, (len(cen), 4))
    rec["chi"], rec["n_points"], rec["iterations"] = 0.5, 361, 5
    good = rng.random(len(cen)) < 0.9
    got, status = ca.lens_correct_records(model, lens_ref.as_record(L), cen, rec, good=good)
    want, want_status = lens_ref.correct(model, L, cen, rec, good)
    assert (status == want_status).all() and set(status) == {0, 1}
    n_par = _ffi.N_PARAMS[model]
    # one rounding to float of values a few double roundings apart
    err = np.abs(got["p"].astype(np.float64) - want)
    tol = 2.0 ** -23 * np.abs(want) + 1e-12
    assert (err[:, :n_par] <= tol[:, :n_par]).all(), err.max()
    assert got[~good].tobytes() == rec[~good].tobytes()
    changed = (got["p"] != rec["p"])
    assert changed[good, 0].all() and not changed[:, n_par:].any()
    for k in ("chi", "n_points", "iterations", "error_code", "und_cx", "und_cy"):
        assert got[k].tobytes() == rec[k].tobytes()
    if model == ca.FM_U:
        assert not changed[:, 1:].any()                    # u alone
        # ... and v = 0 on input whatever p[1] holds
        other = rec.copy()
        other["p"][:, 1] = 7.0
        again, _ = ca.lens_correct_records(model, lens_ref.as_record(L), cen, other, good=good)
        assert again["p"][:, 0].tobytes() == got["p"][:, 0].tobytes() and (again["p"][:, 1] == 7.0).all()
    # the correction does take the distortion out: records of a pure shift come back uniform
    if model != ca.FM_U:
        shifted = lens_ref.shifted_records(cen, L)[4]
        flat, st = ca.lens_correct_records(model, lens_ref.as_record(L), cen, shifted)
        assert not st.any() and np.abs(flat["p"][:, :2].astype(np.float64) - SHIFTS[4]).max() <= 2e-6
        assert np.abs(shifted["p"][:, :2].astype(np.float64) - SHIFTS[4]).max() > 0.1


@pytest.mark.parametrize("model", MODELS)
def test_a_zero_lens_returns_the_record(engine_lib, model):
    rng = np.random.default_rng(30 + model)
    cen = lattice()
    rec = np.zeros(len(cen), ca.RESULT_DTYPE)
    rec["p"][:, :2] = rng.normal(0, 5.0, (len(cen), 2))
    rec["p"][:, 2:6] = rng.normal(0, 0.01, (len(cen), 4))
    got, status = ca.lens_correct_records(model, ca.make_lens(121.5, 121.5, 147.785), cen, rec)
    assert not status.any()
    n_par = _ffi.N_PARAMS[model]
    # (X + u) - X in double, rounded to float: within one float ulp of u
    assert (np.abs(got["p"] - rec["p"])[:, :n_par] <= np.spacing(np.abs(rec["p"]))[:, :n_par]).all()
    assert got["p"][:, n_par:].tobytes() == rec["p"][:, n_par:].tobytes()


def synthetic_sums(nuisance, L, nu, rec, cen):
    sums, _, _ = lens_ref.all_sums(L, nuisance, nu, cen, rec, ca.FM_UVUXUYVXVY)
    return sums


@pytest.mark.parametrize("nuisance,free", [(ca.LENS_TRANSLATION, ALL_FREE & ~(ca.LENS_FREE_P1 | ca.LENS_FREE_P2)), (ca.LENS_TRANSLATION, ca.LENS_FREE_K1),
                                           (ca.LENS_SIMILARITY, ca.LENS_FREE_K1 | ca.LENS_FREE_K2 | ca.LENS_FREE_CENTRE),
                                           (ca.LENS_AFFINE, ca.LENS_FREE_K1 | ca.LENS_FREE_K2 | ca.LENS_FREE_P1 | ca.LENS_FREE_P2)])
def test_step_from_sums_matches_dense_normal_equations(engine_lib, nuisance, free):
    cen = lattice()
    rec = lens_ref.shifted_records(cen, noise=0.01, seed=7)
    L = make_lens(121.5, 121.5, 147.785, -0.01, 0.0, 0.0, 0.0)          # away from the truth: a real step
    nu = np.zeros((5, 6))
    nu[:, :2] = SHIFTS * 0.9
    sums = synthetic_sums(nuisance, L, nu, rec, cen)
    sums[2, 0] = 1                                                           # a frame with too few members is skipped
    got, dn = ca.lens_step_from_sums(nuisance, free, L["rn"], sums)
    ref = lens_ref.step_from_sums(nuisance, free, L["rn"], lens_ref.Q_OF[nuisance], sums)
    assert got["status"] == ca.LENS_OK and not ref["degenerate"]
    assert got["n_records"] == ref["n_records"] == 4 * 144 and got["n_frames_used"] == 4 and got["n_outside"] == 0
    H, _, _, _, _ = lens_ref.dense_system(nuisance, free, lens_ref.Q_OF[nuisance], sums)
    d = np.sqrt(np.diag(H))
    cond = np.linalg.cond(H / np.outer(d, d))
    tol = 100 * cond * 2.0 ** -53                # two solutions of one scaled system, each good to cond * 2^-53 and a factor
    idx = lens_ref.free_index(free)
    for name, a, b in (("delta", got["delta"], ref["delta"]), ("sigma", got["sigma"], ref["sigma"]), ("nuisance", dn, ref["nuisance_delta"])):
        # the scaled unknowns are of one size; unscaled, a parameter's error is relative to the largest of its own kind
        for cols in ((slice(0, 4), slice(4, 6)) if name != "nuisance" else (slice(0, 2), slice(2, 6))):
            size = np.abs(b[..., cols]).max()
            err = np.abs(a[..., cols] - b[..., cols]).max()
            print(f"nuisance {nuisance} free {free} {name}{cols}: |difference| {err:.3g}, size {size:.3g}, tolerance {tol * max(size, 1e-300):.3g} (cond {cond:.3g})")
            assert err <= tol * size + 1e-300
    held = [j for j in range(6) if j not in idx]
    assert not got["delta"][held].any() and not got["sigma"][held].any() and not dn[2].any()
    assert abs(got["chi2"] - ref["chi2"]) <= 1e-12 * ref["chi2"] and 0 < got["chi2_profiled"] <= got["chi2"]
    assert got["scaled_step"] == max(abs(got["delta"][j]) / (1.0 if j < 4 else L["rn"]) for j in idx)


def test_degenerate_sums(engine_lib):
    cen = lattice()
    L = make_lens(121.5, 121.5, 147.785, -0.01)
    nu = np.zeros((2, 6))
    # no translation at all: the lens columns vanish
    still = lens_ref.shifted_records(cen, shifts=np.zeros((2, 2)))
    still["p"][:] = 0
    sums = synthetic_sums(ca.LENS_TRANSLATION, L, nu, still, cen)
    got, dn = ca.lens_step_from_sums(ca.LENS_TRANSLATION, ca.LENS_FREE_K1, L["rn"], sums)
    assert got["status"] == ca.LENS_DEGENERATE and not got["delta"].any() and not got["sigma"].any() and not dn.any()
    assert got["n_records"] == 288 and got["n_frames_used"] == 2
    # one parameter too many: under a purely radial k1 a shift of the centre and the two tangential terms bend a shifted field
    # the same way (both are quadratic in rho, so their difference between x and X is linear in X)
    five = lens_ref.shifted_records(cen)
    sums = synthetic_sums(ca.LENS_TRANSLATION, L, np.zeros((5, 6)), five, cen)
    got, _ = ca.lens_step_from_sums(ca.LENS_TRANSLATION, ALL_FREE, L["rn"], sums)
    assert got["status"] == ca.LENS_DEGENERATE
    got, _ = ca.lens_step_from_sums(ca.LENS_TRANSLATION, ALL_FREE & ~(ca.LENS_FREE_P1 | ca.LENS_FREE_P2), L["rn"], sums)
    assert got["status"] == ca.LENS_OK
    # ... and the centre of a lens without coefficients has no columns at all
    one = lens_ref.shifted_records(cen, shifts=np.float64([(12.0, 0.0)]))
    zero = make_lens(121.5, 121.5, 147.785)
    sums = synthetic_sums(ca.LENS_TRANSLATION, zero, np.zeros((1, 6)), one, cen)
    got, _ = ca.lens_step_from_sums(ca.LENS_TRANSLATION, ca.LENS_FREE_K1 | ca.LENS_FREE_CENTRE, zero["rn"], sums)
    assert got["status"] == ca.LENS_DEGENERATE
    got, _ = ca.lens_step_from_sums(ca.LENS_TRANSLATION, ca.LENS_FREE_K1, zero["rn"], sums)
    assert got["status"] == ca.LENS_OK and abs(got["delta"][0] + 0.03) < 0.01
    # every frame too few
    got, _ = ca.lens_step_from_sums(ca.LENS_TRANSLATION, ca.LENS_FREE_K1, zero["rn"], sums, min_sectors=145)
    assert got["status"] == ca.LENS_DEGENERATE and got["n_frames_used"] == 0 and got["n_records"] == 0
    # a similarity needs spread: all members at one place
    same = np.repeat(lattice()[:1], 144, axis=0)
    sums = synthetic_sums(ca.LENS_SIMILARITY, L, np.zeros((1, 6)), one, same)
    got, _ = ca.lens_step_from_sums(ca.LENS_SIMILARITY, ca.LENS_FREE_K1, L["rn"], sums)
    assert got["status"] == ca.LENS_DEGENERATE


def test_refusals_of_the_host_functions(engine_lib):
    lib = engine_lib
    good = ca.make_lens(121.5, 121.5, 147.785, -0.03)
    xy = np.zeros((3, 2))
    out = np.full((3, 2), 7.0)
    st = np.full(3, 9, np.uint8)

    def lens_with(**kw):
        lens = np.array([good], ca.LENS_DTYPE)
        for k, v in kw.items():
            lens[k] = v
        return lens

    bad_lenses = [lens_with(rn=0.0), lens_with(rn=-1.0), lens_with(rn=np.nan), lens_with(rn=np.inf), lens_with(k1=np.nan), lens_with(cx=np.inf),
                  lens_with(p2=-np.inf), lens_with(reserved=1.0)]
    rec = np.zeros(1, ca.RESULT_DTYPE)
    rec_out = np.full(1, 3, ca.RESULT_DTYPE)
    code = C.c_int(5)
    ok = lens_with()
    for lens in bad_lenses + [None]:
        lp = lens.ctypes.data_as(P) if lens is not None else None
        assert lib.lk_lens_distort(lp, 3, xy.ctypes.data_as(P), out.ctypes.data_as(P)) == ca.ERROR_BAD_DOMAIN
        assert lib.lk_lens_undistort(lp, 3, xy.ctypes.data_as(P), out.ctypes.data_as(P), st.ctypes.data_as(P)) == ca.ERROR_BAD_DOMAIN
        assert lib.lk_lens_correct_record(ca.FM_UV, lp, 1.0, 1.0, rec.ctypes.data_as(P), rec_out.ctypes.data_as(P), C.byref(code)) == ca.ERROR_BAD_DOMAIN
    op = ok.ctypes.data_as(P)
    assert lib.lk_lens_distort(op, 0, xy.ctypes.data_as(P), out.ctypes.data_as(P)) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_lens_distort(op, 3, None, out.ctypes.data_as(P)) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_lens_distort(op, 3, xy.ctypes.data_as(P), None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_lens_undistort(op, -1, xy.ctypes.data_as(P), out.ctypes.data_as(P), None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_lens_undistort(op, 3, None, out.ctypes.data_as(P), None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_lens_undistort(op, 3, xy.ctypes.data_as(P), None, None) == ca.ERROR_BAD_DOMAIN
    for model in (ca.FM_U - 1, ca.FM_UVUXUYVXVY + 1):
        assert lib.lk_lens_correct_record(model, op, 1.0, 1.0, rec.ctypes.data_as(P), rec_out.ctypes.data_as(P), None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_lens_correct_record(ca.FM_UV, op, 1.0, 1.0, None, rec_out.ctypes.data_as(P), None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_lens_correct_record(ca.FM_UV, op, 1.0, 1.0, rec.ctypes.data_as(P), None, None) == ca.ERROR_BAD_DOMAIN
    assert (out == 7.0).all() and (st == 9).all() and code.value == 5 and (rec_out == np.full(1, 3, ca.RESULT_DTYPE)).all()
    # a null status is allowed
    assert lib.lk_lens_undistort(op, 3, xy.ctypes.data_as(P), out.ctypes.data_as(P), None) == 0
    assert lib.lk_lens_correct_record(ca.FM_UV, op, 1.0, 1.0, rec.ctypes.data_as(P), rec_out.ctypes.data_as(P), None) == 0
    # the step
    sums = np.zeros((1, ca.lens_sums_len(ca.LENS_TRANSLATION)))
    step = np.full(1, 1, ca.LENS_STEP_DTYPE)
    sp, tp = sums.ctypes.data_as(P), step.ctypes.data_as(P)
    fn = lib.lk_lens_step_from_sums
    K1 = ca.LENS_FREE_K1
    assert fn(ca.LENS_TRANSLATION, K1, 100.0, 2, 1, None, tp, None) == ca.ERROR_BAD_DOMAIN
    assert fn(ca.LENS_TRANSLATION, K1, 100.0, 2, 1, sp, None, None) == ca.ERROR_BAD_DOMAIN
    for nuisance in (-1, 3):
        assert fn(nuisance, K1, 100.0, 6, 1, sp, tp, None) == ca.ERROR_BAD_DOMAIN
    for free in (0, 32, 64 | K1):
        assert fn(ca.LENS_TRANSLATION, free, 100.0, 2, 1, sp, tp, None) == ca.ERROR_BAD_DOMAIN
    for rn in (0.0, -1.0, float("nan"), float("inf")):
        assert fn(ca.LENS_TRANSLATION, K1, rn, 2, 1, sp, tp, None) == ca.ERROR_BAD_DOMAIN
    assert fn(ca.LENS_TRANSLATION, K1, 100.0, 2, 0, sp, tp, None) == ca.ERROR_BAD_DOMAIN
    for nuisance, q in ((ca.LENS_TRANSLATION, 2), (ca.LENS_SIMILARITY, 4), (ca.LENS_AFFINE, 6)):
        assert fn(nuisance, K1, 100.0, q - 1, 1, sp, tp, None) == ca.ERROR_BAD_DOMAIN
    assert (step == np.full(1, 1, ca.LENS_STEP_DTYPE)).all()
    assert fn(ca.LENS_TRANSLATION, K1, 100.0, 2, 1, sp, tp, None) == 0 and step["status"][0] == ca.LENS_DEGENERATE
    with pytest.raises(ValueError):
        ca.lens_distort(lens_with(rn=0.0), xy)
    with pytest.raises(ValueError):
        ca.lens_step_from_sums(ca.LENS_TRANSLATION, 0, 100.0, sums)


def test_rendered_frames_recover_the_lens_from_the_oracle_s_records(oracle):
    """The end-to-end conditions of tests/test_lens_gpu.py, checked first where no GPU is needed: the CPU oracle solves the
    four shifted frames of lens_ref.lens_frames() against the unshifted one, the restatement fits k1 and the centre with a
    translation per frame and corrects the records.  k1 within 10 % of the truth; the rms of the corrected displacements
    about their frame mean at most a third of the uncorrected.  Measured: k1 -0.03034 (1.1 % off), 0.2199 -> 0.0201 px."""
    from test_strain_gpu import grid_rects
    und, shifted = lens_ref.lens_frames()
    rects = grid_rects()
    lists = [oracle.rect_points(*r) for r in rects]
    cen = lattice()
    rec = np.zeros((4, len(rects)), ca.RESULT_DTYPE)
    for f, t in enumerate(lens_ref.IMAGE_SHIFTS):
        o = oracle.Oracle(model=oracle.FM_UVUXUYVXVY, precision=1e-3, py_stop=2)
        o.set_image(0, und)
        o.set_image(1, shifted[f])
        g = np.zeros((len(rects), 6), np.float32)
        g[:, :2] = t
        rec[f] = o.correlate_sectors(lists, cen, g)
        o.close()
    good = lens_ref.is_good(rec, 6, 0.0)
    assert good.sum() >= 4 * 130
    ref = lens_ref.fit(make_lens(121.5, 121.5, 147.785), ca.LENS_FREE_K1 | ca.LENS_FREE_CENTRE, ca.LENS_TRANSLATION, cen, rec)
    fixed = rec.copy()
    for f in range(4):
        fixed[f]["p"], _ = lens_ref.correct(ca.FM_UVUXUYVXVY, ref["lens"], cen, rec[f], good[f])
    before, after = lens_ref.spread_about_frame_mean(rec, good), lens_ref.spread_about_frame_mean(fixed, good)
    k1, true = ref["lens"]["k1"], lens_ref.IMAGE_LENS["k1"]
    print(f"CPU oracle records, float64 restatement (status {ref['status']}, {ref['iterations']} iterations): k1 {k1:.5f} +- "
          f"{ref['sigma'][0]:.2g} of {true} ({100 * abs(k1 - true) / abs(true):.1f} % off), centre ({ref['lens']['cx']:.2f}, "
          f"{ref['lens']['cy']:.2f}) of (126, 117); rms about the frame mean {before:.4f} -> {after:.4f} px (ratio {after / before:.3f}); "
          f"residual rms {ref['rms_before']:.4f} -> {ref['rms']:.4f} px over {ref['n_records']} records")
    assert ref["status"] == ca.LENS_OK and abs(k1 - true) <= 0.1 * abs(true) and after <= before / 3.0
