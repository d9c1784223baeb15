"""Outlier flags, host side (include/lk_engine.h: lk_outlier_from_window - the kernel's own selection and ratio arithmetic
compiled for the host) against the numpy restatement (outlier_ref.py), byte for byte: a median is a selection and the
ratio is a handful of correctly rounded double operations, so there is no tolerance.  Also the record layout, the new
error code and the refusals.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import outlier_ref as oref

SIZES = [1, 2, 3, 8, 9, 20, 21, 173, 1500]
F32 = np.float32
TINY = np.finfo(F32).smallest_subnormal


def check(e_u, e_v, es_u, es_v, eps=0.02, threshold=3.0, what=""):
    got = ca.outlier_from_window(e_u, e_v, es_u, es_v, eps, threshold)
    want, ratios = oref.window_record(e_u, e_v, es_u, es_v, eps, threshold)
    assert got.tobytes() == want.tobytes(), (what, got, want)
    return got, ratios


def families(n, rng):
    """name -> one component's window of n float32 values"""
    base = F32(rng.normal(0, 3))
    ulps = np.arange(n, dtype=np.int32) % 5 - 2
    zeros = np.zeros(n, F32)
    zeros[::2] = -0.0
    denormal = (rng.integers(-40, 41, n) * np.float64(TINY)).astype(F32)
    return {
        "random": rng.normal(0, 2, n).astype(F32),
        "all_equal": np.full(n, base, F32),
        "many_ties": rng.integers(-3, 4, n).astype(F32) * F32(0.25),
        "last_bit": (np.full(n, F32(1.7)).view(np.int32) + rng.permutation(ulps)).view(F32),
        "signed_zeros": rng.permutation(zeros),
        "zeros_and_tiny": rng.permutation(np.where(np.arange(n) % 3 == 0, zeros, rng.choice([-1, 1], n) * TINY).astype(F32)),
        "denormals": denormal,
        "both_signs": (rng.normal(0, 1, n) * 10.0 ** rng.integers(-30, 30, n)).astype(F32),
    }


@pytest.mark.parametrize("n", SIZES)
def test_window_function_matches_numpy_restatement_byte_for_byte(engine_lib, n):
    rng = np.random.default_rng(1000 + n)
    fam = families(n, rng)
    names = sorted(fam)
    for i, a in enumerate(names):
        b = names[(i + 3) % len(names)]          # u and v of one call come from different families
        e_u, e_v = fam[a], fam[b]
        for es_u, es_v in ((e_u[0], e_v[-1]), (F32(0.5), F32(-0.5)), (F32(-0.0), F32(1e-40)), (F32(1e30), F32(-1e30))):
            got, _ = check(e_u, e_v, es_u, es_v, what=(n, a, b))
            assert got["neighbours"] == n and got["status"] in (ca.OUTLIER_OK, ca.OUTLIER_FLAGGED)
        if a == "all_equal":                     # mad = 0: ratio = |e_s - med| / eps
            got, _ = check(e_u, e_v, e_u[0] + F32(0.5), e_v[0], eps=0.125, what=(n, "mad 0"))
            assert got["mad_u"] == 0 and got["med_u"] == e_u[0]
            assert got["ratio_u"] == F32(abs(np.float64(e_u[0] + F32(0.5)) - np.float64(e_u[0])) / 0.125)
        if a == "signed_zeros":
            got, _ = check(e_u, e_u, 0.0, -0.0, what=(n, "zeros"))
            assert got["med_u"].tobytes() == F32(0.0).tobytes() and got["mad_u"].tobytes() == F32(0.0).tobytes()


def test_the_median_does_not_depend_on_the_order(engine_lib):
    rng = np.random.default_rng(5)
    e_u, e_v = rng.normal(0, 1, 173).astype(F32), rng.integers(-2, 3, 173).astype(F32)
    first = ca.outlier_from_window(e_u, e_v, 0.3, 0.1, 0.02, 3.0)
    for _ in range(5):
        p = rng.permutation(173)
        assert ca.outlier_from_window(e_u[p], e_v[p], 0.3, 0.1, 0.02, 3.0).tobytes() == first.tobytes()


def test_a_ratio_at_the_threshold_is_not_flagged_and_one_ulp_above_is(engine_lib):
    quiet = np.zeros(5, F32)
    # med = 1, mad = 0.25, eps = 0.25: mad + eps = 0.5 exactly; e_s = 2.5 gives the ratio 3 exactly: not flagged
    e = F32([0.5, 0.75, 1.0, 1.25, 1.5])
    got, ratios = check(e, quiet, 2.5, 0.0, eps=0.25, threshold=3.0, what="at the threshold")
    assert ratios[0] == 3.0 and got["ratio_u"] == 3.0 and got["status"] == ca.OUTLIER_OK
    # one ulp of the double above: every e_j = -2^-51 (a float), so med = -2^-51 and mad = 0; eps = 1; e_s = 3:
    # ratio = 3 + 2^-51 exactly, the double next to 3.  It rounds to the float 3 = the threshold, and is flagged, because the
    # comparison is made on the doubles before the rounding
    e = np.full(5, F32(-2.0 ** -51), F32)
    got, ratios = check(e, quiet, 3.0, 0.0, eps=1.0, threshold=3.0, what="one ulp above")
    assert ratios[0] == np.nextafter(np.float64(3.0), 4.0) and got["med_u"] == F32(-2.0 ** -51) and got["mad_u"] == 0
    assert got["ratio_u"] == F32(3.0) and got["status"] == ca.OUTLIER_FLAGGED
    # and one ulp below, the same way: not flagged
    got, ratios = check(-e, quiet, 3.0, 0.0, eps=1.0, threshold=3.0, what="one ulp below")
    assert ratios[0] == np.nextafter(np.float64(3.0), 2.0) and got["ratio_u"] == F32(3.0) and got["status"] == ca.OUTLIER_OK
    # the v component decides alike, and the larger of the two ratios is the one compared
    got, _ = check(quiet, e, 0.0, 3.0, eps=1.0, threshold=3.0, what="v decides")
    assert got["ratio_u"] == 0 and got["ratio_v"] == F32(3.0) and got["status"] == ca.OUTLIER_FLAGGED


def test_refusals(engine_lib):
    e = np.arange(5, dtype=F32)
    out = np.zeros(1, ca.OUTLIER_DTYPE)
    out["neighbours"] = 77
    pe, po = _ffi.fptr(e), out.ctypes.data_as(C.c_void_p)
    f = engine_lib.lk_outlier_from_window
    assert f(5, pe, pe, 1.0, 1.0, 0.02, 3.0, po) == ca.ERROR_NONE and out["neighbours"][0] == 5
    out[:] = 0
    out["neighbours"] = 77
    assert f(5, None, pe, 1.0, 1.0, 0.02, 3.0, po) == ca.ERROR_BAD_DOMAIN
    assert f(5, pe, None, 1.0, 1.0, 0.02, 3.0, po) == ca.ERROR_BAD_DOMAIN
    assert f(5, pe, pe, 1.0, 1.0, 0.02, 3.0, None) == ca.ERROR_BAD_DOMAIN
    for n in (0, -1):
        assert f(n, pe, pe, 1.0, 1.0, 0.02, 3.0, po) == ca.ERROR_BAD_DOMAIN
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert f(5, pe, pe, bad, 1.0, 0.02, 3.0, po) == ca.ERROR_BAD_DOMAIN
        assert f(5, pe, pe, 1.0, bad, 0.02, 3.0, po) == ca.ERROR_BAD_DOMAIN
        assert f(5, pe, pe, 1.0, 1.0, bad, 3.0, po) == ca.ERROR_BAD_DOMAIN
        assert f(5, pe, pe, 1.0, 1.0, 0.02, bad, po) == ca.ERROR_BAD_DOMAIN
        spoiled = e.copy()
        spoiled[3] = bad
        assert f(5, _ffi.fptr(spoiled), pe, 1.0, 1.0, 0.02, 3.0, po) == ca.ERROR_BAD_DOMAIN
        assert f(5, pe, _ffi.fptr(spoiled), 1.0, 1.0, 0.02, 3.0, po) == ca.ERROR_BAD_DOMAIN
    for bad in (0.0, -1.0):
        assert f(5, pe, pe, 1.0, 1.0, bad, 3.0, po) == ca.ERROR_BAD_DOMAIN
        assert f(5, pe, pe, 1.0, 1.0, 0.02, bad, po) == ca.ERROR_BAD_DOMAIN
    assert out["neighbours"][0] == 77 and not out["med_u"].any()
    with pytest.raises(ValueError):
        ca.outlier_from_window([], [], 0.0, 0.0, 0.02, 3.0)
    assert engine_lib.lk_flag_outliers(None, None, None, None, None, None) == ca.ERROR_BAD_DOMAIN


def test_symbols_constants_and_record_layout(engine_lib):
    for name in ("lk_flag_outliers", "lk_outlier_from_window"):
        assert hasattr(engine_lib, name) and name in _ffi.SYMBOLS
    assert ca.ERROR_OUTLIER == 8
    assert (ca.OUTLIER_OK, ca.OUTLIER_FLAGGED, ca.OUTLIER_TOO_FEW, ca.OUTLIER_DEGENERATE, ca.OUTLIER_NOT_GOOD) == (0, 1, 2, 3, 4)
    d = ca.OUTLIER_DTYPE
    names = ("med_u", "med_v", "mad_u", "mad_v", "ratio_u", "ratio_v", "neighbours", "status")
    assert d.itemsize == 32 and d.names == names
    assert [d.fields[k][1] for k in names] == [4 * i for i in range(8)]
    assert all(d.fields[k][0] == np.float32 for k in names[:6]) and all(d.fields[k][0] == np.int32 for k in names[6:])
    cfg = _ffi.LkOutlierConfig
    assert C.sizeof(cfg) == 32
    assert [f for f, _ in cfg._fields_] == ["radius", "chi_max", "eps", "threshold", "min_neighbours", "detrend", "passes", "mark"]
    # the C header says the same
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lk_engine.h")).read()
    assert "LK_ERROR_OUTLIER = 8" in header
    assert "LK_OUTLIER_OK = 0, LK_OUTLIER_FLAGGED = 1, LK_OUTLIER_TOO_FEW = 2, LK_OUTLIER_DEGENERATE = 3, LK_OUTLIER_NOT_GOOD = 4" in header
