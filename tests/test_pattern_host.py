"""Host side of the speckle-quality pass (include/lk_engine.h): lk_pattern_from_sums - the kernel's own record function
compiled for the host - against the float64 restatement of pattern_ref.py on random sums, every status, and the refusals of
the host function; the layouts and prototypes of the binding.  No GPU.

Floats: every field but theta is compared bit for bit - the restatement performs the same correctly rounded double
operations in the same order and rounds to float once; theta (atan2) within 1 ulp of float (pattern_ref.check_record)."""
import ctypes as C

import numpy as np

import correlation_amd as ca
from correlation_amd import _ffi

import pattern_ref as pr


def random_sums(rng, n):
    """nine sums a sector of n samples of a random image could have (consistent enough for every branch of the record)"""
    I = rng.integers(0, 256, n)
    gx = rng.integers(-255, 256, n)
    gy = rng.integers(-255, 256, n)
    if rng.random() < 0.3:
        gy = (gx * rng.integers(-1, 2) + rng.integers(-2, 3, n)).clip(-255, 255)   # nearly one-directional
    sums = np.array([I.sum(), (I * I).sum(), (gx * gx).sum(), (gy * gy).sum(), (gx * gy).sum(), (I <= 10).sum(), (I >= 245).sum(),
                     I.min(), I.max()], np.int64)
    return sums, float(np.sqrt((gx * gx + gy * gy).astype(np.float64)).sum())


def test_record_against_the_restatement_on_random_sums():
    rng = np.random.default_rng(21)
    seen = set()
    for trial in range(400):
        n = int(rng.choice([2, 3, 49, 361, 10000, 250000]))
        sums, mig = random_sums(rng, n)
        sigma = float(rng.choice([0.0, -1.0, 0.5, 1.0, 2.75]))
        max_sat = float(rng.choice([0.01, 0.08, 0.5, 1.0]))
        got = ca.pattern_from_sums(n, sums, mig, sigma, max_sat)
        seen.add(pr.check_record(got, n, sums, mig, sigma, max_sat, trial))
    assert seen == {ca.PATTERN_OK, ca.PATTERN_APERTURE, ca.PATTERN_SATURATED}, seen


def test_giant_sector_does_not_overflow():
    # Gxx Gyy of 2^31 - 1 samples of full contrast is about 2^94: the sums are converted to double first
    n = 2 ** 31 - 1
    g = 255 * 255 * n
    sums = np.array([128 * n, 128 * 128 * n + n, g, g, g // 3, 0, 0, 0, 255], np.int64)
    got = ca.pattern_from_sums(n, sums, 360.0 * n, 1.0, 1.0)
    assert pr.check_record(got, n, sums, 360.0 * n) == ca.PATTERN_OK
    assert got["sigma_u"] > 0 and np.isfinite(got["sigma_major"])


def test_every_status():
    ok = np.array([361 * 100, 361 * 100 * 100 + 5000, 40000, 50000, 1000, 3, 4, 17, 240], np.int64)
    assert pr.check_record(ca.pattern_from_sums(361, ok, 900.0), 361, ok, 900.0) == ca.PATTERN_OK
    # TOO_FEW: n < 2, every field but n_points is 0
    for n in (0, 1):
        got = ca.pattern_from_sums(n, ok, 900.0)
        assert got["status"] == ca.PATTERN_TOO_FEW and got["n_points"] == n
        assert not any(got[k] for k in pr.FLOATS) and got["grey_min"] == 0 and got["grey_max"] == 0
    two = ok.copy()
    two[5:7] = 0
    assert ca.pattern_from_sums(2, two, 900.0)["status"] == ca.PATTERN_OK
    # FLAT: no gradient at all; the grey-level fields are still filled
    flat = ok.copy()
    flat[2:5] = 0
    got = ca.pattern_from_sums(361, flat, 0.0)
    assert pr.check_record(got, 361, flat, 0.0) == ca.PATTERN_FLAT
    assert got["mean"] == 100 and got["grey_max"] == 240 and not any(got[k] for k in pr.SIGMAS)
    # APERTURE: one direction only (Gyy = 0), and two directions that are one (Gxy^2 = Gxx Gyy); before SATURATED
    for gxx, gyy, gxy in ((40000, 0, 0), (0, 50000, 0), (40000, 40000, 40000), (40000, 40000, -40000)):
        s = ok.copy()
        s[2:5] = gxx, gyy, gxy
        got = ca.pattern_from_sums(361, s, 900.0, 1.0, 0.0)
        assert pr.check_record(got, 361, s, 900.0, 1.0, 0.0) == ca.PATTERN_APERTURE, (gxx, gyy, gxy)
        assert got["sssig_x"] == gxx / 4 and not any(got[k] for k in pr.SIGMAS)
    # the rule is det <= 1e-6 Gxx Gyy: with Gxx = Gyy = 1e8 the bound is 1e10, and (1e8 - 50)^2 = 1e16 - 1e10 + 2500
    for gxy, want in ((10 ** 8 - 51, ca.PATTERN_OK), (10 ** 8 - 50, ca.PATTERN_APERTURE), (-(10 ** 8 - 50), ca.PATTERN_APERTURE)):
        s = ok.copy()
        s[2:5] = 10 ** 8, 10 ** 8, gxy
        assert (10 ** 16 - gxy * gxy <= 10 ** 10) == (want == ca.PATTERN_APERTURE)
        assert pr.check_record(ca.pattern_from_sums(361, s, 900.0), 361, s, 900.0) == want, gxy
    # SATURATED: strictly more than max_saturated of the samples are low or high; every field is filled
    sat = ok.copy()
    sat[5:7] = 100, 81
    assert ca.pattern_from_sums(361, sat, 900.0, 1.0, 0.5)["status"] == ca.PATTERN_SATURATED      # 181 > 180.5
    sat[6] = 80
    assert ca.pattern_from_sums(361, sat, 900.0, 1.0, 0.5)["status"] == ca.PATTERN_OK             # 180 <= 180.5
    sat[6] = 81
    got = ca.pattern_from_sums(361, sat, 900.0, 2.0, 0.5)
    assert pr.check_record(got, 361, sat, 900.0, 2.0, 0.5) == ca.PATTERN_SATURATED and got["sigma_u"] > 0
    # noise_sigma scales the sigmas and nothing else; <= 0 means 1
    one, two = ca.pattern_from_sums(361, ok, 900.0, 1.0), ca.pattern_from_sums(361, ok, 900.0, 2.0)
    assert two["sigma_u"] == 2 * one["sigma_u"] and two["sigma_major"] == 2 * one["sigma_major"] and two["theta"] == one["theta"]
    assert ca.pattern_from_sums(361, ok, 900.0, 0.0).tobytes() == one.tobytes()
    assert ca.pattern_from_sums(361, ok, 900.0, -3.0).tobytes() == one.tobytes()
    # an isotropic pattern: a circle, sigma_u = sigma_v = sigma_major = sqrt(8 / G)
    iso = ok.copy()
    iso[2:5] = 80000, 80000, 0
    got = ca.pattern_from_sums(361, iso, 900.0)
    assert got["sigma_u"] == got["sigma_v"] == got["sigma_major"] == np.float32(np.sqrt(8.0 / 80000))


def test_layouts_prototypes_and_refusals(engine_lib):
    assert ca.PATTERN_DTYPE.itemsize == 64 and ca.SUBSET_DTYPE.itemsize == 32 and ca.PATTERN_SUMS == 9 and ca.PATTERN_MAX_HALF == 128
    assert [ca.PATTERN_DTYPE.fields[k][1] for k in ("n_points", "status", "mean", "std", "grey_min", "grey_max", "frac_low",
                                                    "frac_high", "sssig_x", "sssig_y", "mig", "sigma_u", "sigma_v", "sigma_major",
                                                    "theta", "reserved")] == list(range(0, 64, 4))
    assert [ca.SUBSET_DTYPE.fields[k][1] for k in ("half", "status", "n_pixels", "clipped", "sssig_x", "sssig_y", "sigma_u",
                                                   "sigma_v")] == list(range(0, 32, 4))
    assert [ca.PATTERN_OK, ca.PATTERN_TOO_FEW, ca.PATTERN_FLAT, ca.PATTERN_APERTURE, ca.PATTERN_SATURATED] == list(range(5))
    assert [ca.SUBSET_OK, ca.SUBSET_NONE, ca.SUBSET_BAD_POINT] == list(range(3))
    assert C.sizeof(_ffi.LkPatternConfig) == 32 and C.sizeof(_ffi.LkSubsetConfig) == 32
    for name in ("lk_pattern_quality", "lk_pattern_from_sums", "lk_suggest_subset"):
        assert name in _ffi.SYMBOLS and hasattr(engine_lib, name)
    assert hasattr(engine_lib, "lk_internal_pattern_last")          # the bench hook: exported, not in include/
    sums = np.arange(9, dtype=np.int64)
    out = np.full(64, 7, np.uint8).view(ca.PATTERN_DTYPE)
    ptr = C.c_void_p
    f = engine_lib.lk_pattern_from_sums
    assert f(3, None, 1.0, 1.0, 1.0, out.ctypes.data_as(ptr)) == ca.ERROR_BAD_DOMAIN
    assert f(3, sums.ctypes.data_as(ptr), 1.0, 1.0, 1.0, None) == ca.ERROR_BAD_DOMAIN
    assert f(-1, sums.ctypes.data_as(ptr), 1.0, 1.0, 1.0, out.ctypes.data_as(ptr)) == ca.ERROR_BAD_DOMAIN
    for bad in (float("nan"), float("inf")):
        assert f(3, sums.ctypes.data_as(ptr), 1.0, bad, 1.0, out.ctypes.data_as(ptr)) == ca.ERROR_BAD_DOMAIN
        assert f(3, sums.ctypes.data_as(ptr), 1.0, 1.0, bad, out.ctypes.data_as(ptr)) == ca.ERROR_BAD_DOMAIN
    assert (out.view(np.uint8) == 7).all()                          # a refusal leaves the output untouched
    assert f(3, sums.ctypes.data_as(ptr), 1.0, 1.0, 1.0, out.ctypes.data_as(ptr)) == 0 and out["n_points"][0] == 3
    # the engine entry points refuse a null engine without touching anything
    assert engine_lib.lk_pattern_quality(None, None, None, None, None) == ca.ERROR_BAD_DOMAIN
    assert engine_lib.lk_suggest_subset(None, None, 0, None, None, None) == ca.ERROR_BAD_DOMAIN


def test_restatement_of_the_tables_is_a_brute_force_sum():
    # the int64 tables and the scan of pattern_ref.suggest against direct sums over the boxes, on a small image
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (23, 31)).astype(np.uint8)
    gx2, gy2 = pr.gradients(img)
    assert gx2[5, 0] == int(img[5, 1]) - int(img[5, 0]) and gx2[5, 30] == int(img[5, 30]) - int(img[5, 29])
    assert gy2[0, 7] == int(img[1, 7]) - int(img[0, 7]) and gy2[22, 7] == int(img[22, 7]) - int(img[21, 7])
    pts = np.float32([[0, 0], [30, 22], [15.4, 11.6], [-0.6, 3], [31.4, 3], [np.nan, 2], [4, np.inf], [30.49, 22.49], [30.5, 5]])
    rec, sums = pr.suggest(img, pts, 2e4, 1, 9, 2)
    assert rec["status"].tolist()[4:7] == [ca.SUBSET_BAD_POINT] * 3 and rec["status"][8] == ca.SUBSET_BAD_POINT
    assert rec["status"][3] != ca.SUBSET_BAD_POINT          # (int)(-0.6f + 0.5f) = 0: the conversion truncates towards zero
    for q, (x, y) in enumerate([(0, 0), (30, 22), (15, 12), (0, 3)]):
        for c, h in enumerate(range(1, 10, 2)):
            x0, x1, y0, y1 = max(x - h, 0), min(x + h, 30), max(y - h, 0), min(y + h, 22)
            assert sums[q, c, 0] == (gx2[y0:y1 + 1, x0:x1 + 1] ** 2).sum() and sums[q, c, 1] == (gy2[y0:y1 + 1, x0:x1 + 1] ** 2).sum()
        k = int(np.argmax((sums[q] >= 8e4).all(axis=1))) if (sums[q] >= 8e4).all(axis=1).any() else 4
        h = 1 + 2 * k
        assert rec["half"][q] == h and rec["clipped"][q] == int(x - h < 0 or y - h < 0 or x + h > 30 or y + h > 22)
        assert rec["n_pixels"][q] == (min(x + h, 30) - max(x - h, 0) + 1) * (min(y + h, 22) - max(y - h, 0) + 1)
