"""Host side of the camera-noise pass (include/lk_engine.h): lk_noise_from_bins and lk_noise_from_sums - the only place a
floating-point number of the pass is made - against the restatement of noise_ref.py, the detrending identity against the
direct sum, the recovery of a known photon-transfer curve, the refusals, and the layouts of the binding.  No GPU.

Tolerances: integers equal; doubles to 1e-12 relative (both sides divide exact integer combinations once); float fields
exactly the restatement's value rounded to float."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import noise_ref as nr

# 5 x the standard deviation, over 20 seeds, of the restatement's own estimates of (a, b, pooled variance) on the recovery
# experiment: profiles/noise_recovery.txt, written by scripts/noise_recovery.py.  {(K, a0, b0): bounds}
RECOVERY_BOUNDS = {
    (2, 4.0, 0.0): (0.4000452474090971, 0.0034481260240318157, 0.15342456641692864),
    (2, 1.0, 0.03): (0.48535112566438987, 0.0049467905420081965, 0.21777910730048694),
    (2, 0.25, 0.0): (0.02982666924709779, 0.00023871808402249088, 0.010918965601621925),
    (8, 4.0, 0.0): (0.17812151975549514, 0.0012900293137992093, 0.05441786780094874),
    (8, 1.0, 0.03): (0.19748063732118337, 0.0016913086848846636, 0.06233713060051338),
    (8, 0.25, 0.0): (0.016051192948559476, 0.00011110136970655012, 0.005090883970125235),
}
RECOVERY_SEED = 1000   # (not one of the seeds the bounds were measured on)


def random_frames(rng, K, shape=(37, 53), spread=3.0, offsets=None):
    base = rng.integers(20, 236, shape).astype(np.float64)
    out = []
    for f in range(K):
        x = base + spread * rng.standard_normal(shape) + (offsets[f] if offsets is not None else 0.0)
        out.append(np.clip(np.rint(x), 0, 255).astype(np.uint8))
    return np.stack(out)


def test_library_exports_the_pass(engine_lib):
    for name in ("lk_camera_noise", "lk_sector_noise", "lk_noise_from_bins", "lk_noise_from_sums"):
        assert hasattr(engine_lib, name) and name in _ffi.SYMBOLS
    assert hasattr(engine_lib, "lk_internal_noise_last")


def test_records_against_the_restatement_on_random_frames():
    rng = np.random.default_rng(31)
    seen = set()
    for trial in range(60):
        K = int(rng.choice([2, 3, 5, 8, 16]))
        offsets = rng.normal(0.0, 2.0, K) if trial % 2 else None
        frames = random_frames(rng, K, spread=float(rng.choice([0.0, 0.6, 3.0, 9.0])), offsets=offsets)
        bins, fs = nr.tables(frames)
        fit = dict(grey_low=int(rng.choice([0, 30])), grey_high=int(rng.choice([255, 200])), min_count=int(rng.choice([2, 5, 12])))
        got = ca.noise_from_bins(K, bins, fs, **fit)
        want = nr.from_bins(K, bins, fs, **fit)
        nr.check_record(got, want, trial)
        seen.add(int(got["status"]))
        # a sector's record from three sums of the same frames
        ys, xs = np.mgrid[3:20, 5:26]
        sums = nr.sector_sums(frames, np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32))
        assert sums[0] == 17 * 21
        nr.check_sector_record(ca.noise_from_sums(K, sums), nr.from_sums(K, sums), trial)
    assert seen == {ca.NOISE_OK}


def test_every_status_and_the_edge_tables():
    K = 3
    empty = np.zeros((256, 2), np.int64)
    got = ca.noise_from_bins(K, empty, np.zeros(K, np.int64))
    nr.check_record(got, nr.from_bins(K, empty, np.zeros(K, np.int64)), "empty")
    assert got["status"] == ca.NOISE_TOO_FEW and got["n_pixels"] == 0 and got["n_frames"] == K
    one_pixel = empty.copy()
    one_pixel[77] = (1, 6)
    got = ca.noise_from_bins(K, one_pixel, np.int64([77, 78, 76]))
    nr.check_record(got, nr.from_bins(K, one_pixel, [77, 78, 76]), "one pixel")
    assert got["status"] == ca.NOISE_TOO_FEW and got["n_pixels"] == 1 and not any(got[k] for k in nr.DOUBLES + nr.FLOATS)
    # one bin: the pooled fields are valid, the model is the constant
    one_bin = empty.copy()
    one_bin[77] = (1000, 5400)
    fs = np.int64([77000, 77010, 76990])
    got = ca.noise_from_bins(K, one_bin, fs)
    nr.check_record(got, nr.from_bins(K, one_bin, fs), "one bin")
    assert got["status"] == ca.NOISE_NO_MODEL and got["bins_used"] == 1 and got["a"] == got["var"] == 0.9 and got["b"] == 0
    assert got["fit_rms"] == 0 and got["flicker"] > 0 and got["sigma_at_mean"] == np.float32(np.sqrt(0.9))
    # two bins of which min_count or the grey window leaves one: NO_MODEL; with both: a line through both, rms 0
    two = empty.copy()
    two[50] = (400, 2400)
    two[200] = (9, 270)
    fs = np.int64([21800, 21800, 21800])
    for fit, status, used in ((dict(min_count=10), ca.NOISE_NO_MODEL, 1), (dict(grey_high=199), ca.NOISE_NO_MODEL, 1),
                              (dict(grey_low=51, grey_high=199), ca.NOISE_NO_MODEL, 0), (dict(), ca.NOISE_OK, 2)):
        got = ca.noise_from_bins(K, two, fs, **fit)
        nr.check_record(got, nr.from_bins(K, two, fs, **fit), fit)
        assert got["status"] == status and got["bins_used"] == used and got["fit_rms"] == 0
    assert got["b"] == pytest.approx((5.0 - 1.0) / 150.0, rel=1e-14) and got["a"] == pytest.approx(1.0 - 50 * 4.0 / 150.0, rel=1e-13)
    # a falling curve is reported as fitted
    falling = empty.copy()
    for g, v in ((40, 9.0), (90, 7.0), (140, 5.5), (230, 1.0)):
        falling[g] = (600, int(v * 600 * 6))
    got = ca.noise_from_bins(K, falling, np.int64([300000] * 3))
    nr.check_record(got, nr.from_bins(K, falling, [300000] * 3), "falling")
    assert got["status"] == ca.NOISE_OK and got["b"] < 0 and got["bins_used"] == 4 and got["fit_rms"] > 0
    # sectors
    for sums, status in (([0, 0, 0], ca.NOISE_TOO_FEW), ([1, 0, 300], ca.NOISE_TOO_FEW), ([2, 12, 600], ca.NOISE_OK)):
        got = ca.noise_from_sums(K, sums)
        nr.check_sector_record(got, nr.from_sums(K, sums), sums)
        assert got["status"] == status and got["n"] == sums[0]
    assert got["var"] == 1.0 and got["sigma"] == 1.0 and got["mean"] == 100.0


def test_large_tables_do_not_overflow():
    # 2^31 pixels of K = 16 frames at the largest q, 16^2 255^2 / 4: SQ K N is about 2^89
    K, n = 16, 2 ** 31
    bins = np.zeros((256, 2), np.int64)
    bins[100] = (n // 2, (n // 2) * 4161600)
    bins[128] = (n // 4, (n // 4) * 4161600)
    bins[131] = (n // 4, (n // 4) * 3000000)
    fs = np.int64([n * 120 + f * 1000003 for f in range(K)])
    got = ca.noise_from_bins(K, bins, fs)
    nr.check_record(got, nr.from_bins(K, bins, fs), "large")
    assert got["status"] == ca.NOISE_OK and got["n_pixels"] == n and np.isfinite(got["fit_rms"]) and got["var_detrended"] > 0


def test_the_detrending_identity():
    """frames with their own offsets and integer noise (no rounding anywhere): var_detrended is the variance of the residual
    x - mean_p - o_f computed directly"""
    rng = np.random.default_rng(8)
    for K in (2, 3, 8):
        base = rng.integers(60, 190, (41, 59))
        off = rng.integers(-6, 7, K)
        x = np.stack([base + off[f] + rng.integers(-4, 5, base.shape) for f in range(K)])
        assert x.min() >= 0 and x.max() <= 255
        frames = x.astype(np.uint8)
        bins, fs = nr.tables(frames)
        got = ca.noise_from_bins(K, bins, fs)
        N = base.size
        xd = x.astype(np.float64)
        o = xd.mean(axis=(1, 2)) - xd.mean()
        r = xd - xd.mean(axis=0) - o[:, None, None]
        direct = float((r * r).sum()) / ((N - 1) * (K - 1))
        print(f"K {K}: var {got['var']:.6f}, detrended {got['var_detrended']:.6f}, direct {direct:.6f}, flicker {got['flicker']:.4f}")
        assert abs(got["var_detrended"] - direct) <= 1e-10 * direct
        assert got["flicker"] == pytest.approx(np.sqrt((o * o).mean()), rel=1e-6)
        assert got["var_detrended"] < got["var"]           # the offsets were part of the pooled variance
        # the variance of the integers -4 .. 4; five standard deviations of the estimate from 41 x 59 pixels are below 10 %
        assert got["var_detrended"] == pytest.approx(20.0 / 3.0, rel=0.1)


@pytest.mark.parametrize("K", nr.RECOVERY_FRAMES)
@pytest.mark.parametrize("a0,b0", nr.RECOVERY_CASES)
def test_recovery_of_a_known_curve(K, a0, b0):
    frames = nr.recovery_frames(K, a0, b0, RECOVERY_SEED)
    assert frames.shape == (K, 150, 232) and frames.min() > 25 and frames.max() < 235
    got = ca.noise_from_bins(K, *nr.tables(frames), **nr.RECOVERY_FIT)
    want = nr.recovery_expectation(a0, b0)
    bound = RECOVERY_BOUNDS[(K, a0, b0)]
    err = [float(got[k]) - w for k, w in zip(("a", "b", "var"), want)]
    print(f"K {K} a0 {a0} b0 {b0}: a {got['a']:.4f} b {got['b']:.5f} var {got['var']:.4f}; errors {err}, bounds {bound}")
    assert got["status"] == ca.NOISE_OK and got["bins_used"] > 150
    for e, b in zip(err, bound):
        assert abs(e) <= b, (err, bound)
    assert got["sigma_at_mean"] == pytest.approx(np.sqrt(got["a"] + got["b"] * got["mean"]), rel=1e-6)


def test_refusals_of_the_host_functions():
    L = _ffi.load_library()
    P = C.c_void_p
    bins = np.zeros((256, 2), np.int64)
    bins[10] = (5, 20)
    fs = np.int64([50, 50, 50])
    out = np.full(96, 7, np.uint8)
    sec = np.full(32, 7, np.uint8)

    def ptr(a):
        return a.ctypes.data_as(P) if a is not None else None

    def from_bins(K=3, b=bins, f=fs, low=0, high=255, count=2, o=out):
        return L.lk_noise_from_bins(K, ptr(b), ptr(f), low, high, count, ptr(o))

    assert from_bins(b=None) == from_bins(f=None) == from_bins(o=None) == ca.ERROR_BAD_DOMAIN
    for K in (-1, 0, 1, 17):
        assert from_bins(K=K) == ca.ERROR_BAD_DOMAIN
        assert L.lk_noise_from_sums(K, ptr(np.int64([4, 8, 400])), ptr(sec)) == ca.ERROR_BAD_DOMAIN
    for low, high in ((-1, 255), (256, 255), (0, -1), (0, 256)):
        assert from_bins(low=low, high=high) == ca.ERROR_BAD_DOMAIN
    for count in (1, 0, -5):
        assert from_bins(count=count) == ca.ERROR_BAD_DOMAIN
    for at in ((10, 0), (200, 1)):
        bad = bins.copy()
        bad[at] = -1
        assert from_bins(b=bad) == ca.ERROR_BAD_DOMAIN
    assert from_bins(f=np.int64([50, -1, 50])) == ca.ERROR_BAD_DOMAIN
    assert L.lk_noise_from_sums(3, None, ptr(sec)) == L.lk_noise_from_sums(3, ptr(np.int64([4, 8, 400])), None) == ca.ERROR_BAD_DOMAIN
    for bad in ([-1, 8, 400], [4, -8, 400], [4, 8, -400], [2 ** 31, 8, 400]):
        assert L.lk_noise_from_sums(3, ptr(np.int64(bad)), ptr(sec)) == ca.ERROR_BAD_DOMAIN
    assert (out == 7).all() and (sec == 7).all()         # the outputs are untouched
    assert from_bins() == 0 and L.lk_noise_from_sums(16, ptr(np.int64([4, 8, 400])), ptr(sec)) == 0
    with pytest.raises(ValueError):
        ca.noise_from_bins(3, bins, fs[:2])


def test_struct_sizes_and_field_offsets():
    d = ca.NOISE_DTYPE
    assert d.itemsize == 96
    assert [d.fields[k][1] for k in ("n_pixels", "var", "var_detrended", "a", "b", "status", "n_frames", "bins_used", "sigma",
                                     "sigma_detrended", "flicker", "mean", "sigma_at_mean", "fit_rms", "reserved")] == \
        [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60, 64, 68, 72, 76]
    s = ca.SECTOR_NOISE_DTYPE
    assert s.itemsize == 32 and [s.fields[k][1] for k in ("n", "status", "sigma", "mean", "var", "reserved")] == [0, 4, 8, 12, 16, 24]
    c = _ffi.LkNoiseConfig
    assert C.sizeof(c) == 64
    assert [getattr(c, k).offset for k in ("source", "n_frames", "slots", "first", "x0", "y0", "x1", "y1", "grey_low", "grey_high",
                                           "min_count", "reserved")] == [0, 4, 8, 20, 24, 28, 32, 36, 40, 44, 48, 52]
    # the library writes exactly these bytes: a record into a guarded buffer, the fields where the dtype has them
    L = _ffi.load_library()
    bins = np.zeros((256, 2), np.int64)
    bins[40] = (30, 360)
    bins[90] = (50, 1500)
    fs = np.int64([3000, 3100, 2900, 3000])
    buf = np.full(96 + 16, 0xA5, np.uint8)
    assert L.lk_noise_from_bins(4, bins.ctypes.data_as(C.c_void_p), fs.ctypes.data_as(C.c_void_p), 0, 255, 2, buf.ctypes.data_as(C.c_void_p)) == 0
    assert (buf[96:] == 0xA5).all()
    rec = buf[:96].view(d)[0]
    assert rec["n_pixels"] == 80 and rec["n_frames"] == 4 and rec["bins_used"] == 2 and rec["status"] == ca.NOISE_OK
    assert rec["var"] == 1860 / (80 * 12) and rec["mean"] == np.float32(12000 / 320) and not rec["reserved"].any()
    buf = np.full(32 + 16, 0xA5, np.uint8)
    assert L.lk_noise_from_sums(2, np.int64([8, 64, 1600]).ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)) == 0
    rec = buf[:32].view(s)[0]
    assert (buf[32:] == 0xA5).all() and rec["n"] == 8 and rec["var"] == 4.0 and rec["sigma"] == 2.0 and rec["mean"] == 100.0
    assert (ca.NOISE_IMAGES, ca.NOISE_RING, ca.NOISE_MAX_FRAMES) == (0, 1, 16)
    assert (ca.NOISE_OK, ca.NOISE_TOO_FEW, ca.NOISE_NO_MODEL) == (0, 1, 2)
