"""A numpy restatement of the camera-noise pass (include/lk_engine.h: lk_camera_noise, lk_sector_noise, lk_noise_from_bins,
lk_noise_from_sums), written from the definitions, not from the C++: the integer tables with plain numpy int64 sums, the
records with Python's exact integers and fractions - every quotient below is the correctly rounded value of the exact
rational, so the library's doubles (exact integer combinations, one conversion and one division each) agree to a few ulp."""
import math
from fractions import Fraction

import numpy as np

OK, TOO_FEW, NO_MODEL = 0, 1, 2


def pixel_terms(frames):
    """frames [K][...] u8 -> (s1, q, g) int64 per pixel: s1 = sum x_f, q = K sum x_f^2 - s1^2, g = (2 s1 + K) // (2 K)"""
    x = np.asarray(frames).astype(np.int64)
    K = x.shape[0]
    s1 = x.sum(axis=0)
    q = K * (x * x).sum(axis=0) - s1 * s1
    return s1, q, (2 * s1 + K) // (2 * K)


def tables(frames, region=None, mask=None):
    """-> bins [256][2] int64 {count, sum q}, frame_sums [K] int64 over the counted pixels: region (x0, y0, x1, y1)
    inclusive or None = the whole frame, and of those the pixels with a nonzero mask byte"""
    x = np.asarray(frames)
    use = np.zeros(x.shape[1:], bool)
    if region is None:
        use[:] = True
    else:
        x0, y0, x1, y1 = region
        use[y0:y1 + 1, x0:x1 + 1] = True
    if mask is not None:
        use &= np.asarray(mask) != 0
    _, q, g = pixel_terms(x)
    bins = np.zeros((256, 2), np.int64)
    bins[:, 0] = np.bincount(g[use], minlength=256)
    for k in np.unique(g[use]):
        bins[k, 1] = q[use & (g == k)].sum()
    return bins, np.array([int(f[use].astype(np.int64).sum()) for f in x], np.int64)


def node(q, size):
    """the node of float32 positions along an axis: trunc(q + 0.5f) for 0 <= q + 0.5f < size, else -1 (outside)"""
    f = np.asarray(q, np.float32) + np.float32(0.5)
    ok = np.isfinite(f) & (f >= 0) & (f < size)
    return np.where(ok, np.trunc(np.where(ok, f, 0)).astype(np.int64), -1)


def sector_sums(frames, xy):
    """{n, sum q, sum s1} of the samples xy [n][2] whose node lies inside the frame"""
    x = np.asarray(frames)
    ix, iy = node(xy[:, 0], x.shape[2]), node(xy[:, 1], x.shape[1])
    ok = (ix >= 0) & (iy >= 0)
    s1, q, _ = pixel_terms(x[:, iy[ok], ix[ok]])
    return np.array([int(ok.sum()), int(q.sum()), int(s1.sum())], np.int64)


# ---- the recovery experiment (test_noise_host.py, scripts/noise_recovery.py -> profiles/noise_recovery.txt) ----------------
RECOVERY_SHAPE = (150, 232)
RECOVERY_CASES = ((4.0, 0.0), (1.0, 0.03), (0.25, 0.0))          # (a0, b0): var(g) = a0 + b0 g before rounding
RECOVERY_FRAMES = (2, 8)
RECOVERY_FIT = dict(grey_low=10, grey_high=245, min_count=30)


def recovery_base():
    """a smooth pattern over about 40 .. 220: a ramp along x, tilted a little along y"""
    rows, cols = RECOVERY_SHAPE
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    return 40.0 + 180.0 * (0.8 * x / (cols - 1) + 0.2 * y / (rows - 1))


def recovery_frames(K, a0, b0, seed):
    """K frames of the base with Gaussian noise of variance a0 + b0 g, rounded and clipped"""
    base = recovery_base()
    rng = np.random.default_rng(seed)
    sd = np.sqrt(a0 + b0 * base)
    return np.stack([np.clip(np.rint(base + sd * rng.standard_normal(base.shape)), 0, 255).astype(np.uint8) for _ in range(K)])


def recovery_expectation(a0, b0):
    """(a, b, pooled variance): rounding adds the quantisation variance 1 / 12"""
    return a0 + 1.0 / 12.0, b0, a0 + 1.0 / 12.0 + b0 * float(recovery_base().mean())


def _f(num, den=1):
    return float(Fraction(int(num), int(den)))


def from_bins(K, bins, frame_sums, grey_low=0, grey_high=255, min_count=2):
    """the record of lk_noise_from_bins as a dict"""
    c = [int(v) for v in np.asarray(bins)[:, 0]]
    sq = [int(v) for v in np.asarray(bins)[:, 1]]
    fs = [int(v) for v in frame_sums]
    N, SQ, F = sum(c), sum(sq), sum(fs)
    out = dict(n_pixels=N, n_frames=K, status=TOO_FEW, bins_used=0, var=0.0, var_detrended=0.0, a=0.0, b=0.0, sigma=0.0,
               sigma_detrended=0.0, flicker=0.0, mean=0.0, sigma_at_mean=0.0, fit_rms=0.0)
    if N < 2:
        return out
    kk1 = K * (K - 1)
    var = Fraction(SQ, N * kk1)
    mean = Fraction(F, K * N)
    o = [Fraction(f, N) - mean for f in fs]                      # the offset of every frame
    o2 = sum(v * v for v in o)
    det = (Fraction(SQ, K) - N * o2) / ((N - 1) * (K - 1))
    det = max(det, Fraction(0))
    used = [g for g in range(grey_low, grey_high + 1) if c[g] >= min_count]
    a, b, rms, status = var, Fraction(0), 0.0, NO_MODEL
    if len(used) >= 2:
        W = sum(c[g] for g in used)
        mg = Fraction(sum(c[g] * g for g in used), W)
        y = {g: Fraction(sq[g], c[g] * kk1) for g in used}
        my = sum(c[g] * y[g] for g in used) / W
        sgg = sum(c[g] * (g - mg) ** 2 for g in used)
        if sgg > 0:
            status = OK
            b = sum(c[g] * (g - mg) * (y[g] - my) for g in used) / sgg
            a = my - b * mg
            if len(used) > 2:
                rms = math.sqrt(float(sum(c[g] * (y[g] - a - b * g) ** 2 for g in used) / W))
    at_mean = float(a + b * mean)
    out.update(status=status, bins_used=len(used), var=float(var), var_detrended=float(det), a=float(a), b=float(b),
               sigma=math.sqrt(float(var)), sigma_detrended=math.sqrt(float(det)), flicker=math.sqrt(float(o2 / K)),
               mean=float(mean), sigma_at_mean=math.sqrt(max(at_mean, 0.0)), fit_rms=rms)
    return out


def from_sums(K, sums3):
    n, sq, s1 = (int(v) for v in sums3)
    if n < 2:
        return dict(n=n, status=TOO_FEW, sigma=0.0, mean=0.0, var=0.0)
    var = _f(sq, n * K * (K - 1))
    return dict(n=n, status=OK, sigma=math.sqrt(var), mean=_f(s1, n * K), var=var)


DOUBLES = ("var", "var_detrended", "a", "b")
FLOATS = ("sigma", "sigma_detrended", "flicker", "mean", "sigma_at_mean", "fit_rms")
INTS = ("n_pixels", "n_frames", "status", "bins_used")


def check_record(got, want, what=""):
    """integers equal, doubles to 1e-12 relative, float fields exactly the restatement's value rounded to float"""
    for k in INTS:
        assert int(got[k]) == want[k], (what, k, got[k], want[k])
    for k in DOUBLES:
        assert abs(float(got[k]) - want[k]) <= 1e-12 * abs(want[k]), (what, k, got[k], want[k])
    for k in FLOATS:
        assert np.float32(got[k]) == np.float32(want[k]), (what, k, got[k], want[k])
    assert not np.asarray(got["reserved"]).any()


def check_sector_record(got, want, what=""):
    assert int(got["n"]) == want["n"] and int(got["status"]) == want["status"], (what, got, want)
    assert abs(float(got["var"]) - want["var"]) <= 1e-12 * abs(want["var"]), (what, got, want)
    assert np.float32(got["sigma"]) == np.float32(want["sigma"]) and np.float32(got["mean"]) == np.float32(want["mean"]), (what, got, want)
    assert not np.asarray(got["reserved"]).any()
