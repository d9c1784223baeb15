"""Restatements behind the photometry and residual-map tests (include/lk_engine.h: lk_photometry, lk_residual_map): the
oracle's per-sample floats of a sector, a float64 numpy restatement of the photometry record from the samples themselves
(centred, not from the sums), the brute-force owner rule, and the oracle's back-warped values of a window.  Shared by
test_residual_host.py and test_residual_gpu.py."""
import numpy as np

import correlation_amd as ca
from correlation_amd import _ffi

FLOATS = ("mean_f", "mean_g", "std_f", "std_g", "zncc", "gain", "offset", "rms", "rms_zn", "znssd", "max_abs")
FLAT = 1e-12
KAPPA_MAX = 1e4

# ---- the lighting experiment ---------------------------------------------------------------------------------------------
# D = the deformed frame with its lowest bit cleared, D' = D / 2 + 32 (exact in u8).  The bicubic weights sum to one, so at
# the same records zncc' = zncc, gain' = gain / 2, offset' = offset / 2 + 32 and rms_zn' = rms_zn / 2 up to the sampler's
# float rounding.  Measured with the oracle restatement alone on the CPU (test_residual_host.py prints and pins them;
# DESIGN.md section 19), over the four rectangles of test_residual_gpu.py at its near-truth records, the largest
# |left - right| per field (rounded up in the third digit) was
#   zncc 0 (the same float in all four sectors), gain 2.99e-08, offset 5.73e-06, rms_zn 3.34e-06
# and the allowed difference is twice that - but never less than one float32 step at the compared value: every field is a
# double rounded to float once, and two doubles that differ in their ninth digit (the two sides are sums of differently
# rounded samples) can fall on either side of a rounding boundary.  That floor is what decides for zncc.
LIGHTING_MEASURED = {"zncc": 0.0, "gain": 2.99e-08, "offset": 5.73e-06, "rms_zn": 3.34e-06}


def lighting_tol(field, value):
    return max(2.0 * LIGHTING_MEASURED[field], float(np.spacing(np.float32(abs(float(value))))))


def lighting_sides(a, b):
    """records a (pair with D) and b (pair with D'): per field (left, right) of the four identities"""
    return {"zncc": (b["zncc"], a["zncc"]), "gain": (b["gain"], a["gain"] * np.float32(0.5)),
            "offset": (b["offset"], a["offset"] * np.float32(0.5) + np.float32(32.0)),
            "rms_zn": (b["rms_zn"], a["rms_zn"] * np.float32(0.5))}


def lighting_frames(dfm):
    d = (dfm & 0xFE).astype(np.uint8)
    return d, (d // 2 + 32).astype(np.uint8)


# ---- photometry ------------------------------------------------------------------------------------------------------------
def sample_values(oracle, interp, model, und, dfm, xy, cx, cy, p, sampler=None):
    """f, g, V float32 [n] of every sample of one sector and whether the sampler flagged a sample.  und, dfm: the images of
    the level; xy [n][2], (cx, cy) and p in that level's scale.  From the oracle alone: (xd, yd) by model_point, the deformed
    value there by interpolate_many, f the undeformed node.  sampler: stands in for interpolate_many where the oracle has no
    such sampler (the separable bicubic extension): points [n][2] -> [n][4] = W, dW/dx, dW/dy, flag."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    warped = np.zeros((len(xy), 2), np.float32)
    for k in range(len(xy)):
        warped[k] = oracle.model_point(model, float(xy[k, 0]), float(xy[k, 1]), float(cx), float(cy), p)[:2]
    w = sampler(warped) if sampler is not None else oracle.interpolate_many(interp, dfm, warped)
    bad = bool((w[:, 3] != 0).any())
    node = (xy + np.float32(0.5)).astype(np.int32)
    f = und[node[:, 1], node[:, 0]].astype(np.float32)
    g = w[:, 0].astype(np.float32)
    V = f - g
    assert V.dtype == np.float32
    return f, g, V, bad


def sum_terms(f, g, V):
    """the six summed products of every sample, [n][6] float64 (each exact, or rounded once)"""
    f, g, V = (np.asarray(a, np.float32).astype(np.float64) for a in (f, g, V))
    return np.stack([f, g, f * f, g * g, f * g, V * V], 1)


def sums_of(f, g, V):
    """the eight sums of an evaluated sector in numpy's order"""
    t = sum_terms(f, g, V)
    mx = float(np.abs(np.asarray(V, np.float32)).max()) if len(t) else 0.0
    return np.concatenate([t.sum(axis=0), [0.0, mx]])


def kappa(n, sums):
    """n sum x^2 / (n sum x^2 - (sum x)^2) of the worse of f and g (inf for a flat patch)"""
    out = 0.0
    for sx, sxx in ((sums[0], sums[2]), (sums[1], sums[3])):
        q = n * sxx
        v = q - sx * sx
        out = max(out, q / v if v > 0 else np.inf)
    return out


def restatement(f, g, V):
    """float64 restatement of the header from the samples themselves, centred -> (status, dict of float64 fields)"""
    f, g, V = (np.asarray(a, np.float32).astype(np.float64) for a in (f, g, V))
    n = len(f)
    zero = {k: 0.0 for k in FLOATS}
    if n < 2:
        return ca.PHOTO_TOO_FEW, zero
    mf, mg = f.mean(), g.mean()
    df, dg = f - mf, g - mg
    vf, vg, c = (df * df).mean(), (dg * dg).mean(), (df * dg).mean()
    out = dict(zero, mean_f=mf, mean_g=mg, std_f=np.sqrt(vf), std_g=np.sqrt(vg), rms=np.sqrt((V * V).mean()),
               max_abs=float(np.abs(V).max()))
    # the FLAT rule in the header's own terms (the tests' flat patches are constant: both forms give exactly 0)
    if not vf > FLAT * (f * f).mean() or not vg > FLAT * (g * g).mean():
        return ca.PHOTO_FLAT, out
    z = c / np.sqrt(vf * vg)
    gain = c / vf
    out.update(zncc=z, gain=gain, offset=mg - gain * mf, rms_zn=np.sqrt(vg) * np.sqrt(max(0.0, 1.0 - z * z)), znssd=2.0 * (1.0 - z))
    return ca.PHOTO_OK, out


def check_record(got, f, g, V, sums=None, what=None):
    """got: one PHOTOMETRY_DTYPE record of the samples f, g, V.  Statuses exactly.  Per float field the project's form
    (uncertainty_ref.check_record): 2^-22 |ref| + 1e-12 kappa |ref| - the float rounding of the output and the error of
    working from raw sums in double - with kappa = n sum x^2 / (n sum x^2 - (sum x)^2) of the worse of f and g; kappa > 1e4:
    status only.  Three fields are differences of nearly equal numbers, where an error relative to the result has no meaning
    (the result may be 0); there the error dz = 1e-12 kappa of zncc and gain is carried through the formula instead:
      offset = mean_g - gain mean_f          + dz (|mean_g| + |gain mean_f|)
      znssd  = 2 (1 - zncc)                  + 2 dz
      rms_zn = std_g sqrt(1 - zncc^2)        + std_g min(sqrt(2 dz), 2 dz / sqrt(1 - zncc^2))
    (|h(a) - h(b)| <= sqrt|h(a)^2 - h(b)^2| and = |h(a)^2 - h(b)^2| / (h(a) + h(b)) for h = sqrt(1 - z^2), |a^2 - b^2| <= 2 dz).
    max_abs is compared exactly.  -> worst error / tolerance"""
    n = len(f)
    status, ref = restatement(f, g, V)
    assert got["status"] == status and got["n_points"] == n and not got["reserved"].any(), (what, got, status)
    if status == ca.PHOTO_TOO_FEW:
        assert not any(got[k] for k in FLOATS), (what, got)
        return 0.0
    if sums is None:
        sums = sums_of(f, g, V)
    assert float(got["max_abs"]) == ref["max_abs"], (what, got["max_abs"], ref["max_abs"])
    if status == ca.PHOTO_FLAT:
        assert not any(got[k] for k in ("zncc", "gain", "offset", "rms_zn", "znssd")), (what, got)
        for k in ("mean_f", "mean_g", "rms"):
            assert abs(float(got[k]) - ref[k]) <= 2.0 ** -22 * abs(ref[k]), (what, k, got[k], ref[k])
        return 0.0
    kap = kappa(n, sums)
    if kap > KAPPA_MAX:
        return 0.0
    dz = 1e-12 * kap
    rel = 2.0 ** -22 + dz
    h = np.sqrt(max(0.0, 1.0 - ref["zncc"] ** 2))
    extra = {"offset": dz * (abs(ref["mean_g"]) + abs(ref["gain"] * ref["mean_f"])), "znssd": 2.0 * dz,
             "rms_zn": ref["std_g"] * min(np.sqrt(2.0 * dz), 2.0 * dz / h if h > 0 else np.inf)}
    worst = 0.0
    for k in FLOATS:
        err = abs(float(got[k]) - ref[k])
        tol = rel * abs(ref[k]) + extra.get(k, 0.0)
        assert err <= tol, (what, k, float(got[k]), ref[k], err, tol)
        if tol > 0:
            worst = max(worst, err / tol)
    return worst


# ---- the residual map ------------------------------------------------------------------------------------------------------
def brute_owner(centres, good, radius, x0, y0, w, h, level=0):
    """the owner rule by brute force in float64, [h][w] int32: rounded squares, one rounded sum, the first (lowest) index of
    the smallest d2 among the good sectors with d2 <= radius^2, else -1"""
    c = np.asarray(centres, np.float32).astype(np.float64)
    r = float(np.float32(radius))
    r2 = r * r
    ys, xs = np.mgrid[y0:y0 + h, x0:x0 + w]
    X, Y = xs.astype(np.float64) * (1 << level), ys.astype(np.float64) * (1 << level)
    dx = c[:, 0][:, None, None] - X[None]
    dy = c[:, 1][:, None, None] - Y[None]
    d2 = dx * dx + dy * dy
    ok = (d2 <= r2) & np.asarray(good, bool)[:, None, None]
    d2 = np.where(ok, d2, np.inf)
    own = d2.argmin(axis=0).astype(np.int32)
    own[~ok.any(axis=0)] = -1
    return own


def good_records(rec, model, chi_max=0.0):
    P = _ffi.N_PARAMS[model]
    g = (rec["error_code"] == 0) & np.isfinite(rec["chi"]) & np.isfinite(rec["p"][:, :P]).all(axis=1)
    if chi_max > 0:
        g &= rec["chi"] <= chi_max
    return g


def oracle_map(oracle, interp, model, und, dfm, centres, rec, good, radius, window, level=0, sampler=None):
    """(warped, residual, owner) of a window from the oracle alone: the brute-force owner; model_point of ((float)x, (float)y)
    about the owner's level-L centre with its level-L parameters; interpolate_many (or `sampler`) there; a flagged position
    gives owner -2 - s and NaN; residual = f - warped in float32."""
    x0, y0, w, h = window
    P = _ffi.N_PARAMS[model]
    own = brute_owner(centres, good, radius, x0, y0, w, h, level)
    scale = np.float32(1.0 / (1 << level))
    warped = np.full((h, w), np.nan, np.float32)
    idx = np.argwhere(own >= 0)
    pts = np.zeros((len(idx), 2), np.float32)
    for k, (j, i) in enumerate(idx):
        s = own[j, i]
        p = rec["p"][s].copy()
        p[:2] *= scale
        cx = np.float32(centres[s][0]) * scale if level else np.float32(centres[s][0])
        cy = np.float32(centres[s][1]) * scale if level else np.float32(centres[s][1])
        pts[k] = oracle.model_point(model, float(x0 + i), float(y0 + j), float(cx), float(cy), p[:P])[:2]
    val = (sampler(pts) if sampler is not None else oracle.interpolate_many(interp, dfm, pts)) if len(pts) else np.zeros((0, 4), np.float32)
    for k, (j, i) in enumerate(idx):
        if val[k, 3] != 0:
            own[j, i] = -2 - own[j, i]
        else:
            warped[j, i] = val[k, 0]
    residual = und[y0:y0 + h, x0:x0 + w].astype(np.float32) - warped
    return warped, residual.astype(np.float32), own
