"""The numpy restatement of include/lk_engine.h's lk_flag_outliers paragraph: the median of n floats, the record of one
window (what lk_outlier_from_window computes), and the whole pass by brute force over all pairs.  Shared by
test_outlier_host.py and test_outlier_gpu.py.  Floats stay float32 and doubles float64 exactly where the header says so:
the plain test and the window function are restated bit for bit; the detrended pass differs from the device only in the
order of the plane's double sums."""
import numpy as np

import correlation_amd as ca
from correlation_amd import _ffi

FLOATS = ("med_u", "med_v", "mad_u", "mad_v", "ratio_u", "ratio_v")
F32, F64 = np.float32, np.float64


def median32(x):
    """(float)(((double)x[(n - 1) / 2] + (double)x[n / 2]) / 2) of the sorted values; a zero of either sign counts as +0"""
    x = np.sort(np.asarray(x, F32) + F32(0.0))
    n = len(x)
    return F32((F64(x[(n - 1) // 2]) + F64(x[n // 2])) / F64(2.0))


def window_record(e_u, e_v, es_u, es_v, eps, threshold):
    """-> an OUTLIER_DTYPE record (status OK / FLAGGED) and the two ratios as doubles"""
    out = np.zeros(1, ca.OUTLIER_DTYPE)[0]
    ratios = []
    for name, e, es in (("u", e_u, es_u), ("v", e_v, es_v)):
        e = np.asarray(e, F32)
        med = median32(e)
        mad = median32(np.abs(e.astype(F64) - F64(med)).astype(F32))
        r = np.abs(F64(F32(es)) - F64(med)) / (F64(mad) + F64(F32(eps)))
        out["med_" + name], out["mad_" + name], out["ratio_" + name] = med, mad, F32(r)
        ratios.append(r)
    out["neighbours"] = len(e_u)
    out["status"] = ca.OUTLIER_FLAGGED if max(ratios) > F64(F32(threshold)) else ca.OUTLIER_OK
    return out, ratios


def is_good(rec, n_params, chi_max):
    ok = (rec["error_code"] == 0) & np.isfinite(rec["chi"]) & np.isfinite(rec["p"][:, :n_params]).all(axis=1)
    if chi_max > 0:
        with np.errstate(invalid="ignore"):
            ok &= rec["chi"] <= F32(chi_max)
    return ok


def one_pass(c, u, v, good, member, r2, eps, threshold, min_neighbours, detrend):
    """c [S][2] float64 centres, u, v [S] float32; member [S]: may sit in a window (good and not excluded)"""
    S = len(c)
    out = np.zeros(S, ca.OUTLIER_DTYPE)
    ratio = np.zeros((S, 2))
    ud, vd = u.astype(F64), v.astype(F64)
    for s in range(S):
        d = c - c[s]
        near = member & (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= r2)
        near[s] = False
        n = int(near.sum())
        out["neighbours"][s] = n
        if n < min_neighbours:
            out["status"][s] = ca.OUTLIER_TOO_FEW
            continue
        if detrend:
            x, y, uu, vv = d[near, 0], d[near, 1], ud[near], vd[near]
            Sx, Sy, Su, Sv = x.sum(), y.sum(), uu.sum(), vv.sum()
            Cxx, Cxy, Cyy = (x * x).sum() - Sx * Sx / n, (x * y).sum() - Sx * Sy / n, (y * y).sum() - Sy * Sy / n
            Cxu, Cyu = (x * uu).sum() - Sx * Su / n, (y * uu).sum() - Sy * Su / n
            Cxv, Cyv = (x * vv).sum() - Sx * Sv / n, (y * vv).sum() - Sy * Sv / n
            D = Cxx * Cyy - Cxy * Cxy
            if Cxx * Cyy == 0 or not D > 1e-6 * (Cxx * Cyy):
                out["status"][s] = ca.OUTLIER_DEGENERATE
                continue
            ux, uy = (Cyy * Cxu - Cxy * Cyu) / D, (Cxx * Cyu - Cxy * Cxu) / D
            vx, vy = (Cyy * Cxv - Cxy * Cyv) / D, (Cxx * Cyv - Cxy * Cxv) / D
            u0, v0 = Su / n - ux * (Sx / n) - uy * (Sy / n), Sv / n - vx * (Sx / n) - vy * (Sy / n)
            e_u, e_v = (uu - (u0 + ux * x + uy * y)).astype(F32), (vv - (v0 + vx * x + vy * y)).astype(F32)
            es_u, es_v = F32(ud[s] - u0), F32(vd[s] - v0)
        else:
            e_u, e_v, es_u, es_v = u[near], v[near], u[s], v[s]
        if good[s]:
            out[s], ratio[s] = window_record(e_u, e_v, es_u, es_v, eps, threshold)
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                rec, _ = window_record(e_u, e_v, 0.0, 0.0, eps, threshold)
            rec["ratio_u"] = rec["ratio_v"] = 0
            rec["status"] = ca.OUTLIER_NOT_GOOD
            out[s] = rec
    return out, ratio


def flag_reference(cen, rec, model, radius, chi_max=0.0, eps=0.02, threshold=3.0, min_neighbours=4, detrend=True, passes=1):
    """-> (OUTLIER_DTYPE [S] of the last pass, its ratios as doubles [S][2], the flags of every pass [passes][S])"""
    good = is_good(rec, _ffi.N_PARAMS[model], chi_max)
    c = np.asarray(cen, F32).astype(F64)
    with np.errstate(invalid="ignore"):
        u = rec["p"][:, 0].astype(F32) + F32(0.0)
        v = rec["p"][:, 1].astype(F32) + F32(0.0) if model != ca.FM_U else np.zeros(len(c), F32)
    u, v = np.where(good, u, F32(0.0)), np.where(good, v, F32(0.0))   # (a bad record's values are never used)
    r2 = F64(F32(radius)) ** 2
    member = good.copy()
    history = []
    for _ in range(passes):
        out, ratio = one_pass(c, u, v, good, member, r2, eps, threshold, min_neighbours, detrend)
        flags = out["status"] == ca.OUTLIER_FLAGGED
        history.append(flags)
        member = good & ~flags
    return out, ratio, np.array(history)


def tolerances(ref, U, eps):
    """the detrended comparison's bounds per float field (test_outlier_gpu.py's docstring): tol_e for med and mad,
    (2 + ratio) tol_e / eps + 2^-22 ratio for the ratios, with tol_e = 2^-22 |ref| + 1e-9 max(U, 1)"""
    tol = {}
    base = 1e-9 * max(U, 1.0)
    for k in ("med_u", "med_v", "mad_u", "mad_v"):
        tol[k] = 2.0 ** -22 * np.abs(ref[k].astype(F64)) + base
    for k, m, a in (("ratio_u", "med_u", "mad_u"), ("ratio_v", "med_v", "mad_v")):
        r = ref[k].astype(F64)
        tol_e = np.maximum(tol[m], tol[a])
        tol[k] = (2.0 + r) * tol_e / eps + 2.0 ** -22 * r
    return tol
