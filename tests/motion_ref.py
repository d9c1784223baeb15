"""A float64 brute-force restatement of lk_rigid_motion (include/lk_engine.h): the same products as the kernel, plain np.sum
instead of its chunks and butterflies.  Shared by tests/test_motion_host.py and tests/test_motion_gpu.py.

What the restatement and the device may differ in is the order of the double sums, so the restatement also returns what
bounds that difference:
  abs_sums   sum |term| of each of the twelve sums.  Any two summation orders of n terms differ by at most
             2 (n - 1) 2^-53 sum |term| =: eps sum |term| (each partial sum is off by at most 2^-53 of its own size, which no
             partial sum's size exceeds sum |term|; there are n - 1 additions on either side).
  bound      what that does to the record's floats, to first order and with every constant rounded up.  With
             P = sum (x^2 + y^2), Q = sum (u^2 + v^2) over the fit set, R = max |x|, |y| (all relative to the origin):
               a centred moment C_ab = S_ab - S_a S_b / n moves by at most 6 eps sqrt(sum a^2 sum b^2)   (three sums, and
               sum |a| sum |b| / n <= sqrt(sum a^2 sum b^2)), hence dCxx, dCxy, dCyy <= 6 eps P =: dP and
               dCxu .. dCyv <= 6 eps sqrt(P Q) =: dX;  dnum <= 2 dX,  dden <= 2 dP + 2 dX;
               c: eps R;  t: eps max |u|, |v|;
               A  rigid: a unit vector of (den, num): 2 (dnum + dden) / h;  similarity: (dnum + dden) / W + |A| 2 dP / W with
                  W = Cxx + Cyy;  affine: g = M^-1 b, so (2 dX + 4 dP |g|) / lambda_min(M);  translation: 0;
               scale = sqrt |det A|: 2 |A| dA / scale;  theta: 4 dA / |(ayx - axy, axx + ayy)|;
               rms, max_residual: a residual moves by at most 2 (dt + dc (1 + 2 |A|) + 2 R dA), and the sum of their squares
               adds eps rms.
             |A| is the largest |entry|.  Against the restatement a float of the device is then within
             2^-22 |ref| + bound: the first term is its own rounding to float (2^-24) with room for the few double roundings
             of the formulas."""
import numpy as np

import correlation_amd as ca
from correlation_amd import _ffi

FLOATS = ("cx", "cy", "tx", "ty", "axx", "axy", "ayx", "ayy", "theta", "scale", "rms", "max_residual")
FROM_SUMS = ("cx", "cy", "tx", "ty", "axx", "axy", "ayx", "ayy", "scale", "n_fit", "status")   # byte for byte from the sums
MIN_SECTORS = {ca.MOTION_TRANSLATION: 1, ca.MOTION_RIGID: 2, ca.MOTION_SIMILARITY: 2, ca.MOTION_AFFINE: 3}


def is_good(rec, n_params, chi_max):
    ok = (rec["error_code"] == 0) & np.isfinite(rec["chi"]) & np.isfinite(rec["p"][..., :n_params]).all(axis=-1)
    if chi_max > 0:
        with np.errstate(invalid="ignore"):
            ok &= rec["chi"] <= np.float32(chi_max)
    return ok


def origin_of(cen):
    c = np.asarray(cen, np.float32).astype(np.float64)
    return (c.min(axis=0) + c.max(axis=0)) / 2.0


def terms_of(x, y, u, v):
    return [x, y, x * x, x * y, y * y, u, x * u, y * u, v, x * v, y * v]


def fit_from_sums(kind, min_sectors, n, s):
    """-> (status, c (relative to the origin), t, A) in float64"""
    I = np.eye(2)
    if n < min_sectors:
        return ca.MOTION_TOO_FEW, None, None, None
    Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv = s
    Cxx, Cxy, Cyy = Sxx - Sx * Sx / n, Sxy - Sx * Sy / n, Syy - Sy * Sy / n
    Cxu, Cyu, Cxv, Cyv = Sxu - Sx * Su / n, Syu - Sy * Su / n, Sxv - Sx * Sv / n, Syv - Sy * Sv / n
    c, t = np.float64([Sx / n, Sy / n]), np.float64([Su / n, Sv / n])
    if kind == ca.MOTION_TRANSLATION:
        return ca.MOTION_OK, c, t, I
    if kind in (ca.MOTION_RIGID, ca.MOTION_SIMILARITY):
        num, den = Cxv - Cyu, Cxx + Cxu + Cyy + Cyv
        h = np.sqrt(num * num + den * den)
        if Cxx + Cyy == 0 or h == 0:
            return ca.MOTION_DEGENERATE, None, None, None
        return ca.MOTION_OK, c, t, np.float64([[den, -num], [num, den]]) / (h if kind == ca.MOTION_RIGID else Cxx + Cyy)
    D = Cxx * Cyy - Cxy * Cxy
    if Cxx * Cyy == 0 or not D > 1e-6 * Cxx * Cyy:
        return ca.MOTION_DEGENERATE, None, None, None
    ux, uy = (Cyy * Cxu - Cxy * Cyu) / D, (Cxx * Cyu - Cxy * Cxu) / D
    vx, vy = (Cyy * Cxv - Cxy * Cyv) / D, (Cxx * Cyv - Cxy * Cxv) / D
    A = np.float64([[1 + ux, uy], [vx, 1 + vy]])
    if np.linalg.det(A) == 0:
        return ca.MOTION_DEGENERATE, None, None, None
    return ca.MOTION_OK, c, t, A


def propagated_bound(kind, n, x, y, u, v, s, A, rms):
    """the docstring's `bound` per float field"""
    eps = 2.0 * max(n - 1, 0) * 2.0 ** -53
    P, Q = float((x * x + y * y).sum()), float((u * u + v * v).sum())
    R, U = float(np.abs(np.concatenate([x, y])).max()), float(np.abs(np.concatenate([u, v])).max())
    dP, dX = 6 * eps * P, 6 * eps * np.sqrt(P * Q)
    dnum, dden = 2 * dX, 2 * dP + 2 * dX
    Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv = s
    Cxx, Cxy, Cyy = Sxx - Sx * Sx / n, Sxy - Sx * Sy / n, Syy - Sy * Sy / n
    num, den = (Sxv - Sx * Sv / n) - (Syu - Sy * Su / n), Cxx + (Sxu - Sx * Su / n) + Cyy + (Syv - Sy * Sv / n)
    a = float(np.abs(A).max())
    if kind == ca.MOTION_TRANSLATION:
        dA = 0.0
    elif kind == ca.MOTION_RIGID:
        dA = 2 * (dnum + dden) / np.hypot(num, den)
    elif kind == ca.MOTION_SIMILARITY:
        dA = (dnum + dden) / (Cxx + Cyy) + a * 2 * dP / (Cxx + Cyy)
    else:
        lam = np.linalg.eigvalsh(np.float64([[Cxx, Cxy], [Cxy, Cyy]]))[0]
        dA = (2 * dX + 2 * dP * float(np.abs(A - np.eye(2)).max()) * 2) / lam
    dc, dt = eps * R, eps * U
    scale = np.sqrt(abs(np.linalg.det(A)))
    dr = 2 * (dt + dc * (1 + 2 * a) + 2 * R * dA) + eps * rms
    return dict(cx=dc, cy=dc, tx=dt, ty=dt, axx=dA, axy=dA, ayx=dA, ayy=dA, scale=2 * a * dA / scale,
                theta=4 * dA / np.hypot(A[1, 0] - A[0, 1], A[0, 0] + A[1, 1]), rms=dr, max_residual=dr)


def motion_reference(cen, rec, model, kind, chi_max=0.0, fit_mask=None, reject=0.0, passes=1, min_sectors=None):
    """One frame.  cen [S][2] float32, rec [S] -> a dict: the record's fields in float64 (the float fields 0 unless OK), `sums`
    [12] and `abs_sums` [12] of the last pass that ran, `bound` (propagated_bound; None unless OK), `keep` (the last fit set),
    `margin` (the smallest |r_j - threshold| met by a trimming decision, inf without one), `good`."""
    if min_sectors is None:
        min_sectors = MIN_SECTORS[kind]
    o = origin_of(cen)
    c = np.asarray(cen, np.float32).astype(np.float64) - o
    good = is_good(rec, _ffi.N_PARAMS[model], chi_max)
    with np.errstate(invalid="ignore"):
        u = rec["p"][:, 0].astype(np.float64)
        v = rec["p"][:, 1].astype(np.float64) if model != ca.FM_U else np.zeros(len(c))
    base = good if fit_mask is None else good & (np.asarray(fit_mask) != 0)
    out = dict(good=good, margin=np.inf)
    keep, thr, prev = base.copy(), np.inf, None
    for k in range(passes):
        if k > 0:
            r_prev = residuals(prev, c[base, 0], c[base, 1], u[base], v[base])
            out["margin"] = min(out["margin"], float(np.abs(r_prev - thr).min()))
            keep = base.copy()
            keep[np.flatnonzero(base)[r_prev > thr]] = False
        x, y, uu, vv = c[keep, 0], c[keep, 1], u[keep], v[keep]
        n = int(keep.sum())
        terms = terms_of(x, y, uu, vv)
        s = [t.sum() for t in terms]
        status, cc, tt, A = fit_from_sums(kind, min_sectors, n, s)
        out.update(n_fit=n, n_rejected=int(base.sum()) - n, status=status, passes_run=k + 1, keep=keep,
                   sums=np.float64([n] + s), abs_sums=np.float64([n] + [np.abs(t).sum() for t in terms]), bound=None)
        for name in FLOATS:
            out[name] = 0.0
        if status != ca.MOTION_OK:
            break
        prev = (cc, tt, A)
        r = residuals(prev, x, y, uu, vv)
        rms = np.sqrt((r * r).sum() / n)
        thr = np.float64(np.float32(reject)) * rms if reject > 0 else np.inf
        out.update(cx=o[0] + cc[0], cy=o[1] + cc[1], tx=tt[0], ty=tt[1], axx=A[0, 0], axy=A[0, 1], ayx=A[1, 0], ayy=A[1, 1],
                   theta=np.arctan2(A[1, 0] - A[0, 1], A[0, 0] + A[1, 1]), scale=np.sqrt(abs(np.linalg.det(A))), rms=rms,
                   max_residual=r.max(), bound=propagated_bound(kind, n, x, y, uu, vv, s, A, rms))
    return out


def residuals(fit, x, y, u, v):
    c, t, A = fit
    dx, dy = x - c[0], y - c[1]
    rx = (x + u) - (c[0] + t[0] + (A[0, 0] * dx + A[0, 1] * dy))
    ry = (y + v) - (c[1] + t[1] + (A[1, 0] * dx + A[1, 1] * dy))
    return np.sqrt(rx * rx + ry * ry)


def remove_reference(model, m, cen, rec, good):
    """the `removal` paragraph in float64 from a MOTION_DTYPE-like record m: -> p [S][6] float64 (unchanged where not good)"""
    p = rec["p"].astype(np.float64)
    if int(m["status"]) != ca.MOTION_OK:
        return p
    A = np.float64([[m["axx"], m["axy"]], [m["ayx"], m["ayy"]]])
    Ai = np.linalg.inv(A)
    c, t = np.float64([m["cx"], m["cy"]]), np.float64([m["tx"], m["ty"]])
    X = np.asarray(cen, np.float32).astype(np.float64)
    for s in np.flatnonzero(good):
        uv = np.float64([p[s, 0], p[s, 1] if model != ca.FM_U else 0.0])
        x2 = c + Ai @ (X[s] + uv - c - t)
        p[s, 0] = x2[0] - X[s, 0]
        if model != ca.FM_U:
            p[s, 1] = x2[1] - X[s, 1]
        if model == ca.FM_UVQ:
            G = Ai @ np.float64([[1, -p[s, 2]], [p[s, 2], 1]])
            p[s, 2] = (G[1, 0] - G[0, 1]) / 2
        elif model == ca.FM_UVUXUYVXVY:
            G = Ai @ np.float64([[1 + p[s, 2], p[s, 3]], [p[s, 4], 1 + p[s, 5]]])
            p[s, 2:6] = [G[0, 0] - 1, G[0, 1], G[1, 0], G[1, 1] - 1]
    return p


def sums_of_points(x, y, u, v):
    """n and the eleven sums of positions (relative to an origin of the caller's) and displacements, for lk_motion_from_sums"""
    x, y, u, v = (np.asarray(a, np.float64) for a in (x, y, u, v))
    return len(x), np.float64([t.sum() for t in terms_of(x, y, u, v)])
