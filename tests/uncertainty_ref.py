"""Restatements behind the uncertainty tests (include/lk_engine.h: lk_parameter_uncertainty): the oracle's per-sample
values turned into the 28 sums of a sector, a float64 numpy restatement of lk_uncertainty_from_sums, and the consistency
experiment (is the predicted sigma the scatter of u?).  Shared by test_uncertainty_host.py and test_uncertainty_gpu.py."""
import numpy as np

import correlation_amd as ca
from correlation_amd import _ffi

FLOATS = ("noise", "rho_uv", "sigma_major", "sigma_minor", "theta", "sssig_x", "sssig_y")
MIN_PIVOT = 1e-10


def sample_terms(oracle, interp, model, und, dfm, xy, cx, cy, p, sampler=None):
    """The 28 products of every sample of one sector, [n][28] float64, and whether the sampler flagged a sample.
    und, dfm: the images of the level; xy [n][2], (cx, cy) and p in that level's scale.  Per sample, from the oracle alone:
    (xd, yd) and dT/dp by model_point, the deformed value and gradient there by interpolate_many, the residual against the
    undeformed node, J_k = Wx dTx[k] + Wy dTy[k] with float32 products and a float32 sum - the reference's per-sample
    floats.  The products J_a J_b, J_a V, V V of those floats are formed in float64 (exact, or rounded once).
    sampler: stands in for interpolate_many where the oracle has no such sampler (the separable bicubic extension):
    points [n][2] -> [n][4] = W, dW/dx, dW/dy, flag."""
    P = _ffi.N_PARAMS[model]
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    n = len(xy)
    warped = np.zeros((n, 2), np.float32)
    dTx, dTy = np.zeros((n, 6), np.float32), np.zeros((n, 6), np.float32)
    for k in range(n):
        xd, yd, dTx[k], dTy[k] = oracle.model_point(model, float(xy[k, 0]), float(xy[k, 1]), float(cx), float(cy), p)
        warped[k] = xd, yd
    w = sampler(warped) if sampler is not None else oracle.interpolate_many(interp, dfm, warped)
    bad = bool((w[:, 3] != 0).any())
    node = (xy + np.float32(0.5)).astype(np.int32)
    V = und[node[:, 1], node[:, 0]].astype(np.float32) - w[:, 0]
    J = (w[:, 1:2] * dTx[:, :P] + w[:, 2:3] * dTy[:, :P]).astype(np.float32)
    assert J.dtype == np.float32 and V.dtype == np.float32
    J64, V64 = J.astype(np.float64), V.astype(np.float64)
    cols = [J64[:, a] * J64[:, b] for a in range(P) for b in range(a, P)] + [J64[:, a] * V64 for a in range(P)] + [V64 * V64]
    terms = np.zeros((n, _ffi.UNC_SUMS))
    terms[:, :len(cols)] = np.stack(cols, 1)
    return terms, bad


def unpack(model, sums):
    P = _ffi.N_PARAMS[model]
    A = np.zeros((P, P))
    iu = np.triu_indices(P)
    A[iu] = sums[:len(iu[0])]
    A = A + np.triu(A, 1).T
    return A, np.asarray(sums[len(iu[0]):len(iu[0]) + P], np.float64), float(sums[len(iu[0]) + P])


def restatement(model, n, sums, level=0):
    """float64 restatement of the header: -> (status, dict of float64 fields with sigma [6], cond(C) or nan)"""
    P = _ffi.N_PARAMS[model]
    zero = dict(sigma=np.zeros(6), **{k: 0.0 for k in FLOATS})
    if n <= P:
        return ca.UNC_TOO_FEW, zero, np.nan
    A, _, chi = unpack(model, np.asarray(sums, np.float64))
    d = np.diag(A)
    if (d == 0).any():
        return ca.UNC_SINGULAR, zero, np.nan
    scale = np.sqrt(np.outer(d, d))
    Cm = A / scale
    # the pivots of the unpivoted L D L^T, for the status alone
    L, D = np.eye(P), np.zeros(P)
    for j in range(P):
        D[j] = Cm[j, j] - (L[j, :j] ** 2 * D[:j]).sum()
        if D[j] <= MIN_PIVOT:
            return ca.UNC_SINGULAR, zero, np.nan
        for i in range(j + 1, P):
            L[i, j] = (Cm[i, j] - (L[i, :j] * L[j, :j] * D[:j]).sum()) / D[j]
    s2 = chi / (n - P)
    cov = s2 * np.linalg.inv(Cm) / scale
    up = float(1 << level)
    sigma = np.zeros(6)
    sigma[:P] = np.sqrt(np.diag(cov))
    sigma[:2] *= up
    out = dict(sigma=sigma, noise=np.sqrt(s2), sssig_x=A[0, 0] / n, sssig_y=0.0, rho_uv=0.0, sigma_major=sigma[0],
               sigma_minor=0.0, theta=0.0)
    if P >= 2:
        blk = cov[:2, :2] * up * up
        w, vec = np.linalg.eigh(blk)
        theta = np.arctan2(vec[1, 1], vec[0, 1])
        theta = (theta + np.pi / 2) % np.pi - np.pi / 2
        out.update(sssig_y=A[1, 1] / n, rho_uv=blk[0, 1] / np.sqrt(blk[0, 0] * blk[1, 1]), sigma_major=np.sqrt(w[1]),
                   sigma_minor=np.sqrt(max(w[0], 0.0)), theta=theta)
    return ca.UNC_OK, out, float(np.linalg.cond(Cm))


def check_record(got, model, n, sums, level=0, what=None, cond_max=1e4):
    """got: one UNCERTAINTY_DTYPE record.  Tolerance per float field: 2^-22 |ref| + 1e-12 cond(C) |ref| - the float rounding
    of the output, and the error of inverting in double.  theta is an angle of an axis: compared modulo pi.
    -> worst error / tolerance"""
    status, ref, cond = restatement(model, n, sums, level)
    assert got["status"] == status and got["n_points"] == n and got["reserved"] == 0, (what, got, status)
    if status != ca.UNC_OK:
        assert not got["sigma"].any() and not any(got[k] for k in FLOATS), (what, got)
        return 0.0
    assert cond < cond_max, (what, cond)
    worst = 0.0
    pairs = [(got["sigma"][k], ref["sigma"][k], f"sigma[{k}]") for k in range(6)] + [(got[k], ref[k], k) for k in FLOATS]
    for g, r, name in pairs:
        err = abs(float(g) - r)
        if name == "theta":
            err = min(err, abs(err - np.pi))
        tol = (2.0 ** -22 + 1e-12 * cond) * abs(r)
        assert err <= tol, (what, name, float(g), r, err, tol)
        if tol > 0:
            worst = max(worst, err / tol)
    return worst


# ---- the consistency experiment ---------------------------------------------------------------------------------------
# One speckle image, twice, with independent Gaussian noise on both copies before rounding to u8: the true displacement
# of every sector is 0, the scatter of the solved u over the sectors is the measurement error, and the mean predicted
# sigma[0] should be that scatter.  12 x 12 sectors of 19 x 19, LK_FM_UV, bicubic, py_stop = 2.
EXP_SIDE, EXP_N, EXP_X0 = 19, 12, 8
EXP_NOISE = 4.0          # grey levels, each image
EXP_PRECISION = 1e-3
# std(u over the sectors) / mean(predicted sigma_u), measured with the oracle alone (test_uncertainty_host.py prints and
# pins it).  144 sectors: about +-6 % statistical spread around the ideal 1.
R_ORACLE = 1.3388


def experiment_pair():
    from correlation_amd import speckle
    base = speckle.speckle_pair(256, 256, p=(0, 0, 0, 0, 0, 0), seed=11)[0].astype(np.float64)
    rng = np.random.default_rng(2024)
    noisy = [np.clip(np.rint(base + rng.normal(0.0, EXP_NOISE, base.shape)), 0, 255).astype(np.uint8) for _ in range(2)]
    return noisy[0], noisy[1]


def experiment_rects():
    """sector i * n + j = column i, row j (lk_set_rect_grid's numbering)"""
    return [(EXP_X0 + EXP_SIDE * i, EXP_X0 + EXP_SIDE * j, EXP_X0 + EXP_SIDE * i + EXP_SIDE - 1, EXP_X0 + EXP_SIDE * j + EXP_SIDE - 1)
            for i in range(EXP_N) for j in range(EXP_N)]


def rect_rows(x0, y0, x1, y1):
    """the samples of a rectangle row by row (y outer, x inner): the order the pass walks an implicit rectangle in"""
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)


def rect_level(r, level):
    """a rectangle at a pyramid level: the coordinates divisible by 2^level, divided (pyramid_class.cpp:301-322)"""
    m = 1 << level
    return (-(-r[0] // m), -(-r[1] // m), r[2] // m, r[3] // m)


def experiment_ratio(oracle, und, dfm, rec, centres):
    """R = std(u) / mean(sigma_u predicted from the restated sums at the records' parameters, through the host function)"""
    sig = []
    for s, r in enumerate(experiment_rects()):
        terms, bad = sample_terms(oracle, ca.IM_BICUBIC, ca.FM_UV, und, dfm, rect_rows(*r), centres[s][0], centres[s][1],
                                  rec["p"][s][:2])
        assert not bad
        got = ca.uncertainty_from_sums(ca.FM_UV, len(terms), terms.sum(axis=0), 0)
        assert got["status"] == ca.UNC_OK
        sig.append(float(got["sigma"][0]))
    return float(np.std(rec["p"][:, 0].astype(np.float64)) / np.mean(sig)), float(np.mean(sig))
