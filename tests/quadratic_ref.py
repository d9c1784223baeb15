"""Restatements behind the second-order refinement tests (include/lk_engine.h: lk_refine_quadratic,
lk_quadratic_step_from_sums): the float32 warp, the per-sample terms of the 87 sums, the expansion of the sums into SH, SHH,
SHf, SHg of the twelve parameters, a float64 numpy restatement of the criterion and the damped step (znssd_ref.step on
twelve parameters), the Levenberg-Marquardt loop around them, the test pair with its exactly quadratic field, the test
geometry and the bounds measured with the restatement alone.  Shared by test_quadratic_host.py and test_quadratic_gpu.py."""
import functools

import numpy as np

import correlation_amd as ca
from correlation_amd import speckle

import znssd_ref as zr

P = 12
FLAT, MIN_PIVOT, LAMBDA0, PRECISION, MAX_ITERS = zr.FLAT, zr.MIN_PIVOT, zr.LAMBDA0, zr.PRECISION, zr.MAX_ITERS
W0, T0, TF0, TG0, SPARE, FLAGGED = 5, 50, 62, 74, 86, 87
# the 15 monomials X^a Y^b, a + b <= 4, by degree, then by falling a
MONO = [(d - b, b) for d in range(5) for b in range(d + 1)]
# parameter k: H_k = COEF[k] g_(COMP[k]) X^a Y^b, (a, b) = EXPO[k]; COMP 0: g_x (the u terms), 1: g_y (the v terms)
COMP = [0, 1, 0, 0, 1, 1, 0, 0, 0, 1, 1, 1]
EXPO = [(0, 0), (0, 0), (1, 0), (0, 1), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (2, 0), (1, 1), (0, 2)]
COEF = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 1.0, 0.5, 0.5, 1.0, 0.5]

# ---- the test pair ---------------------------------------------------------------------------------------------------------
# D(x) = B(x), the analytic blob sum; U(X) = B(X + w(X)) at the pixel nodes with the quadratic field w about (128, 128): U(X) =
# D(X + w(X)) exactly before the rounding to u8, so the truth at a subset centre is w and its derivatives there.  (Moving the
# blob centres instead, as speckle_pair does, leaves 0.1 - 0.3 px of model error in the "truth".)
SIZE, SIGMA, AMP = 256, 2.5, 0.6
FIELD = (1.3, -0.7, 0.002, 0.0, 0.0, -0.001, 1.2e-3, -4e-4, 6e-4, -5e-4, 6e-4, -1e-3)
FIELD_CENTRE = (128.0, 128.0)

# squares centred on range(48, 210, 40)^2 with sides 21 (a 16-lane row), 31 and 49 (a wavefront), one 96 x 96 square (the
# 512-lane group) and one annular list sector
CENTRES = [(x, y) for y in range(48, 210, 40) for x in range(48, 210, 40)]
SIDES = (21, 31, 49)


def square(x, y, side):
    h = side // 2
    return (x - h, y - h, x + h, y + h)


RECTS = [square(x, y, side) for side in SIDES for (x, y) in CENTRES] + [(80, 80, 175, 175)]
SIDE_OF = [side for side in SIDES for _ in CENTRES] + [96]
ANNULAR = zr.ANNULAR
N_SECTORS = len(RECTS) + len(ANNULAR)
BIG, RING = len(RECTS) - 1, len(RECTS)

# ---- bounds measured with this restatement alone, on the CPU --------------------------------------------------------------
# python -m pytest tests/test_quadratic_host.py -s -k accuracy prints them and pins them.  The loop
# runs in float64 around the oracle's own float bicubic sampler, from the zero-gradient seed at the true translation.
# ACCURACY_Q[side]: the largest |(u, v) - truth| over the 25 squares of that side, twelve parameters.
# SECOND_Q[side]: the largest |second-order term - truth| of the same refinement.
# AFFINE_BIAS[side]: the mean over the same squares of max(|u - truth|, |v - truth|) of the six-parameter loop (znssd_ref.loop).
# The GPU tests allow 1.5 times ACCURACY_Q and SECOND_Q - znssd_ref's margin for the float sampling of the device against
# the float64 loop - and ask lk_refine_znssd for at least half of AFFINE_BIAS.
ACCURACY_Q = {21: 0.0162, 31: 0.0065, 49: 0.0045}      # measured 0.016085, 0.006395, 0.004443 px
ACCURACY_BIG, ACCURACY_RING = 0.0026, 0.057             # the same figure of the 96 x 96 square (measured 0.002554) and of the
#                                                         annular sector (280 samples on a thin arc: measured 0.0563)
SECOND_Q = {21: 5.3e-4, 31: 2.0e-4, 49: 3.8e-5}         # measured 5.264e-4, 1.979e-4, 3.765e-5 per px
AFFINE_BIAS = {21: 0.0349, 31: 0.0747, 49: 0.1764}      # measured 0.034861, 0.074653, 0.176335 px (largest 0.048, 0.113, 0.237)


def field_at(X, Y):
    """w(X, Y) -> (wx, wy), float64"""
    u, v, ux, uy, vx, vy, uxx, uxy, uyy, vxx, vxy, vyy = FIELD
    dx, dy = np.asarray(X, np.float64) - FIELD_CENTRE[0], np.asarray(Y, np.float64) - FIELD_CENTRE[1]
    return (u + ux * dx + uy * dy + 0.5 * uxx * dx * dx + uxy * dx * dy + 0.5 * uyy * dy * dy,
            v + vx * dx + vy * dy + 0.5 * vxx * dx * dx + vxy * dx * dy + 0.5 * vyy * dy * dy)


def truth_at(cx, cy):
    """the twelve parameters of the field about (cx, cy), float64"""
    u, v, ux, uy, vx, vy, uxx, uxy, uyy, vxx, vxy, vyy = FIELD
    dx, dy = float(cx) - FIELD_CENTRE[0], float(cy) - FIELD_CENTRE[1]
    wx, wy = field_at(cx, cy)
    return np.array([wx, wy, ux + uxx * dx + uxy * dy, uy + uxy * dx + uyy * dy, vx + vxx * dx + vxy * dy, vy + vxy * dx + vyy * dy,
                     uxx, uxy, uyy, vxx, vxy, vyy])


def blob_sum(xs, ys, amps, X, Y):
    """sum of the blobs at the points (X, Y) [n], float64"""
    X, Y = np.asarray(X, np.float64).ravel(), np.asarray(Y, np.float64).ravel()
    out = np.zeros(len(X))
    inv = -0.5 / (SIGMA * SIGMA)
    for a in range(0, len(X), 1024):
        dx = X[a:a + 1024, None] - xs[None, :]
        dy = Y[a:a + 1024, None] - ys[None, :]
        out[a:a + 1024] = (amps[None, :] * np.exp((dx * dx + dy * dy) * inv)).sum(axis=1)
    return out


@functools.lru_cache(maxsize=None)
def _pair():
    xs, ys, amps = (a.astype(np.float64) for a in speckle.blobs(SIZE, SIZE, 5))
    amps = amps * AMP
    Y, X = np.mgrid[0:SIZE, 0:SIZE].astype(np.float64)
    wx, wy = field_at(X, Y)

    def grey(v):
        return np.rint(np.minimum(v, 1.0) * 255.0).astype(np.uint8).reshape(SIZE, SIZE)
    dfm = grey(blob_sum(xs, ys, amps, X, Y))
    und = grey(blob_sum(xs, ys, amps, X + wx, Y + wy))
    und.setflags(write=False)
    dfm.setflags(write=False)
    return und, dfm


def pair():
    """(undeformed, deformed) u8 [256][256]; computed once and shared, read-only"""
    return _pair()


def rect_rows(x0, y0, x1, y1):
    return zr.rect_rows(x0, y0, x1, y1)


def sector_lists(oracle, rects=RECTS, annular=ANNULAR):
    """the samples of the sectors in the pass's order, and their centres (float32, as the engine commits them)"""
    lists = [rect_rows(*r) for r in rects] + [np.asarray(oracle.annular_points(*q), np.float32).reshape(-1, 2) for q in annular]
    centres = [(np.float32(l[:, 0].astype(np.float64).mean()), np.float32(l[:, 1].astype(np.float64).mean())) for l in lists]
    return lists, centres


def true_translation_seeds(centres):
    """-> (guesses [S][6]: the field's translation at the centre, gradients 0; truth [S][12])"""
    truth = np.array([truth_at(cx, cy) for cx, cy in centres])
    g = np.zeros((len(centres), 6), np.float32)
    g[:, :2] = truth[:, :2]
    return g, truth


# ---- the warp and the per-sample floats ------------------------------------------------------------------------------------
def warp(xy, cx, cy, p):
    """the header's float32 warp without contraction -> (xd, yd, dx, dy) float32 [n]"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    p = np.asarray(p, np.float32)
    assert p.shape == (P,)
    x, y = xy[:, 0], xy[:, 1]
    dx, dy = x - np.float32(cx), y - np.float32(cy)
    half = np.float32(0.5)
    hxx, hxy, hyy = half * (dx * dx), dx * dy, half * (dy * dy)
    xd = (((((x + p[0]) + p[2] * dx) + p[3] * dy) + p[6] * hxx) + p[7] * hxy) + p[8] * hyy
    yd = (((((y + p[1]) + p[4] * dx) + p[5] * dy) + p[9] * hxx) + p[10] * hxy) + p[11] * hyy
    assert xd.dtype == np.float32 and yd.dtype == np.float32
    return xd, yd, dx, dy


def sample_floats(oracle, interp, und, dfm, xy, cx, cy, p, sampler=None):
    """f, g, gx, gy, dx, dy float32 [n] of every sample of one sector and which samples the sampler flagged: the warp above,
    the deformed value and gradient there by the oracle's interpolate_many (or `sampler`: points [n][2] -> [n][4] = W, dW/dx,
    dW/dy, flag), f the undeformed node."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    xd, yd, dx, dy = warp(xy, cx, cy, p)
    warped = np.stack([xd, yd], 1)
    w = sampler(warped) if sampler is not None else oracle.interpolate_many(interp, dfm, warped)
    bad = w[:, 3] != 0
    node = (xy + np.float32(0.5)).astype(np.int32)
    f = und[node[:, 1], node[:, 0]].astype(np.float32)
    return f, w[:, 0].astype(np.float32), w[:, 1].astype(np.float32), w[:, 2].astype(np.float32), dx, dy, bad


def affine_H(gx, gy, dx, dy):
    """H of the six-parameter model in float32, as the solve's own jacobian forms it"""
    H = np.stack([gx, gy, gx * dx, gx * dy, gy * dx, gy * dy], 1)
    assert H.dtype == np.float32
    return H


def sum_terms(f, g, gx, gy, dx, dy):
    """the summed products of every sample in the layout of the sums, [n][87] float64 (the spare column is 0): every product
    rounded once, in the header's order of operations"""
    f, g, gx, gy, X, Y = (np.asarray(a, np.float32).astype(np.float64) for a in (f, g, gx, gy, dx, dy))
    one = np.ones_like(X)
    X2, Y2 = X * X, Y * Y
    Xa, Yb = [one, X, X2, X2 * X, X2 * X2], [one, Y, Y2, Y2 * Y, Y2 * Y2]
    M = [Xa[a] * Yb[b] for a, b in MONO]
    cols = [f, g, f * f, g * g, f * g]
    for w in (gx * gx, gx * gy, gy * gy):
        cols += [w * m for m in M]
    t = [gx * m for m in M[:6]] + [gy * m for m in M[:6]]
    cols += t + [k * f for k in t] + [k * g for k in t] + [np.zeros_like(X)]
    out = np.stack(cols, 1)
    assert out.shape[1] == FLAGGED
    return out


def sums_of(f, g, gx, gy, dx, dy, bad):
    """QD_SUMS doubles of one evaluation in numpy's order: the flagged samples are left out and counted"""
    ok = ~np.asarray(bad, bool)
    out = np.zeros(ca.QD_SUMS)
    out[:FLAGGED] = sum_terms(f[ok], g[ok], gx[ok], gy[ok], dx[ok], dy[ok]).sum(axis=0)
    out[FLAGGED] = float((~ok).sum())
    return out


def sums_from_H(f, g, gx, gy, dx, dy):
    """the 88 sums in plain float64 from float64 samples (no float32 anywhere): for tests of the step alone"""
    X, Y = np.asarray(dx, np.float64), np.asarray(dy, np.float64)
    M = [X ** a * Y ** b for a, b in MONO]
    cols = [f, g, f * f, g * g, f * g]
    for w in (gx * gx, gx * gy, gy * gy):
        cols += [w * m for m in M]
    t = [gx * m for m in M[:6]] + [gy * m for m in M[:6]]
    cols += t + [k * f for k in t] + [k * g for k in t]
    out = np.zeros(ca.QD_SUMS)
    out[:SPARE] = np.stack(cols, 1).sum(axis=0)
    return out


# ---- expansion, criterion and step -------------------------------------------------------------------------------------------
def expand(sums):
    """SH [12], SHH [12][12], SHf [12], SHg [12] of the twelve parameters from the 88 sums: moments times 1, 1/2 or 1/4"""
    s = np.asarray(sums, np.float64)
    at = [COMP[k] * 6 + MONO.index(EXPO[k]) for k in range(P)]
    SH = np.array([COEF[k] * s[T0 + at[k]] for k in range(P)])
    SHf = np.array([COEF[k] * s[TF0 + at[k]] for k in range(P)])
    SHg = np.array([COEF[k] * s[TG0 + at[k]] for k in range(P)])
    SHH = np.zeros((P, P))
    for k in range(P):
        for l in range(P):
            e = (EXPO[k][0] + EXPO[l][0], EXPO[k][1] + EXPO[l][1])
            SHH[k, l] = (COEF[k] * COEF[l]) * s[W0 + (COMP[k] + COMP[l]) * 15 + MONO.index(e)]
    return SH, SHH, SHf, SHg


def criterion(n, sums):
    """-> (refusing status or 0, crit, gain, offset, zncc) in float64: znssd_ref.criterion with twelve parameters"""
    if n < P + 2:
        return ca.ZN_TOO_FEW, 0.0, 0.0, 0.0, 0.0
    N = float(n)
    Sf, Sg, Sff, Sgg, Sfg = (float(t) for t in sums[:5])
    qf, qg = N * Sff, N * Sgg
    vf, vg, c = qf - Sf * Sf, qg - Sg * Sg, N * Sfg - Sf * Sg
    if not vf > FLAT * qf or not vg > FLAT * qg:
        return ca.ZN_FLAT, 0.0, 0.0, 0.0, 0.0
    vv = vf * vg
    gain = c / vg
    rest = 1.0 - c * c / vv
    out = (rest if rest > 0.0 else 0.0, gain, (Sf - gain * Sg) / N, c / np.sqrt(vv))
    return (0 if c > 0.0 else ca.ZN_NEGATIVE,) + out


def normal_equations(n, sums, gain):
    """A [12][12] and b [12] of the header, undamped"""
    SH, SHH, SHf, SHg = expand(sums)
    N = float(n)
    A = gain * gain * (SHH - np.outer(SH, SH) / N) / N
    b = gain * ((SHf - SH * sums[0] / N) - gain * (SHg - SH * sums[1] / N)) / N
    return A, b


def step(n, sums, lam):
    """float64 restatement of lk_quadratic_step_from_sums -> (status, delta [12], crit, gain, offset, zncc, scaled), scaled =
    delta sqrt(diag A), the unknowns of the unit-diagonal system (zeros unless status is 0).  The status comes from the
    pivots of the unpivoted L D L^T of the scaled, damped matrix; the solution from numpy's solver on the same matrix."""
    delta, scaled = np.zeros(P), np.zeros(P)
    refused, crit, gain, offset, zncc = criterion(n, sums)
    if refused:
        return refused, delta, crit, gain, offset, zncc, scaled
    A, b = normal_equations(n, sums, gain)
    d = np.diag(A)
    if not (d > 0).all():
        return ca.ZN_SINGULAR, delta, crit, gain, offset, zncc, scaled
    root = np.sqrt(d)
    Cm = A / np.outer(root, root)
    Cm[np.diag_indices(P)] = 1.0 + lam
    L, D = np.eye(P), np.zeros(P)
    for j in range(P):
        D[j] = Cm[j, j] - (L[j, :j] ** 2 * D[:j]).sum()
        if not D[j] > MIN_PIVOT:
            return ca.ZN_SINGULAR, delta, crit, gain, offset, zncc, scaled
        for i in range(j + 1, P):
            L[i, j] = (Cm[i, j] - (L[i, :j] * L[j, :j] * D[:j]).sum()) / D[j]
    y = np.linalg.solve(Cm, b / root)
    return 0, y / root, crit, gain, offset, zncc, y


def weights(n):
    h = max(1.0, np.sqrt(float(n)) / 2.0)
    return np.array([1.0, 1.0, h, h, h, h, h * h / 2.0, h * h, h * h / 2.0, h * h / 2.0, h * h, h * h / 2.0])


def weighted_step(n, delta):
    return float((weights(n) * np.abs(delta)).max())


def bend(p, n0):
    """the info's bend from level-0 parameters, float64"""
    p = np.asarray(p, np.float32).astype(np.float64)
    h0 = np.sqrt(float(n0)) / 2.0
    return h0 * h0 * max(abs(p[6]) / 2.0 + abs(p[7]) + abs(p[8]) / 2.0, abs(p[9]) / 2.0 + abs(p[10]) + abs(p[11]) / 2.0)


# ---- the loop ----------------------------------------------------------------------------------------------------------------
def loop(evaluate, n, seed, max_iters=MAX_ITERS, precision=PRECISION, lambda0=LAMBDA0):
    """The header's loop (znssd_ref.loop on twelve parameters) in float64 around evaluate(p float32 [12]) -> QD_SUMS sums.
    -> dict(status, p float32 [12], iterations, evaluations, lam, last_step, sums, crit, gain, offset, zncc, zncc_seed)."""
    p = np.asarray(seed, np.float32).copy()
    out = dict(status=None, p=p, iterations=0, evaluations=1, lam=float(lambda0), last_step=0.0, sums=np.zeros(ca.QD_SUMS),
               crit=0.0, gain=0.0, offset=0.0, zncc=0.0, zncc_seed=0.0)
    sums = evaluate(p)
    if sums[FLAGGED] != 0:
        out["status"] = ca.ZN_OUT_OF_IMAGE
        return out
    refused, crit, gain, offset, zncc = criterion(n, sums)
    out.update(sums=sums, crit=crit, gain=gain, offset=offset, zncc=zncc)
    if refused:
        out["status"] = refused
        return out
    out["zncc_seed"] = zncc
    lam = float(lambda0)
    while out["status"] is None:
        if out["iterations"] >= max_iters:
            out["status"] = ca.ZN_MAX_ITERS
            break
        out["iterations"] += 1
        st, delta = step(n, out["sums"], lam)[:2]
        accepted = small_rejected = False
        if st == 0:
            trial = (out["p"].astype(np.float64) + delta).astype(np.float32)
            sums = evaluate(trial)
            out["evaluations"] += 1
            if sums[FLAGGED] == 0:
                refused, crit, gain, offset, zncc = criterion(n, sums)
                accepted = refused == 0 and crit < out["crit"]
                small_rejected = refused == 0 and not accepted and weighted_step(n, delta) < precision
        if accepted:
            lam = max(0.1 * lam, 1e-9)
            out.update(p=trial, sums=sums, crit=crit, gain=gain, offset=offset, zncc=zncc, last_step=weighted_step(n, delta))
            if out["last_step"] < precision:
                out["status"] = ca.ZN_CONVERGED
        elif st == 0 and small_rejected:
            out["status"] = ca.ZN_CONVERGED   # a step below the precision that the float samples cannot resolve: p stays
        else:
            lam = 10.0 * lam
            if lam >= 1e9:
                out["status"] = ca.ZN_STALLED
        out["lam"] = lam
    return out


def sector_evaluator(oracle, interp, und, dfm, xy, cx, cy, sampler=None):
    """evaluate(p [12]) of one sector for loop(): the sums of the per-sample floats at p"""
    def evaluate(p):
        return sums_of(*sample_floats(oracle, interp, und, dfm, xy, cx, cy, p, sampler))
    return evaluate


def affine_evaluator(oracle, interp, und, dfm, xy, cx, cy):
    """evaluate(p [6]) of one sector for znssd_ref.loop(): the six-parameter sums from the same sampler (with zero
    second-order terms the warp above gives the bits of the affine warp)"""
    def evaluate(p):
        p12 = np.zeros(P, np.float32)
        p12[:6] = p
        f, g, gx, gy, dx, dy, bad = sample_floats(oracle, interp, und, dfm, xy, cx, cy, p12)
        return zr.sums_of(f, g, affine_H(gx, gy, dx, dy), bad)
    return evaluate
