"""Restatements behind the ZNSSD refinement tests (include/lk_engine.h: lk_refine_znssd, lk_znssd_step_from_sums): the
oracle's per-sample floats turned into the sums of a sector, a float64 numpy restatement of the criterion and the damped
step, the Levenberg-Marquardt loop around them, the test geometry and the bounds measured with the restatement alone.
Shared by test_znssd_host.py and test_znssd_gpu.py."""
import numpy as np

import correlation_amd as ca
from correlation_amd import _ffi, speckle

from residual_ref import lighting_frames  # noqa: F401  (D and D' = D / 2 + 32)

FLAT = 1e-12
MIN_PIVOT = 1e-10
LAMBDA0 = float(np.float32(1e-3))
PRECISION = float(np.float32(1e-3))
MAX_ITERS = 50

# ---- the test geometry --------------------------------------------------------------------------------------------------
# a 256 x 256 speckle pair with a known affine map; an 8 x 8 grid of 19 x 19 rectangles (16-lane rows), one 24 x 24 rectangle
# (a wavefront), one 96 x 96 rectangle (9 216 samples: the 512-lane group and its LDS reduction), one annular list sector
TRUTH = (1.3, -0.7, 0.002, 0.0, 0.0, -0.001)
SIDE, GRID_N, GRID_X0 = 19, 8, 8
GRID = [(GRID_X0 + SIDE * i, GRID_X0 + SIDE * j, GRID_X0 + SIDE * i + SIDE - 1, GRID_X0 + SIDE * j + SIDE - 1)
        for i in range(GRID_N) for j in range(GRID_N)]
RECTS = GRID + [(170, 20, 193, 43), (150, 150, 245, 245)]
ANNULAR = [(20.0, 12.0, 0.3, 0.9, 70.0, 205.0, 6)]
N_SECTORS = len(RECTS) + len(ANNULAR)

# ---- bounds measured with this restatement alone, on the CPU ---------------------------------------------------------------
# python -m pytest tests/test_znssd_host.py -s -k "lighting or accuracy" prints both and pins them.
# D_LIGHT: the largest |(u, v) on D - (u, v) on D'| over the N_SECTORS sectors, each refined by loop() from the zero-gradient
# seed (TRUTH's translation, gradients 0), six parameters, bicubic.  The GPU tests allow twice that: the margin covers the
# float sampling of the device against this restatement's float64 loop around the same float samples' sums.
# ACCURACY: the largest |(u, v) - analytic map at the sector's centre| of the same refinement on the clean pair; the GPU
# tests allow 1.5 times that.
D_LIGHT = 1.6e-4     # measured 0.000154 px
ACCURACY = 0.0265    # measured 0.026415 px


def pair():
    return speckle.speckle_pair(256, 256, p=TRUTH, seed=5)


def analytic_uv(cx, cy, size=256):
    u, v, ux, uy, vx, vy = TRUTH
    dx, dy = cx - size / 2.0, cy - size / 2.0
    return u + ux * dx + uy * dy, v + vx * dx + vy * dy


def rect_rows(x0, y0, x1, y1):
    """the samples of a rectangle row by row (y outer, x inner): the order the pass walks an implicit rectangle in"""
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)


def rect_centre(r):
    xy = rect_rows(*r)
    return np.float32(xy[:, 0].astype(np.float64).mean()), np.float32(xy[:, 1].astype(np.float64).mean())


def zero_gradient_seeds(S):
    g = np.zeros((S, 6), np.float32)
    g[:, :2] = TRUTH[:2]
    return g


# ---- sums ------------------------------------------------------------------------------------------------------------------
def layout(P):
    """offsets of SH, SHH, SHf, SHg, the flagged count, and the length"""
    NA = P * (P + 1) // 2
    H = 5
    HH = H + P
    HF = HH + NA
    HG = HF + P
    return H, HH, HF, HG, HG + P, HG + P + 1


def sample_floats(oracle, interp, model, und, dfm, xy, cx, cy, p, sampler=None):
    """f, g [n] and H [n][P] float32 of every sample of one sector, and whether the sampler flagged a sample - from the oracle
    alone, as uncertainty_ref.sample_terms: (xd, yd) and dT/dp by model_point, the deformed value and gradient there by
    interpolate_many (or `sampler`), f the undeformed node, H_k = g_x dTx[k] + g_y dTy[k] with float32 products and a
    float32 sum."""
    P = _ffi.N_PARAMS[model]
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    n = len(xy)
    warped = np.zeros((n, 2), np.float32)
    dTx, dTy = np.zeros((n, 6), np.float32), np.zeros((n, 6), np.float32)
    pp = np.asarray(p, np.float32)[:P]
    for k in range(n):
        xd, yd, dTx[k], dTy[k] = oracle.model_point(model, float(xy[k, 0]), float(xy[k, 1]), float(cx), float(cy), pp)
        warped[k] = xd, yd
    w = sampler(warped) if sampler is not None else oracle.interpolate_many(interp, dfm, warped)
    bad = w[:, 3] != 0
    node = (xy + np.float32(0.5)).astype(np.int32)
    f = und[node[:, 1], node[:, 0]].astype(np.float32)
    H = (w[:, 1:2] * dTx[:, :P] + w[:, 2:3] * dTy[:, :P]).astype(np.float32)
    assert H.dtype == np.float32
    return f, w[:, 0].astype(np.float32), H, bad


def sum_terms(f, g, H):
    """the summed products of every sample in the layout of the sums (without the flagged count), [n][5 + 3 P + NA] float64:
    each product exact or rounded once"""
    f, g, H = (np.asarray(a, np.float32).astype(np.float64) for a in (f, g, H))
    P = H.shape[1]
    cols = [f, g, f * f, g * g, f * g] + [H[:, k] for k in range(P)]
    cols += [H[:, a] * H[:, b] for a in range(P) for b in range(a, P)]
    cols += [H[:, k] * f for k in range(P)] + [H[:, k] * g for k in range(P)]
    return np.stack(cols, 1)


def sums_of(f, g, H, bad):
    """ZN_SUMS doubles of one evaluation in numpy's order: the flagged samples are left out and counted"""
    ok = ~np.asarray(bad, bool)
    t = sum_terms(f[ok], g[ok], H[ok])
    out = np.zeros(ca.ZN_SUMS)
    out[:t.shape[1]] = t.sum(axis=0)
    out[t.shape[1]] = float((~ok).sum())
    return out


# ---- criterion and step ------------------------------------------------------------------------------------------------------
def criterion(model, n, sums):
    """-> (refusing status or 0, crit, gain, offset, zncc) in float64, by the header's formulas"""
    P = _ffi.N_PARAMS[model]
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


def normal_equations(model, n, sums, gain):
    """A [P][P] and b [P] of the header, undamped"""
    P = _ffi.N_PARAMS[model]
    H, HH, HF, HG, _, _ = layout(P)
    N = float(n)
    s = np.asarray(sums, np.float64)
    SH = s[H:H + P]
    M = np.zeros((P, P))
    iu = np.triu_indices(P)
    M[iu] = s[HH:HF]
    M = M + np.triu(M, 1).T
    A = gain * gain * (M - np.outer(SH, SH) / N) / N
    b = gain * ((s[HF:HF + P] - SH * s[0] / N) - gain * (s[HG:HG + P] - SH * s[1] / N)) / N
    return A, b


def step(model, n, sums, lam):
    """float64 restatement of lk_znssd_step_from_sums -> (status, delta [6], crit, gain, offset, zncc, scaled), scaled =
    delta sqrt(diag A), the unknowns of the unit-diagonal system (zeros unless status is 0).  The status comes from the
    pivots of the unpivoted L D L^T of the scaled, damped matrix; the solution from numpy's solver on the same matrix."""
    P = _ffi.N_PARAMS[model]
    delta, scaled = np.zeros(6), np.zeros(6)
    refused, crit, gain, offset, zncc = criterion(model, n, sums)
    if refused:
        return refused, delta, crit, gain, offset, zncc, scaled
    A, b = normal_equations(model, n, sums, gain)
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
    scaled[:P] = y
    delta[:P] = y / root
    return 0, delta, crit, gain, offset, zncc, scaled


def weights(model, n):
    P = _ffi.N_PARAMS[model]
    w = np.full(6, max(1.0, np.sqrt(float(n)) / 2.0))
    w[:1 if P == 1 else 2] = 1.0
    w[P:] = 0.0
    return w


def weighted_step(model, n, delta):
    return float((weights(model, n) * np.abs(delta)).max())


# ---- the loop ----------------------------------------------------------------------------------------------------------------
def loop(evaluate, model, n, seed, max_iters=MAX_ITERS, precision=PRECISION, lambda0=LAMBDA0):
    """The header's loop in float64 around evaluate(p float32 [6]) -> ZN_SUMS sums (last used entry: the flagged count).
    seed: float32 [6] at the level of the evaluation.  -> dict(status, p float32 [6], iterations, evaluations, lam,
    last_step, sums, crit, gain, offset, zncc, zncc_seed)."""
    P = _ffi.N_PARAMS[model]
    flagged_at = layout(P)[4]
    p = np.zeros(6, np.float32)
    p[:P] = np.asarray(seed, np.float32)[:P]
    out = dict(status=None, p=p, iterations=0, evaluations=1, lam=float(lambda0), last_step=0.0, sums=np.zeros(ca.ZN_SUMS),
               crit=0.0, gain=0.0, offset=0.0, zncc=0.0, zncc_seed=0.0)
    sums = evaluate(p)
    if sums[flagged_at] != 0:
        out["status"] = ca.ZN_OUT_OF_IMAGE
        return out
    refused, crit, gain, offset, zncc = criterion(model, n, sums)
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
        st, delta = step(model, n, out["sums"], lam)[:2]
        accepted = small_rejected = False
        if st == 0:
            trial = (out["p"].astype(np.float64) + delta).astype(np.float32)
            trial[P:] = 0
            sums = evaluate(trial)
            out["evaluations"] += 1
            if sums[flagged_at] == 0:
                refused, crit, gain, offset, zncc = criterion(model, n, sums)
                accepted = refused == 0 and crit < out["crit"]
                small_rejected = refused == 0 and not accepted and weighted_step(model, n, delta) < precision
        if accepted:
            lam = max(0.1 * lam, 1e-9)
            out.update(p=trial, sums=sums, crit=crit, gain=gain, offset=offset, zncc=zncc, last_step=weighted_step(model, n, delta))
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


def sector_evaluator(oracle, interp, model, und, dfm, xy, cx, cy, sampler=None):
    """evaluate(p) of one sector for loop(): the sums of the oracle's per-sample floats at p"""
    def evaluate(p):
        return sums_of(*sample_floats(oracle, interp, model, und, dfm, xy, cx, cy, p, sampler))
    return evaluate


def sector_lists(oracle):
    """the samples of the test geometry's sectors in the pass's order, and their centres (float32, as the engine commits them)"""
    lists = [rect_rows(*r) for r in RECTS] + [np.asarray(oracle.annular_points(*q), np.float32).reshape(-1, 2) for q in ANNULAR]
    centres = [(np.float32(l[:, 0].astype(np.float64).mean()), np.float32(l[:, 1].astype(np.float64).mean())) for l in lists]
    return lists, centres


def refine_all(oracle, und, dfm, lists, centres, seeds, model=ca.FM_UVUXUYVXVY, interp=ca.IM_BICUBIC, **kw):
    """loop() over the sectors -> list of its dicts"""
    return [loop(sector_evaluator(oracle, interp, model, und, dfm, xy, cx, cy), model, len(xy), seeds[s], **kw)
            for s, (xy, (cx, cy)) in enumerate(zip(lists, centres))]
