"""Restatements behind the composed refinement tests (include/lk_engine.h: lk_refine_composed, lk_composed_step_from_sums),
composed from quadratic_ref (the twelve-parameter warp, terms, expansion and loop), weighted_ref (the window, the prologue,
device_sum, the (n_valid, N) loop of the first-order model) and spline_ref (the prefilter and the float64 sampler), which
stay as they are: the weighted 88 sums, the criterion and the step of twelve parameters with N = sum w, the loop around them,
the rim pair, the shifted pairs, and the figures measured with the restatement alone.  Shared by test_composed_host.py and
test_composed_gpu.py."""
import functools

import numpy as np

import correlation_amd as ca
from correlation_amd import speckle

import quadratic_ref as qr
import spline_ref as sr
import weighted_ref as wr
import znssd_ref as zr

P = qr.P
FLAT, MIN_PIVOT, LAMBDA0, PRECISION, MAX_ITERS = zr.FLAT, zr.MIN_PIVOT, zr.LAMBDA0, zr.PRECISION, zr.MAX_ITERS

# ---- figures measured with this restatement alone, on the CPU ---------------------------------------------------------------
# python -m pytest tests/test_composed_host.py -s -k "rim or curve" prints them and pins them.  The
# loops run in float64 around the oracle's own float bicubic sampler, or around spline_ref's float64 sampler of the float32
# coefficient image, from the zero-gradient seed at the true translation.
# RIM_SIDE: the side among quadratic_ref.SIDES at which all eight rim sectors are CONVERGED under (order 2, mask).
# RIM[run] = (largest, mean) over the eight sectors of |(u, v) - quadratic_ref.truth_at| in pixels; the runs: "composed" =
# (order 2, mask), "quadratic" = twelve parameters without a mask, "weighted" = six parameters under the same mask.
# CURVE[shift][sampler] = the mean over the 64 sectors of u - shift of (order 2, sampler, unit weights), sampler 0 (the
# bicubic) or 5.
# The GPU tests allow 1.5 times the pinned figure - the project's margin for a float trajectory against the double
# restatement.
# Measured at the three sides, (largest, mean) of composed / quadratic / weighted, all eight sectors of the composed run
# CONVERGED at every side: 21: (0.040098, 0.015525) / (0.971409, 0.448382; two sectors MAX_ITERS) / (0.158151, 0.037125);
# 31: (0.100231, 0.020783) / (0.809159, 0.307782) / (0.207508, 0.061292); 49: below.  49 is the side of the test: all three runs
# are CONVERGED there and the mask leaves the twelve parameters the most samples.
RIM_SIDE = 49
RIM = {"composed": (0.018829, 0.006273), "quadratic": (1.442292, 0.484037), "weighted": (0.162342, 0.096648)}
CURVE = {0.25: {0: +0.007626, 5: +0.000686}, 0.75: {0: -0.004883, 5: +0.002404}}

# ---- the rim pair and its sectors ---------------------------------------------------------------------------------------------
RIM_X, RIM_SWITCH = wr.EDGE_X, wr.EDGE_SWITCH   # left of RIM_X the curved pair; the deformed frame is the static one from RIM_SWITCH on
RIM_KEEP = wr.EDGE_KEEP                         # the mask keeps x <= RIM_KEEP
RIM_CENTRES = wr.EDGE_CENTRES                   # eight sectors centred on x = 120


def rim_rects(side):
    return [qr.square(x, y, side) for x, y in RIM_CENTRES]


@functools.lru_cache(maxsize=None)
def _rim_pair():
    mu, md = qr.pair()
    su, sd = speckle.speckle_pair(256, 256, p=(0.0,) * 6, seed=11)
    x = np.arange(256)[None, :]
    und = np.where(x < RIM_X, mu, su).astype(np.uint8)
    dfm = np.where(x < RIM_SWITCH, md, sd).astype(np.uint8)
    und.setflags(write=False)
    dfm.setflags(write=False)
    return und, dfm


def rim_pair():
    """(undeformed, deformed) u8 [256][256]: quadratic_ref's curved pair left of x = 128, a static speckle right of it"""
    return _rim_pair()


def rim_mask():
    return wr.column_mask(RIM_KEEP + 1)


# ---- the shifted pairs (the S-curve of the bicubic) ------------------------------------------------------------------------------
CURVE_SIDE, CURVE_GRID, CURVE_SIZE = 21, 8, 192
CURVE_RECTS = [(12 + CURVE_SIDE * i, 12 + CURVE_SIDE * j, 12 + CURVE_SIDE * i + CURVE_SIDE - 1, 12 + CURVE_SIDE * j + CURVE_SIDE - 1)
               for j in range(CURVE_GRID) for i in range(CURVE_GRID)]
CURVE_SHIFTS = (0.25, 0.75)


@functools.lru_cache(maxsize=None)
def shifted_pair(s):
    """(undeformed, deformed) u8 [192][192]: one speckle rendered at its blobs and at the blobs moved by (s, 0.3)"""
    xs, ys, amps = speckle.blobs(CURVE_SIZE, CURVE_SIZE, 7)
    und = speckle._render(CURVE_SIZE, CURVE_SIZE, xs, ys, amps, 2.5)
    dfm = speckle._render(CURVE_SIZE, CURVE_SIZE, xs + np.float32(s), ys + np.float32(0.3), amps, 2.5)
    return np.asarray(und), np.asarray(dfm)


def curve_seeds(s, n=len(CURVE_RECTS)):
    g = np.zeros((n, 6), np.float32)
    g[:, 0], g[:, 1] = s + 0.2, 0.1
    return g


# ---- the samplers -----------------------------------------------------------------------------------------------------------------
def spline_sampler64(dfm, order):
    """points [n][2] float32 -> [n][4] = W, dW/dx, dW/dy, flag: spline_ref's float64 sampler of the float32 coefficient image,
    rounded to float32; the flag by the pass's validity rule"""
    coef = sr.prefilter(dfm, order)
    rows, cols = coef.shape

    def sampler(pts):
        pts = np.asarray(pts, np.float32).reshape(-1, 2)
        ok = sr.valid(order, pts, rows, cols)
        out = np.zeros((len(pts), 4), np.float32)
        out[~ok, 3] = 1
        if ok.any():
            W, Wx, Wy = sr.sample64(coef, pts[ok], order)
            out[ok, 0], out[ok, 1], out[ok, 2] = W, Wx, Wy
        return out
    return sampler


# ---- the weighted 88 sums -----------------------------------------------------------------------------------------------------------
def weighted_terms(f, g, gx, gy, dx, dy, w):
    """quadratic_ref.sum_terms times (double)w, a rounded product, [n][87] float64"""
    return qr.sum_terms(f, g, gx, gy, dx, dy) * np.asarray(w, np.float32).astype(np.float64)[:, None]


def sums_of(f, g, gx, gy, dx, dy, bad, w):
    """QD_SUMS doubles of one weighted evaluation in numpy's order: the samples of weight 0 take no part - they are neither
    added nor flagged - and the flagged ones of the others are left out and counted, unweighted"""
    live = np.asarray(w) > 0
    ok = live & ~np.asarray(bad, bool)
    out = np.zeros(ca.QD_SUMS)
    out[:qr.FLAGGED] = weighted_terms(f[ok], g[ok], gx[ok], gy[ok], dx[ok], dy[ok], w[ok]).sum(axis=0)
    out[qr.FLAGGED] = float((live & ~ok).sum())
    return out


# ---- criterion and step of twelve parameters with N = sum w ----------------------------------------------------------------------
# quadratic_ref's criterion, step and loop take the sample count alone, so the three are restated here with (n_valid, N) in its
# place and nothing else changed, as weighted_ref does for znssd_ref; test_composed_host.py ties them to quadratic_ref's at N = n.
def criterion(n_valid, N, sums):
    if n_valid < P + 2:
        return ca.ZN_TOO_FEW, 0.0, 0.0, 0.0, 0.0
    N = float(N)
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


def step(n_valid, N, sums, lam):
    """quadratic_ref.step with N = sum w -> (status, delta [12], crit, gain, offset, zncc, scaled)"""
    delta, scaled = np.zeros(P), np.zeros(P)
    refused, crit, gain, offset, zncc = criterion(n_valid, N, sums)
    if refused:
        return refused, delta, crit, gain, offset, zncc, scaled
    A, b = qr.normal_equations(float(N), sums, gain)   # (its N = float(n) is this N)
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


def loop(evaluate, n, n_valid, N, seed, min_fraction=0.0, max_iters=MAX_ITERS, precision=PRECISION, lambda0=LAMBDA0):
    """quadratic_ref.loop around evaluate(p float32 [12]) -> the weighted QD_SUMS sums, with (n_valid, N) in the criterion and
    the step and n, the full count, in the convergence weights; the prologue's refusal comes first.  -> the same dict."""
    p = np.asarray(seed, np.float32).copy()
    out = dict(status=None, p=p, iterations=0, evaluations=0, lam=float(lambda0), last_step=0.0, sums=np.zeros(ca.QD_SUMS),
               crit=0.0, gain=0.0, offset=0.0, zncc=0.0, zncc_seed=0.0)
    if n_valid < P + 2 or float(n_valid) < float(np.float32(min_fraction)) * float(n):
        out["status"] = ca.ZN_TOO_FEW
        return out
    out["evaluations"] = 1
    sums = evaluate(p)
    if sums[qr.FLAGGED] != 0:
        out["status"] = ca.ZN_OUT_OF_IMAGE
        return out
    refused, crit, gain, offset, zncc = criterion(n_valid, N, sums)
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
        st, delta = step(n_valid, N, out["sums"], lam)[:2]
        accepted = small_rejected = False
        if st == 0:
            trial = (out["p"].astype(np.float64) + delta).astype(np.float32)
            sums = evaluate(trial)
            out["evaluations"] += 1
            if sums[qr.FLAGGED] == 0:
                refused, crit, gain, offset, zncc = criterion(n_valid, N, sums)
                accepted = refused == 0 and crit < out["crit"]
                small_rejected = refused == 0 and not accepted and qr.weighted_step(n, delta) < precision
        if accepted:
            lam = max(0.1 * lam, 1e-9)
            out.update(p=trial, sums=sums, crit=crit, gain=gain, offset=offset, zncc=zncc, last_step=qr.weighted_step(n, delta))
            if out["last_step"] < precision:
                out["status"] = ca.ZN_CONVERGED
        elif st == 0 and small_rejected:
            out["status"] = ca.ZN_CONVERGED
        else:
            lam = 10.0 * lam
            if lam >= 1e9:
                out["status"] = ca.ZN_STALLED
        out["lam"] = lam
    return out


def refine(oracle, und, dfm, xy, cx, cy, seed6, sigma=0.0, mask=None, sampler=None, interp=ca.IM_BICUBIC, **kw):
    """loop() of one sector at level 0 under (order 2, sampler, weights), from a six-parameter seed with zero second-order
    terms -> (its dict, the weights, the prologue)"""
    w = wr.sample_weights(xy, cx, cy, wr.inv_of(sigma) if sigma > 0 else 0.0, mask)
    pro = wr.prologue(xy, cx, cy, w)
    seed = np.zeros(P, np.float32)
    seed[:6] = np.asarray(seed6, np.float32)[:6]

    def evaluate(p):
        return sums_of(*qr.sample_floats(oracle, interp, und, dfm, xy, cx, cy, p, sampler), w)
    return loop(evaluate, len(xy), pro["n_valid"], pro["sw"], seed, **kw), w, pro


# ---- the two measurements ---------------------------------------------------------------------------------------------------------
def uv_error(p, truth):
    """|(u, v) - truth| of every sector: [S] float64"""
    d = np.asarray(p, np.float64)[:, :2] - np.asarray(truth, np.float64)[:, :2]
    return np.hypot(d[:, 0], d[:, 1])


def rim_restated(oracle, side):
    """the three runs of the rim test in the restatement -> {run: (statuses, errors [8])}"""
    und, dfm = rim_pair()
    lists, centres = qr.sector_lists(oracle, rim_rects(side), ())
    g, truth = qr.true_translation_seeds(centres)
    mask = rim_mask()
    runs = {"composed": [], "quadratic": [], "weighted": []}
    for xy, (cx, cy), seed in zip(lists, centres, g):
        runs["composed"].append(refine(oracle, und, dfm, xy, cx, cy, seed, mask=mask)[0])
        seed12 = np.zeros(P, np.float32)
        seed12[:6] = seed
        runs["quadratic"].append(qr.loop(qr.sector_evaluator(oracle, ca.IM_BICUBIC, und, dfm, xy, cx, cy), len(xy), seed12))
        runs["weighted"].append(wr.refine(oracle, und, dfm, xy, cx, cy, seed, mask=mask)[0])
    return {k: ([r["status"] for r in v], uv_error([r["p"] for r in v], truth)) for k, v in runs.items()}


def curve_restated(oracle, shift, sampler):
    """(order 2, sampler, unit weights) on the shifted pair in the restatement -> (statuses, u - shift [64])"""
    und, dfm = shifted_pair(shift)
    fn = spline_sampler64(dfm, sampler) if sampler else None
    lists, centres = qr.sector_lists(oracle, CURVE_RECTS, ())
    g = curve_seeds(shift)
    out = [refine(oracle, und, dfm, xy, cx, cy, g[s], sampler=fn)[0] for s, (xy, (cx, cy)) in enumerate(zip(lists, centres))]
    return [r["status"] for r in out], np.array([float(r["p"][0]) for r in out]) - shift
