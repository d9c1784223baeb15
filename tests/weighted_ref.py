"""Restatements behind the weighted refinement tests (include/lk_engine.h: lk_refine_weighted, lk_weight_window,
lk_weighted_step_from_sums): the window function in float32 with an exact fused multiply-add, the weights of a sector's
samples, the prologue's sums, the weighted sums of an evaluation from znssd_ref's per-sample terms, the criterion and the
damped step with N = sum w, the loop (znssd_ref.loop with n_valid and N in the criterion and the step and n_L in the
convergence weights), the edge pair, the geometries and the bounds measured with the restatement alone.  Shared by
test_weighted_host.py and test_weighted_gpu.py."""
import functools

import numpy as np

import correlation_amd as ca
from correlation_amd import _ffi, speckle

import quadratic_ref as qr
import znssd_ref as zr

LOG2E = 1.4426950408889634     # log2(e), the double the host forms inv from
CUT = np.float32(126.0)        # t at and above which the window is 0
# (-ln 2)^j / j!, j = 0 .. 7: the Taylor polynomial of exp(-x ln 2) = 2^-x; the kernel holds the floats nearest these doubles
COEF = [1.0, -0.6931471805599453, 0.2402265069591007, -0.05550410866482158, 0.009618129107628477, -0.0013333558146428443,
        0.00015403530393381608, -1.5252733804059841e-05]
FLAT, MIN_PIVOT, LAMBDA0, PRECISION, MAX_ITERS = zr.FLAT, zr.MIN_PIVOT, zr.LAMBDA0, zr.PRECISION, zr.MAX_ITERS

# ---- bounds measured with this restatement alone, on the CPU ---------------------------------------------------------------
# python -m pytest tests/test_weighted_host.py -s -k "edge or gaussian or border" prints them and pins them (DESIGN.md section
# 26).  The loop runs in float64 around the oracle's own float bicubic sampler, six parameters.
# EDGE_MASKED: the largest |(u, v) - analytic map at the committed centre| over the eight edge sectors under the mask, from
# the zero-gradient seed.  EDGE_UNMASKED: the mean over the same sectors of max(|u - analytic|, |v - analytic|) without a mask
# (znssd_ref.loop).  BORDER: the same figure as EDGE_MASKED for the border sector under its mask.
# GAUSS[side]: the mean over the 25 squares of that side of max(|u - truth|, |v - truth|) with sigma = side / 6, from the seed at
# the true translation - the figure quadratic_ref.AFFINE_BIAS[side] is for unit weights.
# The GPU tests allow 1.5 times EDGE_MASKED and GAUSS - znssd_ref's margin for the float sampling of the device against the
# float64 loop around the same float samples.
EDGE_MASKED = 0.0265           # measured 0.026385 px (mean 0.011039)
EDGE_UNMASKED = 0.2218         # measured 0.221834 px: 8.4 times EDGE_MASKED
BORDER = 0.0074                # measured 0.007273 px
GAUSS = {31: 0.0280, 49: 0.0628}   # measured 0.027967, 0.062692 px: 0.37 and 0.36 of AFFINE_BIAS (0.0747, 0.1764)

# ---- the edge pair and its sectors --------------------------------------------------------------------------------------------
TRUTH = zr.TRUTH
EDGE_X, EDGE_SWITCH = 128, 129     # left of EDGE_X the moving pair; the deformed frame is the static one from EDGE_SWITCH on
EDGE_KEEP = 124                    # the mask keeps x <= EDGE_KEEP
EDGE_SIDE = 31
EDGE_CENTRES = [(120, y) for y in range(30, 206, 25)]
EDGE_RECTS = [qr.square(x, y, EDGE_SIDE) for x, y in EDGE_CENTRES]
# a 31 x 31 sector of znssd_ref's pair that reaches column 253: with u = 1.3 its warped samples leave the bicubic's reach
BORDER_RECT = (223, 100, 253, 130)
BORDER_CUT = 250                   # the mask zeroes x >= BORDER_CUT


@functools.lru_cache(maxsize=None)
def _edge_pair():
    mu, md = speckle.speckle_pair(256, 256, p=TRUTH, seed=5)
    su, sd = speckle.speckle_pair(256, 256, p=(0.0,) * 6, seed=11)
    x = np.arange(256)[None, :]
    und = np.where(x < EDGE_X, mu, su).astype(np.uint8)
    dfm = np.where(x < EDGE_SWITCH, md, sd).astype(np.uint8)
    und.setflags(write=False)
    dfm.setflags(write=False)
    return und, dfm


def edge_pair():
    """(undeformed, deformed) u8 [256][256]: znssd_ref's moving pair left of x = 128, a static speckle right of it"""
    return _edge_pair()


def column_mask(keep_below, shape=(256, 256)):
    """uint8 [rows][cols]: 1 for x < keep_below"""
    m = np.zeros(shape, np.uint8)
    m[:, :keep_below] = 1
    return m


# ---- the window -----------------------------------------------------------------------------------------------------------------
def inv_of(sigma, level=0):
    """the float32 the host forms from a float32 sigma: log2(e) / (2 sigma_L^2) in double, rounded once"""
    s = float(np.float32(sigma)) * 2.0 ** -level
    return np.float32(LOG2E / (2.0 * s * s))


def fma32(a, b, c):
    """fmaf on float32 arrays: a b + c rounded once.  The product is exact in float64; the sum is rounded to odd there (the
    two-sum's error says on which side the exact value lies), which makes the second rounding, to float32, the only one."""
    a, b, c = (np.asarray(t, np.float32).astype(np.float64) for t in (a, b, c))
    p = a * b
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    fix = (err != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def window32(inv, dx, dy):
    """the header's window, operation by operation, on float32 arrays -> float32"""
    inv = np.float32(inv)
    dx, dy = np.atleast_1d(np.asarray(dx, np.float32)), np.atleast_1d(np.asarray(dy, np.float32))
    r2 = fma32(dy, dy, dx * dx)
    t = r2 * inv
    assert t.dtype == np.float32
    live = t < CUT
    ts = np.where(live, t, np.float32(0.0))
    k = (ts + np.float32(0.5)).astype(np.int32)
    x = ts - k.astype(np.float32)
    v = np.full(x.shape, np.float32(COEF[7]), np.float32)
    for j in range(6, -1, -1):
        v = fma32(v, x, np.full(x.shape, np.float32(COEF[j]), np.float32))
    out = np.ldexp(v, -k).astype(np.float32)
    return np.where(live, out, np.float32(0.0))


def window64(sigma, dx, dy):
    """exp(-r^2 / (2 sigma^2)) in float64 from the float32 offsets"""
    dx, dy = np.asarray(dx, np.float32).astype(np.float64), np.asarray(dy, np.float32).astype(np.float64)
    return np.exp(-(dx * dx + dy * dy) / (2.0 * float(sigma) ** 2))


def sample_weights(xy, cx, cy, inv=0.0, mask=None):
    """w float32 [n] of a sector's samples: the mask byte at the undeformed node times the window about (cx, cy)"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    w = np.ones(len(xy), np.float32)
    if inv > 0:
        w = window32(inv, xy[:, 0] - np.float32(cx), xy[:, 1] - np.float32(cy))
    if mask is not None:
        node = (xy + np.float32(0.5)).astype(np.int32)
        w = np.where(mask[node[:, 1], node[:, 0]] != 0, w, np.float32(0.0))
    return w.astype(np.float32)


def group_of(n0):
    """the lane group of a sector with n0 level-0 samples (lk_bw_group)"""
    return 16 if n0 <= 512 else 64 if n0 <= 8192 else 512


def device_sum(values, group):
    """The float64 sum of a sector's per-sample values in the order of the pass's reduction: lane j of the group adds the
    samples j, j + G, ... in turn; a balanced tree over the 16 lanes of a row (pairs, quads, halves, the row); the four rows
    of a wavefront as (r0 + r1) + (r2 + r3); the wavefronts of a 512-lane group one after the other.  The additions commute,
    so this is the value every lane ends with, bit for bit."""
    v = np.asarray(values, np.float64)
    lanes = np.zeros(group)
    for j in range(group):
        acc = 0.0
        for t in v[j::group]:
            acc = acc + t
        lanes[j] = acc
    rows = lanes.reshape(-1, 16)
    for _ in range(4):   # 16 -> 8 -> 4 -> 2 -> 1, neighbours added
        rows = rows.reshape(len(rows), -1, 2)
        rows = rows[:, :, 0] + rows[:, :, 1]
    rows = rows.reshape(-1)
    if group == 16:
        return float(rows[0])
    waves = [(r[0] + r[1]) + (r[2] + r[3]) for r in rows.reshape(-1, 4)]
    total = waves[0]
    for t in waves[1:]:
        total = total + t
    return float(total)


def prologue(xy, cx, cy, w, level=0):
    """-> dict(n_valid, sw, sww, n_eff, centroid (dx, dy) in level-0 pixels) in float64, numpy's order of additions"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    wd = np.asarray(w, np.float32).astype(np.float64)
    dx = (xy[:, 0] - np.float32(cx)).astype(np.float64)
    dy = (xy[:, 1] - np.float32(cy)).astype(np.float64)
    sw, sww = wd.sum(), (wd * wd).sum()
    scale = float(1 << level)
    return dict(n_valid=int((wd > 0).sum()), sw=sw, sww=sww, n_eff=sw * sw / sww if sw > 0 else 0.0,
                centroid=((wd * dx).sum() / sw * scale, (wd * dy).sum() / sw * scale) if sw > 0 else (0.0, 0.0))


# ---- the weighted sums ----------------------------------------------------------------------------------------------------------
def weighted_terms(f, g, H, w):
    """znssd_ref.sum_terms times (double)w, a rounded product, [n][5 + 3 P + NA] float64"""
    return zr.sum_terms(f, g, H) * np.asarray(w, np.float32).astype(np.float64)[:, None]


def sums_of(f, g, H, bad, w):
    """ZN_SUMS doubles of one weighted evaluation in numpy's order: the samples of weight 0 take no part - they are neither
    added nor flagged - and the flagged ones of the others are left out and counted"""
    live = np.asarray(w) > 0
    ok = live & ~np.asarray(bad, bool)
    t = weighted_terms(f[ok], g[ok], H[ok], w[ok])
    out = np.zeros(ca.ZN_SUMS)
    out[:t.shape[1]] = t.sum(axis=0)
    out[t.shape[1]] = float((live & ~ok).sum())
    return out


# ---- criterion and step with N = sum w ------------------------------------------------------------------------------------------
# znssd_ref's criterion, step and loop take the sample count alone, so the three are restated here with (n_valid, N) in its
# place and nothing else changed: they must track znssd_ref.  test_weighted_host.py ties the exported steps to each other at
# N = n bit for bit; test_restatements_agree_at_unit_weights there ties these copies to znssd_ref's.
def criterion(model, n_valid, N, sums):
    """znssd_ref.criterion with n_valid in the too-few test and N for float(n)"""
    P = _ffi.N_PARAMS[model]
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


def step(model, n_valid, N, sums, lam):
    """znssd_ref.step with N = sum w -> (status, delta [6], crit, gain, offset, zncc, scaled)"""
    P = _ffi.N_PARAMS[model]
    delta, scaled = np.zeros(6), np.zeros(6)
    refused, crit, gain, offset, zncc = criterion(model, n_valid, N, sums)
    if refused:
        return refused, delta, crit, gain, offset, zncc, scaled
    H, HH, HF, HG, _, _ = zr.layout(P)
    N = float(N)
    s = np.asarray(sums, np.float64)
    SH = s[H:H + P]
    M = np.zeros((P, P))
    M[np.triu_indices(P)] = s[HH:HF]
    M = M + np.triu(M, 1).T
    A = gain * gain * (M - np.outer(SH, SH) / N) / N
    b = gain * ((s[HF:HF + P] - SH * s[0] / N) - gain * (s[HG:HG + P] - SH * s[1] / N)) / N
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


# ---- the loop -------------------------------------------------------------------------------------------------------------------
def loop(evaluate, model, n, n_valid, N, seed, min_fraction=0.0, max_iters=MAX_ITERS, precision=PRECISION, lambda0=LAMBDA0):
    """znssd_ref.loop around evaluate(p float32 [6]) -> the weighted ZN_SUMS sums, with (n_valid, N) in the criterion and the
    step and n, the full count, in the convergence weights; the prologue's refusal comes first.  -> the same dict."""
    P = _ffi.N_PARAMS[model]
    flagged_at = zr.layout(P)[4]
    p = np.zeros(6, np.float32)
    p[:P] = np.asarray(seed, np.float32)[:P]
    out = dict(status=None, p=p, iterations=0, evaluations=0, lam=float(lambda0), last_step=0.0, sums=np.zeros(ca.ZN_SUMS),
               crit=0.0, gain=0.0, offset=0.0, zncc=0.0, zncc_seed=0.0)
    if n_valid < P + 2 or float(n_valid) < float(np.float32(min_fraction)) * float(n):
        out["status"] = ca.ZN_TOO_FEW
        return out
    out["evaluations"] = 1
    sums = evaluate(p)
    if sums[flagged_at] != 0:
        out["status"] = ca.ZN_OUT_OF_IMAGE
        return out
    refused, crit, gain, offset, zncc = criterion(model, n_valid, N, sums)
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
        st, delta = step(model, n_valid, N, out["sums"], lam)[:2]
        accepted = small_rejected = False
        if st == 0:
            trial = (out["p"].astype(np.float64) + delta).astype(np.float32)
            trial[P:] = 0
            sums = evaluate(trial)
            out["evaluations"] += 1
            if sums[flagged_at] == 0:
                refused, crit, gain, offset, zncc = criterion(model, n_valid, N, sums)
                accepted = refused == 0 and crit < out["crit"]
                small_rejected = refused == 0 and not accepted and zr.weighted_step(model, n, delta) < precision
        if accepted:
            lam = max(0.1 * lam, 1e-9)
            out.update(p=trial, sums=sums, crit=crit, gain=gain, offset=offset, zncc=zncc, last_step=zr.weighted_step(model, n, delta))
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


def affine_floats(oracle, und, dfm, xy, cx, cy, p, interp=ca.IM_BICUBIC):
    """f, g [n], H [n][6] float32 and the flags of the six-parameter model, vectorised: quadratic_ref's float32 warp (with
    zero second-order terms the bits of the affine warp) and the solve's own jacobian"""
    p12 = np.zeros(qr.P, np.float32)
    p12[:6] = np.asarray(p, np.float32)[:6]
    f, g, gx, gy, dx, dy, bad = qr.sample_floats(oracle, interp, und, dfm, xy, cx, cy, p12)
    return f, g, qr.affine_H(gx, gy, dx, dy), bad


def refine(oracle, und, dfm, xy, cx, cy, seed, sigma=0.0, mask=None, **kw):
    """loop() of one six-parameter sector at level 0 -> (its dict, the weights, the prologue)"""
    w = sample_weights(xy, cx, cy, inv_of(sigma) if sigma > 0 else 0.0, mask)
    pro = prologue(xy, cx, cy, w)

    def evaluate(p):
        f, g, H, bad = affine_floats(oracle, und, dfm, xy, cx, cy, p)
        return sums_of(f, g, H, bad, w)
    return loop(evaluate, ca.FM_UVUXUYVXVY, len(xy), pro["n_valid"], pro["sw"], seed, **kw), w, pro
