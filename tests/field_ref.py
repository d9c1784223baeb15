"""The float64 restatement of lk_field_map / lk_field_from_sums (include/lk_engine.h, field map), shared by
tests/test_field_host.py and tests/test_field_gpu.py.  Plain numpy, brute force over all sectors for every node: no cell
grid, no tiles, no staging; the same weight, sums, fit, status and iteration rules.  The sums are numpy's (pairwise) sums
over ALL sectors with the weight of a non-member set to 0 - another order than the device's, which is what the tolerance
of the comparisons covers."""
import numpy as np

import correlation_amd as ca
from correlation_amd import _ffi
from track_ref import NOISE, is_good

CHANNELS = _ffi.FIELD_CHANNELS            # u, v, ux, uy, vx, vy, exx, eyy, exy, e1, e2, theta, x0, y0, misfit
POSITION = ("u", "v", "x0", "y0", "misfit")   # lengths; the rest are gradients and tensor fields
CHUNK = 1 << 22                           # node x sector pairs formed at a time


def tensor_reference(tensor, g32):
    """g32 float32 [M][4] as stored -> float64 [M][6] = exx, eyy, exy, e1, e2, theta"""
    ux, uy, vx, vy = np.asarray(g32, np.float32).astype(np.float64).T
    if tensor == ca.STRAIN_GREEN_LAGRANGE:
        exx = ux + 0.5 * (ux * ux + vx * vx)
        eyy = vy + 0.5 * (uy * uy + vy * vy)
        exy = 0.5 * (uy + vx) + 0.5 * (ux * uy + vx * vy)
    else:
        exx, eyy, exy = ux, vy, 0.5 * (uy + vx)
    mean, half = (exx + eyy) * 0.5, (exx - eyy) * 0.5
    rad = np.sqrt(half * half + exy * exy)
    return np.stack([exx, eyy, exy, mean + rad, mean - rad, 0.5 * np.arctan2(2.0 * exy, exx - eyy)], 1)


def fit_reference(min_neighbours, n, W, sums, tensor):
    """n [M], W [M], sums [M][11] -> (status [M], plane float64 [M][6] = u0, v0, ux, uy, vx, vy as exact doubles (nan
    without a fit), tensor float64 [M][6] of the float32 gradients, min(Cxx / Sxx, Cyy / Syy) of every window of at least
    min_neighbours members with W > 0 (nan elsewhere)); the header's `fit` paragraph, each operation in its order"""
    n = np.asarray(n).reshape(-1)
    W = np.asarray(W, np.float64).reshape(-1)
    Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv = np.asarray(sums, np.float64).reshape(-1, 11).T
    with np.errstate(all="ignore"):
        Cxx, Cxy, Cyy = Sxx - Sx * Sx / W, Sxy - Sx * Sy / W, Syy - Sy * Sy / W
        Cxu, Cyu, Cxv, Cyv = Sxu - Sx * Su / W, Syu - Sy * Su / W, Sxv - Sx * Sv / W, Syv - Sy * Sv / W
        CC = Cxx * Cyy
        D = CC - Cxy * Cxy
        ux, uy = (Cyy * Cxu - Cxy * Cyu) / D, (Cxx * Cyu - Cxy * Cxu) / D
        vx, vy = (Cyy * Cxv - Cxy * Cyv) / D, (Cxx * Cyv - Cxy * Cxv) / D
        u0 = Su / W - ux * (Sx / W) - uy * (Sy / W)
        v0 = Sv / W - vx * (Sx / W) - vy * (Sy / W)
        degenerate = ~(W > 0) | (CC == 0) | ~(Cxx > NOISE * Sxx) | ~(Cyy > NOISE * Syy) | ~(D > 1e-6 * CC)
        spread = np.minimum(np.where(Sxx > 0, Cxx / Sxx, 0.0), np.where(Syy > 0, Cyy / Syy, 0.0))
    few = n < min_neighbours
    status = np.where(few, ca.FIELD_TOO_FEW, np.where(degenerate, ca.FIELD_DEGENERATE, ca.FIELD_OK)).astype(np.uint8)
    spread = np.where(few | ~(W > 0), np.nan, spread)
    ok = status == ca.FIELD_OK
    plane = np.stack([u0, v0, ux, uy, vx, vy], 1)
    plane[~ok] = np.nan
    tens = np.full((len(n), 6), np.nan)
    if ok.any():
        tens[ok] = tensor_reference(tensor, plane[ok, 2:].astype(np.float32))
    return status, plane, tens, spread


def window_sums(c, good, u, v, P, r, weight, reverse=False):
    """positions P [M][2] -> (n [M], W [M], sums [M][11], the smallest | |c - P| - r | over the good sectors)"""
    sel = slice(None, None, -1) if reverse else slice(None)
    c, good, u, v = c[sel], good[sel], u[sel], v[sel]
    dx, dy = c[None, :, 0] - P[:, 0, None], c[None, :, 1] - P[:, 1, None]
    d2 = dx * dx + dy * dy
    r2 = r * r
    near = good[None, :] & (d2 <= r2)
    margin = float(np.abs(np.sqrt(d2[:, good]) - r).min()) if good.any() and len(P) else np.inf
    if weight == ca.FIELD_BISQUARE:
        t = 1.0 - d2 / r2
        w = np.where(near, t * t, 0.0)
    else:
        w = near.astype(np.float64)
    uu, vv = np.where(near, u[None, :], 0.0), np.where(near, v[None, :], 0.0)
    wx, wy = w * dx, w * dy
    sums = np.stack([wx.sum(1), wy.sum(1), (wx * dx).sum(1), (wx * dy).sum(1), (wy * dy).sum(1), (w * uu).sum(1),
                     (wx * uu).sum(1), (wy * uu).sum(1), (w * vv).sum(1), (wx * vv).sum(1), (wy * vv).sum(1)], 1)
    return near.sum(1).astype(np.int32), w.sum(1), sums, margin


def field_reference(cen, rec, model, radius, window, stride=1, weight=ca.FIELD_UNIFORM, frame=ca.FIELD_REFERENCE,
                    iterations=4, chi_max=0.0, min_neighbours=3, tensor=ca.STRAIN_GREEN_LAGRANGE, reverse=False):
    """window = (x0, y0, nx, ny) -> dict: every channel of CHANNELS as float64 [ny][nx] (nan without a fit; the plane's six
    as exact doubles, the tensor that of the float32 gradients), "neighbours" int32, "status" uint8, "margin" (the smallest
    | |c - X_k| - r | tested), "spread" [ny][nx] (min(Cxx / Sxx, Cyy / Syy) of the last window fitted or found
    DEGENERATE, nan elsewhere).  reverse: the sectors summed in the opposite order."""
    x0, y0, nx, ny = window
    c = np.asarray(cen, np.float32).astype(np.float64)
    r = np.float64(np.float32(radius))
    good = is_good(rec, _ffi.N_PARAMS[model], chi_max)
    with np.errstate(invalid="ignore"):
        u = rec["p"][:, 0].astype(np.float64)
        v = rec["p"][:, 1].astype(np.float64) if model != ca.FM_U else np.zeros(len(c))
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    nodes = np.stack([x0 + ii.ravel() * stride, y0 + jj.ravel() * stride], 1).astype(np.float64)
    M = len(nodes)
    vals = np.full((M, 15), np.nan)
    nbrs, status, spread = np.zeros(M, np.int32), np.zeros(M, np.uint8), np.full(M, np.nan)
    margin = np.inf
    fits = iterations + 1 if frame == ca.FIELD_DEFORMED else 1
    step = max(1, CHUNK // max(len(c), 1))
    for b in range(0, M, step):
        node = nodes[b:b + step]
        P = node.copy()
        active = np.arange(len(node))
        for k in range(fits):
            n, W, sums, m = window_sums(c, good, u, v, P[active], r, weight, reverse)
            margin = min(margin, m)
            st, plane, tens, spr = fit_reference(min_neighbours, n, W, sums, tensor)
            nbrs[b + active], status[b + active], spread[b + active] = n, st, spr
            ok = st == ca.FIELD_OK
            if k + 1 == fits:
                a = active[ok]
                vals[b + a, :6], vals[b + a, 6:12] = plane[ok], tens[ok]
                vals[b + a, 12:14] = P[a]
                e = (P[a] + plane[ok, :2]) - node[a]
                vals[b + a, 14] = np.hypot(e[:, 0], e[:, 1]) if frame == ca.FIELD_DEFORMED else 0.0
            else:
                active = active[ok]
                P[active] = node[active] - plane[ok, :2]
    out = {k: vals[:, i].reshape(ny, nx) for i, k in enumerate(CHANNELS)}
    out.update(neighbours=nbrs.reshape(ny, nx), status=status.reshape(ny, nx), margin=margin, spread=spread.reshape(ny, nx))
    return out


def clear_of_the_noise_threshold(spread):
    """tests/test_track_gpu.py's condition on the inputs for the DEGENERATE rule's noise guard: every window is either a
    row of centres seen from beyond the hull (below 2^-46) or spread over at least a pitch (above 2^-20), so that the order
    of the sums cannot move a window across 2^-40."""
    s = spread[np.isfinite(spread)]
    return not ((s > 2.0 ** -46) & (s < 2.0 ** -20)).any()


def linear_weights(cen, good, X, Y, radius, weight):
    """The fit is linear in the data: u0 = sum_j l_j u_j over the window's members.  -> (member indices, l [n]) from the
    weighted normal equations of the plane about (X, Y), in float64."""
    c = np.asarray(cen, np.float32).astype(np.float64)
    r = np.float64(np.float32(radius))
    dx, dy = c[:, 0] - X, c[:, 1] - Y
    d2 = dx * dx + dy * dy
    idx = np.flatnonzero(good & (d2 <= r * r))
    w = (1.0 - d2[idx] / (r * r)) ** 2 if weight == ca.FIELD_BISQUARE else np.ones(len(idx))
    A = np.stack([np.ones(len(idx)), dx[idx], dy[idx]], 1)
    N = A.T @ (w[:, None] * A)
    return idx, np.linalg.solve(N, (w[:, None] * A).T)[0]
