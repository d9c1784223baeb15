"""The float64 restatement of lk_track_points / lk_track_step (include/lk_engine.h, material-point tracks), shared by
tests/test_track_host.py and tests/test_track_gpu.py.  Plain numpy, brute force over all sectors: no cell grid, no lanes."""
import numpy as np

import correlation_amd as ca
from correlation_amd import _ffi

FLOATS = ("x", "y", "u", "v", "ux", "uy", "vx", "vy", "exx", "eyy", "exy", "e1", "e2", "theta")
POSITION, GRADIENT = FLOATS[:4], FLOATS[4:]
NOISE = 2.0 ** -40        # a centred moment below this share of its raw sum is rounding, not spread (the header's DEGENERATE rule)


def is_good(rec, n_params, chi_max):
    ok = (rec["error_code"] == 0) & np.isfinite(rec["chi"]) & np.isfinite(rec["p"][..., :n_params]).all(axis=-1)
    if chi_max > 0:
        with np.errstate(invalid="ignore"):
            ok &= rec["chi"] <= np.float32(chi_max)
    return ok


def tensor_reference(tensor, g32):
    ux, uy, vx, vy = np.asarray(g32, np.float32).astype(np.float64)
    if tensor == ca.STRAIN_GREEN_LAGRANGE:
        exx = ux + 0.5 * (ux * ux + vx * vx)
        eyy = vy + 0.5 * (uy * uy + vy * vy)
        exy = 0.5 * (uy + vx) + 0.5 * (ux * uy + vx * vy)
    else:
        exx, eyy, exy = ux, vy, 0.5 * (uy + vx)
    rad = np.sqrt(((exx - eyy) / 2) ** 2 + exy ** 2)
    return [exx, eyy, exy, (exx + eyy) / 2 + rad, (exx + eyy) / 2 - rad, 0.5 * np.arctan2(2 * exy, exx - eyy)]


def step_reference(mode, min_neighbours, n, sums, state, tensor):
    """-> (float64 [14] in FLOATS' order, neighbours, status, new state [8]); the header's `step` and `status` paragraphs"""
    return step_reference_with_spread(mode, min_neighbours, n, sums, state, tensor)[:4]


def step_reference_with_spread(mode, min_neighbours, n, sums, state, tensor):
    """step_reference, and fifth the smaller of Cxx / Sxx and Cyy / Syy of a window that was fitted or found DEGENERATE
    (nan otherwise): how far the window is from the noise threshold of the DEGENERATE rule"""
    st = np.array(state, np.float64)
    X, Y = st[0], st[1]
    status = ca.TRACK_OK
    D, spread = None, np.nan
    if not (np.isfinite(X) and np.isfinite(Y)):
        status = ca.TRACK_BAD_POINT
    elif mode == ca.TRACK_INCREMENTAL and not np.isfinite(st[2:]).all():
        status = ca.TRACK_LOST
    elif n < min_neighbours:
        status = ca.TRACK_TOO_FEW
    else:
        Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv = [np.float64(t) for t in sums]
        Cxx, Cxy, Cyy = Sxx - Sx * Sx / n, Sxy - Sx * Sy / n, Syy - Sy * Sy / n
        Cxu, Cyu, Cxv, Cyv = Sxu - Sx * Su / n, Syu - Sy * Su / n, Sxv - Sx * Sv / n, Syv - Sy * Sv / n
        D = Cxx * Cyy - Cxy * Cxy
        with np.errstate(invalid="ignore", divide="ignore"):
            spread = min(np.float64(Cxx) / Sxx if Sxx > 0 else 0.0, np.float64(Cyy) / Syy if Syy > 0 else 0.0)
        if Cxx * Cyy == 0 or not Cxx > NOISE * Sxx or not Cyy > NOISE * Syy or not D > 1e-6 * (Cxx * Cyy):
            status = ca.TRACK_DEGENERATE
    if status != ca.TRACK_OK:
        st[2:] = np.nan
        return np.zeros(14), 0 if status in (ca.TRACK_BAD_POINT, ca.TRACK_LOST) else n, status, st, spread
    gux, guy = (Cyy * Cxu - Cxy * Cyu) / D, (Cxx * Cyu - Cxy * Cxu) / D
    gvx, gvy = (Cyy * Cxv - Cxy * Cyv) / D, (Cxx * Cyv - Cxy * Cxv) / D
    du, dv = Su / n - gux * (Sx / n) - guy * (Sy / n), Sv / n - gvx * (Sx / n) - gvy * (Sy / n)
    G = np.float64([[1 + gux, guy], [gvx, 1 + gvy]])
    if mode == ca.TRACK_INCREMENTAL:
        x, y = st[2] + du, st[3] + dv
        P = st[4:].reshape(2, 2)
        F = np.float64([[G[0, 0] * P[0, 0] + G[0, 1] * P[1, 0], G[0, 0] * P[0, 1] + G[0, 1] * P[1, 1]],
                        [G[1, 0] * P[0, 0] + G[1, 1] * P[1, 0], G[1, 0] * P[0, 1] + G[1, 1] * P[1, 1]]])
    else:
        x, y, F = X + du, Y + dv, G
    st[2:] = [x, y, F[0, 0], F[0, 1], F[1, 0], F[1, 1]]
    g32 = np.float32([F[0, 0] - 1, F[0, 1], F[1, 0], F[1, 1] - 1])
    vals = [x, y, x - X, y - Y] + [float(t) for t in g32.astype(np.float64)] + tensor_reference(tensor, g32)
    # (the gradient fields are compared as the exact doubles, the tensor is that of the floats as stored)
    vals[4:8] = [F[0, 0] - 1, F[0, 1], F[1, 0], F[1, 1] - 1]
    return np.float64(vals), n, status, st, spread


def fresh_state(points):
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 2)
    st = np.zeros((len(p), 8))
    st[:, 0], st[:, 1], st[:, 2], st[:, 3], st[:, 4], st[:, 7] = p[:, 0], p[:, 1], p[:, 0], p[:, 1], 1.0, 1.0
    return st


def track_reference(cen, records, model, state, radius, chi_max=0.0, min_neighbours=3, tensor=ca.STRAIN_GREEN_LAGRANGE,
                    mode=ca.TRACK_TOTAL):
    """records [F][S], state [Q][8] (fresh_state(points) to start) -> (vals float64 [F][Q][14], neighbours [F][Q], status
    [F][Q], the state after the last frame, the smallest |distance - radius| of any (frame, point, sector) that was tested,
    min(Cxx / Sxx, Cyy / Syy) of every window of at least min_neighbours sectors [F][Q], nan elsewhere)"""
    records = np.asarray(records).reshape(-1, len(cen))
    F, Q = len(records), len(state)
    c = np.asarray(cen, np.float32).astype(np.float64)
    r = np.float64(np.float32(radius))
    state = np.array(state, np.float64)
    vals, nbrs, status = np.zeros((F, Q, 14)), np.zeros((F, Q), np.int32), np.zeros((F, Q), np.int32)
    margin, spread = np.inf, np.full((F, Q), np.nan)
    for f in range(F):
        rec = records[f]
        good = is_good(rec, _ffi.N_PARAMS[model], chi_max)
        with np.errstate(invalid="ignore"):
            u = rec["p"][:, 0].astype(np.float64)
            v = rec["p"][:, 1].astype(np.float64) if model != ca.FM_U else np.zeros(len(c))
        for q in range(Q):
            st = state[q]
            px, py = (st[2], st[3]) if mode == ca.TRACK_INCREMENTAL else (st[0], st[1])
            n, sums = 0, np.zeros(11)
            if np.isfinite(px) and np.isfinite(py) and np.isfinite(st[:2]).all():
                dx, dy = c[:, 0] - px, c[:, 1] - py
                d2 = dx * dx + dy * dy
                if good.any():
                    margin = min(margin, float(np.abs(np.sqrt(d2[good]) - r).min()))
                near = good & (d2 <= r * r)
                n = int(near.sum())
                x, y, uu, vv = dx[near], dy[near], u[near], v[near]
                sums = np.float64([x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum(), uu.sum(), (x * uu).sum(),
                                   (y * uu).sum(), vv.sum(), (x * vv).sum(), (y * vv).sum()])
            vals[f, q], nbrs[f, q], status[f, q], state[q], spread[f, q] = step_reference_with_spread(mode, min_neighbours, n, sums,
                                                                                                    st, tensor)
    return vals, nbrs, status, state, margin, spread
