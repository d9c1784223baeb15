"""Float64 numpy restatement of the epipolar curve (include/lk_engine.h: lk_epipolar_curves), written from the interface's
text on tests/stereo_ref.py's camera, and a brute force of the search along it (lk_search_epipolar) with exact integer sums and
float32 positions operation by operation.  The brute force reads the LIBRARY's tables (curves, other, node, inv_depth, shape):
a last-bit difference in the host's curve cannot turn into another candidate set; the restatement checks the tables themselves.

Tolerances of the table, from rounding alone (e64 = 2^-53).

  A node is q_k = project1(o + z d): the undistortion of c (6 Newton steps), the ray, the projection and the lens of camera 1,
  some 100 operations on numbers of order 1 scaled to pixels of order 256 and displacements below 64: stereo_ref.PIXEL_TOL,
  2e-10 px, bounds the difference between the library's node and the restated one.  A station's `other` is the rounding of a
  point of the chord between two nodes, so library and restatement give the same integer unless the restated real value lies
  within 1e-9 of a half, and the same stations unless an end coordinate lies within 1e-9 of an integer: the test asserts that
  its centres avoid both and then asks |other - restated| <= 0.5 + 1e-9.  inv_depth is rho_k + lambda (rho_{k+1} - rho_k) with
  lambda = (t - a_k) / (a_{k+1} - a_k): an error of 2e-10 px in a_k over a node spacing of >= 1 px moves lambda by < 1e-9 and
  inv_depth by 1e-9 of a node step, which is at most 1 / 16 of a range whose ends differ by less than 2 in ratio on every rig of
  the tests: < 1e-10 relative, from rounding in the nodes alone.  The issue sets 1e-12 relative, and the test asserts that: it
  is not a bound on two independent computations but a statement that the library performs the header's operations in the
  header's order - rho_k, lambda and the interpolation are written here exactly as there, and the library's host file is built
  with -ffp-contract=off (correlation_amd/build.py), so the two sides differ only through the last bits of a_k, which move
  lambda by ~1e-15 on these rigs.  A build that contracts products and sums into fused operations, or another order of
  operations, may miss 1e-12 and stay within the derived 1e-10; no such build has been measured.

  SHAPE_TOL.  A_k is a central difference with h = 1 px of f = (project1 o plane o ray0).  Both sides evaluate the same
  formula, so the finite-difference (truncation) term cancels between them and what is left is rounding: four pixels of
  camera 1, each known to PIXEL_TOL, subtracted and halved - 2e-10 absolute - and one rounding to float, 2^-24 |A| (2^-23 |A|
  asked).  Against the ANALYTIC Jacobian of the plane-induced map (shape_truth, by a central difference with h = 1e-3, whose own
  truncation is 1e-6 of the figure below) the truncation term is h^2 / 6 |f'''|.  f is a homography H (planes map to
  planes) between two lenses.  For a homography x -> (a x + b) / (g x + 1) the third derivative is 6 g^2 (a - b g) / (g x + 1)^4;
  with camera 1 turned by theta about the target at distance Z, g = tan(theta) / f_px = 4.5e-4 / px at 20 degrees (8.8e-4 at
  35), so |f'''| h^2 / 6 = g^2 = 2.1e-7 (7.7e-7).  A lens adds rn (k1 rho^3 + k2 rho^5) with rho = pixel / rn <= 0.9: third derivative
  (6 k1 + 60 k2 rho^2) / rn^2; LENS0: (0.18 + 0.39) / 148^2 = 2.6e-5 per px^2, / 6 = 4.3e-6; LENS1: 0.12 / 150^2 / 6 = 0.9e-6; the
  tangential terms (p = 1e-3: 2 p / rn^2 / 6 ~ 1.5e-8) are below both.  The sum is 5.4e-6 at 20 degrees, taken with every term
  at its largest and at full weight through the chain (|A| <= 1.01); SHAPE_TRUTH_TOL = 1e-5 leaves the cross terms of the
  chain rule (products of second derivatives, each below 2e-4) a factor of two.  It is derived, not measured."""
import numpy as np

import correlation_amd as ca
from correlation_amd import _ffi

import stereo_ref as sr

F32 = np.float32
SHAPE_TOL_ABS = 2e-10
SHAPE_TRUTH_TOL = 1e-5


# ---- the curve, restated ------------------------------------------------------------------------------------------------------
def nodes(rig, c, z_near, z_far, level, n_nodes):
    """-> (w [N][2] level-L displacements, rho [N], P [N][3], ok)"""
    c = np.float64(c)
    m, outside = sr.undistort(rig[0]["lens"], c[None])
    if outside[0]:
        return None, None, None, False
    o, d = sr.rays(rig[0], m)
    d = d[0]
    rho_near, rho_far = 1.0 / z_near, 1.0 / z_far
    step = (rho_far - rho_near) / (n_nodes - 1)
    rho = rho_near + np.arange(n_nodes) * step
    P = o[None] + (1.0 / rho)[:, None] * d[None]
    _, depth = sr.pinhole(rig[1], P)
    if not (depth > 0).all():
        return None, rho, P, False
    q = sr.project(rig[1], P)
    w = (q - c[None]) / (1 << level)
    return w, rho, P, bool(np.isfinite(w).all() and (np.abs(w) < 2.0 ** 30).all())


def over_plane(rig, p, P, nrm):
    """camera-0 pixels p [n][2] -> (camera-1 pixels over the plane nrm . (X - P) = 0, failed [n]).  A point fails where the
    undistortion or the projection refuses it, d . n is 0, z is not > 0 or a value is not finite (the header's list)."""
    m, outside = sr.undistort(rig[0]["lens"], p)
    m = np.where(outside[:, None], 0.0, m)
    o, d = sr.rays(rig[0], m)
    dn = d @ nrm
    with np.errstate(all="ignore"):
        z = ((P - o) @ nrm) / dn
        failed = outside | (dn == 0.0) | ~(z > 0.0)
        X = o + np.where(failed, 1.0, z)[:, None] * d
        behind = ~(sr.pinhole(rig[1], X)[1] > 0.0)
        q = sr.project(rig[1], np.where(behind[:, None], [0.0, 0.0, sr.Z0], X))
    failed = failed | behind | ~np.isfinite(q).all(axis=1)
    return q, failed


def shape_matrices(rig, c, P, normal, h=1.0):
    """[N][4] float64 {a11, a12, a21, a22}: central differences with step h of the plane-induced map at c; None where a
    point fails"""
    nrm = np.float64(normal)
    if not nrm.any():
        nrm = np.float64(rig[0]["R"][2])
    c = np.float64(c)
    pts = c[None] + h * np.float64([[1, 0], [-1, 0], [0, 1], [0, -1]])
    out = np.empty((len(P), 4))
    for k in range(len(P)):
        f, failed = over_plane(rig, pts, P[k], nrm)
        if failed.any():
            return None
        out[k] = ((f[0, 0] - f[1, 0]) / (2 * h), (f[2, 0] - f[3, 0]) / (2 * h), (f[0, 1] - f[1, 1]) / (2 * h), (f[2, 1] - f[3, 1]) / (2 * h))
    return out


def curve(rig, c, z_near, z_far, level, n_nodes=17, band=1, shape=0, normal=(0.0, 0.0, 0.0)):
    """the restated curve of one centre: dict(status, axis, first, count, t [count], other_real [count] (before the rounding),
    node [count], inv_depth [count], w, rho, P, A)"""
    N = n_nodes
    w, rho, P, ok = nodes(rig, c, z_near, z_far, level, N)
    out = dict(status=ca.GS_NO_CURVE, axis=0, first=0, count=0, w=w, rho=rho, P=P, A=None)
    if not ok:
        return out
    axis = 0 if abs(w[-1, 0] - w[0, 0]) >= abs(w[-1, 1] - w[0, 1]) else 1
    a, b = w[:, axis], w[:, 1 - axis]
    up = a[-1] >= a[0]
    if not ((np.diff(a) >= 0).all() if up else (np.diff(a) <= 0).all()):
        return out
    if shape:
        out["A"] = shape_matrices(rig, c, P, normal)
        if out["A"] is None:
            return out
    lo, hi = min(a[0], a[-1]), max(a[0], a[-1])
    t0, t1 = np.ceil(lo), np.floor(hi)
    if t0 > t1:
        t0 = t1 = np.floor((lo + hi) / 2.0 + 0.5)
    out.update(status=ca.GS_TOO_LONG, axis=axis)
    if t1 - t0 + 1 > ca.EP_MAX_STATIONS:
        return out
    ts = np.arange(int(t0), int(t1) + 1)
    order = list(range(N - 1)) if up else list(range(N - 2, -1, -1))   # the segments by increasing a
    other, node, inv = [], [], []
    for t in ts:
        k = next((k for k in order if (a[k + 1] if up else a[k]) >= t), order[-1])
        den = a[k + 1] - a[k]
        lam = 0.0 if den == 0.0 else min(max((t - a[k]) / den, 0.0), 1.0)
        other.append(b[k] + lam * (b[k + 1] - b[k]))
        node.append(k if lam < 0.5 else k + 1)
        inv.append(rho[k] + lam * (rho[k + 1] - rho[k]))
    node = np.int64(node)
    runs = np.diff(np.flatnonzero(np.concatenate([[True], np.diff(node) != 0, [True]])))
    if (runs * (2 * band + 1) > ca.EP_MAX_GROUP).any():
        return out
    out.update(status=0, first=int(t0), count=len(ts), t=ts, other_real=np.float64(other), node=node, inv_depth=np.float64(inv))
    return out


def point_on_ray(rig, c, z):
    """camera 1's pixel of the point of camera 0's ray through c at depth z"""
    m, _ = sr.undistort(rig[0]["lens"], np.float64(c)[None])
    o, d = sr.rays(rig[0], m)
    return sr.project(rig[1], o[None] + z * d)[0]


# ---- the engine's samples -----------------------------------------------------------------------------------------------------
def round_like_host(v):
    """(int)(v + 0.5f) in float32, truncated toward zero"""
    return np.trunc(np.asarray(v, F32) + F32(0.5)).astype(np.int64)


def level_points(e, s, level):
    """a sector's level-L samples as the engine holds them: the explicit list, or the implicit rectangle's decimation"""
    xy = e.level_xy(level, s)
    if len(xy):
        return xy
    pts = np.ascontiguousarray(e.getUndXY0ToCPU(s), F32).reshape(-1, 2)
    for _ in range(level):
        out = np.zeros_like(pts)
        pts = out[:e.lib.lk_roi_decimate(_ffi.fptr(pts), len(pts), 1, _ffi.fptr(out))]
    return pts


# ---- the search, by brute force -----------------------------------------------------------------------------------------------
def positions(x, y, centre0, level, A):
    """where template sample (x, y) reads before the displacement: float32, every product and sum rounded on its own"""
    if A is None:
        return x.astype(np.int64), y.astype(np.int64)
    inv = F32(1.0 / (1 << level))
    Cx, Cy = F32(centre0[0]) * inv, F32(centre0[1]) * inv
    a11, a12, a21, a22 = (F32(v) for v in A)
    dx, dy = x.astype(F32) - Cx, y.astype(F32) - Cy
    rx, ry = a11 * dx + a12 * dy, a21 * dx + a22 * dy
    assert rx.dtype == F32
    return np.floor((Cx + rx) + F32(0.5)).astype(np.int64), np.floor((Cy + ry) + F32(0.5)).astype(np.int64)


def brute_sector(und, dfm, pts, centre0, level, band, cv, table, shape_s, g_in, min_samples=0, min_score=0.0):
    """one sector: -> (match as an EPIPOLAR_MATCH_DTYPE record, profile [n_stations], the guess [6])"""
    n, B = len(pts), band
    m = np.zeros(1, ca.EPIPOLAR_MATCH_DTYPE)[0]
    m["n_samples"], m["score"], m["runner_up"] = n, -2.0, -2.0
    count, first = int(cv["n_stations"]), int(cv["first_index"])
    prof = np.full(count, -2.0)
    g = np.array(g_in, F32)

    def done(status):
        m["status"] = status
        return m, prof, g
    if cv["status"]:
        return done(int(cv["status"]))
    if n > _ffi.GS_MAX_SAMPLES:
        return done(ca.GS_TOO_LARGE)
    if n < (min_samples if min_samples > 0 else 9):
        return done(ca.GS_TOO_FEW)
    x = np.clip(round_like_host(pts[:, 0]), 0, und.shape[1] - 1)
    y = np.clip(round_like_host(pts[:, 1]), 0, und.shape[0] - 1)
    t = und[y, x].astype(np.int64)
    St, Stt = int(t.sum()), int((t * t).sum())
    varT = n * Stt - St * St
    if varT == 0:
        return done(ca.GS_TEXTURELESS)
    other, node = table["other"][first:first + count].astype(np.int64), table["node"][first:first + count]
    H, W = dfm.shape
    D64 = dfm.astype(np.int64)
    cand = []   # (score, m, b)
    for nd in np.unique(node):
        X, Y = positions(x, y, centre0, level, None if shape_s is None else shape_s[nd])
        ms = np.flatnonzero(node == nd)
        mm, bb = np.meshgrid(ms, np.arange(-B, B + 1), indexing="ij")
        mm, bb = mm.ravel(), bb.ravel()
        along, across = int(cv["first_station"]) + mm, other[mm] + bb
        dx, dy = (along, across) if cv["axis"] == 0 else (across, along)
        ok = (X.min() + dx >= 0) & (X.max() + dx <= W - 1) & (Y.min() + dy >= 0) & (Y.max() + dy <= H - 1)
        for q in np.flatnonzero(ok):
            d = D64[Y + dy[q], X + dx[q]]
            Sd, Sdd, Std = int(d.sum()), int((d * d).sum()), int((t * d).sum())
            varD = n * Sdd - Sd * Sd
            if varD > 0:
                cand.append((float(n * Std - St * Sd) / float(np.sqrt(np.float64(varT) * np.float64(varD))), int(mm[q]), int(bb[q])))
    if not cand:
        return done(ca.GS_NO_CANDIDATE)
    for sc, mq, _ in cand:
        prof[mq] = max(prof[mq], sc)
    cand.sort(key=lambda c: (-c[0], abs(c[2]), c[2], c[1]))
    best, mw, bw = cand[0]
    along, across = int(cv["first_station"]) + mw, int(other[mw]) + bw
    dx, dy = (along, across) if cv["axis"] == 0 else (across, along)
    far = prof[np.abs(np.arange(count) - mw) >= 2]
    off = 0.0
    if 0 < mw < count - 1 and prof[mw - 1] > -1.5 and prof[mw + 1] > -1.5:
        sm, sp = prof[mw - 1], prof[mw + 1]
        den = sm - 2.0 * best + sp
        if den < 0.0:
            off = min(max(0.5 * (sm - sp) / den, -0.5), 0.5)
    rho = table["inv_depth"][first + mw]
    if off > 0.0:
        rho = rho + off * (table["inv_depth"][first + mw + 1] - rho)
    elif off < 0.0:
        rho = rho + (0.0 - off) * (table["inv_depth"][first + mw - 1] - rho)
    m["shift_x"], m["shift_y"], m["station"], m["band_offset"], m["node"] = dx, dy, mw, bw, node[mw]
    m["n_valid"], m["score"], m["runner_up"] = len(cand), best, far.max() if len(far) else -2.0
    m["station_refined"], m["inv_depth"] = F32(np.float64(mw) + off), F32(rho)
    m["status"] = ca.GS_OK if best > np.float64(F32(min_score)) else ca.GS_WEAK
    if m["status"] == ca.GS_OK:
        g[0], g[1] = F32(np.float64(dx) * (1 << level)), F32(np.float64(dy) * (1 << level))
        if shape_s is not None:
            A = shape_s[node[mw]]
            g[2:] = (A[0] - F32(1), A[1], A[2], A[3] - F32(1))
    return m, prof, g


def brute_force_arrays(und, dfm, pts_list, cen, cams, guesses_in, level, band, z_near, z_far, n_nodes=17, shape=0, normal=None,
                       depth_range=None, min_samples=0, min_score=0.0):
    """every sector from level-L images, level-L sample lists and level-0 centres: -> (matches [S], profile (concatenated),
    guesses [S][6], the library's table)"""
    S = len(pts_list)
    cen = np.asarray(cen, F32).reshape(S, 2)
    table = ca.epipolar_curves(cams, cen, z_near, z_far, level, band=band, n_nodes=n_nodes, shape=shape, normal=normal,
                               depth_range=depth_range)
    match = np.zeros(S, ca.EPIPOLAR_MATCH_DTYPE)
    prof = np.full(len(table["other"]), -2.0)
    g = np.array(guesses_in, F32).reshape(S, 6).copy()
    for s in range(S):
        cv = table["curves"][s]
        match[s], p, g[s] = brute_sector(und, dfm, pts_list[s], cen[s], level, band, cv, table, table["shape"][s] if shape else None,
                                         g[s], min_samples, min_score)
        prof[cv["first_index"]:cv["first_index"] + cv["n_stations"]] = p
    return match, prof, g, table


def brute_force(e, cams, guesses_in, level, band, z_near, z_far, dfm=None, **kw):
    """the same of engine e's own pyramid levels (dfm: another level-L deformed image, a ring slot's), lists and centres"""
    S = e.n_sectors
    cen = np.array([e.sector_info(s)[1:] for s in range(S)], F32)
    und = e.get_pyramid_level(ca.IMG_UND, level)
    dfm = e.get_pyramid_level(ca.IMG_DEF, level) if dfm is None else dfm
    return brute_force_arrays(und, dfm, [level_points(e, s, level) for s in range(S)], cen, cams, guesses_in, level, band, z_near,
                              z_far, **kw)
