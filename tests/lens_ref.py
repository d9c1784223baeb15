"""A float64 numpy restatement of the lens distortion (include/lk_engine.h: lk_lens_fit, lk_lens_correct): the model D, its
inverse U, the rows of the fit, a frame's sums with sum |term|, the Gauss-Newton step from DENSE normal equations (every
lens and nuisance parameter in one matrix, np.linalg - not the library's Schur complement), the whole fit and the
correction of records.  Shared by tests/test_lens_host.py and tests/test_lens_gpu.py.

Bounds of the comparisons with the device (used by tests/test_lens_gpu.py):
  sums   any two summation orders of n terms differ by at most 2 (n - 1) 2^-53 sum |term| =: eps sum |term| (as
         tests/motion_ref.py); `abs_sums` holds sum |term|.  The count and n_outside are exact.
  lens   Newton's iteration corrects its own earlier errors, so with both fits run to a step below 1e-12 the two results
         differ by what the LAST evaluation's differences do to the root of the gradient, to first order
           d theta = H^-1 dg,   H the dense normal matrix at the result, g its right-hand side,
         where dg_k is at most eps sum |a_k r| from the order of the sums, plus rho sum |a_k| from the rounding of the rows
         themselves: a residual is a difference of positions of at most 256 px that went through fewer than 100 double
         operations each, rho = 100 * 2^-53 * 256 = 2.9e-12 px, every constant rounded up.  With |H^-1| taken entry by entry:
           bound_j = sum_k |H^-1|_jk (2 eps sum |a_k r| + rho sum |a_k|) + 2^-50 |theta_j| + 2e-12 s_j
         (the last two: the additions of the steps to theta, and the steps both fits still had in hand; s = 1, rn)."""
import numpy as np

import correlation_amd as ca
from correlation_amd import _ffi

NEWTON = 6
PARAMS = ("k1", "k2", "p1", "p2", "cx", "cy")
Q_OF = {ca.LENS_TRANSLATION: 2, ca.LENS_SIMILARITY: 4, ca.LENS_AFFINE: 6}
RHO = 100 * 2.0 ** -53 * 256


def make_lens(cx, cy, rn, k1=0.0, k2=0.0, p1=0.0, p2=0.0):
    return dict(cx=float(cx), cy=float(cy), rn=float(rn), k1=float(k1), k2=float(k2), p1=float(p1), p2=float(p2))


def as_record(lens):
    return _ffi.make_lens(*(float(lens[k]) for k in ("cx", "cy", "rn", "k1", "k2", "p1", "p2")))


def as_dict(rec):
    return {k: float(rec[k]) for k in ("cx", "cy", "rn", "k1", "k2", "p1", "p2")}


def d_of(L, rho):
    """d(rho) [n][2] and J = (xx, xy, yy, det)"""
    rx, ry = rho[:, 0], rho[:, 1]
    xx, yy, xy = rx * rx, ry * ry, rx * ry
    r2 = xx + yy
    radial = 1.0 + L["k1"] * r2 + L["k2"] * (r2 * r2)
    g = 2.0 * L["k1"] + 4.0 * L["k2"] * r2
    dx = rx * radial + (2.0 * L["p1"] * xy + L["p2"] * (r2 + 2.0 * xx))
    dy = ry * radial + (L["p1"] * (r2 + 2.0 * yy) + 2.0 * L["p2"] * xy)
    jxx = radial + g * xx + (2.0 * L["p1"] * ry + 6.0 * L["p2"] * rx)
    jxy = g * xy + (2.0 * L["p1"] * rx + 2.0 * L["p2"] * ry)
    jyy = radial + g * yy + (6.0 * L["p1"] * ry + 2.0 * L["p2"] * rx)
    return np.stack([dx, dy], axis=1), (jxx, jxy, jyy, jxx * jyy - jxy * jxy)


def distort(L, xy):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    c = np.float64([L["cx"], L["cy"]])
    d, _ = d_of(L, (xy - c) / L["rn"])
    return c + L["rn"] * d


def undistort_rho(L, q, steps=NEWTON):
    """-> rho_u [n][2], J there, outside [n]"""
    rho = q.copy()
    outside = np.zeros(len(q), bool)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            d, (jxx, jxy, jyy, det) = d_of(L, rho)
            outside |= ~(det > 0)
            e = d - q
            rho = np.stack([rho[:, 0] - (jyy * e[:, 0] - jxy * e[:, 1]) / det, rho[:, 1] - (jxx * e[:, 1] - jxy * e[:, 0]) / det], axis=1)
        _, J = d_of(L, rho)
        outside |= ~(J[3] > 0) | ~np.isfinite(J[3])
    return rho, J, outside


def undistort(L, xy, steps=NEWTON):
    """-> positions [n][2] (the input where outside), outside [n]"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    c = np.float64([L["cx"], L["cy"]])
    rho, _, outside = undistort_rho(L, (xy - c) / L["rn"], steps)
    out = c + L["rn"] * rho
    out[outside] = xy[outside]
    return out, outside


def du_of(L, rho, J):
    """dU / d(k1, k2, p1, p2, cx, cy) [n][6][2], pixels"""
    rx, ry = rho[:, 0], rho[:, 1]
    jxx, jxy, jyy, det = J
    xx, yy, xy = rx * rx, ry * ry, rx * ry
    r2 = xx + yy
    r4 = r2 * r2
    ixx, ixy, iyy = jyy / det, -jxy / det, jxx / det
    rn = L["rn"]
    dDx = [rn * (rx * r2), rn * (rx * r4), rn * (2.0 * xy), rn * (r2 + 2.0 * xx)]
    dDy = [rn * (ry * r2), rn * (ry * r4), rn * (r2 + 2.0 * yy), rn * (2.0 * xy)]
    out = np.zeros((len(rho), 6, 2))
    for j in range(4):
        out[:, j, 0] = -(ixx * dDx[j] + ixy * dDy[j])
        out[:, j, 1] = -(ixy * dDx[j] + iyy * dDy[j])
    out[:, 4, 0], out[:, 4, 1] = 1.0 - ixx, -ixy
    out[:, 5, 0], out[:, 5, 1] = -ixy, 1.0 - iyy
    return out


def grad_n(nuisance, nu):
    if nuisance == ca.LENS_SIMILARITY:
        return np.float64([[nu[2], -nu[3]], [nu[3], nu[2]]])
    if nuisance == ca.LENS_AFFINE:
        return np.float64([[nu[2], nu[3]], [nu[4], nu[5]]])
    return np.zeros((2, 2))


def residuals(L, nuisance, nu, o, X, uv):
    """r [n][2] = U(X + u) - U(X) - N(U(X)), outside [n]"""
    Xu, out_X = undistort(L, X)
    xu, out_x = undistort(L, X + uv)
    e = Xu - o
    return (xu - Xu) - (np.float64(nu[:2]) + e @ grad_n(nuisance, nu).T), out_X | out_x


def rows(L, nuisance, nu, o, X, uv):
    """the two rows of every record: ax, ay [n][W], outside [n] (rows of outside records are not to be used)"""
    Q = Q_OF[nuisance]
    W = 7 + Q
    c = np.float64([L["cx"], L["cy"]])
    RX, A, out_X = undistort_rho(L, (X - c) / L["rn"])
    rx, B, out_x = undistort_rho(L, ((X + uv) - c) / L["rn"])
    Xu, xu = c + L["rn"] * RX, c + L["rn"] * rx
    with np.errstate(all="ignore"):
        dX, dx = du_of(L, RX, A), du_of(L, rx, B)
    G = grad_n(nuisance, nu)
    M = np.eye(2) + G
    e = Xu - o
    ax, ay = np.zeros((len(X), W)), np.zeros((len(X), W))
    for j in range(6):
        ax[:, j] = dx[:, j, 0] - (M[0, 0] * dX[:, j, 0] + M[0, 1] * dX[:, j, 1])
        ay[:, j] = dx[:, j, 1] - (M[1, 0] * dX[:, j, 0] + M[1, 1] * dX[:, j, 1])
    ax[:, 6], ay[:, 7] = -1.0, -1.0
    if Q == 4:
        ax[:, 8], ay[:, 8] = -e[:, 0], -e[:, 1]
        ax[:, 9], ay[:, 9] = e[:, 1], -e[:, 0]
    if Q == 6:
        ax[:, 8], ax[:, 9] = -e[:, 0], -e[:, 1]
        ay[:, 10], ay[:, 11] = -e[:, 0], -e[:, 1]
    ax[:, 6 + Q] = (xu[:, 0] - Xu[:, 0]) - (nu[0] + (G[0, 0] * e[:, 0] + G[0, 1] * e[:, 1]))
    ay[:, 6 + Q] = (xu[:, 1] - Xu[:, 1]) - (nu[1] + (G[1, 0] * e[:, 0] + G[1, 1] * e[:, 1]))
    return ax, ay, out_X | out_x


def triangle(W):
    return [(i, j) for i in range(W) for j in range(i, W)]


def frame_sums(L, nuisance, nu, o, X, uv, member):
    """-> sums [LEN] = {n, the triangle, n_outside}, abs_sums [LEN] (sum |term|), col_abs [W] = sum (|ax_k| + |ay_k|)"""
    W = 7 + Q_OF[nuisance]
    ax, ay, outside = rows(L, nuisance, nu, o, X[member], uv[member])
    ax, ay = ax[~outside], ay[~outside]
    s, a = [float(len(ax))], [float(len(ax))]
    for i, j in triangle(W):
        term = ax[:, i] * ax[:, j] + ay[:, i] * ay[:, j]
        s.append(term.sum())
        a.append(np.abs(term).sum())
    s.append(float(outside.sum()))
    a.append(float(outside.sum()))
    return np.float64(s), np.float64(a), np.abs(ax).sum(axis=0) + np.abs(ay).sum(axis=0)


def matrix_of(s, W):
    m = np.zeros((W, W))
    for k, (i, j) in enumerate(triangle(W)):
        m[i, j] = m[j, i] = s[1 + k]
    return m


def free_index(free):
    return [j for j in range(6) if free & (1 << j if j < 4 else ca.LENS_FREE_CENTRE)]


def dense_system(nuisance, free, min_sectors, sums):
    """the dense normal equations of the used frames: H, g, the frames used, sum |r|^2, the records"""
    Q = Q_OF[nuisance]
    W = 7 + Q
    idx = free_index(free)
    nf = len(idx)
    used = [f for f in range(len(sums)) if int(sums[f][0]) >= min_sectors]
    n = nf + Q * len(used)
    H, g = np.zeros((n, n)), np.zeros(n)
    chi2, records = 0.0, 0
    for k, f in enumerate(used):
        m = matrix_of(sums[f], W)
        cols = idx + list(range(6, 6 + Q))
        where = list(range(nf)) + list(range(nf + Q * k, nf + Q * k + Q))
        H[np.ix_(where, where)] += m[np.ix_(cols, cols)]
        g[where] += m[cols, W - 1]
        chi2 += m[W - 1, W - 1]
        records += int(sums[f][0])
    return H, g, used, chi2, records


def step_from_sums(nuisance, free, rn, min_sectors, sums):
    """one Gauss-Newton step from the dense normal equations -> dict(delta [6], sigma [6], nuisance_delta [F][6], chi2,
    n_records, n_frames_used, scaled_step, degenerate)"""
    Q = Q_OF[nuisance]
    idx = free_index(free)
    nf = len(idx)
    H, g, used, chi2, records = dense_system(nuisance, free, min_sectors, sums)
    out = dict(delta=np.zeros(6), sigma=np.zeros(6), nuisance_delta=np.zeros((len(sums), 6)), chi2=chi2, n_records=records,
               n_frames_used=len(used), scaled_step=0.0, degenerate=False)
    d = np.sqrt(np.abs(np.diag(H)))
    if not used or (np.diag(H) <= 0).any() or np.linalg.eigvalsh(H / np.outer(d, d)).min() < 1e-12:
        out["degenerate"] = True
        return out
    sol = (np.linalg.solve(H / np.outer(d, d), -g / d)) / d
    cov = np.linalg.inv(H / np.outer(d, d)) / np.outer(d, d)
    dof = 2.0 * records - nf - Q * len(used)
    for i, j in enumerate(idx):
        out["delta"][j] = sol[i]
        out["sigma"][j] = np.sqrt(chi2 / dof * cov[i, i]) if dof > 0 else 0.0
        out["scaled_step"] = max(out["scaled_step"], abs(sol[i]) / (1.0 if j < 4 else rn))
    for k, f in enumerate(used):
        out["nuisance_delta"][f, :Q] = sol[nf + Q * k: nf + Q * k + Q]
    return out


def is_good(rec, n_params, chi_max):
    ok = (rec["error_code"] == 0) & np.isfinite(rec["chi"]) & np.isfinite(rec["p"][..., :n_params]).all(axis=-1)
    if chi_max > 0:
        with np.errstate(invalid="ignore"):
            ok &= rec["chi"] <= np.float32(chi_max)
    return ok


def origin_of(cen):
    c = np.asarray(cen, np.float32).astype(np.float64)
    return (c.min(axis=0) + c.max(axis=0)) / 2.0


def all_sums(L, nuisance, nu, cen, rec, model, chi_max=0.0, fit_mask=None):
    """every frame's sums: rec [F][S] -> sums [F][LEN], abs_sums [F][LEN], col_abs [F][W]"""
    X = np.asarray(cen, np.float32).astype(np.float64)
    o = origin_of(cen)
    out = []
    for f in range(len(rec)):
        member = is_good(rec[f], _ffi.N_PARAMS[model], chi_max)
        if fit_mask is not None:
            member &= np.asarray(fit_mask) != 0
        with np.errstate(invalid="ignore"):
            uv = rec[f]["p"][:, :2].astype(np.float64)
        out.append(frame_sums(L, nuisance, nu[f], o, X, uv, member))
    return tuple(np.stack(t) for t in zip(*out))


def fit(init, free, nuisance, cen, rec, model=None, chi_max=0.0, fit_mask=None, min_sectors=None, max_iters=10, tol=1e-8):
    """lk_lens_fit in float64 with the dense step -> dict(lens, nuisance [F][6], sigma [6], rms_before, rms, iterations, last_step, status, n_records, n_outside, sums, abs_sums, col_abs (of the last evaluation))"""
    model = ca.FM_UVUXUYVXVY if model is None else model
    Q = Q_OF[nuisance]
    min_sectors = Q if min_sectors is None else min_sectors
    L = dict(init)
    nu = np.zeros((len(rec), 6))
    status, iterations, last, rms_before = ca.LENS_MAX_ITERS, 0, 0.0, 0.0
    for it in range(max_iters):
        sums, _, _ = all_sums(L, nuisance, nu, cen, rec, model, chi_max, fit_mask)
        if it == 0:      # the rms at init with every frame's nuisance at its best
            W, chi2, records = 7 + Q, 0.0, 0
            for s in sums:
                if int(s[0]) >= min_sectors:
                    m = matrix_of(s, W)
                    chi2 += m[W - 1, W - 1] - m[6:6 + Q, W - 1] @ np.linalg.solve(m[6:6 + Q, 6:6 + Q], m[6:6 + Q, W - 1])
                    records += int(s[0])
            rms_before = np.sqrt(max(chi2, 0.0) / max(records, 1))
        zero = L["k1"] == 0 and L["k2"] == 0 and L["p1"] == 0 and L["p2"] == 0
        now = free & ~ca.LENS_FREE_CENTRE if zero else free
        st = step_from_sums(nuisance, now, L["rn"], min_sectors, sums) if now else dict(degenerate=True)
        if st["degenerate"]:
            status = ca.LENS_DEGENERATE
            break
        for j, k in enumerate(PARAMS):
            L[k] += st["delta"][j]
        nu += st["nuisance_delta"]
        iterations, last = it + 1, st["scaled_step"]
        if last <= tol:
            status = ca.LENS_OK
            break
    sums, abs_sums, col_abs = all_sums(L, nuisance, nu, cen, rec, model, chi_max, fit_mask)
    zero = L["k1"] == 0 and L["k2"] == 0 and L["p1"] == 0 and L["p2"] == 0
    st = step_from_sums(nuisance, (free & ~ca.LENS_FREE_CENTRE if zero else free) or free, L["rn"], min_sectors, sums)
    return dict(lens=L, nuisance=nu, sigma=st["sigma"], rms=np.sqrt(st["chi2"] / max(st["n_records"], 1)), iterations=iterations,
                last_step=last, status=status, rms_before=rms_before, n_records=st["n_records"], n_outside=int(sums[:, -1].sum()), sums=sums,
                abs_sums=abs_sums, col_abs=col_abs, n_frames_used=st["n_frames_used"])


def lens_bound(ref, free, nuisance, min_sectors=None):
    """the docstring's `lens` bound per parameter [6] (0 for held ones), at the result `ref` of fit()"""
    Q = Q_OF[nuisance]
    W = 7 + Q
    min_sectors = Q if min_sectors is None else min_sectors
    idx = free_index(free)
    nf = len(idx)
    H, _, used, _, _ = dense_system(nuisance, free, min_sectors, ref["sums"])
    dg = np.zeros(len(H))
    tri = triangle(W)
    for k, f in enumerate(used):
        n = int(ref["sums"][f][0])
        eps = 2.0 * max(n - 1, 0) * 2.0 ** -53
        abs_g = np.float64([ref["abs_sums"][f][1 + tri.index((c, W - 1))] for c in range(W - 1)])
        term = 2 * eps * abs_g + RHO * ref["col_abs"][f][:W - 1]
        cols = idx + list(range(6, 6 + Q))
        where = list(range(nf)) + list(range(nf + Q * k, nf + Q * k + Q))
        dg[where] += term[cols]
    Hinv = np.abs(np.linalg.inv(H))
    bound = np.zeros(6)
    for i, j in enumerate(idx):
        s = 1.0 if j < 4 else ref["lens"]["rn"]
        bound[j] = Hinv[i] @ dg + 2.0 ** -50 * abs(ref["lens"][PARAMS[j]]) + 2e-12 * s
    return bound


def correct(model, L, cen, rec, good):
    """lk_lens_correct of one frame in float64 -> p [S][6] float64 (unchanged where not corrected), status [S]"""
    with np.errstate(invalid="ignore"):
        p = rec["p"].astype(np.float64)
    X = np.asarray(cen, np.float32).astype(np.float64)
    uv = p[:, :2].copy()
    if model == ca.FM_U:
        uv[:, 1] = 0.0
    c = np.float64([L["cx"], L["cy"]])
    status = np.where(good, 0, 1).astype(np.uint8)
    RX, A, out_X = undistort_rho(L, (X - c) / L["rn"])
    rx, B, out_x = undistort_rho(L, ((X + np.nan_to_num(uv)) - c) / L["rn"])
    status[good & (out_X | out_x)] = 2
    Xu, xu = c + L["rn"] * RX, c + L["rn"] * rx
    for s in np.flatnonzero(status == 0):
        p[s, 0] = xu[s, 0] - Xu[s, 0]
        if model != ca.FM_U:
            p[s, 1] = xu[s, 1] - Xu[s, 1]
        JA = np.float64([[A[0][s], A[1][s]], [A[1][s], A[2][s]]])
        JB = np.float64([[B[0][s], B[1][s]], [B[1][s], B[2][s]]])
        if model == ca.FM_UVQ:
            G = np.linalg.inv(JB) @ np.float64([[1, -p[s, 2]], [p[s, 2], 1]]) @ JA
            p[s, 2] = (G[1, 0] - G[0, 1]) / 2
        elif model == ca.FM_UVUXUYVXVY:
            G = np.linalg.inv(JB) @ np.float64([[1 + p[s, 2], p[s, 3]], [p[s, 4], 1 + p[s, 5]]]) @ JA
            p[s, 2:6] = [G[0, 0] - 1, G[0, 1], G[1, 0], G[1, 1] - 1]
    return p, status


# ---- the synthetic data of the tests -------------------------------------------------------------------------------------
TRUE = make_lens(126.0, 117.0, 147.785, k1=-0.03, k2=0.008)
SHIFTS = np.float64([(12, 0), (-12, 0), (0, 9), (0, -9), (8, -6)])


def shifted_records(cen, L=TRUE, shifts=SHIFTS, similarity=None, noise=0.0, seed=0):
    """records u = D(U(X) + N_f(U(X))) - X rounded to float, all good; similarity [F][2]: the frames' (a, b) about the centre of
    the centres' bounding box; noise: sigma of N(0, sigma) px added to u and v before the rounding"""
    X = np.asarray(cen, np.float32).astype(np.float64)
    o = origin_of(cen)
    Xu, outside = undistort(L, X)
    assert not outside.any()
    rng = np.random.default_rng(seed)
    rec = np.zeros((len(shifts), len(X)), ca.RESULT_DTYPE)
    for f, t in enumerate(shifts):
        N = np.float64(t) + np.zeros_like(Xu)
        if similarity is not None:
            a, b = similarity[f]
            e = Xu - o
            N = N + a * e + b * np.stack([-e[:, 1], e[:, 0]], axis=1)
        uv = distort(L, Xu + N) - X
        if noise > 0:
            uv = uv + rng.normal(0.0, noise, uv.shape)
        rec[f]["p"][:, :2] = uv
    rec["chi"], rec["n_points"], rec["iterations"] = 0.5, 361, 5
    rec["und_cx"], rec["und_cy"] = X[:, 0], X[:, 1]
    return rec


# ---- frames seen through a lens, for the end-to-end tests -------------------------------------------------------------------
IMAGE_LENS = make_lens(126.0, 117.0, 147.785, k1=-0.03)
IMAGE_SHIFTS = np.float64([(12, 0), (-12, 0), (0, 9), (0, -9)])


def lens_frames(size=256, margin=40, seed=5, sigma=2.5):
    """-> (the unshifted frame, the four shifted ones): speckle.blobs on a canvas `margin` px larger all round, the blob centres
    carried through t and then through the lens (ca.lens_distort), rendered by the module's renderer at size x size"""
    from correlation_amd import speckle
    xs, ys, amps = speckle.blobs(size + 2 * margin, size + 2 * margin, seed)
    base = np.stack([xs.astype(np.float64) - margin, ys.astype(np.float64) - margin], axis=1)
    frames = []
    for t in np.concatenate([np.zeros((1, 2)), IMAGE_SHIFTS]):
        d = ca.lens_distort(as_record(IMAGE_LENS), base + t)
        frames.append(speckle._render(size, size, d[:, 0].astype(np.float32), d[:, 1].astype(np.float32), amps, sigma))
    return frames[0], frames[1:]


def spread_about_frame_mean(rec, good):
    """rms over the good records of (u, v) about their frame's mean"""
    total, n = 0.0, 0
    for f in range(len(rec)):
        uv = rec[f]["p"][good[f], :2].astype(np.float64)
        total += ((uv - uv.mean(axis=0)) ** 2).sum()
        n += len(uv)
    return np.sqrt(total / n)
