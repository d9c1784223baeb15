"""Float64 numpy restatement of the two-camera rig (include/lk_engine.h: lk_stereo_project, lk_stereo_triangulate,
lk_stereo_fundamental, lk_stereo_strain), written from the interface's text, and the synthetic rig, surfaces and records of
tests/test_stereo_host.py and tests/test_stereo_gpu.py.

The rig: 256 x 256 images, f = 800 px, principal point (127.5, 127.5), stand-off Z = 400 world units.  Camera 0 sits at the
origin and looks along +Z; camera 1 is turned 20 degrees about Y around the target (0, 0, 400) and looks at it, so the
baseline is b = 2 Z sin(10 deg) = 138.9.  Each camera has its own lens (LENS0, LENS1).

Tolerances, from rounding alone.

  e64 = 2^-53, e32 = 2^-24.  One pixel of matching error moves a triangulated point by about Z^2 / (f b) = 1.44 units in
  depth and Z / f = 0.5 units sideways: DEPTH_PER_PIXEL.

  POINT_TOL (library against restatement, and project(triangulate(x)) = x).  Both are double computations of the same
  minimiser from the same pixels.  Pixels are ~256 and go through the lens (6 Newton steps, each a handful of operations on
  numbers of order 1 scaled by rn ~ 150): an absolute error of some 50 e64 256 = 1.4e-12 px per undistorted pixel.  The
  Gauss-Newton fixed point inherits the rounding of its last step: J^T r is formed from residuals of order <= 1 px with
  entries of J of order f / Z = 2, and the 3 x 3 solve has condition (Z / b)^2 ~ 8 along depth, so the point is known to
  about 8 * 50 e64 * 256 * DEPTH_PER_PIXEL ~ 2e-11 units.  POINT_TOL = 1e-10 units leaves a factor of five; in pixels
  (PIXEL_TOL) the same bound divided by Z / f, 2e-10 px.  Both figures are derived, not measured.

  GRADIENT_TOL (J^T r = 0 at the solution).  The residuals are differences of pixels of order 256 that carry the absolute
  rounding above, 1.4e-12 px, whatever their own size; J^T r adds four of them per component with |J| ~ f / Z = 2, twice
  over for the two roundings (observed and projected): 16 * 1.4e-12 = 2.3e-11.  A Gauss-Newton iteration that stopped a step
  delta short of its fixed point has J^T r = J^T J delta ~ 4 delta, so the bound says delta <= 6e-12 units: the fixed step
  count has converged to the rounding of the data.  GRADIENT_TOL = 2.5e-11, with pixel noise up to 0.5 px.

  SURFACE_TOL (device or library surface record against the restatement on the same float64 points).  As
  tests/test_strain_gpu.py: the two differ only in the order of double sums of at most ~200 terms, about 1e-13 relative on
  moments whose condition stays below ~100, and the strain is a difference of metrics of order |a|^2 divided by |a|^2: 1e-11
  absolute.  Every float field is also rounded to float once: 2^-22 |ref| covers one rounding plus a double-rounding
  neighbour.  SURFACE_TOL(ref, scale) = 2^-22 |ref| + 1e-9 scale, scale = 1 for strains, normal components and angles
  and the size of the numbers (Z) for lengths.  theta = atan2(2 exy, exx - eyy) / 2 moves by the strains' error divided by
  e1 - e2: its second term is 1e-9 / (e1 - e2), and it is compared only where e1 - e2 > 1e-6 (elsewhere it is ill-defined).

  truth_bound(U, sigma) (surface strain from float32 RECORDS against the analytic strain).  A record field is rounded to
  float: an error of at most e32 U px with U the largest |u|, |v| (the cross-camera disparity dominates).  A point reads
  four such fields (two pixels), each moving it by at most DEPTH_PER_PIXEL per pixel: 4 e32 U DEPTH_PER_PIXEL.  The
  displacement is a difference of two points: x 2.  A worst-case (not statistical) error eps in every member moves a
  least-squares gradient by at most eps / sigma, sigma the rms spread of the window's centres along the weaker axis in
  pixels.  The strain is the relative change of the tangents' metric: divide by |a| = Z / f, and x 2 for the two tangents
  entering a component.  Altogether 16 e32 U Z / (b sigma): 1.5e-5 for U = 100 px and sigma = 19 px.

  The end-to-end bounds of tests/test_stereo_gpu.py are measured against the CPU oracle as that file says."""
import numpy as np

import correlation_amd as ca

E64, E32 = 2.0 ** -53, 2.0 ** -24
SIZE, FOCAL, CENTRE, Z0, ANGLE = 256, 800.0, 127.5, 400.0, np.deg2rad(20.0)
BASELINE = 2.0 * Z0 * np.sin(ANGLE / 2.0)
DEPTH_PER_PIXEL = Z0 * Z0 / (FOCAL * BASELINE)
POINT_TOL, PIXEL_TOL = 1e-10, 2e-10
LENS0 = dict(cx=126.0, cy=117.0, rn=147.785, k1=-0.03, k2=0.008, p1=0.0, p2=0.0)
LENS1 = dict(cx=130.0, cy=125.0, rn=150.0, k1=0.02, k2=0.0, p1=1e-3, p2=-5e-4)
NO_LENS = dict(cx=0.0, cy=0.0, rn=0.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0)


GRADIENT_TOL = 2.5e-11


def surface_tol(ref, scale):
    return 2.0 ** -22 * np.abs(ref) + 1e-9 * scale


def truth_bound(U, sigma):
    return 16.0 * E32 * U * Z0 / (BASELINE * sigma)


# ---- the rig ------------------------------------------------------------------------------------------------------------------
def look_at(position, target):
    z = np.float64(target) - np.float64(position)
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ np.float64(position)


def make_rig(lenses=(LENS0, LENS1), angle=ANGLE):
    """-> two camera dicts {fx, fy, cx, cy, skew, R, t, lens}"""
    c1 = np.float64([Z0 * np.sin(angle), 0.0, Z0 * (1.0 - np.cos(angle))])
    R1, t1 = look_at(c1, (0.0, 0.0, Z0))
    base = dict(fx=FOCAL, fy=FOCAL * 1.002, cx=CENTRE, cy=CENTRE - 2.0, skew=0.0)
    return [dict(base, R=np.eye(3), t=np.zeros(3), lens=dict(lenses[0])),
            dict(base, skew=0.05, R=R1, t=t1, lens=dict(lenses[1]))]


def as_records(rig):
    """the rig as CAMERA_DTYPE records for the library"""
    out = []
    for c in rig:
        L = c["lens"]
        lens = ca.make_lens(L["cx"], L["cy"], L["rn"], L["k1"], L["k2"], L["p1"], L["p2"])
        out.append(ca.make_camera(c["fx"], c["fy"], c["cx"], c["cy"], R=c["R"], t=c["t"], skew=c["skew"], lens=lens))
    return out


# ---- the camera ---------------------------------------------------------------------------------------------------------------
def has_lens(L):
    return any(L[k] != 0.0 for k in ("k1", "k2", "p1", "p2"))


def lens_d(L, rho):
    """D in units of rn about the centre, and its Jacobian [n][2][2]"""
    rx, ry = rho[:, 0], rho[:, 1]
    r2 = rx * rx + ry * ry
    radial = 1.0 + L["k1"] * r2 + L["k2"] * r2 * r2
    g = 2.0 * L["k1"] + 4.0 * L["k2"] * r2
    d = np.stack([rx * radial + 2.0 * L["p1"] * rx * ry + L["p2"] * (r2 + 2.0 * rx * rx),
                  ry * radial + L["p1"] * (r2 + 2.0 * ry * ry) + 2.0 * L["p2"] * rx * ry], 1)
    J = np.empty((len(rx), 2, 2))
    J[:, 0, 0] = radial + g * rx * rx + 2.0 * L["p1"] * ry + 6.0 * L["p2"] * rx
    J[:, 0, 1] = J[:, 1, 0] = g * rx * ry + 2.0 * L["p1"] * rx + 2.0 * L["p2"] * ry
    J[:, 1, 1] = radial + g * ry * ry + 6.0 * L["p1"] * ry + 2.0 * L["p2"] * rx
    return d, J


def distort(L, xy):
    if not has_lens(L):
        return np.array(xy, np.float64)
    c = np.float64([L["cx"], L["cy"]])
    return c + L["rn"] * lens_d(L, (np.float64(xy) - c) / L["rn"])[0]


def undistort(L, xy):
    """-> (undistorted [n][2], outside [n]): Newton from rho_d; outside: det J <= 0 at an iterate or at the result"""
    xy = np.float64(xy).reshape(-1, 2)
    if not has_lens(L):
        return xy.copy(), np.zeros(len(xy), bool)
    c = np.float64([L["cx"], L["cy"]])
    q = (xy - c) / L["rn"]
    rho, outside = q.copy(), np.zeros(len(q), bool)
    with np.errstate(all="ignore"):
        for _ in range(6):
            d, J = lens_d(L, rho)
            det = np.linalg.det(J)
            outside |= ~(det > 0)
            rho = rho - np.linalg.solve(np.where(outside[:, None, None], np.eye(2), J), (d - q)[..., None])[..., 0]
        det = np.linalg.det(lens_d(L, rho)[1])
    outside |= ~(det > 0) | ~np.isfinite(det)
    return c + L["rn"] * rho, outside


def intrinsics(c):
    return np.float64([[c["fx"], c["skew"], c["cx"]], [0.0, c["fy"], c["cy"]], [0.0, 0.0, 1.0]])


def pinhole(c, X):
    xc = np.float64(X).reshape(-1, 3) @ c["R"].T + c["t"]
    m = xc @ intrinsics(c).T
    return m[:, :2] / m[:, 2:], xc[:, 2]


def project(c, X):
    """world points -> pixels as the camera shows them"""
    return distort(c["lens"], pinhole(c, X)[0])


def fundamental(rig):
    Rr = rig[1]["R"] @ rig[0]["R"].T
    tr = rig[1]["t"] - Rr @ rig[0]["t"]
    Tx = np.float64([[0, -tr[2], tr[1]], [tr[2], 0, -tr[0]], [-tr[1], tr[0], 0]])
    return np.linalg.inv(intrinsics(rig[1])).T @ Tx @ Rr @ np.linalg.inv(intrinsics(rig[0]))


def rays(c, m):
    d = np.linalg.solve(intrinsics(c), np.concatenate([m, np.ones((len(m), 1))], 1).T).T @ c["R"]
    return -c["R"].T @ c["t"], d


def reprojection(rig, P, m0, m1):
    """residuals [n][4] (observed - projected) and Jacobians d(projected)/dX [n][4][3]"""
    r, J = np.empty((len(P), 4)), np.empty((len(P), 4, 3))
    for k, (c, m) in enumerate(zip(rig, (m0, m1))):
        xc = P @ c["R"].T + c["t"]
        xn, yn, z = xc[:, 0] / xc[:, 2], xc[:, 1] / xc[:, 2], xc[:, 2]
        r[:, 2 * k] = m[:, 0] - (c["fx"] * xn + c["skew"] * yn + c["cx"])
        r[:, 2 * k + 1] = m[:, 1] - (c["fy"] * yn + c["cy"])
        ex = c["R"][0][None] - xn[:, None] * c["R"][2][None]
        ey = c["R"][1][None] - yn[:, None] * c["R"][2][None]
        J[:, 2 * k] = (c["fx"] * ex + c["skew"] * ey) / z[:, None]
        J[:, 2 * k + 1] = c["fy"] * ey / z[:, None]
    return r, J


def triangulate(rig, x0, x1, steps=12):
    """-> dict of arrays: P [n][3], residual [n][4], epipolar, angle, status, and m0, m1 (the undistorted pixels).  Gauss-Newton
    run for `steps` steps (well past convergence), every point carried along whatever its status."""
    x0, x1 = np.float64(x0).reshape(-1, 2), np.float64(x1).reshape(-1, 2)
    n = len(x0)
    status = np.zeros(n, np.int32)
    bad = ~(np.isfinite(x0).all(1) & np.isfinite(x1).all(1))
    x0, x1 = np.where(bad[:, None], 0.0, x0), np.where(bad[:, None], 0.0, x1)
    m0, out0 = undistort(rig[0]["lens"], x0)
    m1, out1 = undistort(rig[1]["lens"], x1)
    outside = out0 | out1
    m0, m1 = np.where(outside[:, None], 0.0, m0), np.where(outside[:, None], 0.0, m1)
    o0, d0 = rays(rig[0], m0)
    o1, d1 = rays(rig[1], m1)
    w = o0 - o1
    a, b, c = (d0 * d0).sum(1), (d0 * d1).sum(1), (d1 * d1).sum(1)
    d, e = d0 @ w, d1 @ w
    det = a * c - b * b
    parallel = ~(det > 1e-12 * a * c)
    with np.errstate(all="ignore"):
        s, t = (b * e - c * d) / det, (a * e - b * d) / det
    behind = ~(s > 0) | ~(t > 0)
    dead = bad | outside | parallel | behind
    s, t = np.where(dead, 1.0, s), np.where(dead, 1.0, t)
    P = ((o0 + s[:, None] * d0) + (o1 + t[:, None] * d1)) / 2.0
    P[dead] = (0.0, 0.0, Z0)
    for _ in range(steps):
        r, J = reprojection(rig, P, m0, m1)
        P = P + np.linalg.solve(J.transpose(0, 2, 1) @ J, (J.transpose(0, 2, 1) @ r[..., None]))[..., 0]
    r, J = reprojection(rig, P, m0, m1)
    line = np.concatenate([m0, np.ones((n, 1))], 1) @ fundamental(rig).T
    epipolar = ((line[:, :2] * m1).sum(1) + line[:, 2]) / np.hypot(line[:, 0], line[:, 1])
    angle = np.arctan2(np.linalg.norm(np.cross(d0, d1), axis=1), b)
    for flag, code in ((behind, ca.STEREO_BEHIND), (parallel, ca.STEREO_PARALLEL), (outside, ca.STEREO_OUTSIDE_LENS), (bad, ca.STEREO_BAD_RECORD)):
        status[flag] = code            # (the last written wins: the order of the checks)
    dead = status != 0
    for arr in (P, r, epipolar, angle):
        arr[dead] = 0.0
    return dict(P=P, residual=r, J=J, epipolar=epipolar, angle=angle, status=status, m0=m0, m1=m1)


def as_points(tri):
    """a triangulate() result as STEREO_POINT_DTYPE records (X, Y, Z exact, the rest rounded to float)"""
    out = np.zeros(len(tri["P"]), ca.STEREO_POINT_DTYPE)
    out["X"], out["Y"], out["Z"] = tri["P"].T
    out["residual"], out["epipolar"], out["angle"], out["status"] = tri["residual"], tri["epipolar"], tri["angle"], tri["status"]
    return out


# ---- surfaces, deformations, records ------------------------------------------------------------------------------------------
def camera0_rays(rig, pixels):
    m, outside = undistort(rig[0]["lens"], pixels)
    assert not outside.any()
    return rays(rig[0], m)


def on_plane(rig, pixels, normal=(0.25, -0.15, 1.0), point=(0.0, 0.0, Z0)):
    """where camera 0's rays through `pixels` meet the plane normal . (X - point) = 0"""
    o, d = camera0_rays(rig, pixels)
    nrm = np.float64(normal)
    s = ((np.float64(point) - o) @ nrm) / (d @ nrm)
    return o + s[:, None] * d


def on_cylinder(rig, pixels, radius=120.0, axis_z=Z0 + 120.0, axis_x=5.0):
    """... the near side of the cylinder of axis (axis_x, *, axis_z) along Y"""
    o, d = camera0_rays(rig, pixels)
    ox, oz = o[0] - axis_x, o[2] - axis_z
    a = d[:, 0] ** 2 + d[:, 2] ** 2
    b = 2.0 * (ox * d[:, 0] + oz * d[:, 2])
    c = ox * ox + oz * oz - radius * radius
    s = (-b - np.sqrt(b * b - 4.0 * a * c)) / (2.0 * a)
    return o + s[:, None] * d


def rotation(axis, angle):
    k = np.float64(axis) / np.linalg.norm(axis)
    K = np.float64([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * K @ K


def plane_basis(normal=(0.25, -0.15, 1.0)):
    """an orthonormal (t1, t2, n) of the plane"""
    n = np.float64(normal) / np.linalg.norm(normal)
    t1 = np.cross([0.0, 1.0, 0.0], n)
    t1 /= np.linalg.norm(t1)
    return t1, np.cross(n, t1), n


def to_records(pixels_from, pixels_to, bad=()):
    """float32 records u = to - from (six-parameter layout, the gradients 0), all good but `bad`"""
    rec = np.zeros(len(pixels_from), ca.RESULT_DTYPE)
    rec["p"][:, :2] = (np.float64(pixels_to) - np.float64(pixels_from)).astype(np.float32)
    rec["chi"], rec["n_points"], rec["iterations"] = 0.5, 361, 5
    rec["error_code"][list(bad)] = 2
    return rec


def rig_records(rig, cen, P_ref, P_frames, bad_ref=(), bad0=(), bad1=()):
    """ref1 [S], rec0 [F][S], rec1 [F][S] from exact projections of the reference points and of every frame's points"""
    c = cen.astype(np.float64)
    ref1 = to_records(c, project(rig[1], P_ref), bad_ref)
    rec0 = np.stack([to_records(c, project(rig[0], P), bad0) for P in P_frames]) if len(P_frames) else None
    rec1 = np.stack([to_records(c, project(rig[1], P), bad1) for P in P_frames]) if len(P_frames) else None
    return ref1, rec0, rec1


def record_pixels(cen, rec):
    """the pixel a record points at: c + (u, v), formed in double from the floats"""
    return cen.astype(np.float64) + rec["p"][..., :2].astype(np.float64)


# ---- the surface fit ----------------------------------------------------------------------------------------------------------
def window_sums(x, y, f6):
    """the 23 sums of a window: x, y [n], f6 [n][6]"""
    s = [x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum()]
    for k in range(6):
        s += [f6[:, k].sum(), (x * f6[:, k]).sum(), (y * f6[:, k]).sum()]
    return np.float64(s)


def surface_from_window(x, y, f6, min_neighbours, self_good):
    """-> (19 float64 values in STEREO_SURFACE_FLOATS' order, status, the edge-on ratio or nan)"""
    n = len(x)
    vals = np.zeros(19)
    if n < min_neighbours:
        return vals, ca.STEREO_SURFACE_TOO_FEW, np.nan, np.nan
    Sx, Sy = x.sum(), y.sum()
    Cxx, Cxy, Cyy = (x * x).sum() - Sx * Sx / n, (x * y).sum() - Sx * Sy / n, (y * y).sum() - Sy * Sy / n
    D = Cxx * Cyy - Cxy * Cxy
    ratio = D / (Cxx * Cyy) if Cxx * Cyy != 0 else np.nan
    if Cxx * Cyy == 0 or D <= 1e-6 * Cxx * Cyy:
        return vals, ca.STEREO_SURFACE_DEGENERATE, ratio, np.nan
    Sf = f6.sum(0)
    Cxf, Cyf = x @ f6 - Sx * Sf / n, y @ f6 - Sy * Sf / n
    fx, fy = (Cyy * Cxf - Cxy * Cyf) / D, (Cxx * Cyf - Cxy * Cxf) / D
    f0 = Sf / n - fx * Sx / n - fy * Sy / n
    a1, a2 = fx[:3], fy[:3]
    b1, b2 = a1 + fx[3:], a2 + fy[3:]
    G = np.float64([[a1 @ a1, a1 @ a2], [a1 @ a2, a2 @ a2]])
    g = np.float64([[b1 @ b1, b1 @ b2], [b1 @ b2, b2 @ b2]])
    edge = (G[0, 0] * G[1, 1] - G[0, 1] ** 2) / (G[0, 0] * G[1, 1]) if G[0, 0] * G[1, 1] != 0 else 0.0
    if not edge > 1e-12:
        return vals, ca.STEREO_SURFACE_DEGENERATE, ratio, edge
    r11 = np.sqrt(G[0, 0])
    r12 = G[0, 1] / r11
    Ra = np.float64([[r11, r12], [0.0, np.sqrt(G[1, 1] - r12 * r12)]])
    Ri = np.linalg.inv(Ra)
    E = (Ri.T @ g @ Ri - np.eye(2)) / 2.0
    exx, eyy, exy = E[0, 0], E[1, 1], E[0, 1]
    rad = np.sqrt(((exx - eyy) / 2) ** 2 + exy ** 2)
    p1, p2 = (exx + eyy) / 2 + rad, (exx + eyy) / 2 - rad
    nrm = np.cross(a1, a2)
    nrm /= np.linalg.norm(nrm)
    misfit = f6[:, 3:] - (f0[3:] + x[:, None] * fx[3:] + y[:, None] * fy[3:])
    vals[:] = list(f0) + list(nrm) + [exx, eyy, exy, p1, p2, 0.5 * np.arctan2(2 * exy, exx - eyy), np.sqrt(1 + 2 * p1) - 1,
                                      np.sqrt(1 + 2 * p2) - 1, f0[3:] @ nrm, np.sqrt((misfit ** 2).sum() / n)]
    return vals, (ca.STEREO_SURFACE_OK if self_good else ca.STEREO_SURFACE_FILLED), ratio, edge


def surface_reference(cen, ref_points, points, radius, min_neighbours=3):
    """brute force over all pairs: ref_points [S], points [F][S] (STEREO_POINT_DTYPE) -> (values [F][S][19], neighbours [F][S],
    status [F][S], ratios [F][S][2])"""
    c = cen.astype(np.float64)
    S, F = len(c), len(points)
    vals, nbrs = np.zeros((F, S, 19)), np.zeros((F, S), np.int32)
    status, ratios = np.zeros((F, S), np.int32), np.full((F, S, 2), np.nan)
    r2 = np.float64(np.float32(radius)) ** 2
    Pr = np.stack([ref_points["X"], ref_points["Y"], ref_points["Z"]], 1)
    for f in range(F):
        Pf = np.stack([points[f]["X"], points[f]["Y"], points[f]["Z"]], 1)
        good = (ref_points["status"] == 0) & (points[f]["status"] == 0)
        f6 = np.concatenate([Pr, Pf - Pr], 1)
        for s in range(S):
            d = c - c[s]
            near = good & (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= r2)
            nbrs[f, s] = near.sum()
            vals[f, s], status[f, s], ratios[f, s, 0], ratios[f, s, 1] = surface_from_window(d[near, 0], d[near, 1], f6[near], min_neighbours,
                                                                                           bool(good[s]))
    return vals, nbrs, status, ratios


def check_surface(got, ref, what, length_scale=Z0):
    """a STEREO_SURFACE_DTYPE array against surface_reference's tables: counts and statuses exact, floats within
    surface_tol; -> the worst error / tolerance"""
    vals, nbrs, status, _ = ref
    assert np.array_equal(got["status"], status), (what, np.argwhere(got["status"] != status)[:5])
    assert np.array_equal(got["neighbours"], nbrs), what
    assert not got["reserved"].any()
    worst = 0.0
    for k, name in enumerate(ca.STEREO_SURFACE_FLOATS):
        scale = length_scale if name in ("X", "Y", "Z", "U", "V", "W", "normal", "residual") else 1.0
        tol = surface_tol(vals[..., k], scale)
        err = np.abs(got[name].astype(np.float64) - vals[..., k])
        if name == "theta":                        # ill-defined where the principal strains coincide; a branch cut at +- pi / 2
            gap = vals[..., 12] - vals[..., 13]
            err = np.minimum(err, np.abs(err - np.pi))
            err = np.where(gap > 1e-6, err, 0.0)
            tol = 2.0 ** -22 * np.abs(vals[..., k]) + 1e-9 / np.maximum(gap, 1e-6)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (what, name, np.unravel_index(np.argmax(err / tol), err.shape), float(err.max()))
    dead = np.isin(status, (ca.STEREO_SURFACE_TOO_FEW, ca.STEREO_SURFACE_DEGENERATE))
    for name in ca.STEREO_SURFACE_FLOATS:
        assert not got[name][dead].any(), (what, name)
    return worst


# ---- rendered frames ----------------------------------------------------------------------------------------------------------
def rig_frames(rig, size=SIZE, margin=40, seed=5, sigma=2.5):
    """-> (camera 0's reference image, camera 1's): speckle.blobs on a canvas `margin` px larger all round taken as camera 0's
    pixels, carried along camera 0's rays onto the tilted plane and from there into camera 1, each set rendered by the
    module's renderer at size x size (the way lens_ref.lens_frames renders through a lens)"""
    from correlation_amd import speckle
    xs, ys, amps = speckle.blobs(size + 2 * margin, size + 2 * margin, seed)
    base = np.stack([xs.astype(np.float64) - margin, ys.astype(np.float64) - margin], axis=1)
    seen = project(rig[1], on_plane(rig, base))
    return (speckle._render(size, size, base[:, 0].astype(np.float32), base[:, 1].astype(np.float32), amps, sigma),
            speckle._render(size, size, seen[:, 0].astype(np.float32), seen[:, 1].astype(np.float32), amps, sigma))


def disparity_guess(rig, cen):
    """[S][6] guesses: the true cross-camera disparity of the tilted plane at the centres, rounded to whole pixels"""
    g = np.zeros((len(cen), 6), np.float32)
    g[:, :2] = np.round(project(rig[1], on_plane(rig, cen)) - cen.astype(np.float64))
    return g


def plane_rms(points):
    """rms distance of the OK points from their own least-squares plane, and their count"""
    ok = points["status"] == 0
    Pts = np.stack([points["X"], points["Y"], points["Z"]], 1)[ok]
    d = Pts - Pts.mean(axis=0)
    return float(np.sqrt(np.linalg.svd(d, compute_uv=False)[-1] ** 2 / len(d))), int(ok.sum())
