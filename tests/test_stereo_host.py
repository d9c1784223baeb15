"""The two-camera rig on the host (lk_stereo_project, lk_stereo_triangulate, lk_stereo_fundamental,
lk_stereo_surface_from_sums, include/lk_engine.h): the kernels' own functions compiled for the host, against the float64
restatement of tests/stereo_ref.py.  No GPU.  Every tolerance is derived in stereo_ref's docstring."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi
import stereo_ref as sr
from stereo_ref import GRADIENT_TOL, PIXEL_TOL, POINT_TOL

P = C.c_void_p


@pytest.fixture(scope="module")
def rig(engine_lib):
    r = sr.make_rig()
    return r, sr.as_records(r)


@pytest.fixture(scope="module")
def scene(rig):
    """500 points of the tilted plane seen by both cameras: (world points, pixels 0, pixels 1) of the restatement"""
    r, _ = rig
    px = np.random.default_rng(1).uniform(10.0, 245.0, (500, 2))
    X = sr.on_plane(r, px)
    return X, sr.project(r[0], X), sr.project(r[1], X)


def xyz(t):
    return np.stack([t["X"], t["Y"], t["Z"]], 1)


def test_layouts_and_symbols(engine_lib):
    d = ca.CAMERA_DTYPE
    assert d.itemsize == 256 and [d.fields[k][1] for k in ("fx", "skew", "R", "t", "lens", "reserved")] == [0, 32, 40, 112, 136, 200]
    d = ca.STEREO_POINT_DTYPE
    assert d.itemsize == 64 and [d.fields[k][1] for k in ("X", "Z", "residual", "epipolar", "angle", "status", "reserved")] == \
        [0, 16, 24, 40, 44, 48, 52]
    d = ca.STEREO_SURFACE_DTYPE
    assert d.itemsize == 128 and [d.fields[k][1] for k in ("X", "U", "nx", "exx", "theta", "biot1", "normal", "residual", "neighbours",
                                                            "status", "reserved")] == [0, 12, 24, 36, 56, 60, 68, 72, 76, 80, 84]
    assert C.sizeof(_ffi.LkStereoConfig) == 16
    assert (ca.STEREO_OK, ca.STEREO_BAD_RECORD, ca.STEREO_OUTSIDE_LENS, ca.STEREO_PARALLEL, ca.STEREO_BEHIND) == (0, 1, 2, 3, 4)
    assert (ca.STEREO_SURFACE_OK, ca.STEREO_SURFACE_FILLED, ca.STEREO_SURFACE_TOO_FEW, ca.STEREO_SURFACE_DEGENERATE) == (0, 1, 2, 3)
    for name in ("lk_stereo_project", "lk_stereo_triangulate", "lk_stereo_fundamental", "lk_stereo_surface_from_sums", "lk_stereo_points",
                 "lk_stereo_strain", "lk_internal_stereo_last"):
        assert hasattr(engine_lib, name), name
    blob = open(ca.LIB_PATH, "rb").read()
    assert b"lk_stereo_points_kernel" in blob and b"lk_stereo_strain_kernel" in blob


def test_projection_and_fundamental_match_the_restatement(rig, scene):
    r, cams = rig
    X, x0, x1 = scene
    for k, want in enumerate((x0, x1)):
        got, status = ca.stereo_project(cams[k], X, return_status=True)
        assert not status.any() and np.abs(got - want).max() <= PIXEL_TOL
    assert x1.min() > 0.0 and x1.max() < 257.0           # the second camera is aimed at the same patch
    F, want = ca.stereo_fundamental(cams), sr.fundamental(r)
    assert np.abs(F - want).max() <= 64 * sr.E64 * np.abs(want).max()
    # the epipolar constraint on the undistorted pixels of one point
    m0, m1 = sr.pinhole(r[0], X)[0], sr.pinhole(r[1], X)[0]
    line = np.concatenate([m0, np.ones((len(X), 1))], 1) @ F.T
    dist = ((line[:, :2] * m1).sum(1) + line[:, 2]) / np.hypot(line[:, 0], line[:, 1])
    assert np.abs(dist).max() <= PIXEL_TOL
    # a lens without coefficients is the identity, exactly; behind the camera is a status
    bare = ca.make_camera(800.0, 800.0, 127.5, 127.5)
    assert ca.stereo_project(bare, [[0.0, 0.0, 400.0], [50.0, -25.0, 400.0]]).tolist() == [[127.5, 127.5], [227.5, 77.5]]
    got, status = ca.stereo_project(bare, [[1.0, 2.0, -5.0], [1.0, 2.0, 0.0], [0.0, 0.0, 1.0]], return_status=True)
    assert status.tolist() == [1, 1, 0] and not got[:2].any()


def test_exact_matches_come_back(rig, scene):
    r, cams = rig
    X, x0, x1 = scene
    t = ca.stereo_triangulate(cams, x0, x1)
    assert (t["status"] == ca.STEREO_OK).all() and not t["reserved"].any()
    err = np.abs(xyz(t) - X).max()
    back0, back1 = ca.stereo_project(cams[0], xyz(t)), ca.stereo_project(cams[1], xyz(t))
    print(f"exact matches: |X - truth| {err:.3g} (bound {POINT_TOL}), reprojected {np.abs(back0 - x0).max():.3g}, {np.abs(back1 - x1).max():.3g} px "
          f"(bound {PIXEL_TOL}), |residual| {np.abs(t['residual']).max():.3g}, |epipolar| {np.abs(t['epipolar']).max():.3g}")
    assert err <= POINT_TOL
    assert np.abs(back0 - x0).max() <= PIXEL_TOL and np.abs(back1 - x1).max() <= PIXEL_TOL
    assert np.abs(t["residual"]).max() <= PIXEL_TOL and np.abs(t["epipolar"]).max() <= PIXEL_TOL
    assert np.abs(t["angle"] - sr.ANGLE).max() < 0.06      # 20 degrees at the target, a little more or less across the patch


@pytest.mark.parametrize("sigma", [0.02, 0.1, 0.5])
def test_noisy_matches(rig, scene, sigma):
    """the library against the restatement; J^T r = 0 at the library's point; the residual has one degree of freedom"""
    r, cams = rig
    _, x0, x1 = scene
    rng = np.random.default_rng(int(sigma * 1000))
    n0, n1 = x0 + rng.normal(0, sigma, x0.shape), x1 + rng.normal(0, sigma, x1.shape)
    t, ref = ca.stereo_triangulate(cams, n0, n1), sr.triangulate(r, n0, n1)
    assert (t["status"] == 0).all() and (ref["status"] == 0).all()
    res, J = sr.reprojection(r, xyz(t), ref["m0"], ref["m1"])
    grad = np.abs((J.transpose(0, 2, 1) @ res[..., None])[..., 0]).max()
    msr = float((t["residual"].astype(np.float64) ** 2).sum(1).mean())
    se = sigma ** 2 * np.sqrt(2.0 / len(x0))                # a chi-square of one degree of freedom: variance 2 sigma^4
    print(f"sigma {sigma}: |X - restatement| {np.abs(xyz(t) - ref['P']).max():.3g}, |J^T r| {grad:.3g} (bound {GRADIENT_TOL}), "
          f"mean |r|^2 {msr:.5g} of {sigma ** 2:.5g} ({abs(msr - sigma ** 2) / se:.2f} standard errors)")
    assert np.abs(xyz(t) - ref["P"]).max() <= POINT_TOL
    assert grad <= GRADIENT_TOL
    assert abs(msr - sigma ** 2) <= 5.0 * se
    for k in ("residual", "epipolar", "angle"):
        want = ref[k]
        assert np.abs(t[k] - want).max() <= 2.0 ** -22 * np.abs(want).max() + PIXEL_TOL, k
    assert np.abs(t["epipolar"]).max() > 0.5 * sigma        # (the noise is seen)


def test_every_status(rig, scene):
    r, cams = rig
    X, x0, x1 = scene
    a, b = x0[:6].copy(), x1[:6].copy()
    a[1, 0], b[2, 1] = np.nan, np.inf                       # 1, 2: not finite
    t = ca.stereo_triangulate(cams, a, b)
    assert t["status"].tolist() == [0, 1, 1, 0, 0, 0]
    # a fold: pixels far out are outside a lens that turns back
    fold = sr.make_rig(lenses=(dict(sr.LENS0, k1=-0.5, k2=0.0), sr.LENS1))
    fcams = sr.as_records(fold)
    corner = np.float64([[3.0, 2.0], [250.0, 4.0], [126.0, 117.0]])
    _, outside = sr.undistort(fold[0]["lens"], corner)
    assert outside.tolist() == [True, True, False]
    t2 = ca.stereo_triangulate(fcams, corner, np.float64([[128.0, 128.0]] * 3))
    assert t2["status"][:2].tolist() == [ca.STEREO_OUTSIDE_LENS] * 2 and t2["status"][2] != ca.STEREO_OUTSIDE_LENS
    # bad record comes before outside: a NaN pixel and a folded one
    assert ca.stereo_triangulate(fcams, [[np.nan, 2.0]], [[128.0, 128.0]])["status"][0] == ca.STEREO_BAD_RECORD
    # parallel rays: two cameras in the same pose but a shift see a point at infinity at the same pixel
    c0 = ca.make_camera(800.0, 800.0, 127.5, 127.5)
    c1 = ca.make_camera(800.0, 800.0, 127.5, 127.5, t=(-100.0, 0.0, 0.0))
    par = ca.stereo_triangulate([c0, c1], [[140.0, 90.0], [140.0, 90.0], [140.0, 90.0]], [[140.0, 90.0], [139.0, 90.0], [141.0, 90.0]])
    # same pixel: parallel; a disparity of the right sign: a point in front (Z = f b / d = 80 000); of the wrong sign: behind
    assert par["status"].tolist() == [ca.STEREO_PARALLEL, ca.STEREO_OK, ca.STEREO_BEHIND]
    assert abs(par["Z"][1] - 80000.0) < 1e-3
    ref = sr.triangulate([dict(fx=800.0, fy=800.0, cx=127.5, cy=127.5, skew=0.0, R=np.eye(3), t=np.zeros(3), lens=sr.NO_LENS),
                          dict(fx=800.0, fy=800.0, cx=127.5, cy=127.5, skew=0.0, R=np.eye(3), t=np.float64([-100.0, 0, 0]), lens=sr.NO_LENS)],
                         [[140.0, 90.0]] * 3, [[140.0, 90.0], [139.0, 90.0], [141.0, 90.0]])
    assert ref["status"].tolist() == par["status"].tolist()
    # whatever is not OK is all zeros, never NaN
    for rec in (t[1:3], t2[:2], par[[0, 2]]):
        for k in ("X", "Y", "Z", "residual", "epipolar", "angle", "reserved"):
            assert not rec[k].any() and np.isfinite(rec[k]).all(), k
    # and the restatement agrees on the first set
    assert sr.triangulate(r, a, b)["status"].tolist() == t["status"].tolist()


def test_refusals(rig, engine_lib):
    _, cams = rig
    lib = engine_lib
    good = _ffi._rig(cams)
    xy, out2 = np.zeros((2, 2)), np.zeros((2, 2))
    pts = np.zeros(2, ca.STEREO_POINT_DTYPE)
    X = np.float64([[0.0, 0.0, 400.0], [1.0, 1.0, 400.0]])
    Fm = np.zeros(9)

    def all_three(rig2):
        p = rig2.ctypes.data_as(P) if rig2 is not None else None
        return (lib.lk_stereo_project(p, 2, X.ctypes.data_as(P), out2.ctypes.data_as(P), None),
                lib.lk_stereo_fundamental(p, Fm.ctypes.data_as(P)),
                lib.lk_stereo_triangulate(p, 2, xy.ctypes.data_as(P), xy.ctypes.data_as(P), pts.ctypes.data_as(P)))

    assert all_three(good) == (0, 0, 0)
    assert all_three(None) == (ca.ERROR_BAD_DOMAIN,) * 3

    def broken(**kw):
        bad = good.copy()
        for k, v in kw.items():
            if k == "R01":
                bad["R"][0][0, 1] = v
            elif k.startswith("lens_"):
                bad["lens"][k[5:]][0] = v
            elif k == "reserved":
                bad["reserved"][0][3] = v
            elif k == "t":
                bad["t"][0][1] = v
            else:
                bad[k][0] = v
        return bad

    for kw in (dict(reserved=1.0), dict(fx=0.0), dict(fx=-800.0), dict(fy=0.0), dict(fx=np.nan), dict(fy=np.inf), dict(cx=np.nan), dict(cy=np.inf),
               dict(skew=np.nan), dict(R01=1e-6), dict(R01=np.nan), dict(t=np.inf), dict(lens_k1=np.nan), dict(lens_rn=0.0),
               dict(lens_rn=np.nan), dict(lens_cx=np.inf), dict(lens_reserved=1.0)):
        assert all_three(broken(**kw)) == (ca.ERROR_BAD_DOMAIN,) * 3, kw
    assert all_three(broken(R01=1e-12)) == (0, 0, 0)       # within the bound on R^T R
    # a refused second camera: project reads the first alone
    second = good.copy()
    second["fx"][1] = 0.0
    assert all_three(second) == (0, ca.ERROR_BAD_DOMAIN, ca.ERROR_BAD_DOMAIN)
    # a lens without coefficients is not read at all
    bare = good.copy()
    bare["lens"] = np.zeros(1, ca.LENS_DTYPE)[0]
    assert all_three(bare) == (0, 0, 0)
    g = good.ctypes.data_as(P)
    # nulls and counts
    assert lib.lk_stereo_project(g, 0, X.ctypes.data_as(P), out2.ctypes.data_as(P), None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_stereo_project(g, 2, None, out2.ctypes.data_as(P), None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_stereo_project(g, 2, X.ctypes.data_as(P), None, None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_stereo_fundamental(g, None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_stereo_triangulate(g, 0, xy.ctypes.data_as(P), xy.ctypes.data_as(P), pts.ctypes.data_as(P)) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_stereo_triangulate(g, 2, None, xy.ctypes.data_as(P), pts.ctypes.data_as(P)) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_stereo_triangulate(g, 2, xy.ctypes.data_as(P), None, pts.ctypes.data_as(P)) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_stereo_triangulate(g, 2, xy.ctypes.data_as(P), xy.ctypes.data_as(P), None) == ca.ERROR_BAD_DOMAIN
    s23, surf = np.zeros(23), np.zeros(1, ca.STEREO_SURFACE_DTYPE)
    fn = lib.lk_stereo_surface_from_sums
    assert fn(5, s23.ctypes.data_as(P), 3, 1, 0.0, surf.ctypes.data_as(P), None) == 0
    assert fn(-1, s23.ctypes.data_as(P), 3, 1, 0.0, surf.ctypes.data_as(P), None) == ca.ERROR_BAD_DOMAIN
    assert fn(5, s23.ctypes.data_as(P), 2, 1, 0.0, surf.ctypes.data_as(P), None) == ca.ERROR_BAD_DOMAIN
    assert fn(5, None, 3, 1, 0.0, surf.ctypes.data_as(P), None) == ca.ERROR_BAD_DOMAIN
    assert fn(5, s23.ctypes.data_as(P), 3, 1, 0.0, None, None) == ca.ERROR_BAD_DOMAIN
    with pytest.raises(ValueError):
        ca.stereo_triangulate(cams, np.zeros((2, 2)), np.zeros((3, 2)))


def window(rig_dicts, rng, n=21, stretch=(1.03, 0.98), self_good=True):
    """a window of n centres within 45 px of (120, 130) on the tilted plane, stretched in the plane, then turned and shifted"""
    c = np.float64([120.0, 130.0])
    d = rng.uniform(-45.0, 45.0, (n, 2))
    Pr = sr.on_plane(rig_dicts, c + d)
    t1, t2, nrm = sr.plane_basis()
    A = stretch[0] * np.outer(t1, t1) + stretch[1] * np.outer(t2, t2) + np.outer(nrm, nrm)
    Q = sr.rotation((0.3, 1.0, -0.2), 0.2)
    Pf = (Pr - Pr[0]) @ (Q @ A).T + Pr[0] + np.float64([3.0, -2.0, 5.0])
    return d[:, 0], d[:, 1], np.concatenate([Pr, Pf - Pr], 1)


def test_surface_from_sums_matches_the_restatement(rig):
    r, _ = rig
    rng = np.random.default_rng(9)
    for case in range(6):
        x, y, f6 = window(r, rng, n=5 + 8 * case)
        f6[:, 3:] += rng.normal(0, 1e-3, (len(x), 3))       # a misfit to be seen in the residual
        vals, status, _, _ = sr.surface_from_window(x, y, f6, 3, case % 2 == 0)
        sums = sr.window_sums(x, y, f6)
        _, planes = ca.stereo_surface_from_sums(len(x), sums, 3, case % 2 == 0, 0.0, return_planes=True)
        misfit = f6[:, 3:] - (planes[3:, 0] + x[:, None] * planes[3:, 1] + y[:, None] * planes[3:, 2])
        got = ca.stereo_surface_from_sums(len(x), sums, 3, case % 2 == 0, float((misfit ** 2).sum()))
        assert got["status"] == status == (ca.STEREO_SURFACE_OK if case % 2 == 0 else ca.STEREO_SURFACE_FILLED)
        assert got["neighbours"] == len(x) and not got["reserved"].any()
        ref = (vals[None, None], np.int32([[len(x)]]), np.int32([[status]]), None)
        worst = sr.check_surface(np.array([[got]]), ref, case)
        print(f"window of {len(x)}: exx {got['exx']:.6f} eyy {got['eyy']:.6f} exy {got['exy']:.2e}, worst error / tolerance {worst:.3g}")
        # the affine map is exact: E = diag((lambda^2 - 1) / 2) in the plane's own basis, up to the noise put in
        assert abs(got["e1"] - (1.03 ** 2 - 1) / 2) < 2e-4 and abs(got["e2"] - (0.98 ** 2 - 1) / 2) < 2e-4


def test_surface_statuses_from_sums(rig):
    r, _ = rig
    rng = np.random.default_rng(10)
    x, y, f6 = window(r, rng, n=12)
    few = ca.stereo_surface_from_sums(12, sr.window_sums(x, y, f6), 13, True)
    assert few["status"] == ca.STEREO_SURFACE_TOO_FEW and few["neighbours"] == 12
    line = ca.stereo_surface_from_sums(12, sr.window_sums(x, 0.5 * x + 3.0, f6), 3, True)      # the centres on a line
    flat = f6.copy()
    flat[:, :3] = np.outer(x + 0.5 * y, [0.5, 0.1, 0.2]) + [1.0, 2.0, 400.0]                   # the surface edge-on: both tangents along one line
    edge = ca.stereo_surface_from_sums(12, sr.window_sums(x, y, flat), 3, True)
    assert line["status"] == ca.STEREO_SURFACE_DEGENERATE and edge["status"] == ca.STEREO_SURFACE_DEGENERATE
    assert sr.surface_from_window(x, y, flat, 3, True)[1] == ca.STEREO_SURFACE_DEGENERATE
    for rec in (few, line, edge):
        for k in ca.STEREO_SURFACE_FLOATS:
            assert rec[k] == 0.0, k
    none = ca.stereo_surface_from_sums(0, np.zeros(23), 3, False)
    assert none["status"] == ca.STEREO_SURFACE_TOO_FEW and all(none[k] == 0.0 for k in ca.STEREO_SURFACE_FLOATS)


def test_rendered_rig_gives_the_plane_back_from_the_oracle_s_records(oracle):
    """The end-to-end conditions of tests/test_stereo_gpu.py, measured first where no GPU is needed: the CPU oracle solves
    camera 0's reference frame of stereo_ref.rig_frames() against camera 1's from the rounded true disparity, the restatement
    triangulates its good records and a plane is fitted to the points.  Measured: 128 of 143 sectors solved, rms distance from
    the plane 0.4061 world units (0.28 px of matching error at 1.44 units per pixel).  The GPU test asserts twice that rms and
    0.95 of that count (ORACLE_PLANE_RMS, ORACLE_GOOD below)."""
    from test_strain_gpu import grid_rects
    r = sr.make_rig()
    im0, im1 = sr.rig_frames(r)
    rects = grid_rects(n=13, columns=11)
    cen = np.float32([(17 + 19 * i, 17 + 19 * j) for i in range(11) for j in range(13)])
    o = oracle.Oracle(model=oracle.FM_UVUXUYVXVY, precision=1e-3, py_stop=2)
    o.set_image(0, im0)
    o.set_image(1, im1)
    rec = o.correlate_sectors([oracle.rect_points(*q) for q in rects], cen, sr.disparity_guess(r, cen))
    o.close()
    pts = sr.as_points(sr.triangulate(r, cen.astype(np.float64), sr.record_pixels(cen, rec)))
    pts["status"][~((rec["error_code"] == 0) & np.isfinite(rec["chi"]))] = ca.STEREO_BAD_RECORD
    rms, n = sr.plane_rms(pts)
    print(f"CPU oracle records, float64 restatement: {n} of 143 sectors good, rms distance from the fitted plane {rms:.4f} units")
    assert n == ORACLE_GOOD and abs(rms - ORACLE_PLANE_RMS) <= 1e-3


ORACLE_PLANE_RMS, ORACLE_GOOD = 0.4061, 128
