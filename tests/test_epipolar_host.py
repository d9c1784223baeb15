"""The epipolar curve table on the host (lk_epipolar_curves, include/lk_engine.h) against the float64 restatement of
tests/epipolar_ref.py, and what the search along it has to deliver, measured where no GPU is needed: the brute force of the
search on the CPU oracle's pyramid, its guesses solved by the CPU oracle.  No GPU.  The tolerances are derived in
epipolar_ref's docstring."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi
import epipolar_ref as er
import stereo_ref as sr

NORMAL = (0.25, -0.15, 1.0)      # stereo_ref.on_plane's
Z_NEAR, Z_FAR = 340.0, 460.0
CEN = np.float32([(17 + 19 * i, 17 + 19 * j) for i in range(11) for j in range(13)])   # tests/test_stereo_gpu.py's grid


def vertical_rig():
    """stereo_ref's rig with camera 1 above camera 0 instead of beside it: the curves run along y"""
    c1 = np.float64([0.0, sr.Z0 * np.sin(sr.ANGLE), sr.Z0 * (1.0 - np.cos(sr.ANGLE))])
    z = np.float64([0.0, 0.0, sr.Z0]) - c1
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    r = sr.make_rig()
    return [r[0], dict(r[1], R=R, t=-R @ c1)]


@pytest.fixture(scope="module")
def rig(engine_lib):
    r = sr.make_rig()
    return r, sr.as_records(r)


def test_layouts_and_symbols(engine_lib):
    S = _ffi.LkEpipolarSearch
    assert C.sizeof(S) == 80 and [getattr(S, k).offset for k in ("search", "n_nodes", "shape", "reserved", "z_near", "z_far", "normal")] == \
        [0, 20, 24, 28, 40, 48, 56]
    d = ca.EPIPOLAR_CURVE_DTYPE
    assert d.itemsize == 32 and [d.fields[k][1] for k in ("axis", "first_station", "n_stations", "first_index", "status", "reserved")] == \
        [0, 4, 8, 12, 16, 20]
    d = ca.EPIPOLAR_MATCH_DTYPE
    assert d.itemsize == 64 and [d.fields[k][1] for k in ("shift_x", "shift_y", "station", "band_offset", "node", "n_samples", "n_valid",
                                                           "status", "score", "runner_up", "station_refined", "inv_depth", "reserved")] == \
        [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 52, 56]
    assert (ca.GS_NO_CURVE, ca.GS_TOO_LONG) == (6, 7)
    assert (ca.EP_MAX_BAND, ca.EP_MAX_NODES, ca.EP_MAX_STATIONS, ca.EP_MAX_GROUP) == (8, 33, 2048, 4096)
    for name in ("lk_search_epipolar", "lk_get_epipolar_search_info", "lk_get_epipolar_search_profile", "lk_epipolar_curves",
                 "lk_internal_epipolar_last"):
        assert hasattr(engine_lib, name), name
    blob = open(ca.LIB_PATH, "rb").read()
    assert b"lk_epipolar_search_kernel" in blob and b"lk_epipolar_reduce_kernel" in blob


@pytest.mark.parametrize("which", ["horizontal", "vertical"])
@pytest.mark.parametrize("level", [0, 1])
def test_curves_match_the_restatement(engine_lib, which, level):
    r = sr.make_rig() if which == "horizontal" else vertical_rig()
    cen = CEN + np.float32([0.37, -0.21])     # (off the grid: an end coordinate on an integer would be a tie between the two sides)
    t = ca.epipolar_curves(sr.as_records(r), cen, Z_NEAR, Z_FAR, level)
    assert (t["curves"]["status"] == 0).all() and not t["curves"]["reserved"].any()
    assert t["curves"]["first_index"][0] == 0 and (np.diff(t["curves"]["first_index"]) == t["curves"]["n_stations"][:-1]).all()
    assert len(t["other"]) == t["curves"]["n_stations"].sum()
    for s in range(len(cen)):
        c, cv = er.curve(r, cen[s], Z_NEAR, Z_FAR, level), t["curves"][s]
        a = c["w"][:, c["axis"]]
        # the test's own inputs: no end coordinate within 1e-9 of an integer, no `other` within 1e-9 of a half
        assert np.abs(a[[0, -1]] - np.rint(a[[0, -1]])).min() > 1e-9
        assert np.abs(c["other_real"] + 0.5 - np.rint(c["other_real"] + 0.5)).min() > 1e-9
        assert c["axis"] == (0 if which == "horizontal" else 1)
        assert (cv["axis"], cv["first_station"], cv["n_stations"]) == (c["axis"], c["first"], c["count"]), (s, cv, c)
        f, n = cv["first_index"], cv["n_stations"]
        assert np.abs(t["other"][f:f + n] - c["other_real"]).max() <= 0.5 + 1e-9
        assert np.array_equal(t["node"][f:f + n], c["node"])
        assert np.abs(t["inv_depth"][f:f + n] / c["inv_depth"] - 1.0).max() <= 1e-12
        rho = t["inv_depth"][f:f + n]              # inside the range, and running one way along the stations
        assert rho.min() >= 1.0 / Z_FAR and rho.max() <= 1.0 / Z_NEAR and ((np.diff(rho) > 0).all() or (np.diff(rho) < 0).all())


def test_per_sector_depth_ranges(rig):
    r, cams = rig
    dr = np.stack([np.linspace(300.0, 380.0, len(CEN)), np.linspace(420.0, 600.0, len(CEN))], 1)
    t = ca.epipolar_curves(cams, CEN, 1.0, 2.0, 1, depth_range=dr)       # (the configuration's own range is not read)
    for s in (0, 50, 142):
        one = ca.epipolar_curves(cams, CEN[s:s + 1], dr[s, 0], dr[s, 1], 1)
        cv, f = t["curves"][s], t["curves"][s]["first_index"]
        assert (cv["first_station"], cv["n_stations"]) == (one["curves"][0]["first_station"], one["curves"][0]["n_stations"])
        for k in ("other", "node", "inv_depth"):
            assert t[k][f:f + cv["n_stations"]].tobytes() == one[k].tobytes()


@pytest.mark.parametrize("level", [0, 1])
def test_band_one_covers_every_depth_of_the_range(rig, level):
    """The projection of the ray's point at any depth of the range lies within one level-L pixel (Chebyshev) of a candidate at
    band 1.  Why: the nearest station is at most 0.5 away along the axis (a depth between the end stations) or less than 1 (a
    depth beyond them, before the end node); across, the station's `other` is off the curve by its rounding, 0.5, by the chord
    error of 17 nodes, and by the curve's slope over the distance along, <= 0.5 |slope|: 1 + chord at most for |slope| <= 1,
    which the band's +-1 brings to 0.5 (chord is computed below from the restatement, at the middle of every segment)."""
    r, cams = rig
    t = ca.epipolar_curves(cams, CEN, Z_NEAR, Z_FAR, level, band=1)
    worst, chord_worst = 0.0, 0.0
    for s in range(0, len(CEN), 3):
        c, cv = er.curve(r, CEN[s], Z_NEAR, Z_FAR, level), t["curves"][s]
        rho_mid = 0.5 * (c["rho"][1:] + c["rho"][:-1])
        mid = np.array([er.point_on_ray(r, CEN[s], 1.0 / q) for q in rho_mid])
        mid = (mid - CEN[s].astype(np.float64)) / (1 << level)
        seg = c["w"][1:] - c["w"][:-1]
        rel = mid - c["w"][:-1]
        chord = np.abs(rel[:, 0] * seg[:, 1] - rel[:, 1] * seg[:, 0]) / np.linalg.norm(seg, axis=1)
        slope = np.abs(seg[:, 1 - c["axis"]] / seg[:, c["axis"]]).max()
        chord_worst = max(chord_worst, float(chord.max()))
        assert slope <= 1.0 and 0.5 + chord.max() + 0.5 * slope <= 1.5
        f, n = cv["first_index"], cv["n_stations"]
        along = cv["first_station"] + np.arange(n)
        for q in 1.0 / np.linspace(1.0 / Z_NEAR, 1.0 / Z_FAR, 97):
            p = (er.point_on_ray(r, CEN[s], q) - CEN[s].astype(np.float64)) / (1 << level)
            pa, pb = p[c["axis"]], p[1 - c["axis"]]
            d = np.minimum.reduce([np.maximum(np.abs(along - pa), np.abs(t["other"][f:f + n] + b - pb)) for b in (-1, 0, 1)])
            worst = max(worst, float(d.min()))
    print(f"level {level}: farthest point of a curve from its nearest band-1 candidate {worst:.3f} px; chord error of 17 nodes {chord_worst:.2e} px")
    assert worst <= 1.0


def test_shape_matrices(rig):
    r, cams = rig
    t = ca.epipolar_curves(cams, CEN, Z_NEAR, Z_FAR, 0, shape=1, normal=NORMAL)
    assert t["shape"].shape == (len(CEN), 17, 4) and (t["curves"]["status"] == 0).all()
    for s in range(0, len(CEN), 5):
        c = er.curve(r, CEN[s], Z_NEAR, Z_FAR, 0, shape=1, normal=NORMAL)
        assert (np.abs(t["shape"][s] - c["A"]) <= 2.0 ** -23 * np.abs(c["A"]) + er.SHAPE_TOL_ABS).all(), s
        truth = er.shape_matrices(r, CEN[s], c["P"], NORMAL, h=1e-3)
        assert (np.abs(t["shape"][s] - truth) <= 2.0 ** -23 * np.abs(truth) + er.SHAPE_TRUTH_TOL).all(), s
    # the optical axis of camera 0 is the default normal
    axis = ca.epipolar_curves(cams, CEN[:3], Z_NEAR, Z_FAR, 0, shape=1)
    named = ca.epipolar_curves(cams, CEN[:3], Z_NEAR, Z_FAR, 0, shape=1, normal=r[0]["R"][2])
    assert axis["shape"].tobytes() == named["shape"].tobytes()
    # a fronto-parallel plane seen by a camera turned about Y: a11 below one, a22 near one
    assert (np.abs(axis["shape"][:, :, 0] - np.cos(sr.ANGLE)) < 0.08).all() and (np.abs(axis["shape"][:, :, 3] - 1.0) < 0.05).all()


def test_equal_depths_give_one_station(rig):
    r, cams = rig
    for level in (0, 1, 2):
        t = ca.epipolar_curves(cams, CEN, 400.0, 400.0, level, n_nodes=5)
        assert (t["curves"]["status"] == 0).all() and (t["curves"]["n_stations"] == 1).all()
        for s in (0, 71, 142):
            w = (er.point_on_ray(r, CEN[s], 400.0) - CEN[s].astype(np.float64)) / (1 << level)
            cv = t["curves"][s]
            assert cv["axis"] == 0 and cv["first_station"] == np.floor(w[0] + 0.5) and t["other"][cv["first_index"]] == np.floor(w[1] + 0.5)
            assert 0 <= t["node"][cv["first_index"]] <= 4 and t["inv_depth"][cv["first_index"]] == 1.0 / 400.0


def test_every_curve_status(rig):
    r, cams = rig
    strong = dict(cx=128.0, cy=128.0, rn=60.0, k1=-0.5, k2=0.0, p1=0.0, p2=0.0)    # folds back at 0.82 rn = 49 px from its centre

    def statuses(rig_, *a, **kw):
        t = ca.epipolar_curves(sr.as_records(rig_), CEN, *a, **kw)
        want = np.int32([er.curve(rig_, c, *a, **kw)["status"] for c in CEN])
        assert np.array_equal(t["curves"]["status"], want), np.flatnonzero(t["curves"]["status"] != want)
        bad = t["curves"]["status"] != 0
        assert not t["curves"]["n_stations"][bad].any() and len(t["other"]) == t["curves"]["n_stations"].sum()
        return t["curves"]["status"]
    # the centre outside camera 0's lens
    got = statuses([dict(r[0], lens=strong), r[1]], Z_NEAR, Z_FAR, 0)
    assert (got == ca.GS_NO_CURVE).sum() > 50 and (got == 0).sum() > 5
    # a node behind camera 1: camera 1 looks away from the scene
    back = dict(r[1], R=np.diag([-1.0, 1.0, -1.0]) @ r[1]["R"], t=np.diag([-1.0, 1.0, -1.0]) @ r[1]["t"])
    assert (statuses([r[0], back], Z_NEAR, Z_FAR, 0) == ca.GS_NO_CURVE).all()
    # node coordinates that are not monotone: camera 1's lens folds the far end of a long curve back
    got = statuses([r[0], dict(r[1], lens=strong)], 150.0, 2000.0, 0)
    assert (got == ca.GS_NO_CURVE).sum() > 50
    # a shape point that fails, 1: a grazing normal.  Camera 0 has R = I, so with the normal (1, 0, 0) d . n changes its sign
    # where the undistorted x passes cx = 127.5: between c - ex and c + ex of the centres at x = 127.7 and 127.2 one neighbour
    # meets the plane behind the camera (z <= 0); the centres further off do not
    graze = np.float32([[127.7, 100.0], [127.2, 60.0], [100.0, 100.0], [126.4, 200.0], [129.5, 30.0]])
    cfg = dict(shape=1, normal=(1.0, 0.0, 0.0))
    t = ca.epipolar_curves(cams, graze, Z_NEAR, Z_FAR, 0, **cfg)
    assert [er.curve(r, c, Z_NEAR, Z_FAR, 0, **cfg)["status"] for c in graze] == [ca.GS_NO_CURVE, ca.GS_NO_CURVE, 0, 0, 0]
    assert t["curves"]["status"].tolist() == [ca.GS_NO_CURVE, ca.GS_NO_CURVE, 0, 0, 0]
    assert not t["curves"]["n_stations"][:2].any() and t["curves"]["n_stations"][2:].all() and len(t["other"]) == t["curves"]["n_stations"].sum()
    assert not t["shape"][:2].any() and t["shape"][2:].any(axis=(1, 2)).all()        # a failed sector's matrices are zeros
    assert (ca.epipolar_curves(cams, graze, Z_NEAR, Z_FAR, 0, shape=0, normal=(1.0, 0.0, 0.0))["curves"]["status"] == 0).all()
    # ... 2: the lens's edge.  Under the strong lens some centres are inside camera 0's lens with a neighbour one pixel away
    # outside it: a curve without shape, NO_CURVE with it
    edge = [dict(r[0], lens=strong), r[1]]
    plain, shaped = statuses(edge, Z_NEAR, Z_FAR, 0), statuses(edge, Z_NEAR, Z_FAR, 0, shape=1)
    assert ((plain == 0) & (shaped == ca.GS_NO_CURVE)).sum() >= 2 and not ((plain != 0) & (shaped == 0)).any()
    # more than LK_EP_MAX_STATIONS stations; a run of one node above LK_EP_MAX_GROUP candidates (and the same curve at band 0)
    assert (statuses(r, 10.0, 460.0, 0) == ca.GS_TOO_LONG).all()
    assert (statuses(r, 100.0, 1000.0, 0, band=8, n_nodes=2) == ca.GS_TOO_LONG).all()
    assert (statuses(r, 100.0, 1000.0, 0, band=0, n_nodes=2) == 0).all()


def test_refusals(rig):
    r, cams = rig

    def refused(cams_=cams, cen=CEN, level=1, depth_range=None, **kw):
        args = dict(dict(z_near=Z_NEAR, z_far=Z_FAR, band=1, n_nodes=17, shape=0, normal=None), **kw)
        with pytest.raises(ValueError):
            ca.epipolar_curves(cams_, cen, args.pop("z_near"), args.pop("z_far"), level, depth_range=depth_range, **args)
    for kw in (dict(band=-1), dict(band=9), dict(n_nodes=1), dict(n_nodes=34), dict(shape=2), dict(shape=-1), dict(z_near=0.0),
               dict(z_near=-1.0), dict(z_near=500.0), dict(z_far=np.inf), dict(z_near=np.nan), dict(normal=(np.nan, 0.0, 1.0)),
               dict(level=-1), dict(level=31)):
        refused(**kw)
    for bad in ((0.0, 400.0), (400.0, 300.0), (300.0, np.inf), (np.nan, 400.0)):
        dr = np.tile([Z_NEAR, Z_FAR], (len(CEN), 1))
        dr[7] = bad
        refused(depth_range=dr)
    broken = np.array([cams[0], cams[1]], ca.CAMERA_DTYPE)       # (copies: the fixture's records stay as they are)
    broken["fx"][1] = 0.0
    refused(cams_=[cams[0], broken[1]])
    broken["reserved"][0, 3] = 1.0
    refused(cams_=[broken[0], cams[1]])
    cfg = _ffi.epipolar_config(Z_NEAR, Z_FAR, 1)
    cfg.reserved[1] = 1
    with pytest.raises(ValueError):
        ca.epipolar_curves(cams, CEN, Z_NEAR, Z_FAR, 1, cfg=cfg)
    lib, out, n = ca.load_library(), np.zeros(1, ca.EPIPOLAR_CURVE_DTYPE), C.c_int(0)
    cfg = _ffi.epipolar_config(Z_NEAR, Z_FAR, 1)
    rig2, one = _ffi._rig(cams), np.float32([[100.0, 100.0]])
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ok = lambda *a: lib.lk_epipolar_curves(*a)  # noqa: E731
    assert ok(C.byref(cfg), p(rig2), 1, _ffi.fptr(one), None, 1, p(out), C.byref(n), 0, None, None, None, None) == 0 and n.value > 3
    assert ok(C.byref(cfg), None, 1, _ffi.fptr(one), None, 1, p(out), C.byref(n), 0, None, None, None, None) == ca.ERROR_BAD_DOMAIN
    assert ok(None, p(rig2), 1, _ffi.fptr(one), None, 1, p(out), C.byref(n), 0, None, None, None, None) == ca.ERROR_BAD_DOMAIN
    assert ok(C.byref(cfg), p(rig2), 0, _ffi.fptr(one), None, 1, p(out), C.byref(n), 0, None, None, None, None) == ca.ERROR_BAD_DOMAIN
    assert ok(C.byref(cfg), p(rig2), 1, None, None, 1, p(out), C.byref(n), 0, None, None, None, None) == ca.ERROR_BAD_DOMAIN
    small = np.zeros(2, np.int32)
    assert ok(C.byref(cfg), p(rig2), 1, _ffi.fptr(one), None, 1, p(out), C.byref(n), 2, p(small), p(small), p(np.zeros(2)),
              None) == ca.ERROR_BAD_DOMAIN                                                  # (a capacity that is too small)


# ---- what the search has to deliver, on the CPU ---------------------------------------------------------------------------------
def cpu_levels(oracle, im0, im1, rects, level):
    und, dfm, pts = im0, im1, [oracle.rect_points(*q) for q in rects]
    for _ in range(level):
        und, dfm, pts = oracle.pyramid_level(und), oracle.pyramid_level(dfm), [oracle.decimate(p, 1) for p in pts]
    return und, dfm, pts


def test_the_oracle_recovers_the_plane_from_the_brute_force_s_guesses(oracle, rig):
    """The end-to-end conditions of tests/test_epipolar_gpu.py, established before any GPU run: the brute force of the search
    (level 1, band 1, depth 340 .. 460) on the CPU oracle's pyramid of stereo_ref.rig_frames(), its guesses solved by the CPU
    oracle, the restatement's triangulation, the plane through the points.  Measured (profiles/epipolar_recovery.txt): 127 of
    143 sectors good, rms distance from the plane 0.4091 units - inside the floor 0.95 ORACLE_GOOD = 121.6 and the bound
    2 ORACLE_PLANE_RMS = 0.8122 of tests/test_stereo_gpu.py, with no outlier pass and no reseeding."""
    from test_stereo_host import ORACLE_GOOD, ORACLE_PLANE_RMS
    from test_strain_gpu import grid_rects
    r, cams = rig
    im0, im1 = sr.rig_frames(r)
    rects = grid_rects(n=13, columns=11)
    und, dfm, pts = cpu_levels(oracle, im0, im1, rects, 1)
    m, _, g, t = er.brute_force_arrays(und, dfm, pts, CEN, cams, np.zeros((len(CEN), 6), np.float32), 1, 1, Z_NEAR, Z_FAR)
    off = np.abs(g[:, :2] - sr.disparity_guess(r, CEN)[:, :2]).max(axis=1)
    o = oracle.Oracle(model=oracle.FM_UVUXUYVXVY, precision=1e-3, py_stop=2)
    o.set_image(0, im0)
    o.set_image(1, im1)
    rec = o.correlate_sectors([oracle.rect_points(*q) for q in rects], CEN, g)
    o.close()
    p = sr.as_points(sr.triangulate(r, CEN.astype(np.float64), sr.record_pixels(CEN, rec)))
    p["status"][~((rec["error_code"] == 0) & np.isfinite(rec["chi"]))] = ca.STEREO_BAD_RECORD
    rms, n = sr.plane_rms(p)
    print(f"brute force, level 1, band 1, depth {Z_NEAR:g} .. {Z_FAR:g}: {t['curves']['n_stations'].mean() * 3:.1f} candidates per sector, "
          f"statuses {np.bincount(m['status']).tolist()}, within 4 px of the true disparity in {(off <= 4).sum()} sectors; CPU oracle from "
          f"its guesses: {n} of 143 good, rms distance from the fitted plane {rms:.4f} units")
    assert n >= 0.95 * ORACLE_GOOD and rms <= 2 * ORACLE_PLANE_RMS


def test_the_plane_induced_shape_helps_on_a_wide_rig(oracle, engine_lib):
    """stereo_ref's rig opened to 35 degrees: the count of sectors the brute force puts within 4 px of the true disparity with
    shape 1 is at least the count with shape 0 (measured: 134 against 123, median scores 0.857 against 0.773)."""
    from test_strain_gpu import grid_rects
    r = sr.make_rig(angle=np.deg2rad(35))
    cams = sr.as_records(r)
    im0, im1 = sr.rig_frames(r)
    und, dfm, pts = cpu_levels(oracle, im0, im1, grid_rects(n=13, columns=11), 1)
    count, score = [], []
    for shape in (0, 1):
        m, _, g, _ = er.brute_force_arrays(und, dfm, pts, CEN, cams, np.zeros((len(CEN), 6), np.float32), 1, 1, Z_NEAR, Z_FAR, shape=shape,
                                           normal=NORMAL)
        off = np.abs(g[:, :2] - sr.disparity_guess(r, CEN)[:, :2]).max(axis=1)
        ok = m["status"] == ca.GS_OK
        count.append(int(((off <= 4) & ok).sum()))
        score.append(float(np.median(m["score"][ok])))
    print(f"35 degrees, level 1, band 1: within 4 px of the true disparity: shape 0 {count[0]}, shape 1 {count[1]}; median scores "
          f"{score[0]:.3f}, {score[1]:.3f}")
    assert count[1] >= count[0]
