"""The stereo initial guess along the epipolar curve (lk_search_epipolar): match, profile and guesses of every sector, byte for
byte, against the numpy brute force of tests/epipolar_ref.py on the engine's own pyramid levels and sample lists, fed by the
library's own curve table; the degenerate case against lk_search_guesses; invariance across batches, modes and other sectors'
depth ranges; status paths; and what the pass is for - the plane of tests/test_stereo_gpu.py's rendered rig recovered without
an outlier pass and without reseeding."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
import epipolar_ref as er
import stereo_ref as sr
from test_epipolar_host import CEN, NORMAL, Z_FAR, Z_NEAR, vertical_rig
from test_strain_gpu import grid_rects, make_engine

pytestmark = pytest.mark.gpu

F32 = np.float32
RECTS = grid_rects(n=13, columns=11)     # 11 x 13 sectors of 19 x 19, tests/test_stereo_gpu.py's


@pytest.fixture(scope="module")
def rig():
    r = sr.make_rig()
    return r, sr.as_records(r), sr.rig_frames(r)


def arbitrary_guesses(S, seed=3):
    """six words per sector that no search would write: whatever stays must stay bit for bit"""
    return (np.random.default_rng(seed).standard_normal((S, 6)) * 3.0).astype(F32)


def check(e, cams, level, band, z_near=Z_NEAR, z_far=Z_FAR, g=None, dfm=None, def_slot=-1, **kw):
    """run search_epipolar and compare every byte with the brute force; -> (matches, guesses, curves, profile)"""
    g = arbitrary_guesses(e.n_sectors) if g is None else g
    got = e.search_epipolar(cams, z_near, z_far, level=level, band=band, guesses=g, def_slot=def_slot, **kw)
    info = e.epipolar_search_info()
    curves, prof = e.epipolar_search_profile()
    assert got.tobytes() == e.get_guesses().tobytes()
    want_m, want_p, want_g, table = er.brute_force(e, cams, g, level, band, z_near, z_far, dfm=dfm, **kw)
    assert curves.tobytes() == table["curves"].tobytes()
    for s in range(e.n_sectors):
        assert info[s].tobytes() == want_m[s].tobytes(), (s, info[s], want_m[s])
        assert got[s].tobytes() == want_g[s].tobytes(), (s, got[s], want_g[s])
    assert prof.tobytes() == want_p.tobytes()
    quiet = info["status"] != ca.GS_OK
    assert got[quiet].tobytes() == g[quiet].tobytes()
    dead = ~np.isin(info["status"], (ca.GS_OK, ca.GS_WEAK))
    for k in ("shift_x", "shift_y", "station", "band_offset", "node", "n_valid", "station_refined", "inv_depth"):
        assert not info[k][dead].any(), k
    assert (info["score"][dead] == -2.0).all() and (info["runner_up"][dead] == -2.0).all() and not info["reserved"].any()
    return info, got, curves, prof


# ---- bytes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", [0, 2])
@pytest.mark.parametrize("level", [0, 1])
def test_rect_grid_matches_the_brute_force(rig, level, band):
    r, cams, (im0, im1) = rig
    with make_engine(im0, im1, RECTS) as e:
        info, got, curves, _ = check(e, cams, level, band)
        ok = info["status"] == ca.GS_OK
        off = np.abs(got[:, :2] - sr.disparity_guess(r, CEN)[:, :2]).max(axis=1)
        assert ok.sum() >= 130 and (off[ok] <= 4).mean() > 0.9
        assert got[ok, 2:].tobytes() == arbitrary_guesses(e.n_sectors)[ok, 2:].tobytes()       # shape 0: g[2..5] stay
        # border sectors: one with none of its candidates inside camera 1's frame, one with part of them
        total = curves["n_stations"] * (2 * band + 1)
        assert (info["status"] == ca.GS_NO_CANDIDATE).any() and ((info["n_valid"] > 0) & (info["n_valid"] < total)).any()


@pytest.mark.parametrize("model", [ca.FM_UV, ca.FM_UVQ])
def test_models_without_a_matrix(rig, model):
    r, cams, (im0, im1) = rig
    with make_engine(im0, im1, RECTS[:40], model=model) as e:
        info, _, _, _ = check(e, cams, 1, 1)
        assert (info["status"] == ca.GS_OK).sum() >= 30


@pytest.mark.parametrize("level", [0, 1])
def test_shape_one_maps_the_template(rig, level):
    r, cams, (im0, im1) = rig
    with make_engine(im0, im1, RECTS) as e:
        info, got, _, _ = check(e, cams, level, 1, shape=1, normal=NORMAL)
        ok = info["status"] == ca.GS_OK
        assert ok.sum() >= 130 and (np.abs(got[ok, 2] - (np.cos(sr.ANGLE) - 1.0)) < 0.15).all()


def test_curves_along_y(rig):
    r = vertical_rig()
    im0, im1 = sr.rig_frames(r)
    with make_engine(im0, im1, RECTS[:60]) as e:
        info, got, curves, _ = check(e, sr.as_records(r), 1, 1)
        ok = info["status"] == ca.GS_OK
        off = np.abs(got[:, :2] - sr.disparity_guess(r, CEN[:60])[:, :2]).max(axis=1)
        assert (curves["axis"] == 1).all() and ok.sum() >= 50 and (off[ok] <= 4).mean() > 0.9


@pytest.mark.parametrize("level", [0, 1])
def test_the_cut_into_runs_changes_no_byte(rig, level, monkeypatch):
    """Without shape a curve is cut into stretches of up to 1024 candidates; LK_EPIPOLAR_RUNS=1 cuts it by node as with shape
    (the decomposition scripts/epipolar_bench.py times against): both against the brute force, and against each other."""
    r, cams, (im0, im1) = rig
    with make_engine(im0, im1, RECTS) as e:
        out = []
        for hook in (None, "1"):
            if hook:
                monkeypatch.setenv("LK_EPIPOLAR_RUNS", hook)
            info, got, curves, prof = check(e, cams, level, 1)
            out.append((info.tobytes(), got.tobytes(), prof.tobytes(), e.epipolar_last()[5]))
        assert out[0][:3] == out[1][:3]
        assert out[0][3] == curves["n_stations"].max() and out[1][3] <= 2 + out[0][3] // 16       # whole curves; a node's few stations


def test_per_sector_depth_ranges(rig):
    r, cams, (im0, im1) = rig
    with make_engine(im0, im1, RECTS) as e:
        z = sr.on_plane(r, CEN)[:, 2]
        dr = np.stack([z - 15.0, z + 15.0], 1)
        info, got, curves, _ = check(e, cams, 1, 1, 1.0, 2.0, depth_range=dr)      # (the call's own range is not read)
        assert curves["n_stations"].max() <= 12 and (info["status"] == ca.GS_OK).sum() >= 130


def test_large_sectors_two_chunks_and_the_window_read_in_place(rig):
    r, cams, (im0, im1) = rig
    # 41 x 41 = 1681 samples: two template chunks; 210 x 210 with 2 nodes and band 8: runs of some 30 stations, a window of
    # (209 + 30) x (209 + 17 + the curve's own rise) bytes, above what the scores and the chunk leave of 64 KB
    with make_engine(im0, im1, [(100, 100, 140, 140), (23, 23, 232, 232)]) as e:
        info, _, _, _ = check(e, cams, 0, 1)
        assert info["n_samples"].tolist() == [1681, 44100] and info["status"][0] == ca.GS_OK
        info, _, curves, _ = check(e, cams, 0, 8, n_nodes=2)
        _, _, _, candidates, win_bytes, max_run = e.epipolar_last()
        assert info["status"].tolist() == [ca.GS_OK, ca.GS_OK] and info["n_valid"][1] > 100
        assert candidates == curves["n_stations"].sum() * 17 and max_run >= 25
        # the window of the large sector's runs (every candidate of a sector in the middle of the frame is inside) is read in place
        assert (209 + max_run) * (209 + 17) > win_bytes


def test_annular_blob_and_float_point_sectors(rig):
    r, cams, (im0, im1) = rig
    e = ca.HipCorrelationEngine(py_stop=2)
    e.set_undeformed_image(im0)
    e.set_deformed_image(im1)
    s = 0
    for k in range(4):
        e.resetPolygon_annular(s, 40.0, 30.0, 0.3 + k * 1.5, 0.9, 128.0, 125.0, 4)
        s += 1
    ang = 2 * np.pi * np.arange(24) / 24
    e.resetPolygon_blob(s, np.stack([128.3 + 70 * np.cos(ang), 127.7 + 60 * np.sin(ang)], 1).astype(F32))
    s += 1
    rng = np.random.default_rng(5)
    for k in range(3):   # float lists: the rounding rule
        e.set_sector_points(s, (rng.random((300, 2)) * 30 + 60 + 40 * k).astype(F32))
        s += 1
    e.commit_sectors()
    for level in (0, 1, 2):
        info, _, _, _ = check(e, cams, level, 1)
        assert (info["status"] == ca.GS_OK).sum() >= 6
    e.close()


def test_ring_slot_as_the_deformed_image(rig):
    r, cams, (im0, im1) = rig
    with make_engine(im0, im0, RECTS[:40]) as e:          # (LK_IMG_DEF holds camera 0's own frame: not what is searched)
        e.sequence_reserve(3)
        e.sequence_set_frame(2, im1)
        probe = ca.HipCorrelationEngine(py_stop=2)
        probe.set_undeformed_image(im1)
        ring_l1 = probe.get_pyramid_level(ca.IMG_UND, 1)
        probe.close()
        info, got, _, _ = check(e, cams, 1, 1, dfm=ring_l1, def_slot=2)
        ok = info["status"] == ca.GS_OK
        off = np.abs(got[:, :2] - sr.disparity_guess(r, CEN[:40])[:, :2]).max(axis=1)
        assert ok.sum() >= 30 and (off[ok] <= 4).mean() > 0.9


# ---- against the existing search --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1])
def test_one_candidate_equals_the_plain_search_with_radius_zero(rig, level):
    r, cams, (im0, im1) = rig
    with make_engine(im0, im1, RECTS) as e:
        g = arbitrary_guesses(e.n_sectors)
        got = e.search_epipolar(cams, 400.0, 400.0, level=level, band=0, guesses=g)
        m = e.epipolar_search_info()
        curves, prof = e.epipolar_search_profile()
        assert (curves["n_stations"] == 1).all() and prof.tobytes() == m["score"].tobytes()
        about = g.copy()
        about[:, 0], about[:, 1] = m["shift_x"] * F32(1 << level), m["shift_y"] * F32(1 << level)
        plain_g = e.search_guesses(0, level=level, guesses=about)
        p = e.guess_search_info()
        has = np.isin(m["status"], (ca.GS_OK, ca.GS_WEAK))
        assert has.sum() >= 130 and (m["status"] == ca.GS_NO_CANDIDATE).any()
        assert np.array_equal(p["center_x"][has], m["shift_x"][has]) and np.array_equal(p["center_y"][has], m["shift_y"][has])
        assert not p["shift_x"].any() and not p["shift_y"].any()
        for k in ("n_samples", "n_valid", "status", "score"):
            assert p[k][has].tobytes() == m[k][has].tobytes(), k
        assert (m["n_valid"][has] == 1).all() and (m["runner_up"] == -2.0).all()
        ok = m["status"] == ca.GS_OK
        assert got[ok].tobytes() == plain_g[ok].tobytes() and got[~ok].tobytes() == g[~ok].tobytes()


# ---- the same bytes anywhere --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "batch_invariant", "reference_order"])
def test_a_sector_gets_the_same_bits_in_any_batch_and_mode(rig, mode):
    r, cams, (im0, im1) = rig
    z = sr.on_plane(r, CEN)[:, 2]
    ranges = np.stack([z - 40.0, z + 60.0], 1)

    def run(first, count, dr):
        e = ca.HipCorrelationEngine(py_stop=2)
        if mode == "batch_invariant":
            e.set_batch_invariant(True)
        elif mode == "reference_order":
            e.set_reference_order(1)
        e.set_undeformed_image(im0)
        e.set_deformed_image(im1)
        for s, q in enumerate(RECTS[first:first + count]):
            e.resetPolygon_rect(s, *q)
        e.commit_sectors()
        g = arbitrary_guesses(143)[first:first + count]
        out = []
        for _ in range(2):
            got = e.search_epipolar(cams, Z_NEAR, Z_FAR, level=1, band=1, shape=1, normal=NORMAL, guesses=g,
                                    depth_range=dr[first:first + count])
            curves, prof = e.epipolar_search_profile()
            out.append((got, e.epipolar_search_info(), [prof[c["first_index"]:c["first_index"] + c["n_stations"]].tobytes() for c in curves]))
        e.close()
        assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes() and out[0][2] == out[1][2]
        return out[0]

    full = run(0, 143, ranges)
    halves = [run(0, 70, ranges), run(70, 73, ranges)]
    assert np.concatenate([halves[0][0], halves[1][0]]).tobytes() == full[0].tobytes()
    assert np.concatenate([halves[0][1], halves[1][1]]).tobytes() == full[1].tobytes()
    assert halves[0][2] + halves[1][2] == full[2]
    for s in (0, 71, 142):
        one = run(s, 1, ranges)
        assert one[0].tobytes() == full[0][s:s + 1].tobytes() and one[1].tobytes() == full[1][s:s + 1].tobytes() and one[2] == full[2][s:s + 1]
    moved = ranges * np.where(np.arange(143) % 2 == 0, 1.0, 1.3)[:, None]      # the odd sectors' ranges change, the even ones' stay
    other = run(0, 143, moved)
    even = np.arange(0, 143, 2)
    assert other[0][even].tobytes() == full[0][even].tobytes() and other[1][even].tobytes() == full[1][even].tobytes()
    assert [other[2][s] for s in even] == [full[2][s] for s in even]
    assert other[1][1::2].tobytes() != full[1][1::2].tobytes()


# ---- status paths -------------------------------------------------------------------------------------------------------------------
def device_records(e):
    """the engine-held records, copied from the device"""
    d = C.c_void_p()
    assert e.lib.lk_get_results_device(e._h, C.byref(d)) == 0
    out = np.zeros(e.n_sectors, ca.RESULT_DTYPE)
    assert e.lib.lk_synchronize(e._h) == 0
    hip = C.CDLL("libamdhip64.so")   # the runtime the engine library itself is linked to
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), d, out.nbytes, 2) == 0
    return out


def test_status_paths_and_nothing_else_moves(rig):
    r, cams, (im0, im1) = rig
    und = im0.copy()
    und[100:140, 100:140] = 77                      # a uniform patch
    rects = [(105, 105, 134, 134),                  # TEXTURELESS
             (236, 2, 254, 20),                     # in a corner: every candidate leaves camera 1's frame
             (200, 200, 202, 201),                  # 6 samples at level 0: TOO_FEW
             (150, 60, 168, 78),                    # an ordinary sector (WEAK with min_score 2)
             (60, 150, 78, 168)]                    # another: NO_CURVE or TOO_LONG by its own depth range
    with make_engine(und, im1, rects) as e:
        g = arbitrary_guesses(5)
        rec0 = e.correlate_all(g)
        # (the counters of lk_get_stats; its two times are read back from events and their last digits differ between two reads)
        state = lambda: ({k: v for k, v in e.stats().items() if not k.endswith("_ms")}, e.get_pyramid_level(ca.IMG_UND, 0), e.get_pyramid_level(ca.IMG_DEF, 1),  # noqa: E731
                         [e.getUndXY0ToCPU(s) for s in range(5)], [e.sector_info(s) for s in range(5)])
        before = state()
        dr = np.tile([Z_NEAR, Z_FAR], (5, 1))
        dr[4] = (5.0, Z_FAR)                        # a curve of more than LK_EP_MAX_STATIONS stations
        info, got, _, _ = check(e, cams, 0, 1, g=g, depth_range=dr)
        assert info["status"].tolist() == [ca.GS_TEXTURELESS, ca.GS_NO_CANDIDATE, ca.GS_TOO_FEW, ca.GS_OK, ca.GS_TOO_LONG]
        info, got, _, _ = check(e, cams, 0, 1, g=g, min_score=2.0)
        assert info["status"][3] == info["status"][4] == ca.GS_WEAK and got.tobytes() == g.tobytes()
        assert info["score"][3] > 0.5 and info["n_valid"][3] > 0          # a weak sector still reports its winner
        info, got, _, _ = check(e, cams, 0, 1, g=g, min_samples=1000)
        assert (info["status"] == ca.GS_TOO_FEW).all() and got.tobytes() == g.tobytes()
        strong = dict(cx=128.0, cy=128.0, rn=60.0, k1=-0.5, k2=0.0, p1=0.0, p2=0.0)
        folded = sr.as_records([dict(r[0], lens=strong), r[1]])
        info, got, _, _ = check(e, folded, 0, 1, g=g)
        assert (info["status"] == ca.GS_NO_CURVE).any() and got[info["status"] == ca.GS_NO_CURVE].tobytes() == g[info["status"] == ca.GS_NO_CURVE].tobytes()
        after = state()
        assert before[0] == after[0] and before[4] == after[4]
        assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
        assert all(np.array_equal(a, b) for a, b in zip(before[3], after[3]))
        assert device_records(e).tobytes() == rec0.tobytes()       # the engine-held records


def test_the_history_is_written_as_the_plain_search_writes_it(rig):
    r, cams, (im0, im1) = rig

    def follow(e):
        """what a pair loop makes of the state a search leaves: frame 0's solve, then frame 1's constant-velocity guesses"""
        rec = e.correlate_all(None)
        e.adjust_initial_guess(1, True, np.zeros(6, F32), (127.5, 127.5))
        return rec, e.get_guesses()
    g = arbitrary_guesses(143) * F32(0.01)
    with make_engine(im0, im1, RECTS) as a, make_engine(im0, im1, RECTS) as b:
        got = a.search_epipolar(cams, Z_NEAR, Z_FAR, level=1, band=1, shape=1, normal=NORMAL, guesses=g)
        status = a.epipolar_search_info()["status"]
        assert (status == ca.GS_OK).sum() >= 130 and (status != ca.GS_OK).any()
        # the plain search with a min_score no score reaches writes no guess: the engine-held guesses and the history it leaves
        # are the words it was given
        same = b.search_guesses(0, level=1, guesses=got, min_score=2.0)
        assert same.tobytes() == got.tobytes()
        rec_a, next_a = follow(a)
        rec_b, next_b = follow(b)
        assert rec_a.tobytes() == rec_b.tobytes() and next_a.tobytes() == next_b.tobytes()


def test_refusals(rig):
    r, cams, (im0, im1) = rig
    with make_engine(im0, im1, RECTS[:6]) as e:
        g = arbitrary_guesses(6)
        base = dict(cams=cams, z_near=Z_NEAR, z_far=Z_FAR, level=1, band=1, guesses=g)
        dr = np.tile([Z_NEAR, Z_FAR], (6, 1))
        dr[2, 0] = -1.0
        broken = np.array([cams[0], cams[1]], ca.CAMERA_DTYPE)
        broken["fy"][1] = -800.0
        for kw in (dict(band=9), dict(band=-1), dict(n_nodes=1), dict(n_nodes=34), dict(shape=2), dict(z_near=0.0), dict(z_far=300.0),
                   dict(z_far=np.inf), dict(z_near=np.nan), dict(normal=(0.0, np.inf, 1.0)), dict(level=5), dict(min_score=np.nan),
                   dict(def_slot=3), dict(depth_range=dr), dict(cams=[cams[0], broken[1]]), dict(cams=None)):
            with pytest.raises(ca.LkError) as err:
                e.search_epipolar(**dict(base, **kw))
            assert err.value.code == ca.ERROR_BAD_DOMAIN and "lk_search_epipolar" in str(err.value), kw
        assert e.get_guesses().tobytes() != g.tobytes()       # (nothing was uploaded by a refused call)
        with pytest.raises(ca.LkError):
            e.epipolar_search_info()                           # no search yet
        e.search_epipolar(**base)
        assert len(e.epipolar_search_info()) == 6
    for model, kw in ((ca.FM_U, {}), (ca.FM_UV, dict(shape=1)), (ca.FM_UVQ, dict(shape=1))):
        with make_engine(im0, im1, RECTS[:6], model=model) as e:
            with pytest.raises(ca.LkError) as err:
                e.search_epipolar(cams, Z_NEAR, Z_FAR, level=1, guesses=arbitrary_guesses(6), **kw)
            assert err.value.code == ca.ERROR_BAD_DOMAIN and "lk_search_epipolar" in str(err.value)


# ---- what the pass is for -------------------------------------------------------------------------------------------------------------
def test_end_to_end_on_rendered_frames(rig):
    """tests/test_stereo_gpu.py's end-to-end test with the search along the curve (level 1, band 1, depth 340 .. 460) in place
    of the square search, and neither lk_flag_outliers nor lk_reseed_failed behind the solve.  Established on the CPU first
    (tests/test_epipolar_host.py, profiles/epipolar_recovery.txt): the CPU oracle from the brute force's guesses gives 127 good
    sectors and 0.4091 units of rms; the margins are test_stereo_gpu.py's: 0.95 of ORACLE_GOOD, twice ORACLE_PLANE_RMS."""
    from test_stereo_host import ORACLE_GOOD, ORACLE_PLANE_RMS
    r, cams, (im0, im1) = rig
    with make_engine(im0, im1, RECTS) as e:
        e.search_epipolar(cams, Z_NEAR, Z_FAR, level=1, band=1)
        found = e.get_guesses()
        rec = e.correlate_all(None)
        ref_pts, _ = e.stereo_points(cams, rec)
        rms, n = sr.plane_rms(ref_pts)
        off = np.abs(found[:, :2] - sr.disparity_guess(r, CEN)[:, :2]).max(axis=1)
        e.search_guesses(8, guesses=np.zeros((143, 6), F32))          # the square search of test_stereo_gpu.py, for contrast
        sq_found = e.get_guesses()
        sq_pts, _ = e.stereo_points(cams, e.correlate_all(None))
        sq_rms, sq_n = sr.plane_rms(sq_pts)
        sq_off = np.abs(sq_found[:, :2] - sr.disparity_guess(r, CEN)[:, :2]).max(axis=1)
        print(f"lk_search_epipolar + solve + lk_stereo_points: {n} of 143 sectors good (floor {0.95 * ORACLE_GOOD:.1f}), rms distance from the "
              f"fitted plane {rms:.4f} units (bound {2 * ORACLE_PLANE_RMS:.4f}), within 4 px of the true disparity in {(off <= 4).sum()} "
              f"sectors; the square search (level 2, R 8) on the same frames, no outlier pass: {sq_n} good, rms {sq_rms:.4f}, within 4 px in "
              f"{(sq_off <= 4).sum()}")
        assert n >= 0.95 * ORACLE_GOOD
        assert rms <= 2 * ORACLE_PLANE_RMS


def test_the_plane_induced_shape_helps_on_a_wide_rig():
    """The counts the brute force gives on the CPU (tests/test_epipolar_host.py: 134 against 123) are the device's, because the
    bytes are: check() compares them."""
    r = sr.make_rig(angle=np.deg2rad(35))
    cams = sr.as_records(r)
    im0, im1 = sr.rig_frames(r)
    count = []
    with make_engine(im0, im1, RECTS) as e:
        for shape in (0, 1):
            info, got, _, _ = check(e, cams, 1, 1, shape=shape, normal=NORMAL)
            off = np.abs(got[:, :2] - sr.disparity_guess(r, CEN)[:, :2]).max(axis=1)
            count.append(int(((off <= 4) & (info["status"] == ca.GS_OK)).sum()))
    print(f"35 degrees, level 1, band 1: within 4 px of the true disparity: shape 0 {count[0]}, shape 1 {count[1]}")
    assert count[1] >= count[0]
