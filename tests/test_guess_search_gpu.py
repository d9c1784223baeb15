"""Automatic initial guess (lk_search_guesses): the integer-pixel ZNCC search of every sector against a numpy brute force on
the engine's own pyramid levels and sample lists; status paths; invariance across batches and modes; the capture range it
opens for the LM solve; and the sequence history it leaves for the frames after frame 0."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

pytestmark = pytest.mark.gpu

AFFINE = (21.3, -12.8, 0.004, 0.002, -0.003, 0.001)


def round_like_host(v):
    """(int)(v + 0.5f) in float32, truncated toward zero"""
    return np.trunc(np.asarray(v, np.float32) + np.float32(0.5)).astype(np.int64)


def decimate(lib, pts, delta=1):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    out = np.zeros_like(pts)
    k = lib.lk_roi_decimate(_ffi.fptr(pts), len(pts), delta, _ffi.fptr(out))
    return out[:k]


def level_points(e, s, level):
    """a sector's level-L samples as the engine holds them: the explicit list, or the implicit rectangle's decimation"""
    xy = e.level_xy(level, s)
    if len(xy):
        return xy
    pts = e.getUndXY0ToCPU(s)
    for _ in range(level):
        pts = decimate(e.lib, pts)
    return pts


def ref_search(und, dfm, pts, g, level, radius, has_v=True, min_samples=9, min_score=0.0):
    """numpy brute force of the semantics in include/lk_engine.h; returns a dict (and the refined g[0], g[1])"""
    n = len(pts)
    inv = np.float32(1.0 / (1 << level))
    cx = int(np.floor(np.float32(g[0]) * inv + np.float32(0.5)))
    cy = int(np.floor(np.float32(g[1]) * inv + np.float32(0.5))) if has_v else 0
    out = dict(center_x=cx, center_y=cy, shift_x=0, shift_y=0, n_samples=n, n_valid=0, score=-2.0, runner_up=-2.0,
               any_second=-2.0, g=(np.float32(g[0]), np.float32(g[1])))
    if n > _ffi.GS_MAX_SAMPLES:
        return dict(out, status=ca.GS_TOO_LARGE)
    if n < (min_samples if min_samples > 0 else 9):
        return dict(out, status=ca.GS_TOO_FEW)
    x = np.clip(round_like_host(pts[:, 0]), 0, und.shape[1] - 1)
    y = np.clip(round_like_host(pts[:, 1]), 0, und.shape[0] - 1)
    t = und[y, x].astype(np.int64)
    St, Stt = int(t.sum()), int((t * t).sum())
    varT = n * Stt - St * St
    if varT == 0:
        return dict(out, status=ca.GS_TEXTURELESS)
    jr = radius if has_v else 0
    cand = []
    for j in range(-jr, jr + 1):
        for i in range(-radius, radius + 1):
            xs, ys = x + cx + i, y + cy + j
            if xs.min() < 0 or ys.min() < 0 or xs.max() >= dfm.shape[1] or ys.max() >= dfm.shape[0]:
                continue
            d = dfm[ys, xs].astype(np.int64)
            Sd, Sdd, Std = int(d.sum()), int((d * d).sum()), int((t * d).sum())
            varD = n * Sdd - Sd * Sd
            if varD == 0:
                continue
            cand.append((float(n * Std - St * Sd) / np.sqrt(float(varT) * float(varD)), i, j))
    if not cand:
        return dict(out, status=ca.GS_NO_CANDIDATE)
    cand.sort(key=lambda c: (-c[0], c[1] ** 2 + c[2] ** 2, c[2], c[1]))
    best, bi, bj = cand[0]
    far = [c[0] for c in cand if max(abs(c[1] - bi), abs(c[2] - bj)) >= 2]
    out.update(shift_x=bi, shift_y=bj, n_valid=len(cand), score=best, runner_up=max(far) if far else -2.0,
               any_second=cand[1][0] if len(cand) > 1 else -2.0,
               tie_band={(c[1], c[2]) for c in cand if c[0] >= best - 1e-9 * abs(best)})
    status = ca.GS_OK if best > min_score else ca.GS_WEAK
    if status == ca.GS_OK:
        out["g"] = (np.float32((cx + bi) * (1 << level)), np.float32((cy + bj) * (1 << level)) if has_v else np.float32(g[1]))
    return dict(out, status=status)


def check_against_reference(e, guesses_in, level, radius, slot=ca.IMG_DEF, def_img=None, min_samples=0, min_score=0.0):
    has_v = e.cfg.fitting_model != ca.FM_U
    und = e.get_pyramid_level(ca.IMG_UND, level)
    dfm = def_img if def_img is not None else e.get_pyramid_level(slot, level)
    got = e.search_guesses(radius, level=level, guesses=guesses_in, min_samples=min_samples, min_score=min_score,
                           def_slot=-1 if def_img is None else slot)
    info = e.guess_search_info()
    assert np.array_equal(got, e.get_guesses())
    S = e.n_sectors
    for s in range(S):
        want = ref_search(und, dfm, level_points(e, s, level), guesses_in[s], level, radius, has_v, min_samples, min_score)
        m = info[s]
        for k in ("center_x", "center_y", "n_samples", "n_valid", "status"):
            assert m[k] == want[k], (s, k, m, want)
        if want["status"] in (ca.GS_OK, ca.GS_WEAK):
            assert abs(m["score"] - want["score"]) <= 1e-12, (s, m, want)
            assert abs(m["runner_up"] - want["runner_up"]) <= 1e-12, (s, m, want)
            if want["score"] - want["any_second"] > 1e-9 * abs(want["score"]):
                assert (m["shift_x"], m["shift_y"]) == (want["shift_x"], want["shift_y"]), (s, m, want)
            else:
                assert (m["shift_x"], m["shift_y"]) in want["tie_band"], (s, m, want)
        if m["status"] == ca.GS_OK:
            assert got[s, 0] == np.float32((m["center_x"] + m["shift_x"]) * (1 << level))
            if has_v:
                assert got[s, 1] == np.float32((m["center_y"] + m["shift_y"]) * (1 << level))
            else:
                assert got[s, 1].tobytes() == guesses_in[s, 1].tobytes()
        else:
            assert got[s].tobytes() == guesses_in[s].tobytes()
        assert got[s, 2:].tobytes() == guesses_in[s, 2:].tobytes()
    return info, got


@pytest.fixture(scope="module")
def affine512():
    return ca.speckle.speckle_pair(512, 512, p=AFFINE, seed=11)


def rect_engine(pair, model=ca.FM_UVUXUYVXVY, grid=(60.0, 60.0, 451.0, 451.0, 12, 12)):
    e = ca.HipCorrelationEngine(fitting_model=model)
    e.set_undeformed_image(pair[0])
    e.set_deformed_image(pair[1])
    e.set_rect_grid(*grid)
    e.commit_sectors()
    return e


@pytest.mark.parametrize("level,radius", [(0, 3), (1, 12), (2, 6), (2, 8)])
def test_rect_grid_matches_the_numpy_reference(affine512, level, radius):
    e = rect_engine(affine512)
    rng = np.random.default_rng(level * 100 + radius)
    g = np.zeros((e.n_sectors, 6), np.float32)
    g[:, :2] = np.float32(AFFINE[:2]) + rng.uniform(-radius, radius, (e.n_sectors, 2)).astype(np.float32) * (1 << level) * 0.7
    g[:, 2:] = rng.standard_normal((e.n_sectors, 4)).astype(np.float32) * 1e-3
    info, got = check_against_reference(e, g, level, radius)
    assert (info["status"] == ca.GS_OK).mean() > 0.9
    e.close()


def test_one_dimensional_model_searches_only_u(affine512):
    und, _ = affine512
    dfm = ca.speckle.speckle_pair(512, 512, p=(-9.6, 0.0, 0, 0, 0, 0), seed=11)[1]
    e = rect_engine((und, dfm), model=ca.FM_U)
    g = np.zeros((e.n_sectors, 6), np.float32)
    info, got = check_against_reference(e, g, 1, 10)
    assert (info["shift_y"] == 0).all() and (info["center_y"] == 0).all()
    ok = info["status"] == ca.GS_OK
    assert ok.mean() > 0.9 and np.median(got[ok, 0]) == -10.0
    e.close()


def test_annular_blob_and_float_point_sectors(affine512):
    und, dfm = affine512
    e = ca.HipCorrelationEngine()
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    s = 0
    for k in range(6):
        e.resetPolygon_annular(s, 60.0, 50.0, 0.3 + k * 1.0, 0.8, 256.0, 250.0, 4)
        s += 1
    ang = 2 * np.pi * np.arange(24) / 24
    blob = np.stack([256.3 + 150 * np.cos(ang), 255.7 + 130 * np.sin(ang)], 1).astype(np.float32)
    e.resetPolygon_blob(s, blob)
    s += 1
    rng = np.random.default_rng(5)
    for k in range(4):   # float lists: the rounding rule
        pts = (rng.random((300, 2)) * 40 + 100 + 60 * k).astype(np.float32)
        e.set_sector_points(s, pts)
        s += 1
    e.commit_sectors()
    g = np.zeros((e.n_sectors, 6), np.float32)
    g[:, 0], g[:, 1] = 19.0, -11.0
    for level, radius in ((0, 5), (1, 4), (2, 3)):
        info, _ = check_against_reference(e, g, level, radius)
        assert (info["status"] == ca.GS_OK).sum() >= 8
    e.close()


def test_ring_slot_as_the_deformed_image(affine512):
    und, dfm = affine512
    other = ca.speckle.speckle_pair(512, 512, p=(-6.0, 4.0, 0, 0, 0, 0), seed=11)[1]
    e = rect_engine((und, dfm))
    e.sequence_reserve(3)
    e.sequence_set_frame(2, other)
    probe = ca.HipCorrelationEngine()
    probe.set_undeformed_image(other)
    ring_l1 = probe.get_pyramid_level(ca.IMG_UND, 1)
    probe.close()
    g = np.zeros((e.n_sectors, 6), np.float32)
    info, got = check_against_reference(e, g, 1, 6, slot=2, def_img=ring_l1)
    ok = info["status"] == ca.GS_OK
    assert ok.mean() > 0.9 and np.median(got[ok, 0]) == -6.0 and np.median(got[ok, 1]) == 4.0
    e.close()


def test_status_paths_and_untouched_guesses(affine512):
    und, dfm = affine512
    und = und.copy()
    und[200:240, 200:240] = 77                      # a uniform patch
    e = ca.HipCorrelationEngine()
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    e.resetPolygon_rect(0, 205, 205, 234, 234)      # TEXTURELESS
    e.resetPolygon_rect(1, 2, 100, 20, 118)         # at the left border: only the shifts that stay inside
    e.resetPolygon_rect(2, 100, 100, 118, 118)      # blocked: its centre is far outside
    e.resetPolygon_rect(3, 300, 300, 302, 301)      # 6 samples at level 0: TOO_FEW
    e.resetPolygon_rect(4, 300, 100, 318, 118)      # an ordinary sector (WEAK with a high min_score)
    e.commit_sectors()
    g = np.array([[1, 2, 3, 4, 5, 6]] * 5, np.float32) * np.float32(0.001)
    g[1, :2] = (-2.0, 0.0)
    g[2, :2] = (900.0, 0.0)
    g[4, :2] = AFFINE[:2]
    info, got = check_against_reference(e, g, 0, 10)
    assert [info["status"][k] for k in (0, 2, 3, 4)] == [ca.GS_TEXTURELESS, ca.GS_NO_CANDIDATE, ca.GS_TOO_FEW, ca.GS_OK]
    assert info[1]["status"] in (ca.GS_OK, ca.GS_WEAK)
    assert 0 < info[1]["n_valid"] <= 11 * 21  # shifts -10..-1 of the centre -2 leave the image (x0 = 2); a flat window has no score
    info, got = check_against_reference(e, g, 0, 10, min_score=0.9999)
    assert info[4]["status"] == ca.GS_WEAK and got[4].tobytes() == g[4].tobytes()
    info, got = check_against_reference(e, g, 0, 10, min_samples=1000)
    assert (info["status"] == ca.GS_TOO_FEW).all() and got.tobytes() == g.tobytes()
    e.close()


@pytest.mark.parametrize("mode", ["default", "batch_invariant", "reference_order"])
def test_a_sector_gets_the_same_bits_in_any_batch_and_mode(affine512, mode):
    und, dfm = affine512
    grid = (60.0, 60.0, 451.0, 451.0, 12, 12)

    def run(first, count):
        e = ca.HipCorrelationEngine()
        if mode == "batch_invariant":
            e.set_batch_invariant(True)
        elif mode == "reference_order":
            e.set_reference_order(1)
        e.set_undeformed_image(und)
        e.set_deformed_image(dfm)
        e.set_rect_grid(*grid, first, count)
        e.commit_sectors()
        g = np.zeros((e.n_sectors, 6), np.float32)
        g[:, 0] = 16.0
        out = [(e.search_guesses(9, level=1, guesses=g), e.guess_search_info()) for _ in range(2)]
        e.close()
        assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
        return out[0]

    full_g, full_m = run(0, -1)
    for s in (0, 37, 143):
        one_g, one_m = run(s, 1)
        assert one_g.tobytes() == full_g[s:s + 1].tobytes() and one_m.tobytes() == full_m[s:s + 1].tobytes()


TRUTH = (37.0, -23.0, 0.002, 0.0, 0.0, -0.001)


@pytest.fixture(scope="module")
def far512():
    return ca.speckle.speckle_pair(512, 512, p=TRUTH, seed=17)


def test_the_search_opens_the_capture_range(far512):
    und, dfm = far512
    e = ca.HipCorrelationEngine()
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    e.set_rect_grid(60.0, 60.0, 451.0, 451.0, 16, 16)
    e.commit_sectors()
    S = e.n_sectors
    cen = np.array([e.sector_info(s)[1:] for s in range(S)], np.float64)
    zero = e.correlate_all(np.zeros(6, np.float32))
    e.search_guesses(20, level=1)                 # about the engine-held guesses: zeros after commit
    g = e.get_guesses()
    info = e.guess_search_info()
    assert (info["status"] == ca.GS_OK).mean() > 0.99
    rec = e.correlate_all(None)
    host = e.correlate_all(g)
    assert rec.tobytes() == host.tobytes()
    ok = rec["error_code"] == ca.ERROR_NONE
    assert ok.mean() >= 0.99
    # converged to the same field from every start: the sectors agree with a smooth affine fit within 0.05 px
    A = np.c_[np.ones(S), cen]
    for k in range(2):
        coef, *_ = np.linalg.lstsq(A[ok], rec["p"][ok, k], rcond=None)
        assert np.abs(A[ok] @ coef - rec["p"][ok, k]).max() < 0.05
        assert np.abs(rec["p"][ok, k] - g[ok, k]).max() <= 3.0    # the solve refined the searched integer guess
    assert abs(np.median(rec["p"][ok, 0]) - TRUTH[0]) < 3 and abs(np.median(rec["p"][ok, 1]) - TRUTH[1]) < 3
    # from zero guesses most sectors fail or land far off
    off = (zero["error_code"] != ca.ERROR_NONE) | (np.abs(zero["p"][:, :2] - rec["p"][:, :2]).max(1) > 1.0)
    assert off.mean() > 0.5
    e.close()


def test_reference_order_records_equal_the_oracle_from_the_searched_guesses(far512, oracle):
    und, dfm = far512
    e = ca.HipCorrelationEngine()
    e.set_reference_order(1)
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    grid = (100.0, 100.0, 411.0, 411.0, 5, 5)
    e.set_rect_grid(*grid)
    e.commit_sectors()
    e.search_guesses(20, level=1)
    g = e.get_guesses()
    rec = e.correlate_all(None)
    o = oracle.Oracle(model=oracle.FM_UVUXUYVXVY)
    o.set_image(0, und)
    o.set_image(1, dfm)
    xdim, ydim, cen = oracle.rect_sector_geometry(*grid)
    lists = [oracle.rect_points(cx - xdim, cy - ydim, cx + xdim, cy + ydim) for cx, cy in cen]
    want = o.correlate_sectors(lists, centers=cen.astype(np.float32), guesses=g)
    assert rec.tobytes() == want.tobytes()
    assert (rec["error_code"] == ca.ERROR_NONE).all()
    e.close()


def test_a_window_after_the_search_continues_from_its_history(far512):
    und, _ = far512
    frames = [ca.speckle.speckle_pair(512, 512, p=(TRUTH[0] + 0.6 * k, TRUTH[1] - 0.4 * k) + TRUTH[2:], seed=17)[1]
              for k in range(4)]

    def engine():
        e = ca.HipCorrelationEngine()
        e.set_batch_invariant(True)
        e.set_undeformed_image(und)
        e.set_deformed_image(frames[0])
        e.set_rect_grid(80.0, 80.0, 431.0, 431.0, 8, 8)
        e.commit_sectors()
        e.search_guesses(20, level=1)
        return e

    a = engine()
    a.sequence_reserve(4)
    for i in range(4):
        a.sequence_set_frame(i, frames[i])
    win = a.correlate_sequence(4)
    b = engine()
    for k in range(4):
        b.set_deformed_image(frames[k])
        if k > 0:
            b.adjust_initial_guess(k, True, np.zeros(6, np.float32), (255.5, 255.5))
        rec = b.correlate_all(None)
        assert win[k].tobytes() == rec.tobytes(), k
    assert (win[3]["error_code"] == ca.ERROR_NONE).mean() > 0.95
    a.close()
    b.close()
