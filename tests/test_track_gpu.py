"""Material-point tracks (lk_track_points, include/lk_engine.h) on the GPU: against the float64 brute force of
tests/track_ref.py on synthetic records; affine increments that compose exactly; a rigid rotation; split calls, repeats,
shuffles and subsets byte for byte; a lost point; end to end on a solved window against the analytic map of the speckle
generator; that nothing of the engine moves; arguments.

Domain: 12 x 12 sectors of 19 x 19 (pitch h = 19) on 256 x 256 images, as tests/test_strain_gpu.py.

Tolerance of the comparisons with the restatement, frame f (0-based), U = the largest |displacement| of the good records:
  x, y, u, v                 2^-22 |ref| + 1e-9 U (f + 1)
  gradients, tensor fields   2^-22 |ref| + 1e-9 U (f + 1) / h
The first term is the float rounding of the outputs (it is relative, so it is the same for a length and for a gradient);
the second covers what the device and the restatement differ in - the order of double sums of at most ~60 terms, about 1e-13
relative on moments whose condition number stays below about 100, carried over at most 5 frames - and it is the term that
is divided by h for a gradient."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi, speckle
from test_strain_gpu import SIDE, centres, device_records, grid_rects, make_engine, synthetic_records
from track_ref import FLOATS, POSITION, fresh_state, is_good, track_reference

pytestmark = pytest.mark.gpu

H = float(SIDE)
MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
MODES = [ca.TRACK_TOTAL, ca.TRACK_INCREMENTAL]
LO, HI = 17.0, 226.0            # the hull of the 12 x 12 centres: 8 + 9 + 19 i
CHI_MAX = 8.0


@pytest.fixture(scope="module")
def small_pair():
    return speckle.speckle_pair(256, 256, p=(1.3, -0.7, 0.002, 0.0, 0.0, -0.001), seed=5)


def smooth_records(cen, n_frames, rng, share, amplitude=3.0):
    """[F][S] records: smooth random displacements of a few pixels (an affine part and a slow wave), and in each frame
    `share` of the sectors made bad in each of the three ways of the strain test's synthetic_records"""
    c = cen.astype(np.float64)
    S = len(c)
    out = np.zeros((n_frames, S), ca.RESULT_DTYPE)
    for f in range(n_frames):
        rec = synthetic_records(S, rng, CHI_MAX, share)
        a, G = rng.uniform(-amplitude, amplitude, 2), rng.uniform(-0.02, 0.02, (2, 2))
        k, ph = rng.uniform(0.01, 0.03, (2, 2)), rng.uniform(0, 6.28, 2)
        uv = a + (c - 121.5) @ G.T + 0.5 * np.sin(c @ k.T + ph)
        nan = np.isnan(rec["p"][:, 0])
        rec["p"][:, 0], rec["p"][:, 1] = uv[:, 0], uv[:, 1]
        rec["p"][nan, 0] = np.nan
        out[f] = rec
    return out


def scale_of(records, model):
    good = is_good(records, _ffi.N_PARAMS[model], CHI_MAX)
    return float(np.abs(records["p"][good][:, :1 if model == ca.FM_U else 2]).max())


def random_points(cen, rng, radius, n=300):
    """some exactly on centres, the rest up to two radii outside the hull, one at 1e6 px, one NaN"""
    on = cen[rng.permutation(len(cen))[:40]].astype(np.float64)
    free = rng.uniform(LO - 2 * radius, HI + 2 * radius, (n - 42, 2))
    return np.float32(np.concatenate([on, free, [[1e6, 100.0]], [[np.nan, 50.0]]]))


def clear_of_the_noise_threshold(spread):
    """A second condition on the inputs, for the DEGENERATE rule's noise guard (Cxx <= 2^-40 Sxx: a row of centres seen from
    a point beyond the hull, where Cyy is the rounding of Syy - Sy Sy / n, about 1e-16 Syy): every window is either such a row
    (below 2^-46) or spread over at least a pitch (above 2^-20; (h / r)^2 / n is 1e-3 and more), so that the order of the
    sums cannot move a window across the threshold."""
    s = spread[np.isfinite(spread)]
    return not ((s > 2.0 ** -46) & (s < 2.0 ** -20)).any()


def check_against_reference(got, ref, U, what):
    vals, nbrs, status = ref[:3]
    assert np.array_equal(got["status"], status), what
    assert np.array_equal(got["neighbours"], nbrs), what
    frame = np.arange(1, got.shape[0] + 1, dtype=np.float64)[:, None]
    worst = 0.0
    for k, name in enumerate(FLOATS):
        tol = 2.0 ** -22 * np.abs(vals[..., k]) + 1e-9 * U * frame / (1.0 if name in POSITION else H)
        err = np.abs(got[name].astype(np.float64) - vals[..., k])
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (what, name, np.unravel_index(np.argmax(err / tol), err.shape), float(err.max()))
    for name in FLOATS:
        assert not got[name][status != ca.TRACK_OK].any(), (what, name)
    return worst


# ---- 1. against the float64 brute force ---------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [2.5 * H, 1.5 * H])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("mode", MODES)
def test_tracks_match_float64_brute_force(small_pair, mode, model, radius):
    assert radius == np.float32(radius)
    with make_engine(*small_pair, grid_rects(), model=model) as e:
        cen = centres(e)
        rng = np.random.default_rng(1000 * mode + 100 * model + int(radius))
        rec = smooth_records(cen, 5, rng, 0.07)
        pts = random_points(cen, rng, radius)
        U = scale_of(rec, model)
        tensor = ca.STRAIN_SMALL if model == ca.FM_UVQ else ca.STRAIN_GREEN_LAGRANGE
        ref = track_reference(cen, rec, model, fresh_state(pts), radius, CHI_MAX, 3, tensor, mode)
        # a condition on the inputs: a changed summation order must not flip a window's membership
        print(f"mode {mode} model {model} radius {radius}: smallest |distance - radius| {ref[4]:.3g} px")
        assert ref[4] >= 1e-6, ref[4]
        assert clear_of_the_noise_threshold(ref[5])
        got, state = e.track_points(pts, radius, records=rec, mode=mode, chi_max=CHI_MAX, tensor=tensor)
        assert got.shape == (5, 300) and state.shape == (300, 8)
        worst = check_against_reference(got, ref, U, (mode, model, radius))
        print(f"  worst error / tolerance {worst:.3g}; statuses {np.bincount(ref[2].ravel(), minlength=5).tolist()}, "
              f"neighbours up to {ref[1].max()}")
        # the state: X, Y as passed, the rest the restatement's within 1e-9 U (a lost point: NaN on both sides)
        assert state[:, :2].tobytes() == pts.astype(np.float64).tobytes()
        assert np.array_equal(np.isnan(state[:, 2:]), np.isnan(ref[3][:, 2:]))
        assert np.allclose(np.nan_to_num(state), np.nan_to_num(ref[3]), rtol=2.0 ** -40, atol=1e-9 * U * 5)
        # the special points, and every status the mode can give
        assert (got["status"][:, -1] == ca.TRACK_BAD_POINT).all() and not got["neighbours"][:, -1].any()
        assert got["status"][0, -2] == ca.TRACK_TOO_FEW and got["neighbours"][0, -2] == 0
        seen = set(ref[2].ravel().tolist())
        assert {ca.TRACK_OK, ca.TRACK_TOO_FEW, ca.TRACK_BAD_POINT} <= seen
        assert (ca.TRACK_LOST in seen) == (mode == ca.TRACK_INCREMENTAL)
        if model == ca.FM_U:
            assert not got["v"].any() and not got["vx"].any() and not got["vy"].any()


def test_both_lane_groups(small_pair, monkeypatch):
    """16 lanes per point up to 1024 expected members of the 3 x 3 cells, 64 above (a radius past the whole domain: one
    cell of 144); LK_TRACK_GROUP forces either on both.  Each agrees with the restatement and repeats its bytes."""
    with make_engine(*small_pair, grid_rects()) as e:
        cen = centres(e)
        rng = np.random.default_rng(21)
        rec = smooth_records(cen, 3, rng, 0.07)
        pts = random_points(cen, rng, 2.5 * H, n=100)
        U = scale_of(rec, ca.FM_UVUXUYVXVY)
        for radius in (2.5 * H, 1000.0):
            for mode in MODES:
                ref = track_reference(cen, rec, ca.FM_UVUXUYVXVY, fresh_state(pts), radius, CHI_MAX, mode=mode)
                assert ref[4] >= 1e-6 and clear_of_the_noise_threshold(ref[5])
                for group in (None, "16", "64"):
                    if group is None:
                        monkeypatch.delenv("LK_TRACK_GROUP", raising=False)
                    else:
                        monkeypatch.setenv("LK_TRACK_GROUP", group)
                    got, _ = e.track_points(pts, radius, records=rec, mode=mode, chi_max=CHI_MAX)
                    # (a window of the whole domain: sums of 144 terms and lever arms of 200 px - the same bound holds)
                    check_against_reference(got, ref, U, (radius, mode, group))
                    assert got.tobytes() == e.track_points(pts, radius, records=rec, mode=mode, chi_max=CHI_MAX)[0].tobytes()


# ---- 2. affine increments compose exactly ---------------------------------------------------------------------------------
def test_affine_increments_compose_exactly(small_pair):
    n_frames, radius = 6, 2.5 * H
    x0 = np.float64([121.5, 121.5])
    with make_engine(*small_pair, grid_rects(), model=ca.FM_UV) as e:
        cen = centres(e)
        c = cen.astype(np.float64)
        rng = np.random.default_rng(77)
        a = rng.uniform(-4, 4, (n_frames, 2))
        G = rng.uniform(-0.02, 0.02, (n_frames, 2, 2))
        rec = np.zeros((n_frames, len(c)), ca.RESULT_DTYPE)
        rec["chi"], rec["n_points"] = 1.0, 361
        for f in range(n_frames):
            uv = a[f] + (c - x0) @ G[f].T
            rec["p"][f, :, 0], rec["p"][f, :, 1] = uv[:, 0], uv[:, 1]
            rec["error_code"][f, rng.permutation(len(c))[:10]] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        U = float(np.abs(rec["p"][..., :2]).max())
        pts = np.float32(rng.uniform(LO + 50, HI - 50, (64, 2)))
        got, state = e.track_points(pts, radius, records=rec, mode=ca.TRACK_INCREMENTAL)
        assert (got["status"] == ca.TRACK_OK).all()                      # no point may be lost at 2.5 h
        X = pts.astype(np.float64)
        x, F = X.copy(), np.tile(np.eye(2), (len(X), 1, 1))
        worst_x = worst_g = 0.0
        for f in range(n_frames):
            x = x + a[f] + (x - x0) @ G[f].T
            F = (np.eye(2) + G[f]) @ F
            # the float rounding of the samples (2^-24 U each), once per frame, doubled; + the rounding of the output
            tol_x = 2.0 ** -22 * np.abs(x) + 2 * n_frames * 2.0 ** -24 * U
            tol_g = 2.0 ** -22 + 2 * n_frames * 2.0 ** -24 * U / H
            ex = np.abs(np.stack([got["x"][f], got["y"][f]], 1) - x)
            eu = np.abs(np.stack([got["u"][f], got["v"][f]], 1) - (x - X))
            eg = np.abs(np.stack([got["ux"][f], got["uy"][f], got["vx"][f], got["vy"][f]], 1) - (F - np.eye(2)).reshape(-1, 4))
            worst_x, worst_g = max(worst_x, float(ex.max()), float(eu.max())), max(worst_g, float(eg.max()))
            assert (ex <= tol_x).all() and (eu <= tol_x).all() and (eg <= tol_g).all(), (f, ex.max(), eu.max(), eg.max())
        print(f"affine composition: worst position error {worst_x:.3g} px (second term {2 * n_frames * 2.0 ** -24 * U:.3g}), "
              f"worst gradient error {worst_g:.3g} (second term {2 * n_frames * 2.0 ** -24 * U / H:.3g})")
        assert np.abs(state[:, 2:4] - x).max() <= 2 * n_frames * 2.0 ** -24 * U
        assert np.abs(state[:, 4:].reshape(-1, 2, 2) - F).max() <= 2 * n_frames * 2.0 ** -24 * U / H


# ---- 3. rotation ------------------------------------------------------------------------------------------------------------
def test_rigid_rotation_has_no_green_lagrange_strain(small_pair):
    ang = np.deg2rad(10.0)
    R = np.float64([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    x0 = np.float64([121.5, 121.5])
    with make_engine(*small_pair, grid_rects(), model=ca.FM_UV) as e:
        cen = centres(e)
        c = cen.astype(np.float64)
        rec = np.zeros((1, len(c)), ca.RESULT_DTYPE)
        uv = (c - x0) @ (R - np.eye(2)).T
        rec["p"][0, :, 0], rec["p"][0, :, 1] = uv[:, 0], uv[:, 1]
        rec["chi"], rec["n_points"] = 1.0, 361
        rng = np.random.default_rng(4)
        pts = np.float32(rng.uniform(LO + 2.5 * H, HI - 2.5 * H, (64, 2)))       # interior: a radius inside the hull
        gl, _ = e.track_points(pts, 2.5 * H, records=rec, tensor=ca.STRAIN_GREEN_LAGRANGE)
        sm, _ = e.track_points(pts, 2.5 * H, records=rec, tensor=ca.STRAIN_SMALL)
        assert (gl["status"] == ca.TRACK_OK).all() and (sm["status"] == ca.TRACK_OK).all()
        for name in ("exx", "eyy", "exy"):
            assert np.abs(gl[name]).max() <= 1e-6, (name, np.abs(gl[name]).max())
        assert np.abs(sm["exx"] - (np.cos(ang) - 1)).max() <= 1e-6 and np.abs(sm["eyy"] - (np.cos(ang) - 1)).max() <= 1e-6
        want = pts.astype(np.float64) + (pts.astype(np.float64) - x0) @ (R - np.eye(2)).T
        assert np.abs(np.stack([gl["x"][0], gl["y"][0]], 1) - want).max() <= 2.0 ** -22 * 256 + 1e-5
        for name in ("x", "y", "u", "v", "ux", "uy", "vx", "vy"):
            assert gl[name].tobytes() == sm[name].tobytes()


# ---- 4. split equals whole, and independence -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_split_calls_repeats_shuffles_and_subsets_give_the_same_bytes(small_pair, mode):
    radius = 2.5 * H
    with make_engine(*small_pair, grid_rects()) as e:
        cen = centres(e)
        rng = np.random.default_rng(31 + mode)
        rec = smooth_records(cen, 6, rng, 0.07)
        pts = random_points(cen, rng, radius, n=200)
        kw = dict(mode=mode, chi_max=CHI_MAX)
        whole, st_whole = e.track_points(pts, radius, records=rec, **kw)
        assert set(whole["status"].ravel().tolist()) >= {ca.TRACK_OK, ca.TRACK_TOO_FEW}
        again, st_again = e.track_points(pts, radius, records=rec, **kw)
        assert whole.tobytes() == again.tobytes() and st_whole.tobytes() == st_again.tobytes()
        first, st = e.track_points(pts, radius, records=rec[:3], **kw)
        second, st2 = e.track_points(None, radius, records=rec[3:], state=st, **kw)
        assert np.concatenate([first, second]).tobytes() == whole.tobytes() and st2.tobytes() == st_whole.tobytes()
        # frame by frame through the state as well
        st1, parts = None, []
        for f in range(6):
            part, st1 = e.track_points(pts if f == 0 else None, radius, records=rec[f:f + 1], state=st1, **kw)
            parts.append(part)
        assert np.concatenate(parts).tobytes() == whole.tobytes() and st1.tobytes() == st_whole.tobytes()
        order = rng.permutation(len(pts))
        shuffled, st_s = e.track_points(pts[order], radius, records=rec, **kw)
        assert shuffled.tobytes() == whole[:, order].tobytes() and st_s.tobytes() == st_whole[order].tobytes()
        for q in (1, 17, 64):
            pick = np.sort(rng.permutation(len(pts))[:q])
            sub, st_q = e.track_points(pts[pick], radius, records=rec, **kw)
            assert sub.tobytes() == whole[:, pick].tobytes() and st_q.tobytes() == st_whole[pick].tobytes(), q


# ---- 5. a lost point ---------------------------------------------------------------------------------------------------------
def test_a_point_without_neighbours_is_lost_in_incremental_mode_only(small_pair):
    radius = 1.5 * H
    with make_engine(*small_pair, grid_rects(), model=ca.FM_UV) as e:
        cen = centres(e)
        rec = np.zeros((5, len(cen)), ca.RESULT_DTYPE)
        rec["p"][..., 0], rec["p"][..., 1] = 0.5, -0.25
        rec["chi"], rec["n_points"] = 1.0, 361
        pts = np.float32([[120.0, 125.0], [30.0, 30.0]])
        near = np.hypot(*(cen.astype(np.float64) - pts[0].astype(np.float64)).T) <= 3 * radius
        kept = np.hypot(*(cen.astype(np.float64) - pts[1].astype(np.float64)).T) <= radius
        assert near.sum() > 30 and kept.sum() >= 5 and not (near & kept).any()
        rec["error_code"][2, near] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        inc, st_inc = e.track_points(pts, radius, records=rec, mode=ca.TRACK_INCREMENTAL)
        tot, st_tot = e.track_points(pts, radius, records=rec, mode=ca.TRACK_TOTAL)
        assert inc["status"][:, 0].tolist() == [ca.TRACK_OK, ca.TRACK_OK, ca.TRACK_TOO_FEW, ca.TRACK_LOST, ca.TRACK_LOST]
        assert tot["status"][:, 0].tolist() == [ca.TRACK_OK, ca.TRACK_OK, ca.TRACK_TOO_FEW, ca.TRACK_OK, ca.TRACK_OK]
        assert (inc["status"][:, 1] == ca.TRACK_OK).all() and (tot["status"][:, 1] == ca.TRACK_OK).all()
        assert inc["neighbours"][2:, 0].tolist() == [0, 0, 0] and inc["neighbours"][1, 0] > 3
        for t in (inc[2:, 0], tot[2, 0]):
            for name in FLOATS:
                assert not np.any(t[name]), name
        assert st_inc[0, :2].tolist() == [120.0, 125.0] and np.isnan(st_inc[0, 2:]).all() and np.isfinite(st_inc[1]).all()
        assert np.isfinite(st_tot).all()
        # a uniform field: the point that stays is carried by it, frame after frame / once
        assert np.allclose(inc["u"][:, 1], 0.5 * np.arange(1, 6), rtol=0, atol=1e-5) and np.allclose(tot["u"][:, 1], 0.5, rtol=0, atol=1e-5)
        # continuing from the lost state stays lost; a fresh start finds the point again
        more, _ = e.track_points(None, radius, records=rec[:1], mode=ca.TRACK_INCREMENTAL, state=st_inc)
        assert more["status"][0].tolist() == [ca.TRACK_LOST, ca.TRACK_OK]


# ---- 6. end to end on a real window ---------------------------------------------------------------------------------------
DELTA, VELOCITY, N_PAIRS = 0.004, (0.8, -0.4), 4
CENTRE = np.float64([128.0, 128.0])       # speckle.deform maps about the image centre (w / 2, h / 2)


def analytic_position(X, k):
    """speckle.deform's map of frame k: translation VELOCITY k plus the dilation DELTA k about the image centre"""
    return X + np.float64(VELOCITY) * k + DELTA * k * (X - CENTRE)


def analytic_increment(c, k):
    """displacement from frame k - 1 to frame k of the material that sits at c in frame k - 1"""
    X = CENTRE + (c - CENTRE - np.float64(VELOCITY) * (k - 1)) / (1.0 + DELTA * (k - 1))
    return analytic_position(X, k) - c


def test_end_to_end_on_a_solved_window():
    frames = speckle.speckle_sequence(256, 256, N_PAIRS + 1, velocity=VELOCITY, dilation=DELTA, seed=5)
    radius = 2.5 * H
    rng = np.random.default_rng(8)
    pts = np.float32(rng.uniform(LO + radius, HI - radius, (40, 2)))       # interior: a radius inside the hull
    X = pts.astype(np.float64)
    spread = np.ptp(analytic_position(X, N_PAIRS) - X, axis=0).max()
    assert spread >= 1.0, spread            # the displacement varies by a pixel across the tracked region

    def solve(reference_previous):
        e = make_engine(frames[0], frames[1], grid_rects())
        e.sequence_reserve(N_PAIRS)
        for i in range(N_PAIRS):
            e.sequence_set_frame(i, frames[i + 1])
        e.adjust_initial_guess(0, not reference_previous, np.zeros(6, np.float32), (127.5, 127.5))
        rec = e.correlate_sequence(N_PAIRS, reference_previous=reference_previous, constant_velocity=not reference_previous)
        return e, rec

    e, rec = solve(True)
    c = centres(e).astype(np.float64)
    # (a) the window's device records read in place = the downloaded records passed back in
    inc, st = e.track_points(pts, radius, mode=ca.TRACK_INCREMENTAL, source=ca.TRACK_RECORDS_WINDOW)
    same, st2 = e.track_points(pts, radius, records=rec, mode=ca.TRACK_INCREMENTAL)
    assert inc.shape == (N_PAIRS, len(pts)) and inc.tobytes() == same.tobytes() and st.tobytes() == st2.tobytes()
    assert inc.tobytes() == e.track_points(pts, radius, n_frames=N_PAIRS, mode=ca.TRACK_INCREMENTAL,
                                           source=ca.TRACK_RECORDS_WINDOW)[0].tobytes()
    assert (inc["status"] == ca.TRACK_OK).all()
    # (b) the tracked positions against the analytic map: at most 2 sum_k E_k, E_k measured on the records themselves
    E = np.zeros(N_PAIRS)
    for f in range(N_PAIRS):
        good = is_good(rec[f], 6, 0.0)
        assert good.sum() >= 130
        E[f] = np.abs(rec[f]["p"][good, :2] - analytic_increment(c[good], f + 1)).max()
    bound_inc = 2.0 * np.cumsum(E)
    for f in range(N_PAIRS):
        err = np.abs(np.stack([inc["x"][f], inc["y"][f]], 1) - analytic_position(X, f + 1)).max()
        print(f"incremental window, frame {f + 1}: E = {E[f]:.4f} px, position error {err:.4f} px, error / bound {err / bound_inc[f]:.3f}")
        assert err <= bound_inc[f], (f, err, bound_inc[f])
    e.close()
    # (c) the fixed-reference window tracked in TOTAL mode lands on the same positions
    e, rec_tot = solve(False)
    tot, _ = e.track_points(pts, radius, mode=ca.TRACK_TOTAL, source=ca.TRACK_RECORDS_WINDOW)
    assert tot.tobytes() == e.track_points(pts, radius, records=rec_tot, mode=ca.TRACK_TOTAL)[0].tobytes()
    assert (tot["status"] == ca.TRACK_OK).all()
    for f in range(N_PAIRS):
        good = is_good(rec_tot[f], 6, 0.0)
        E_tot = np.abs(rec_tot[f]["p"][good, :2] - (analytic_position(c[good], f + 1) - c[good])).max()
        bound_tot = 2.0 * E_tot
        err = np.abs(np.stack([tot["x"][f], tot["y"][f]], 1) - analytic_position(X, f + 1)).max()
        gap = np.abs(np.stack([tot["x"][f] - inc["x"][f], tot["y"][f] - inc["y"][f]], 1)).max()
        print(f"fixed-reference window, frame {f + 1}: E = {E_tot:.4f} px, position error {err:.4f} px, "
              f"|total - incremental| {gap:.4f} px of {bound_tot + bound_inc[f]:.4f}")
        assert err <= bound_tot and gap <= bound_tot + bound_inc[f]
    e.close()
    # (d) a virtual extensometer between two interior points reports the map's stretch DELTA k
    i, j = 0, int(np.argmax(np.hypot(*(X - X[0]).T)))
    L0 = float(np.hypot(*(X[j] - X[i])))
    assert L0 > 2 * H
    g = ca.gauges_from_tracks(inc, [[i, j]])
    for f in range(N_PAIRS):
        print(f"gauge, frame {f + 1}: engineering strain {g[f, 0, 1]:.6f} of {DELTA * (f + 1):.6f}, tolerance {2 * bound_inc[f] / L0:.6f}")
        assert abs(g[f, 0, 1] - DELTA * (f + 1)) <= 2.0 * bound_inc[f] / L0
        assert abs(g[f, 0, 0] - L0 * (1 + DELTA * (f + 1))) <= 2.0 * bound_inc[f] + 2.0 ** -22 * L0
        assert abs(g[f, 0, 3]) <= 2.0 * bound_inc[f] / L0 + 1e-6              # the map does not rotate


# ---- 7. nothing of the engine moves ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("reference_order", [0, 1])
def test_engine_state_is_untouched(small_pair, reference_order):
    rects = grid_rects(n=8)
    S = len(rects)
    with make_engine(*small_pair, rects) as e:
        if reference_order:
            e.set_reference_order(1)
        g = np.zeros((S, 6), np.float32)
        g[[9, 27], 0] = 300.0
        first = e.correlate_all(g)
        if not reference_order:
            e.reseed_failed(1.5 * H)
        rng = np.random.default_rng(2)
        pts = np.float32(rng.uniform(17, 150, (50, 2)))

        def state():
            return dict(records=device_records(e), guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(),
                        stats=e.sector_stats(), reseed=e.reseed_info() if not reference_order else np.zeros(1),
                        counters=np.array(sorted(e.stats().items()), dtype=object))

        def same(a, b):
            for k in a:
                assert (a[k] == b[k]).all() if k == "counters" else a[k].tobytes() == b[k].tobytes(), k

        kept = state()
        a, _ = e.track_points(pts, 2.5 * H, source=ca.TRACK_RECORDS_ENGINE)
        b, _ = e.track_points(pts, 2.5 * H)                                  # (no records: the engine's, by default)
        c, _ = e.track_points(pts, 1.5 * H, records=np.stack([first, first]), mode=ca.TRACK_INCREMENTAL, chi_max=5.0, min_neighbours=4)
        assert a.tobytes() == b.tobytes() and a.shape == (1, 50) and c.shape == (2, 50)
        assert a.tobytes() == e.track_points(pts, 2.5 * H, records=kept["records"])[0].tobytes()
        assert (a["status"] == ca.TRACK_OK).sum() >= 40
        same(kept, state())
        # a rebuild of the lists that waits for the next solve keeps waiting: after lk_update_sector has turned a sector
        # into a list the device still holds the centres the records were solved at, and the tracks are the same bytes
        e.update_sector(20, 0)
        kept = state()
        assert e.track_points(pts, 2.5 * H)[0].tobytes() == a.tobytes()
        same(kept, state())
        # ... and the next solve carries the rebuild out as if nothing had been asked in between
        after = e.correlate_all(np.zeros((S, 6), np.float32))
        assert (after["error_code"] == 0).sum() >= S - 2


# ---- 8. arguments ------------------------------------------------------------------------------------------------------------
def test_arguments_and_refusals(small_pair):
    rects = grid_rects(n=3)
    e = make_engine(*small_pair, rects, commit=False)
    lib, h = e.lib, e._h
    P = C.c_void_p
    pts = np.float32([[30.0, 30.0], [40.0, 35.0]])
    rec = np.zeros((2, 9), ca.RESULT_DTYPE)
    rec["p"][..., 0] = np.arange(9)
    out = np.full((2, 2), 7, ca.TRACK_DTYPE)
    state = np.zeros((2, 8))
    GOOD = (47.5, 0.0, 3, 0, ca.TRACK_TOTAL, ca.TRACK_RECORDS_CALLER)

    def refused(cfg=GOOD, n_points=2, points=pts, n_frames=2, records=rec, st=state, output=out):
        c = _ffi.LkTrackConfig(*cfg) if cfg is not None else None
        rc = lib.lk_track_points(h, C.byref(c) if c is not None else None, n_points, _ffi.fptr(points) if points is not None else None,
                                 n_frames, records.ctypes.data_as(P) if records is not None else None,
                                 st.ctypes.data_as(P) if st is not None else None, output.ctypes.data_as(P) if output is not None else None)
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and "lk_track_points" in msg, (rc, msg)
        assert (out == np.full(1, 7, ca.TRACK_DTYPE)).all()
        return msg

    def with_(**kw):
        d = dict(zip(("radius", "chi_max", "min_neighbours", "tensor", "mode", "source"), GOOD))
        d.update(kw)
        return tuple(d.values())

    assert "no committed sectors" in refused()
    e.commit_sectors()
    assert "configuration" in refused(None)
    assert "output" in refused(output=None)
    for bad in (0, -1):
        assert "n_points" in refused(n_points=bad)
        assert "n_frames" in refused(n_frames=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "radius" in refused(with_(radius=bad))
    for bad in (float("nan"), float("inf")):
        assert "chi_max" in refused(with_(chi_max=bad))
    for bad in (2, 0, -1):
        assert "min_neighbours" in refused(with_(min_neighbours=bad))
    for bad in (-1, 2):
        assert "tensor" in refused(with_(tensor=bad))
        assert "mode" in refused(with_(mode=bad))
    for bad in (-1, 3):
        assert "source" in refused(with_(source=bad))
    assert "neither" in refused(points=None, st=None)
    # the records / n_frames / source combinations
    assert "records" in refused(records=None)                                                    # CALLER without records
    assert "records" in refused(with_(source=ca.TRACK_RECORDS_ENGINE), n_frames=1)              # ENGINE with records
    assert "records" in refused(with_(source=ca.TRACK_RECORDS_WINDOW))                          # WINDOW with records
    assert "n_frames" in refused(with_(source=ca.TRACK_RECORDS_ENGINE), records=None, n_frames=2)
    assert "no solve" in refused(with_(source=ca.TRACK_RECORDS_ENGINE), records=None, n_frames=1)
    assert "no window" in refused(with_(source=ca.TRACK_RECORDS_WINDOW), records=None, n_frames=0)
    for n in (None, 0, 2):      # the Python call on an engine that never solved a window: the library's refusal, nothing written
        with pytest.raises(ca.LkError, match="no window"):
            e.track_points(pts, 47.5, n_frames=n, source=ca.TRACK_RECORDS_WINDOW)
    assert "n_frames" in refused(with_(source=ca.TRACK_RECORDS_WINDOW), records=None, n_frames=-1)
    assert lib.lk_track_points(None, None, 2, None, 2, None, None, None) == ca.ERROR_BAD_DOMAIN
    # records passed in need no solve; a state alone continues; no state at all is fine with points
    got, st = e.track_points(pts, 47.5, records=rec)
    assert (got["status"] == ca.TRACK_OK).all() and got["neighbours"].max() <= 9
    c = _ffi.LkTrackConfig(*GOOD)
    direct = np.zeros((2, 2), ca.TRACK_DTYPE)
    assert lib.lk_track_points(h, C.byref(c), 2, _ffi.fptr(pts), 2, rec.ctypes.data_as(P), None, direct.ctypes.data_as(P)) == 0
    assert direct.tobytes() == got.tobytes()
    # a solve in flight refuses the engine-held records and finishes normally afterwards
    e.correlate_all_async()
    assert "waited for" in refused(with_(source=ca.TRACK_RECORDS_ENGINE), records=None, n_frames=1)
    solved = e.wait_results()
    assert e.track_points(pts, 47.5)[0].tobytes() == e.track_points(pts, 47.5, records=solved)[0].tobytes()
    # a window in flight refuses WINDOW (and ENGINE); its frame count must match afterwards
    e.sequence_reserve(2)
    for i in range(2):
        e.sequence_set_frame(i, small_pair[1])
    e.adjust_initial_guess(0, False, np.zeros(6, np.float32), (32.0, 32.0))
    e.correlate_sequence_async(2, constant_velocity=False)
    assert "outstanding" in refused(with_(source=ca.TRACK_RECORDS_WINDOW), records=None, n_frames=0)
    assert "outstanding" in refused(with_(source=ca.TRACK_RECORDS_ENGINE), records=None, n_frames=1)
    win = e.wait_sequence()
    assert "n_frames" in refused(with_(source=ca.TRACK_RECORDS_WINDOW), records=None, n_frames=3)
    want = e.track_points(pts, 47.5, records=win)[0]
    # n_frames None, 0 (the header's "the window's frame count") and the count itself: an output of the window's size
    for n in (None, 0, 2):
        got = e.track_points(pts, 47.5, n_frames=n, source=ca.TRACK_RECORDS_WINDOW)[0]
        assert got.shape == (2, 2) and got.tobytes() == want.tobytes(), n
    c = _ffi.LkTrackConfig(*with_(source=ca.TRACK_RECORDS_WINDOW))
    direct = np.zeros((2, 2), ca.TRACK_DTYPE)
    assert lib.lk_track_points(h, C.byref(c), 2, _ffi.fptr(pts), 0, None, None, direct.ctypes.data_as(P)) == 0
    assert direct.tobytes() == want.tobytes()
    # a window is the window of the sectors it was solved for: a commit that adds a sector, or commits the same number anew,
    # leaves no window to read
    e.resetPolygon_rect(9, 100, 100, 118, 118)
    e.commit_sectors()
    assert e.n_sectors == 10
    assert "no window" in refused(with_(source=ca.TRACK_RECORDS_WINDOW), records=None, n_frames=0)
    e.clear_sectors()
    for s_, r in enumerate(grid_rects(n=3)):
        e.resetPolygon_rect(s_, r[0] + 5, r[1], r[2] + 5, r[3])
    e.commit_sectors()
    assert e.n_sectors == 9
    assert "no window" in refused(with_(source=ca.TRACK_RECORDS_WINDOW), records=None, n_frames=0)
    with pytest.raises(ca.LkError, match="no window"):
        e.track_points(pts, 47.5, n_frames=0, source=ca.TRACK_RECORDS_WINDOW)
    e.close()
