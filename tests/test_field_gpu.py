"""The field map (lk_field_map, include/lk_engine.h) on the GPU: against the float64 brute force of tests/field_ref.py in the
reference and the deformed frame; agreement with lk_track_points; repeats, sub-windows, strides, channel subsets, the
walked path, engine-held records and reference-order mode byte for byte; a dense domain whose tiles do not fit into LDS;
an exact affine field inverted; the bisquare weight's smoothness; end to end on a solved pair; that nothing of the engine
moves; arguments.

Domain: 12 x 12 sectors of 19 x 19 (pitch h = 19) on 256 x 256 images, as tests/test_strain_gpu.py; the centres are the
integers 17 + 19 i and the nodes are integers, so a squared distance is an integer and r^2 (47.5^2, 28.5^2) is not: no
sector lies on a rim, and the nearest one is 7.9e-3 px from it.

Tolerance of the comparisons with the restatement (tests/test_track_gpu.py's rule for one frame), U = the largest
|displacement| of the good records:
  u, v, x0, y0, misfit       2^-22 |ref| + 1e-9 U
  gradients, tensor fields   2^-22 |ref| + 1e-9 U / h
The first term is the float rounding of the outputs; the second covers the order of the double sums (the device adds the
members one after the other, numpy pairwise over all sectors)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi, speckle
from field_ref import CHANNELS, POSITION, clear_of_the_noise_threshold, field_reference, linear_weights
from test_strain_gpu import SIDE, centres, device_records, grid_rects, make_engine
from test_track_gpu import CHI_MAX, DELTA, HI, LO, VELOCITY, analytic_position, smooth_records
from track_ref import is_good

pytestmark = pytest.mark.gpu

H = float(SIDE)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = (-31, -30, 301, 299)       # ragged tiles (301 = 9 x 32 + 13, 299 = 37 x 8 + 3); two radii outside the hull
SHARE = 0.05                        # of the sectors made bad in EACH of three ways: 15 % in all
TWELVE = CHANNELS[:12]


@pytest.fixture(scope="module")
def small_pair():
    return speckle.speckle_pair(256, 256, p=(1.3, -0.7, 0.002, 0.0, 0.0, -0.001), seed=5)


def scale_of(rec, model, chi_max=CHI_MAX):
    good = is_good(rec, _ffi.N_PARAMS[model], chi_max)
    return float(np.abs(rec["p"][good][:, :1 if model == ca.FM_U else 2]).max())


def tolerance(ref, name, U):
    return 2.0 ** -22 * np.abs(np.nan_to_num(ref[name])) + 1e-9 * U / (1.0 if name in POSITION else H)


def check_against_reference(got, ref, U, what, names=CHANNELS):
    assert np.array_equal(got["status"], ref["status"]), what
    assert np.array_equal(got["neighbours"], ref["neighbours"]), what
    ok = ref["status"] == ca.FIELD_OK
    worst = 0.0
    for name in names:
        assert np.array_equal(np.isnan(got[name]), ~ok), (what, name)         # NaN exactly where there is no fit
        tol = tolerance(ref, name, U)
        err = np.abs(got[name].astype(np.float64) - ref[name])[ok]
        if err.size:
            worst = max(worst, float((err / tol[ok]).max()))
            assert (err <= tol[ok]).all(), (what, name, float(err.max()), float((err / tol[ok]).max()))
    return worst


def all_bytes(out):
    return b"".join(out[k].tobytes() for k in sorted(out))


# ---- 1. against the float64 brute force, reference frame ------------------------------------------------------------------
CASES = [(m, ca.FIELD_UNIFORM, 2.5 * H) for m in (ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY)] + \
        [(ca.FM_UVUXUYVXVY, ca.FIELD_BISQUARE, 2.5 * H), (ca.FM_UVUXUYVXVY, ca.FIELD_UNIFORM, 1.5 * H),
         (ca.FM_UVUXUYVXVY, ca.FIELD_BISQUARE, 1.5 * H)]


@pytest.mark.parametrize("model,weight,radius", CASES)
def test_map_matches_float64_brute_force(small_pair, model, weight, radius):
    assert radius == np.float32(radius) and (radius * radius) % 1.0 != 0.0
    with make_engine(*small_pair, grid_rects(), model=model) as e:
        cen = centres(e)
        assert (cen == np.round(cen)).all()
        rng = np.random.default_rng(100 * model + 10 * weight + int(radius))
        rec = smooth_records(cen, 1, rng, SHARE)[0]
        U = scale_of(rec, model)
        tensor = ca.STRAIN_SMALL if model == ca.FM_UVQ else ca.STRAIN_GREEN_LAGRANGE
        kw = dict(weight=weight, chi_max=CHI_MAX, tensor=tensor)
        ref = field_reference(cen, rec, model, radius, WINDOW, **kw)
        # conditions on the inputs: a changed summation order must not flip a membership or cross the noise threshold
        good_windows = ref["spread"][np.isfinite(ref["spread"]) & (ref["spread"] > 2.0 ** -46)]
        print(f"model {model} weight {weight} radius {radius}: smallest |distance - radius| {ref['margin']:.3g} px, "
              f"smallest spread above the band {good_windows.min():.3g}")
        assert ref["margin"] >= 1e-6, ref["margin"]
        assert clear_of_the_noise_threshold(ref["spread"])
        got = e.field_map(radius, WINDOW, channels=ca.FIELD_ALL, records=rec, **kw)
        assert set(got) == set(CHANNELS) | {"neighbours", "status"} and got["u"].shape == (299, 301)
        worst = check_against_reference(got, ref, U, (model, weight, radius))
        ok = ref["status"] == ca.FIELD_OK
        print(f"  worst error / tolerance {worst:.3g}; statuses {np.bincount(ref['status'].ravel(), minlength=3).tolist()}, "
              f"neighbours up to {ref['neighbours'].max()}")
        seen = set(ref["status"].ravel().tolist())
        assert {ca.FIELD_OK, ca.FIELD_TOO_FEW} <= seen and ok.sum() > 40000
        if radius == 2.5 * H:
            assert ca.FIELD_DEGENERATE in seen      # one row of centres seen from beyond the hull
        # the node itself and no misfit in the reference frame; the corner of the window is far from every centre
        xs, ys = WINDOW[0] + np.arange(301.0), WINDOW[1] + np.arange(299.0)
        assert np.array_equal(got["x0"][ok], np.broadcast_to(xs, (299, 301))[ok].astype(np.float32))
        assert np.array_equal(got["y0"][ok], np.broadcast_to(ys[:, None], (299, 301))[ok].astype(np.float32))
        assert not got["misfit"][ok].any()
        assert got["neighbours"][0, 0] == 0 and got["status"][0, 0] == ca.FIELD_TOO_FEW
        if model == ca.FM_U:
            assert not got["v"][ok].any() and not got["vx"][ok].any() and not got["vy"][ok].any()
        if model == ca.FM_UVUXUYVXVY and weight == ca.FIELD_UNIFORM and radius == 2.5 * H:
            # two opposite summation orders of the restatement differ by at most 0.01 of the tolerance
            rev = field_reference(cen, rec, model, radius, WINDOW, reverse=True, **kw)
            assert np.array_equal(rev["status"], ref["status"])
            for name in TWELVE:
                gap = np.abs(rev[name] - ref[name])[ok] / tolerance(ref, name, U)[ok]
                assert gap.max() <= 0.01, (name, float(gap.max()))


# ---- 2. agreement with lk_track_points ---------------------------------------------------------------------------------------
def test_map_agrees_with_track_points(small_pair):
    radius, win = 2.5 * H, (-40, 150, 64, 48)      # over the lower left edge of the hull: every status occurs
    with make_engine(*small_pair, grid_rects()) as e:
        cen = centres(e)
        rec = smooth_records(cen, 1, np.random.default_rng(7), SHARE)[0]
        U = scale_of(rec, ca.FM_UVUXUYVXVY)
        got = e.field_map(radius, win, channels=TWELVE, records=rec, chi_max=CHI_MAX)
        jj, ii = np.meshgrid(np.arange(win[3]), np.arange(win[2]), indexing="ij")
        pts = np.float32(np.stack([win[0] + ii.ravel(), win[1] + jj.ravel()], 1))
        tr, _ = e.track_points(pts, radius, records=rec[None], mode=ca.TRACK_TOTAL, chi_max=CHI_MAX)
        tr = tr[0].reshape(win[3], win[2])
        pairs = {ca.FIELD_OK: ca.TRACK_OK, ca.FIELD_TOO_FEW: ca.TRACK_TOO_FEW, ca.FIELD_DEGENERATE: ca.TRACK_DEGENERATE}
        assert np.array_equal(np.vectorize(pairs.get)(got["status"]), tr["status"])
        assert set(got["status"].ravel().tolist()) == set(pairs)
        assert np.array_equal(got["neighbours"], tr["neighbours"])
        ok = got["status"] == ca.FIELD_OK
        worst = 0.0
        for name in TWELVE:
            a, b = got[name].astype(np.float64)[ok], tr[name].astype(np.float64)[ok]
            # (test 1's rule with the track's float in the reference's place: two floats within 2^-24 of doubles that
            # differ by the order of their sums are 2^-23 apart at the most)
            tol = 2.0 ** -22 * np.abs(b) + 1e-9 * U / (1.0 if name in POSITION else H)
            worst = max(worst, float((np.abs(a - b) / tol).max()))
            assert (np.abs(a - b) <= tol).all(), (name, float(np.abs(a - b).max()))
            assert np.isnan(got[name][~ok]).all() and not tr[name][~ok].any()
        print(f"map against track_points: {int(ok.sum())} fitted nodes, worst difference / tolerance {worst:.3g}")


# ---- 3. bytes -------------------------------------------------------------------------------------------------------------------
WALK_WINDOW = (-31, -30, 120, 75)
WORKER = textwrap.dedent("""
    import os, sys
    sys.path[:0] = [os.environ["LK_ROOT"], os.path.join(os.environ["LK_ROOT"], "tests")]
    import numpy as np
    import test_field_gpu as t
    out, last = t.walk_case()
    np.savez(sys.argv[1], tiles=np.int64(last[1:]), **out)
""")


def walk_case():
    """what the two child processes of the walk test compute: both frames, both weights, on ragged tiles over the hull's edge"""
    pair = speckle.speckle_pair(256, 256, p=(1.3, -0.7, 0.002, 0.0, 0.0, -0.001), seed=5)
    with make_engine(*pair, grid_rects()) as e:
        rec = smooth_records(centres(e), 1, np.random.default_rng(3), SHARE)[0]
        out = {}
        for frame in (ca.FIELD_REFERENCE, ca.FIELD_DEFORMED):
            for weight in (ca.FIELD_UNIFORM, ca.FIELD_BISQUARE):
                got = e.field_map(2.5 * H, WALK_WINDOW, channels=ca.FIELD_ALL, weight=weight, frame=frame, iterations=3,
                                  records=rec, chi_max=CHI_MAX)
                out.update({f"{frame}{weight}_{k}": v for k, v in got.items()})
        return out, e.field_last()


def test_walked_path_gives_the_bytes_of_the_staged_one(tmp_path):
    script = tmp_path / "walk_worker.py"
    script.write_text(WORKER)
    parts = []
    for walk in ("0", "1"):
        path = tmp_path / f"walk{walk}.npz"
        r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [str(script), str(path)],
                           env=dict(os.environ, LK_ROOT=ROOT, LK_FIELD_WALK=walk), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]      # (a failed child ends the test: no second one)
        parts.append(dict(np.load(path)))
    staged, walked = parts
    tiles, fallback = staged.pop("tiles")
    assert fallback == 0 and tiles == 4 * 10
    assert walked.pop("tiles").tolist() == [tiles, tiles]
    assert sorted(staged) == sorted(walked) and len(staged) == 4 * 17
    for k in staged:
        assert staged[k].tobytes() == walked[k].tobytes(), k
    assert np.isfinite(staged["11_u"]).sum() > 3000


def test_bytes_do_not_depend_on_the_call(small_pair):
    radius = 2.5 * H
    with make_engine(*small_pair, grid_rects()) as e:
        cen = centres(e)
        rec = smooth_records(cen, 1, np.random.default_rng(3), SHARE)[0]
        for frame in (ca.FIELD_REFERENCE, ca.FIELD_DEFORMED):
            kw = dict(weight=ca.FIELD_BISQUARE, frame=frame, iterations=3, records=rec, chi_max=CHI_MAX)
            whole = e.field_map(radius, WINDOW, channels=ca.FIELD_ALL, **kw)
            assert all_bytes(whole) == all_bytes(e.field_map(radius, WINDOW, channels=ca.FIELD_ALL, **kw))   # the same call twice
            # a sub-window that starts inside a tile of the whole, against the slice of the whole
            sub = e.field_map(radius, (WINDOW[0] + 45, WINDOW[1] + 13, 101, 67), channels=ca.FIELD_ALL, **kw)
            for k in sub:
                assert sub[k].tobytes() == whole[k][13:13 + 67, 45:45 + 101].tobytes(), (frame, k)
            # stride 3: tiles of 96 x 24 pixels, other rectangles of cells
            third = e.field_map(radius, (WINDOW[0], WINDOW[1], 101, 100), stride=3, channels=ca.FIELD_ALL, **kw)
            for k in third:
                assert third[k].shape == (100, 101) and third[k].tobytes() == whole[k][::3, ::3].tobytes(), (frame, k)
            # a channel subset, in ascending bit order whatever the order asked for; no integer maps
            some = e.field_map(radius, WINDOW, channels=("misfit", "e1", "v"), want=(), **kw)
            assert sorted(some) == ["e1", "misfit", "v"]
            for k in some:
                assert some[k].tobytes() == whole[k].tobytes(), (frame, k)
            only = e.field_map(radius, WINDOW, channels=0, want=("status",), **kw)
            assert list(only) == ["status"] and only["status"].tobytes() == whole["status"].tobytes()
        # engine-held records against the same records passed from the host; reference-order mode against the default
        g = np.zeros((e.n_sectors, 6), np.float32)
        g[:, :2] = (1.3, -0.7)
        g[[9, 27], 0] = 300.0
        solved = e.correlate_all(g)
        assert (solved["error_code"] != 0).sum() >= 2
        held = e.field_map(radius, WINDOW, channels=ca.FIELD_ALL, weight=ca.FIELD_BISQUARE)
        assert all_bytes(held) == all_bytes(e.field_map(radius, WINDOW, channels=ca.FIELD_ALL, weight=ca.FIELD_BISQUARE,
                                                        records=device_records(e)))
        assert all_bytes(held) == all_bytes(e.field_map(radius, WINDOW, channels=ca.FIELD_ALL, weight=ca.FIELD_BISQUARE, records=solved))
        assert np.isfinite(held["u"]).sum() > 40000
        default = e.field_map(radius, WINDOW, channels=ca.FIELD_ALL, records=rec, chi_max=CHI_MAX)
        e.set_reference_order(1)
        assert all_bytes(default) == all_bytes(e.field_map(radius, WINDOW, channels=ca.FIELD_ALL, records=rec, chi_max=CHI_MAX))


# ---- 4. a dense domain: the tiles' rectangles do not fit into LDS ----------------------------------------------------------------
def test_dense_domain_walks_global_memory(small_pair):
    radius, win = 24.0, (100, 96, 64, 40)
    with make_engine(*small_pair, grid_rects(n=80, side=3)) as e:
        cen = centres(e)
        assert len(cen) == 6400
        rec = smooth_records(cen, 1, np.random.default_rng(12), SHARE)[0]
        U = scale_of(rec, ca.FM_UVUXUYVXVY)
        for weight in (ca.FIELD_UNIFORM, ca.FIELD_BISQUARE):
            ref = field_reference(cen, rec, ca.FM_UVUXUYVXVY, radius, win, weight=weight, chi_max=CHI_MAX)
            # (r^2 = 576 is an integer here and sectors lie exactly on the rim, 24 px from a node in x or in y: centres and
            # nodes are integers, so d2 and r2 are exact on both sides and such a member counts on both - with weight 0)
            assert ref["margin"] == 0.0 and clear_of_the_noise_threshold(ref["spread"])
            got = e.field_map(radius, win, channels=ca.FIELD_ALL, weight=weight, records=rec, chi_max=CHI_MAX)
            _, tiles, fallback = e.field_last()
            assert tiles == 2 * 5 and fallback > 0, (tiles, fallback)
            worst = check_against_reference(got, ref, U, ("dense", weight))
            print(f"dense, weight {weight}: {fallback} of {tiles} tiles walked, neighbours up to {ref['neighbours'].max()}, "
                  f"worst error / tolerance {worst:.3g}, margin {ref['margin']:.3g}")
            assert (ref["status"] == ca.FIELD_OK).all() and ref["neighbours"].min() > 100


# ---- 5. the deformed frame -------------------------------------------------------------------------------------------------
G_AFFINE = np.float64([[0.02, -0.012], [0.008, -0.02]])
A_AFFINE = np.float64([2.5, -1.5])


def test_deformed_frame_inverts_an_exact_affine_field(small_pair):
    radius, win = 2.5 * H, (20, 24, 200, 190)
    x0 = np.float64([121.5, 121.5])
    with make_engine(*small_pair, grid_rects(), model=ca.FM_UV) as e:
        c = centres(e).astype(np.float64)
        rec = np.zeros(len(c), ca.RESULT_DTYPE)
        rec["chi"], rec["n_points"] = 1.0, 361
        uv = A_AFFINE + (c - x0) @ G_AFFINE.T
        rec["p"][:, 0], rec["p"][:, 1] = uv[:, 0], uv[:, 1]
        U = float(np.abs(rec["p"][:, :2]).max())
        jj, ii = np.meshgrid(np.arange(win[3]), np.arange(win[2]), indexing="ij")
        x = np.stack([win[0] + ii, win[1] + jj], -1).astype(np.float64)
        X = x0 + (x - A_AFFINE - x0) @ np.linalg.inv(np.eye(2) + G_AFFINE).T        # the analytic inverse map
        worst = []
        for K in (1, 2, 3, 8):
            got = e.field_map(radius, win, channels=ca.FIELD_ALL, frame=ca.FIELD_DEFORMED, iterations=K, records=rec)
            assert (got["status"] == ca.FIELD_OK).all()
            worst.append(float(got["misfit"].max()))
            if K == 1:
                # X_1 = x - u(x), so the misfit |u(X_1) - u(x)| is |G u(x)|: of the order |G| U
                ux = A_AFFINE + (x - x0) @ G_AFFINE.T
                want = np.hypot(*np.moveaxis(ux @ G_AFFINE.T, -1, 0))
                assert np.abs(got["misfit"] - want).max() <= 1e-5 and 0.02 < worst[0] <= np.linalg.norm(G_AFFINE, 2) * U
        print(f"affine field, |G| U = {np.linalg.norm(G_AFFINE, 2) * U:.3g}: largest misfit after 1, 2, 3, 8 steps {worst}")
        assert worst[0] > worst[1] > worst[2] > worst[3] and worst[3] <= 1e-6
        for name, want in (("x0", X[..., 0]), ("y0", X[..., 1])):
            assert (np.abs(got[name] - want) <= 2.0 ** -22 * np.abs(want) + 1e-6).all(), name
        for name, want in zip(("ux", "uy", "vx", "vy"), G_AFFINE.ravel()):
            assert np.abs(got[name] - want).max() <= 1e-6, name
        # the displacement drawn at the node is that of the material point found: x - X
        assert np.abs(got["u"] - (x - X)[..., 0]).max() <= 2e-6 and np.abs(got["v"] - (x - X)[..., 1]).max() <= 2e-6


@pytest.mark.parametrize("weight", [ca.FIELD_UNIFORM, ca.FIELD_BISQUARE])
def test_deformed_frame_matches_float64_brute_force(small_pair, weight):
    radius, win, K = 2.5 * H, (-20, -15, 97, 75), 4
    with make_engine(*small_pair, grid_rects()) as e:
        cen = centres(e)
        rec = smooth_records(cen, 1, np.random.default_rng(46), SHARE)[0]     # (a seed that meets the two conditions below)
        U = scale_of(rec, ca.FM_UVUXUYVXVY)
        kw = dict(stride=3, weight=weight, frame=ca.FIELD_DEFORMED, iterations=K, chi_max=CHI_MAX)
        ref = field_reference(cen, rec, ca.FM_UVUXUYVXVY, radius, win, **kw)
        print(f"deformed frame, weight {weight}: smallest |distance - radius| over all iterates {ref['margin']:.3g} px")
        assert ref["margin"] >= 1e-9, ref["margin"]
        assert clear_of_the_noise_threshold(ref["spread"])
        got = e.field_map(radius, win, channels=ca.FIELD_ALL, records=rec, **kw)
        worst = check_against_reference(got, ref, U, ("deformed", weight))
        ok = ref["status"] == ca.FIELD_OK
        print(f"  worst error / tolerance {worst:.3g}; statuses {np.bincount(ref['status'].ravel(), minlength=3).tolist()}; "
              f"largest misfit {np.nanmax(ref['misfit']):.3g} px")
        assert ok.sum() > 3000 and (~ok).sum() > 500
        # the uniform window's field has steps, which a fixed-point iteration cannot cross: only the bisquare map converges
        assert (np.nanmax(ref["misfit"]) < 1e-3) == (weight == ca.FIELD_BISQUARE)
        # the point found is not the node: the map is drawn where the material went
        assert np.nanmax(np.abs(ref["x0"] - (win[0] + 3.0 * np.arange(win[2])))) > 1.0


# ---- 6. smoothness: what the bisquare weight is for ------------------------------------------------------------------------------
def test_bisquare_map_has_smaller_steps_than_the_uniform_one(small_pair):
    radius, win = 2.5 * H, (70, 121, 110, 1)          # an interior row of nodes, 2.5 pitches inside the hull
    with make_engine(*small_pair, grid_rects(), model=ca.FM_UV) as e:
        cen = centres(e)
        rng = np.random.default_rng(19)
        rec = smooth_records(cen, 1, rng, 0.0)[0]
        rec["error_code"][:] = 0
        rec["chi"][:] = 1.0
        finite = np.isfinite(rec["p"][:, 0])
        rec["p"][~finite, 0] = 0.0
        rec["p"][:, :2] += rng.normal(0, 0.3, (len(cen), 2)).astype(np.float32)      # a noisy field
        U = scale_of(rec, ca.FM_UV, 0.0)
        jump = {}
        for weight in (ca.FIELD_UNIFORM, ca.FIELD_BISQUARE):
            got = e.field_map(radius, win, channels=("u",), weight=weight, records=rec)
            ref = field_reference(cen, rec, ca.FM_UV, radius, win, weight=weight)
            assert (got["status"] == ca.FIELD_OK).all()
            dev, res = np.diff(got["u"][0].astype(np.float64)), np.diff(ref["u"][0])
            tol = tolerance(ref, "u", U)[0]
            assert (np.abs(dev - res) <= tol[1:] + tol[:-1]).all()      # each end within its tolerance
            jump[weight] = float(np.abs(dev).max())
            assert abs(jump[weight] - float(np.abs(res).max())) <= 2 * tol.max()
        print(f"largest step between adjacent nodes: uniform {jump[0]:.3g} px, bisquare {jump[1]:.3g} px")
        assert jump[ca.FIELD_BISQUARE] < jump[ca.FIELD_UNIFORM]


# ---- 7. end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", [ca.FIELD_UNIFORM, ca.FIELD_BISQUARE])
def test_end_to_end_on_a_solved_pair(weight):
    frames = speckle.speckle_sequence(256, 256, 2, velocity=VELOCITY, dilation=DELTA, seed=5)     # the track test's first pair
    radius = 2.5 * H
    lo = int(np.ceil(LO + radius))
    n = (int(np.floor(HI - radius)) - lo) // 4 + 1
    win = (lo, lo, n, n)                                  # interior nodes: a radius inside the hull, every 4th pixel
    with make_engine(frames[0], frames[1], grid_rects()) as e:
        c = centres(e).astype(np.float64)
        g = np.zeros((e.n_sectors, 6), np.float32)
        g[:, :2] = VELOCITY
        rec = e.correlate_all(g)
        good = is_good(rec, 6, 0.0)
        assert good.sum() >= 130
        truth = analytic_position(c, 1) - c                # affine: the fit reproduces it whatever the weights
        E = np.abs(rec["p"][:, :2] - truth)
        got = e.field_map(radius, win, stride=4, channels=("u", "v"), weight=weight)
        assert (got["status"] == ca.FIELD_OK).all()
        worst = 0.0
        for j in range(n):
            for i in range(n):
                X = np.float64([lo + 4 * i, lo + 4 * j])
                idx, l = linear_weights(c, good, X[0], X[1], radius, weight)
                assert len(idx) == got["neighbours"][j, i]
                want = analytic_position(X, 1) - X
                for k, name in enumerate(("u", "v")):
                    # a derived bound: the fit is linear in the data and exact on the affine truth; + the output's rounding
                    bound = np.abs(l).sum() * E[idx, k].max() + 2.0 ** -23 * abs(want[k])
                    err = abs(float(got[name][j, i]) - want[k])
                    worst = max(worst, err / bound)
                    assert err <= bound, (name, i, j, err, bound)
        print(f"end to end, weight {weight}: {n * n} nodes, largest record error {E[good].max():.4f} px, worst error / bound {worst:.3f}")


# ---- 8. nothing of the engine moves; arguments ------------------------------------------------------------------------------
def test_engine_state_is_untouched(small_pair):
    rects = grid_rects(n=8)
    S = len(rects)
    with make_engine(*small_pair, rects) as e:
        g = np.zeros((S, 6), np.float32)
        g[[9, 27], 0] = 300.0
        first = e.correlate_all(g)
        e.reseed_failed(1.5 * H)
        strain = e.strain_field(2.5 * H)
        win = (0, 0, 160, 150)

        def state():
            return dict(records=device_records(e), guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(),
                        stats=e.sector_stats(), reseed=e.reseed_info(), counters=np.array(sorted(e.stats().items()), dtype=object))

        def same(a, b):
            for k in a:
                assert (a[k] == b[k]).all() if k == "counters" else a[k].tobytes() == b[k].tobytes(), k

        kept = state()
        a = e.field_map(2.5 * H, win, channels=ca.FIELD_ALL)
        b = e.field_map(1.5 * H, win, channels=("u", "e1"), weight=ca.FIELD_BISQUARE, frame=ca.FIELD_DEFORMED, records=first,
                        chi_max=5.0, min_neighbours=4, tensor=ca.STRAIN_SMALL)
        assert all_bytes(a) == all_bytes(e.field_map(2.5 * H, win, channels=ca.FIELD_ALL)) and b["u"].tobytes() != a["u"].tobytes()
        assert (a["status"] == ca.FIELD_OK).sum() > 15000
        same(kept, state())
        assert e.strain_field(2.5 * H).tobytes() == strain.tobytes()         # another pass's output
        # a rebuild of the lists that waits for the next solve keeps waiting (as tests/test_track_gpu.py)
        e.update_sector(20, 0)
        kept = state()
        assert all_bytes(e.field_map(2.5 * H, win, channels=ca.FIELD_ALL)) == all_bytes(a)
        same(kept, state())
        after = e.correlate_all(np.zeros((S, 6), np.float32))
        assert (after["error_code"] == 0).sum() >= S - 2


def test_arguments_and_refusals(small_pair):
    e = make_engine(*small_pair, grid_rects(n=3), commit=False)
    lib, h = e.lib, e._h
    P = C.c_void_p
    rec = np.zeros(9, ca.RESULT_DTYPE)
    rec["p"][:, 0] = np.arange(9)
    maps = np.full((2, 5, 6), 7.0, np.float32)
    nbrs, status = np.full((5, 6), 7, np.int32), np.full((5, 6), 7, np.uint8)
    GOOD = dict(radius=47.5, chi_max=0.0, min_neighbours=3, tensor=0, weight=0, frame=0, iterations=0, x0=20, y0=20, nx=6, ny=5,
                stride=2, channels=ca.FIELD_U | ca.FIELD_E1)

    def config(**kw):
        d = dict(GOOD, **kw)
        reserved = d.pop("reserved", (0, 0, 0))
        return _ffi.LkFieldMapConfig(*d.values(), (C.c_int * 3)(*reserved))

    def ptr(a):
        return a.ctypes.data_as(P) if a is not None else None

    def refused(cfg=True, records=rec, m=maps, n=nbrs, s=status, **kw):
        c = config(**kw) if cfg else None
        rc = lib.lk_field_map(h, C.byref(c) if c is not None else None, ptr(records), ptr(m), ptr(n), ptr(s))
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and "lk_field_map" in msg, (rc, msg)
        assert (maps == 7.0).all() and (nbrs == 7).all() and (status == 7).all()      # outputs untouched
        return msg

    assert "no committed sectors" in refused()
    e.commit_sectors()
    assert "no solve" in refused(records=None)                   # records == NULL before any batch solve
    assert "configuration" in refused(cfg=False)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "radius" in refused(radius=bad)
    for bad in (float("nan"), float("inf")):
        assert "chi_max" in refused(chi_max=bad)
    for bad in (2, 0, -1):
        assert "min_neighbours" in refused(min_neighbours=bad)
    for bad in (-1, 2):
        assert "tensor" in refused(tensor=bad)
        assert "weight" in refused(weight=bad)
        assert "frame" in refused(frame=bad)
    for bad in (0, -1, 17):
        assert "iterations" in refused(frame=ca.FIELD_DEFORMED, iterations=bad)
    for bad in (0, -1):
        assert "nx, ny and stride" in refused(nx=bad)
        assert "nx, ny and stride" in refused(ny=bad)
        assert "nx, ny and stride" in refused(stride=bad)
    assert "2^31 - 1" in refused(nx=65536, ny=32768)
    assert "no output" in refused(channels=0, n=None, s=None)
    assert "unknown channel" in refused(channels=1 << 15)
    assert "unknown channel" in refused(channels=0x80000001)
    assert "no maps" in refused(m=None)
    for k in range(3):
        assert "reserved" in refused(reserved=tuple(int(i == k) for i in range(3)))
    assert lib.lk_field_map(None, C.byref(config()), ptr(rec), ptr(maps), ptr(nbrs), ptr(status)) == ca.ERROR_BAD_DOMAIN
    # iterations is not read in the reference frame; the call itself, and through Python
    c = config(iterations=99)
    assert lib.lk_field_map(h, C.byref(c), ptr(rec), ptr(maps), ptr(nbrs), ptr(status)) == 0
    got = e.field_map(47.5, (20, 20, 6, 5), stride=2, channels=("e1", "u"), records=rec)
    assert maps[0].tobytes() == got["u"].tobytes() and maps[1].tobytes() == got["e1"].tobytes()
    assert nbrs.tobytes() == got["neighbours"].tobytes() and status.tobytes() == got["status"].tobytes()
    assert (got["status"] == ca.FIELD_OK).all() and got["neighbours"].max() <= 9
    # each integer map alone, and no map at all but one of them
    assert lib.lk_field_map(h, C.byref(config(channels=0)), ptr(rec), None, ptr(nbrs), None) == 0
    assert lib.lk_field_map(h, C.byref(config(channels=0)), ptr(rec), None, None, ptr(status)) == 0
    # a solve in flight refuses the engine-held records and finishes normally afterwards
    maps[:], nbrs[:], status[:] = 7.0, 7, 7
    e.correlate_all_async()
    assert "waited for" in refused(records=None)
    solved = e.wait_results()
    assert all_bytes(e.field_map(47.5, (20, 20, 6, 5))) == all_bytes(e.field_map(47.5, (20, 20, 6, 5), records=solved))
    e.close()
