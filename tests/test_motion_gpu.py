"""Global motion per frame (lk_rigid_motion, include/lk_engine.h) on the GPU: against the float64 brute force of
tests/motion_ref.py on synthetic records; the small-strain tensor under a rotation, before and after the removal; a datum
mask and trimmed outliers; chunks, repeats, subsets and shuffles byte for byte; the three record sources end to end on a
rotated speckle pair; that nothing of the engine moves; arguments.

Domain: 12 x 12 sectors of 19 x 19 (pitch h = 19) on 256 x 256 images, as tests/test_strain_gpu.py.

Tolerances of the comparisons with the restatement (derived in tests/motion_ref.py's docstring):
  the twelve sums      2 (n - 1) 2^-53 sum |term|: the worst case of any two summation orders of n terms; the count is exact
  the record's floats  2^-22 |ref| + bound, `bound` being what that difference of the sums does to the field, to first order
                       with every constant rounded up (of the order of 1e-12 here): the first term is the rounding to float
Byte for byte: a frame's record against lk_motion_from_sums of the device's own sums (theta: one float ulp, it alone goes
through atan2), and records_out against lk_motion_remove of the device's own record."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi, speckle
from motion_ref import FLOATS, FROM_SUMS, is_good, motion_reference, origin_of
from test_strain_gpu import SIDE, centres, device_records, grid_rects, make_engine
from test_track_gpu import CHI_MAX, smooth_records

pytestmark = pytest.mark.gpu

H = float(SIDE)
KINDS = [ca.MOTION_TRANSLATION, ca.MOTION_RIGID, ca.MOTION_SIMILARITY, ca.MOTION_AFFINE]
CASES = [(k, m) for k in KINDS for m in (ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY)
         if m != ca.FM_U or k == ca.MOTION_TRANSLATION]
MID = np.float64([121.5, 121.5])          # the middle of the 12 x 12 centres 17 + 19 i


@pytest.fixture(scope="module")
def small_pair():
    return speckle.speckle_pair(256, 256, p=(1.3, -0.7, 0.002, 0.0, 0.0, -0.001), seed=5)


def rotation(deg):
    th = np.deg2rad(deg)
    return np.float64([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])


def records_of_map(cen, F, t=(0.0, 0.0), about=MID):
    """six-parameter records of the homogeneous map x -> about + t + F (x - about), all good"""
    X = cen.astype(np.float64)
    rec = np.zeros(len(cen), ca.RESULT_DTYPE)
    rec["p"][:, :2] = (X - about) @ np.float64(F).T + about + np.float64(t) - X
    rec["p"][:, 2:6] = (np.float64(F) - np.eye(2)).ravel()
    rec["chi"], rec["n_points"], rec["iterations"] = 0.5, 361, 5
    rec["und_cx"], rec["und_cy"] = cen[:, 0], cen[:, 1]
    return rec


def check_sums(sums, ref, what):
    n = int(ref["sums"][0])
    assert sums[0] == n, what
    tol = 2.0 * max(n - 1, 0) * 2.0 ** -53 * ref["abs_sums"][1:]
    err = np.abs(sums[1:] - ref["sums"][1:])
    assert (err <= tol).all(), (what, err, tol)
    return float((err / np.maximum(tol, 1e-300)).max())


def check_floats(m, ref, what):
    """the record against the restatement's: ints exact, floats within 2^-22 |ref| + bound"""
    for k in ("n_fit", "n_rejected", "status", "passes_run"):
        assert int(m[k]) == ref[k], (what, k, int(m[k]), ref[k])
    worst = 0.0
    for k in FLOATS:
        if ref["status"] != ca.MOTION_OK:
            assert m[k] == 0, (what, k)
            continue
        tol = 2.0 ** -22 * abs(ref[k]) + ref["bound"][k]
        err = abs(float(m[k]) - ref[k])
        assert err <= tol, (what, k, float(m[k]), ref[k], err, tol)
        worst = max(worst, err / tol) if tol > 0 else worst
    return worst


def check_from_sums(kind, m, sums, origin, min_sectors=None):
    """the record = lk_motion_from_sums of the device's own sums, byte for byte (theta: one float ulp)"""
    host = ca.motion_from_sums(kind, int(sums[0]), sums[1:], origin, min_sectors)
    for k in FROM_SUMS:
        assert m[k].tobytes() == host[k].tobytes(), (k, m[k], host[k])
    assert abs(float(m["theta"]) - float(host["theta"])) <= np.spacing(np.abs(host["theta"])), (m["theta"], host["theta"])


# ---- 1. against the float64 brute force ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,model", CASES)
def test_motion_matches_float64_brute_force(small_pair, kind, model):
    with make_engine(*small_pair, grid_rects(), model=model) as e:
        cen = centres(e)
        o = origin_of(cen)
        rng = np.random.default_rng(100 * kind + model)
        rec = smooth_records(cen, 5, rng, 0.07)
        got, out, sums = e.rigid_motion(kind, records=rec, chi_max=CHI_MAX, return_records=True, return_sums=True)
        assert got.shape == (5,) and out.shape == (5, 144) and sums.shape == (5, 12)
        for f in range(5):
            ref = motion_reference(cen, rec[f], model, kind, CHI_MAX)
            assert ref["status"] == ca.MOTION_OK and 100 <= ref["n_fit"] < 144
            w_s = check_sums(sums[f], ref, (kind, model, f))
            w_f = check_floats(got[f], ref, (kind, model, f))
            check_from_sums(kind, got[f], sums[f], o)
            want = ca.motion_remove(model, got[f], cen, rec[f], good=ref["good"])
            assert out[f].tobytes() == want.tobytes(), (kind, model, f)
            assert out[f][~ref["good"]].tobytes() == rec[f][~ref["good"]].tobytes()
            print(f"kind {kind} model {model} frame {f}: n {ref['n_fit']}, sums error / bound {w_s:.3g}, floats error / tolerance "
                  f"{w_f:.3g}, rms {got[f]['rms']:.4f} px, theta {got[f]['theta']:.6f}")
        if model == ca.FM_U:
            assert not got["ty"].any() and (out["p"][..., 1:] == rec["p"][..., 1:])[np.isfinite(rec["p"][..., 1:])].all()
        # without the outputs that were not asked for: the same motion
        assert e.rigid_motion(kind, records=rec, chi_max=CHI_MAX).tobytes() == got.tobytes()


# ---- 2. the small-strain tensor under a rotation ---------------------------------------------------------------------------
def test_small_strain_is_restored_under_rotation(small_pair):
    with make_engine(*small_pair, grid_rects()) as e:
        cen = centres(e)
        stretch = np.diag([1.01, 1.0])
        rec = records_of_map(cen, rotation(2.0) @ stretch)
        # both expectations in float64: the small-strain exx of the rotated stretch, and of the stretch alone
        exx_rotated, exx_stretch = 1.01 * np.cos(np.deg2rad(2.0)) - 1.0, 0.01
        assert abs((exx_rotated - exx_stretch) - 1.01 * (np.cos(np.deg2rad(2.0)) - 1.0)) < 1e-15
        U = float(np.abs(rec["p"][:, :2]).max())
        tol = float(np.spacing(np.float32(U))) / H          # the float rounding of the records, over one pitch
        before = e.strain_field(2.5 * H, tensor=ca.STRAIN_SMALL, records=rec)
        assert (before["status"] == ca.STRAIN_OK).all()
        off = np.abs(before["exx"].astype(np.float64) - exx_rotated).max()
        m, out = e.rigid_motion(ca.MOTION_RIGID, records=rec, return_records=True)
        assert m["status"][0] == ca.MOTION_OK and abs(float(m["theta"][0]) - np.deg2rad(2.0)) < 1e-6
        after = e.strain_field(2.5 * H, tensor=ca.STRAIN_SMALL, records=out[0])
        err = {k: np.abs(after[k].astype(np.float64) - w).max() for k, w in (("exx", exx_stretch), ("eyy", 0.0), ("exy", 0.0))}
        print(f"small strain: before, |exx - rotated stretch| {off:.3g}; after, |exx - 0.01| {err['exx']:.3g}, |eyy| {err['eyy']:.3g}, "
              f"|exy| {err['exy']:.3g}; tolerance {tol:.3g}; the rotation alone is worth {exx_stretch - exx_rotated:.3g}")
        assert off <= tol
        assert exx_stretch - exx_rotated > 6e-4            # about 1 - cos 2 degrees: what the removal has to bring back
        assert max(err.values()) <= tol
        # the records' own gradients lose the rotation as well
        assert np.abs(out[0]["p"][:, 2:6].astype(np.float64) - [0.01, 0, 0, 0]).max() <= 2.0 ** -22


# ---- 3. a datum mask, and trimmed outliers -----------------------------------------------------------------------------------
def test_datum_mask_and_trimming(small_pair):
    with make_engine(*small_pair, grid_rects()) as e:
        cen = centres(e)
        o = origin_of(cen)
        rng = np.random.default_rng(3)
        # the two left-hand columns (sectors 0 .. 23) turn by 3 degrees and slip; the rest turns by 1 degree and stretches
        rec = records_of_map(cen, rotation(1.0) @ np.diag([1.02, 0.99]), t=(0.5, 0.25))
        grip = records_of_map(cen, rotation(3.0), t=(4.0, -2.5), about=np.float64([26.5, 121.5]))
        mask = np.arange(144) < 24
        rec[mask] = grip[mask]
        rec["p"][:, :2] += rng.normal(0, 0.02, (144, 2))
        rec["error_code"][[5, 40, 77]] = 3
        m, out, sums = e.rigid_motion(ca.MOTION_RIGID, records=rec, fit_mask=mask, return_records=True, return_sums=True)
        ref = motion_reference(cen, rec, ca.FM_UVUXUYVXVY, ca.MOTION_RIGID, fit_mask=mask)
        assert ref["n_fit"] == 23 == m["n_fit"][0]
        check_sums(sums[0], ref, "mask")
        check_floats(m[0], ref, "mask")
        check_from_sums(ca.MOTION_RIGID, m[0], sums[0], o)
        assert abs(float(m["theta"][0]) - np.deg2rad(3.0)) < 2e-3          # the grip's motion, not the specimen's
        # every good sector is un-rotated, in the mask or not
        assert out[0].tobytes() == ca.motion_remove(ca.FM_UVUXUYVXVY, m[0], cen, rec, good=ref["good"]).tobytes()
        moved = out[0]["p"][:, 0] != rec["p"][:, 0]
        assert moved[ref["good"]].all() and not moved[~ref["good"]].any()
        assert np.abs(out[0]["p"][mask & ref["good"], :2]).max() < 0.1     # the grip stands still now

        # 10 % of the sectors displaced by 5 px, in directions that cancel: the second pass leaves them out
        clean = records_of_map(cen, rotation(1.5), t=(2.0, 1.0))
        clean["p"][:, :2] += rng.normal(0, 0.02, (144, 2))
        clean["error_code"][[9, 100]] = 2
        hit = np.sort(rng.permutation(np.flatnonzero(clean["error_code"] == 0))[:14])
        phi = 2 * np.pi * np.arange(14) / 14
        dirty = clean.copy()
        dirty["p"][hit, 0] += 5 * np.cos(phi)
        dirty["p"][hit, 1] += 5 * np.sin(phi)
        ref = motion_reference(cen, dirty, ca.FM_UVUXUYVXVY, ca.MOTION_RIGID, reject=3.0, passes=2)
        print(f"trimming: smallest |residual - threshold| {ref['margin']:.3g} px, rms after {ref['rms']:.4f} px")
        assert ref["margin"] >= 1e-6 and ref["n_rejected"] == 14 and not ref["keep"][hit].any()
        m, sums = e.rigid_motion(ca.MOTION_RIGID, records=dirty, reject=3.0, passes=2, return_sums=True)
        assert m["n_rejected"][0] == 14 and m["passes_run"][0] == 2 and m["n_fit"][0] == 142 - 14
        check_sums(sums[0], ref, "trimmed")
        check_floats(m[0], ref, "trimmed")
        # ... and equals the fit of the clean sectors alone
        alone = clean.copy()
        alone["error_code"][hit] = 1
        ref_clean = motion_reference(cen, alone, ca.FM_UVUXUYVXVY, ca.MOTION_RIGID)
        for k in FLOATS:
            assert abs(float(m[0][k]) - ref_clean[k]) <= 2.0 ** -22 * abs(ref_clean[k]) + ref_clean["bound"][k], k
        one = e.rigid_motion(ca.MOTION_RIGID, records=dirty)
        assert one["n_rejected"][0] == 0 and one["passes_run"][0] == 1 and one["rms"][0] > 1.0 > m["rms"][0]


# ---- 4. chunks and invariance ----------------------------------------------------------------------------------------------
def test_chunks_repeats_subsets_and_shuffles_give_the_same_bytes(small_pair, monkeypatch):
    with make_engine(*small_pair, grid_rects()) as e:
        cen = centres(e)
        rng = np.random.default_rng(4)
        rec = smooth_records(cen, 5, rng, 0.07)
        kw = dict(records=rec, chi_max=CHI_MAX, reject=1.5, passes=2, return_records=True, return_sums=True)
        results = {}
        for chunk in (64, 2048):
            monkeypatch.setenv("LK_MOTION_CHUNK", str(chunk))
            got = e.rigid_motion(ca.MOTION_SIMILARITY, **kw)
            _, used, chunks = e.motion_last()
            assert used == chunk and chunks == (3 if chunk == 64 else 1)       # 144 = 64 + 64 + 16: the last chunk is partial
            for f in range(5):
                ref = motion_reference(cen, rec[f], ca.FM_UVUXUYVXVY, ca.MOTION_SIMILARITY, CHI_MAX, reject=1.5, passes=2)
                assert ref["margin"] >= 1e-6
                check_sums(got[2][f], ref, (chunk, f))
                check_floats(got[0][f], ref, (chunk, f))
            # each repeats its own bytes
            again = e.rigid_motion(ca.MOTION_SIMILARITY, **kw)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
            # frame 3 alone = frame 3 inside the call
            alone = e.rigid_motion(ca.MOTION_SIMILARITY, **dict(kw, records=rec[3:4]))
            assert all(a[0].tobytes() == b[3].tobytes() for a, b in zip(alone, got))
            results[chunk] = got
        monkeypatch.delenv("LK_MOTION_CHUNK")
        default = e.rigid_motion(ca.MOTION_SIMILARITY, **kw)
        assert e.motion_last()[1] == 2048 and all(a.tobytes() == b.tobytes() for a, b in zip(default, results[2048]))
        assert results[64][0]["n_fit"].tobytes() == results[2048][0]["n_fit"].tobytes()
        # under a datum mask, shuffling which sectors outside it are bad changes neither the motion nor the others' records
        mask = np.arange(144) < 36
        base = smooth_records(cen, 1, rng, 0.0)[0]
        base["error_code"][:] = 0
        base["chi"][:] = 1.0
        base["p"][np.isnan(base["p"][:, 0]), 0] = 0.25
        a, b = base.copy(), base.copy()
        a["error_code"][[50, 60, 70, 143]] = 1
        b["error_code"][[51, 60, 99, 100]] = 4
        ma, oa = e.rigid_motion(ca.MOTION_RIGID, records=a, fit_mask=mask, return_records=True)
        mb, ob = e.rigid_motion(ca.MOTION_RIGID, records=b, fit_mask=mask, return_records=True)
        both = (a["error_code"] == 0) & (b["error_code"] == 0)
        assert ma.tobytes() == mb.tobytes() and ma["n_fit"][0] == 36
        assert oa[0][both].tobytes() == ob[0][both].tobytes() and both.sum() == 137


# ---- 5. the three sources, end to end ------------------------------------------------------------------------------------------
ANGLE, SHIFT = 1.0, (1.3, -0.7)


def rotated_pair():
    c, s = np.cos(np.deg2rad(ANGLE)), np.sin(np.deg2rad(ANGLE))
    p = np.float32([SHIFT[0], SHIFT[1], c - 1, -s, s, c - 1])
    und, dfm = speckle.speckle_pair(256, 256, p=tuple(p), seed=5)
    theta_true = float(np.arctan2(np.float64(p[4]), 1.0 + np.float64(p[2])))
    return und, dfm, p, theta_true


def angle_bound(m, cen, good):
    X = cen[good].astype(np.float64)
    return 5.0 * (float(m["rms"]) / np.sqrt(2.0)) / np.sqrt(((X - X.mean(axis=0)) ** 2).sum())


def test_sources_end_to_end_on_a_rotated_pair():
    und, dfm, p, theta_true = rotated_pair()
    with make_engine(und, dfm, grid_rects()) as e:
        cen = centres(e)
        g = np.zeros((144, 6), np.float32)
        g[:, :2] = p[:2] + (cen - 128.0) @ np.float32([[p[2], p[3]], [p[4], p[5]]]).T
        rec = e.correlate_all(g)
        good = is_good(rec, 6, 0.0)
        assert good.sum() >= 140
        # the engine-held records read in place = the fetched records passed back in
        kw = dict(return_records=True, return_sums=True)
        eng = e.rigid_motion(ca.MOTION_RIGID, source=ca.TRACK_RECORDS_ENGINE, **kw)
        default = e.rigid_motion(ca.MOTION_RIGID, **kw)
        caller = e.rigid_motion(ca.MOTION_RIGID, records=rec, **kw)
        for a, b, c in zip(eng, default, caller):
            assert a.tobytes() == c.tobytes() and b.tobytes() == c.tobytes()
        m = eng[0][0]
        assert m["status"] == ca.MOTION_OK and m["n_fit"] == good.sum()
        bound = angle_bound(m, cen, good)
        print(f"rotated pair: theta {float(m['theta']):.7f} of {theta_true:.7f} rad, |difference| {abs(float(m['theta']) - theta_true):.3g}, "
              f"bound {bound:.3g}; rms {float(m['rms']):.4f} px over {int(m['n_fit'])} sectors; t = ({float(m['tx']):.4f}, {float(m['ty']):.4f})")
        assert abs(float(m["theta"]) - theta_true) <= bound
        # a short window: the device records read in place = wait_sequence's host copy passed back in
        e.sequence_reserve(2)
        for i in range(2):
            e.sequence_set_frame(i, dfm)
        e.adjust_initial_guess(0, False, p, (128.0, 128.0))
        win = e.correlate_sequence(2, constant_velocity=False)
        assert win.shape == (2, 144)
        inplace = e.rigid_motion(ca.MOTION_RIGID, source=ca.TRACK_RECORDS_WINDOW, **kw)
        counted = e.rigid_motion(ca.MOTION_RIGID, n_frames=2, source=ca.TRACK_RECORDS_WINDOW, **kw)
        passed = e.rigid_motion(ca.MOTION_RIGID, records=win, **kw)
        for a, b, c in zip(inplace, counted, passed):
            assert a.shape[0] == 2 and a.tobytes() == c.tobytes() and b.tobytes() == c.tobytes()
        for f in range(2):
            gw = is_good(win[f], 6, 0.0)
            assert gw.sum() >= 140 and inplace[0][f]["status"] == ca.MOTION_OK
            assert abs(float(inplace[0][f]["theta"]) - theta_true) <= angle_bound(inplace[0][f], cen, gw)


# ---- 6. nothing of the engine moves ----------------------------------------------------------------------------------------
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

        def state():
            return dict(records=device_records(e), guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(),
                        stats=e.sector_stats(), reseed=e.reseed_info() if not reference_order else np.zeros(1),
                        counters=np.array(sorted(e.stats().items()), dtype=object))

        def same(a, b):
            for k in a:
                assert (a[k] == b[k]).all() if k == "counters" else a[k].tobytes() == b[k].tobytes(), k

        kept = state()
        a = e.rigid_motion(ca.MOTION_RIGID, source=ca.TRACK_RECORDS_ENGINE, return_records=True, return_sums=True)
        b = e.rigid_motion(ca.MOTION_RIGID, return_records=True, return_sums=True)        # (no records: the engine's, by default)
        c = e.rigid_motion(ca.MOTION_AFFINE, records=np.stack([first, first]), chi_max=5.0, reject=3.0, passes=3,
                           fit_mask=np.arange(S) % 2, return_records=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[0].shape == (1,) and c[0].shape == (2,)
        assert a[0].tobytes() == e.rigid_motion(ca.MOTION_RIGID, records=kept["records"]).tobytes()
        assert a[0]["status"][0] == ca.MOTION_OK and a[0]["n_fit"][0] >= S - 4
        same(kept, state())
        # a rebuild of the lists that waits for the next solve keeps waiting: after lk_update_sector has turned a sector
        # into a list the device still holds the centres the records were solved at, and the motion is the same bytes
        e.update_sector(20, 0)
        kept = state()
        assert e.rigid_motion(ca.MOTION_RIGID).tobytes() == a[0].tobytes()
        same(kept, state())
        # ... and the next solve carries the rebuild out as if nothing had been asked in between
        after = e.correlate_all(np.zeros((S, 6), np.float32))
        assert (after["error_code"] == 0).sum() >= S - 2


# ---- 7. arguments ------------------------------------------------------------------------------------------------------------
def test_arguments_and_refusals(small_pair):
    rects = grid_rects(n=3)
    e = make_engine(*small_pair, rects, commit=False)
    lib, h = e.lib, e._h
    P = C.c_void_p
    rec = np.zeros((2, 9), ca.RESULT_DTYPE)
    rec["p"][..., 0] = np.arange(9)
    out = np.full(2, 7, ca.MOTION_DTYPE)
    mask = np.ones(9, np.uint8)
    names = ("kind", "source", "chi_max", "reject", "passes", "min_sectors", "r0", "r1")
    GOOD = (ca.MOTION_RIGID, ca.TRACK_RECORDS_CALLER, 0.0, 0.0, 1, 2, 0, 0)

    def config(values):
        v = dict(zip(names, values))
        c = _ffi.LkMotionConfig(v["kind"], v["source"], v["chi_max"], v["reject"], v["passes"], v["min_sectors"])
        c.reserved[0], c.reserved[1] = v["r0"], v["r1"]
        return c

    def refused(cfg=GOOD, n_frames=2, records=rec, output=out):
        c = config(cfg) if cfg is not None else None
        rc = lib.lk_rigid_motion(h, C.byref(c) if c is not None else None, n_frames,
                                 records.ctypes.data_as(P) if records is not None else None, mask.ctypes.data_as(P),
                                 output.ctypes.data_as(P) if output is not None else None, None, None)
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and "lk_rigid_motion" in msg, (rc, msg)
        assert (out == np.full(1, 7, ca.MOTION_DTYPE)).all()
        return msg

    def with_(**kw):
        d = dict(zip(names, GOOD))
        d.update(kw)
        return tuple(d.values())

    assert "no committed sectors" in refused()
    e.commit_sectors()
    assert "configuration" in refused(None)
    assert "output" in refused(output=None)
    for bad in (-1, 4):
        assert "kind" in refused(with_(kind=bad))
    for bad in (0, -1, 5):
        assert "passes" in refused(with_(passes=bad, reject=3.0))
    for bad in (0.0, -1.0):
        assert "reject" in refused(with_(passes=2, reject=bad))
    for bad in (float("nan"), float("inf")):
        assert "chi_max" in refused(with_(chi_max=bad))
        assert "reject" in refused(with_(reject=bad))
    for kind, least in ((0, 1), (1, 2), (2, 2), (3, 3)):
        for bad in (least - 1, -1):
            assert "min_sectors" in refused(with_(kind=kind, min_sectors=bad))
    assert "reserved" in refused(with_(r0=1)) and "reserved" in refused(with_(r1=-1))
    for bad in (-1, 3):
        assert "source" in refused(with_(source=bad))
    for bad in (0, -1):
        assert "n_frames" in refused(n_frames=bad)
    # the records / n_frames / source combinations of lk_track_points
    assert "records" in refused(records=None)                                                    # CALLER without records
    assert "records" in refused(with_(source=ca.TRACK_RECORDS_ENGINE), n_frames=1)              # ENGINE with records
    assert "records" in refused(with_(source=ca.TRACK_RECORDS_WINDOW))                          # WINDOW with records
    assert "n_frames" in refused(with_(source=ca.TRACK_RECORDS_ENGINE), records=None, n_frames=2)
    assert "no solve" in refused(with_(source=ca.TRACK_RECORDS_ENGINE), records=None, n_frames=1)
    assert "no window" in refused(with_(source=ca.TRACK_RECORDS_WINDOW), records=None, n_frames=0)
    for n in (None, 0, 2):
        with pytest.raises(ca.LkError, match="no window"):
            e.rigid_motion(ca.MOTION_RIGID, n_frames=n, source=ca.TRACK_RECORDS_WINDOW)
    assert "n_frames" in refused(with_(source=ca.TRACK_RECORDS_WINDOW), records=None, n_frames=-1)
    assert lib.lk_rigid_motion(None, None, 2, None, None, None, None, None) == ca.ERROR_BAD_DOMAIN
    with pytest.raises(ValueError):
        e.rigid_motion(ca.MOTION_RIGID, records=rec, fit_mask=np.ones(5))
    # records passed in need no solve; the direct call gives what the Python call gives
    got = e.rigid_motion(ca.MOTION_TRANSLATION, records=rec)
    assert (got["status"] == ca.MOTION_OK).all() and (got["n_fit"] == 9).all() and (got["tx"] == 4.0).all()
    few = e.rigid_motion(ca.MOTION_AFFINE, records=rec, min_sectors=10, return_records=True)
    assert (few[0]["status"] == ca.MOTION_TOO_FEW).all() and few[1].tobytes() == rec.tobytes() and not few[0]["tx"].any()
    c = config(with_(kind=ca.MOTION_TRANSLATION, min_sectors=1))
    direct = np.zeros(2, ca.MOTION_DTYPE)
    assert lib.lk_rigid_motion(h, C.byref(c), 2, rec.ctypes.data_as(P), None, direct.ctypes.data_as(P), None, None) == 0
    assert direct.tobytes() == got.tobytes()
    # a solve in flight refuses the engine-held records and finishes normally afterwards
    e.correlate_all_async()
    assert "waited for" in refused(with_(source=ca.TRACK_RECORDS_ENGINE), records=None, n_frames=1)
    solved = e.wait_results()
    assert e.rigid_motion(ca.MOTION_RIGID).tobytes() == e.rigid_motion(ca.MOTION_RIGID, records=solved).tobytes()
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
    want = e.rigid_motion(ca.MOTION_RIGID, records=win)
    for n in (None, 0, 2):
        got = e.rigid_motion(ca.MOTION_RIGID, n_frames=n, source=ca.TRACK_RECORDS_WINDOW)
        assert got.shape == (2,) and got.tobytes() == want.tobytes(), n
    e.close()
    # a one-parameter model has no v: a translation alone
    with make_engine(*small_pair, rects, model=ca.FM_U) as e1:
        for kind in (ca.MOTION_RIGID, ca.MOTION_SIMILARITY, ca.MOTION_AFFINE):
            with pytest.raises(ca.LkError, match="LK_FM_U"):
                e1.rigid_motion(kind, records=rec)
        assert (e1.rigid_motion(ca.MOTION_TRANSLATION, records=rec)["tx"] == 4.0).all()
