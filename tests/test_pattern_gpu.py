"""Speckle quality on the GPU (lk_pattern_quality, lk_suggest_subset, include/lk_engine.h) against the int64 / float64
restatement of pattern_ref.py.  Everything but one sum is integer arithmetic on u8 pixels, so the device is tested for
equality: the nine sums of a sector, every box sum of every candidate, every integer field of a suggestion.

mig_sum is the one reordered double sum: |device - float64 sum of the terms| <= 64 n 2^-53 sum(terms), the bound form
test_residual_gpu.py derives for a double sum of n terms added in another order (the terms themselves are identical: the
square root of an exact integer is correctly rounded on both sides)."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi, speckle

import pattern_ref as pr
import uncertainty_ref as ur

pytestmark = pytest.mark.gpu

TRUTH = (1.3, -0.7, 0.002, 0.0, 0.0, -0.001)
# the sectors of test_uncertainty_gpu.py: every lane group and both list kinds, no n a multiple of its group
RECTS = [(8, 8, 26, 26), (40, 8, 46, 14), (8, 60, 38, 88), (140, 140, 239, 239)]
ANNULAR = [(20.0, 12.0, 0.3, 0.9, 70.0, 190.0, 6)]
GROUPS = [16, 16, 64, 512]
QUALITY = dict(grey_low=20, grey_high=235, noise_sigma=0.75, max_saturated=0.3)


@pytest.fixture(scope="module")
def pair():
    return speckle.speckle_pair(256, 256, p=TRUTH, seed=5)


def make_engine(images, rects=(), annular=(), py_start=0, commit=True, **kw):
    """images: {slot: pixels}"""
    e = ca.HipCorrelationEngine(precision=ur.EXP_PRECISION, py_start=py_start, py_stop=2, **kw)
    for slot, px in images.items():
        e.set_image(slot, px)
    for s, r in enumerate(rects):
        e.resetPolygon_rect(s, *r)
    for k, q in enumerate(annular):
        e.resetPolygon_annular(len(rects) + k, *q)
    if commit and (rects or annular):
        e.commit_sectors()
    return e


def both(pair):
    return {ca.IMG_UND: pair[0], ca.IMG_DEF: pair[1]}


def sector_list(e, s, level, rects):
    return ur.rect_rows(*ur.rect_level(rects[s], level)) if s < len(rects) else e.level_xy(level, s)


def check_sectors(e, img, level, rects, out, sums, mig, quality=QUALITY):
    """every sector: the nine sums equal, mig_sum within the bound, the record byte for byte the host function of the
    device's sums and the restatement's record -> the statuses"""
    for s in range(e.n_sectors):
        xy = sector_list(e, s, level, rects)
        n = len(xy)
        want, terms = pr.sector_sums(img, xy, quality["grey_low"], quality["grey_high"])
        assert sums[s].tolist() == want.tolist(), (s, sums[s], want)
        bound = 64.0 * n * 2.0 ** -53 * terms.sum()
        err = abs(mig[s] - terms.sum())
        print(f"level {level} sector {s} (n = {n}): mig_sum error {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (s, err, bound)
        host = ca.pattern_from_sums(n, sums[s], mig[s], quality["noise_sigma"], quality["max_saturated"])
        assert host.tobytes() == out[s].tobytes(), (s, host, out[s])
        pr.check_record(out[s], n, sums[s], mig[s], quality["noise_sigma"], quality["max_saturated"], s)
    return out["status"].tolist()


@pytest.mark.parametrize("py_start", [0, 1])
@pytest.mark.parametrize("slot", [ca.IMG_UND, ca.IMG_DEF])
def test_sums_and_records_of_the_sectors(pair, py_start, slot):
    with make_engine(both(pair), RECTS, ANNULAR, py_start=py_start) as e:
        n0 = [e.sector_info(s)[0] for s in range(e.n_sectors)]
        assert n0[:4] == [361, 49, 899, 10000] and 0 < n0[4] <= 512 and all(n % g for n, g in zip(n0, GROUPS))
        out, sums, mig = e.pattern_quality(slot=slot, return_sums=True, **QUALITY)
        img = e.get_pyramid_level(slot, py_start)
        status = check_sectors(e, img, py_start, RECTS, out, sums, mig)
        print(f"py_start {py_start} slot {slot}: status {status}, sssig_x {out['sssig_x']}, sigma_u {out['sigma_u']}, mig {out['mig']}")
        assert set(status) <= {ca.PATTERN_OK, ca.PATTERN_SATURATED}      # (which of the two: check_sectors, by the restatement)
        # the same call again, and without the sums: the same bytes; the other slot: other numbers
        again = e.pattern_quality(slot=slot, **QUALITY)
        assert again.tobytes() == out.tobytes()
        assert e.pattern_quality(slot=1 - slot, **QUALITY).tobytes() != out.tobytes()


def test_a_sector_alone_is_the_sector_in_the_batch(pair):
    with make_engine(both(pair), RECTS, ANNULAR) as e:
        out, sums, mig = e.pattern_quality(return_sums=True, **QUALITY)
    for k in (0, 2, 3):
        with make_engine(both(pair), [RECTS[k]]) as e:
            a, a_sums, a_mig = e.pattern_quality(return_sums=True, **QUALITY)
            assert a[0].tobytes() == out[k].tobytes() and a_sums[0].tobytes() == sums[k].tobytes() and a_mig[0] == mig[k], k
    with make_engine(both(pair), [], ANNULAR) as e:
        a, a_sums, a_mig = e.pattern_quality(return_sums=True, **QUALITY)
        assert a[0].tobytes() == out[4].tobytes() and a_sums[0].tobytes() == sums[4].tobytes() and a_mig[0] == mig[4]


def test_status_cases(pair):
    rects = [(30, 30, 48, 48), (100, 60, 130, 88)]
    flat = np.full((256, 256), 131, np.uint8)
    with make_engine({ca.IMG_UND: flat}, rects) as e:
        out, sums, mig = e.pattern_quality(return_sums=True)
        assert (out["status"] == ca.PATTERN_FLAT).all() and not sums[:, 2:5].any() and not mig.any()
        assert (out["mean"] == 131).all() and not out["std"].any() and not out["sigma_u"].any()
    stripes = np.tile(np.uint8([0, 0, 255, 255]), (256, 64))      # vertical stripes of period 4: Gyy = 0
    with make_engine({ca.IMG_UND: stripes}, rects) as e:
        out, sums, mig = e.pattern_quality(return_sums=True)
        assert (out["status"] == ca.PATTERN_APERTURE).all()
        assert (sums[:, 2] == 255 * 255 * out["n_points"]).all() and not sums[:, 3:5].any()
        assert (out["sssig_x"] > 0).all() and not any(out[k].any() for k in pr.SIGMAS)
    clipped = np.where(pair[0] >= 128, 255, 0).astype(np.uint8)   # speckle clipped to {0, 255}
    with make_engine({ca.IMG_UND: clipped}, rects) as e:
        out, sums, mig = e.pattern_quality(max_saturated=0.5, return_sums=True)
        assert (out["status"] == ca.PATTERN_SATURATED).all() and (sums[:, 5] + sums[:, 6] == out["n_points"]).all()
        assert (out["sigma_u"] > 0).all() and (out["frac_low"] + out["frac_high"] == 1).all()
        assert (e.pattern_quality(max_saturated=1.0)["status"] == ca.PATTERN_OK).all()
        check_sectors(e, clipped, 0, rects, out, sums, mig, dict(grey_low=0, grey_high=255, noise_sigma=1.0, max_saturated=0.5))
    e = make_engine({ca.IMG_UND: pair[0]}, commit=False)
    e.set_sector_points(0, np.float32([[77.0, 91.0]]), center=(77.0, 91.0))     # a one-sample list
    e.resetPolygon_rect(1, *rects[0])
    e.commit_sectors()
    out, sums, mig = e.pattern_quality(return_sums=True)
    assert out["status"].tolist() == [ca.PATTERN_TOO_FEW, ca.PATTERN_OK] and out["n_points"].tolist() == [1, 361]
    assert sums[0, 0] == pair[0][91, 77] and sums[0, 7] == sums[0, 8] == pair[0][91, 77] and not any(out[k][0] for k in pr.FLOATS)
    e.close()


def hip_runtime():
    hip = C.CDLL("libamdhip64.so")   # the runtime the engine library itself is linked to
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def device_records(e):
    d = C.c_void_p()
    assert e.lib.lk_get_results_device(e._h, C.byref(d)) == 0
    out = np.zeros(e.n_sectors, ca.RESULT_DTYPE)
    assert e.lib.lk_synchronize(e._h) == 0
    assert hip_runtime().hipMemcpy(out.ctypes.data_as(C.c_void_p), d, out.nbytes, 2) == 0
    return out


def start_guesses(S):
    g = np.zeros((S, 6), np.float32)
    g[:, :2] = TRUTH[:2]
    return g


def test_engine_state_is_untouched(pair):
    rects = ur.experiment_rects()[:64]
    S = len(rects)
    g = start_guesses(S)
    g[[9, 27], 0] = 300.0
    pts = np.float32([[40, 40], [100.5, 77.25], [250, 3]])
    with make_engine(both(pair), rects) as e, make_engine(both(pair), rects) as plain:
        for x in (e, plain):
            x.correlate_all(g)
            x.reseed_failed(1.5 * ur.EXP_SIDE)

        def state():
            return dict(records=device_records(e), guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(),
                        stats=e.sector_stats(), reseed=e.reseed_info())

        kept = state()
        a = e.pattern_quality(**QUALITY)
        b = e.suggest_subset(pts, 1e5, 2, 40)
        assert e.pattern_quality(**QUALITY).tobytes() == a.tobytes() and e.suggest_subset(pts, 1e5, 2, 40).tobytes() == b.tobytes()
        after = state()
        for k in kept:
            assert kept[k].tobytes() == after[k].tobytes(), k
        # the next solve is the one an engine gives that never made the calls
        assert e.correlate_all(start_guesses(S)).tobytes() == plain.correlate_all(start_guesses(S)).tobytes()
        assert e.last_evaluated_parameters().tobytes() == plain.last_evaluated_parameters().tobytes()


def test_one_slot_is_enough_and_every_mode_is_allowed(pair):
    pts = np.float32([[40, 40], [100.5, 77.25], [250, 3]])
    with make_engine(both(pair), RECTS, ANNULAR) as e:
        want = e.pattern_quality(**QUALITY)
        want_sub = e.suggest_subset(pts, 1e5, 2, 40)
        e.set_reference_order(1)                      # reference-order mode
        assert e.pattern_quality(**QUALITY).tobytes() == want.tobytes() and e.suggest_subset(pts, 1e5, 2, 40).tobytes() == want_sub.tobytes()
        e.set_reference_order(0)
        e.set_update(ca.UPDATE_BACKWARD)
        assert e.pattern_quality(**QUALITY).tobytes() == want.tobytes()
    with make_engine({ca.IMG_UND: pair[0]}, RECTS, ANNULAR) as e:       # the deformed image is not set
        assert e.pattern_quality(**QUALITY).tobytes() == want.tobytes()
        assert e.suggest_subset(pts, 1e5, 2, 40).tobytes() == want_sub.tobytes()
        with pytest.raises(ca.LkError, match="lk_pattern_quality: .*not set"):
            e.pattern_quality(slot=ca.IMG_DEF)
        with pytest.raises(ca.LkError, match="lk_suggest_subset: .*not set"):
            e.suggest_subset(pts, 1e5, slot=ca.IMG_NXT)
    with make_engine({ca.IMG_NXT: pair[0]}, RECTS, ANNULAR) as e:       # the next-frame slot alone
        assert e.pattern_quality(slot=ca.IMG_NXT, **QUALITY).tobytes() == want.tobytes()
        assert e.suggest_subset(pts, 1e5, 2, 40, slot=ca.IMG_NXT).tobytes() == want_sub.tobytes()
    with make_engine({ca.IMG_UND: pair[0]}) as e:                       # no sectors at all: the suggestion needs none
        assert e.suggest_subset(pts, 1e5, 2, 40).tobytes() == want_sub.tobytes()
        with pytest.raises(ca.LkError, match="lk_pattern_quality: no committed sectors"):
            e.pattern_quality()


def test_a_pending_rebuild_of_the_lists_is_carried_out_first(pair):
    with make_engine(both(pair), RECTS, ANNULAR) as e:
        rec = e.correlate_all(start_guesses(5))
        assert (rec["error_code"] == 0).all()
        before, sums_before, _ = e.pattern_quality(return_sums=True, **QUALITY)
        old = e.level_xy(0, 4)
        e.update_sector(4, 1)      # the annular list moves with its record: the lists are rebuilt before the next solve
        out, sums, mig = e.pattern_quality(return_sums=True, **QUALITY)
        moved = e.level_xy(0, 4)
        assert len(moved) == len(old) and np.abs(moved - old).max() >= 0.5
        want, terms = pr.sector_sums(pair[0], moved, QUALITY["grey_low"], QUALITY["grey_high"])
        assert sums[4].tolist() == want.tolist() and sums[4].tolist() != sums_before[4].tolist()
        assert sums[:4].tobytes() == sums_before[:4].tobytes()
        check_sectors(e, pair[0], 0, RECTS, out, sums, mig)


# ---- the tables and the query --------------------------------------------------------------------------------------------------
def check_suggestions(img, pts, got, got_sums, sssig_min, half_min, half_max, half_step=1, noise_sigma=1.0, tabs=None):
    want, want_sums = pr.suggest(img, pts, sssig_min, half_min, half_max, half_step, noise_sigma, tabs)
    assert got_sums.shape == want_sums.shape and (got_sums.astype(np.int64) == want_sums).all(), np.argwhere(got_sums != want_sums)[:5]
    for k in ("half", "status", "n_pixels", "clipped"):
        assert (got[k] == want[k]).all(), (k, np.flatnonzero(got[k] != want[k])[:5])
    assert got.tobytes() == want.tobytes()     # the float fields: exact quotients, correctly rounded square roots
    return want


def test_tables_wrap_and_every_seam_is_crossed():
    with make_engine({ca.IMG_UND: np.zeros((8, 8), np.uint8)}) as e:
        e.suggest_subset(np.float32([[1, 1]]), 1.0, 1, 1)
        _, row_tile, band_rows, _, _ = e.pattern_last()
    rows, cols = 2 * band_rows + 6, 2 * row_tile + 38
    assert cols % 4 == 2                          # the row pitch is padded: the last thread's four columns are cut
    rng = np.random.default_rng(17)
    img = (rng.integers(0, 2, (rows, cols)) * 255).astype(np.uint8)
    tabs = pr.tables(img)
    total = [int(t[-1, -1]) for t in tabs]
    print(f"image {rows} x {cols} (row tile {row_tile}, band {band_rows} rows): table totals {total}, 2^32 = {2 ** 32}")
    assert min(total) > 2 ** 32                   # the uint32 tables wrap; the int64 restatement does not
    with make_engine({ca.IMG_UND: img}) as e:
        ys, xs = np.mgrid[0:rows, 0:cols]
        every = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
        got, sums = e.suggest_subset(every, 3e4, 1, 1, return_sums=True)
        want = check_suggestions(img, every, got, sums, 3e4, 1, 1, tabs=tabs)
        assert {ca.SUBSET_OK, ca.SUBSET_NONE} == set(want["status"].tolist())
        lx = sorted(set(range(0, cols, 97)) | {1, row_tile - 1, row_tile, 2 * row_tile - 1, 2 * row_tile, cols - 2, cols - 1})
        ly = sorted(set(range(0, rows, 9)) | {1, band_rows - 1, band_rows, 2 * band_rows - 1, 2 * band_rows, rows - 2, rows - 1})
        lattice = np.float32([[x, y] for y in ly for x in lx])
        got, sums = e.suggest_subset(lattice, 5e6, 1, 128, 7, return_sums=True)
        want = check_suggestions(img, lattice, got, sums, 5e6, 1, 128, 7, tabs=tabs)
        assert sums.shape[1] == 19 and {ca.SUBSET_OK} == set(want["status"].tolist()) and len(set(want["half"].tolist())) > 1
        got, sums = e.suggest_subset(lattice, 1.2e8, 128, 128, return_sums=True)
        want = check_suggestions(img, lattice, got, sums, 1.2e8, 128, 128, tabs=tabs)
        assert (want["half"] == 128).all() and want["clipped"].all() and {ca.SUBSET_OK, ca.SUBSET_NONE} == set(want["status"].tolist())
        # without the sums the scan stops at the first pass: the same records
        assert e.suggest_subset(lattice, 5e6, 1, 128, 7).tobytes() == e.suggest_subset(lattice, 5e6, 1, 128, 7, return_sums=True)[0].tobytes()


def test_the_largest_box_sum_fits():
    img = np.tile(np.uint8([0, 0, 255, 255]), (300, 150))        # 600 wide: |gx2| = 255 at every interior pixel, gy2 = 0
    with make_engine({ca.IMG_UND: img}) as e:
        pts = np.float32([[300, 150], [301, 149], [0, 0]])
        got, sums = e.suggest_subset(pts, 1e9, 128, 128, return_sums=True)
        assert 257 * 257 * 255 * 255 == 4294836225 < 2 ** 32
        assert sums[:2, 0].tolist() == [[4294836225, 0]] * 2
        assert got["n_pixels"].tolist() == [257 * 257, 257 * 257, 129 * 129] and got["clipped"].tolist() == [0, 0, 1]
        assert (got["status"] == ca.SUBSET_NONE).all()           # Gyy = 0 never reaches a threshold
        check_suggestions(img, pts, got, sums, 1e9, 128, 128)


LATTICE = np.float32([[x, y] for y in range(3, 256, 19) for x in range(5, 256, 17)])


def test_suggestions_on_speckle(pair):
    und = pair[0]
    assert len(LATTICE) == 210
    tabs = pr.tables(und)
    with make_engine({ca.IMG_UND: und}) as e:
        got, sums = e.suggest_subset(LATTICE, 1e5, 2, 40, noise_sigma=0.75, return_sums=True)
        want = check_suggestions(und, LATTICE, got, sums, 1e5, 2, 40, noise_sigma=0.75, tabs=tabs)
        print("sssig_min 1e5, halves 2..40:", np.bincount(want["half"]))
        # none is NONE and none is at half_min: the scan, not a bound, decides every answer
        assert (want["status"] == ca.SUBSET_OK).all() and want["half"].min() == 5 and want["half"].max() == 13
        got, sums = e.suggest_subset(LATTICE, 3e5, 2, 15, return_sums=True)
        want = check_suggestions(und, LATTICE, got, sums, 3e5, 2, 15, tabs=tabs)
        none = want["status"] == ca.SUBSET_NONE
        print("sssig_min 3e5, halves 2..15:", np.bincount(want["half"][~none]), "NONE:", int(none.sum()))
        assert none.sum() == 16 and (want["half"][none] == 15).all() and want["half"][~none].min() == 10 and want["half"][~none].max() == 15
        # a ladder of step 3: the smallest candidate of that ladder
        fine = check_suggestions(und, LATTICE, *e.suggest_subset(LATTICE, 1e5, 2, 40, return_sums=True), 1e5, 2, 40, tabs=tabs)
        got, sums = e.suggest_subset(LATTICE, 1e5, 2, 40, 3, return_sums=True)
        coarse = check_suggestions(und, LATTICE, got, sums, 1e5, 2, 40, 3, tabs=tabs)
        assert (coarse["half"] == 2 + 3 * -((2 - fine["half"]) // 3)).all()


def test_the_two_kernels_agree(pair):
    x, y, halves = 100, 120, (4, 9, 30)
    rects = [(x - h, y - h, x + h, y + h) for h in halves]
    with make_engine({ca.IMG_UND: pair[0]}, rects) as e:
        _, sums, _ = e.pattern_quality(return_sums=True)
        got, box = e.suggest_subset(np.float32([[x, y]]), 1e5, 4, 30, 1, return_sums=True)
        assert got["clipped"][0] == 0
        for s, h in enumerate(halves):
            assert sums[s, 2:4].tolist() == box[0, h - 4].tolist(), h


def test_per_point_cases(pair):
    und = pair[0]
    pts = LATTICE[:40].copy()
    with make_engine({ca.IMG_UND: und}) as e:
        want, want_sums = e.suggest_subset(pts, 1e5, 2, 40, return_sums=True)
        bad = pts.copy()
        bad[7] = (np.nan, 30.0)
        bad[8] = (40.0, -np.inf)
        bad[20] = (256.0, 30.0)        # node 256: one past the last column
        bad[21] = (30.0, -1.5)         # node -1
        bad[22] = (1e30, 1e30)
        edge = [(255.49, 0.0), (-0.5, 255.0), (-1.49, 3.0)]     # nodes (255, 0), (0, 255), (0, 3): inside
        bad[30:33] = edge
        got, sums = e.suggest_subset(bad, 1e5, 2, 40, return_sums=True)
        check_suggestions(und, bad, got, sums, 1e5, 2, 40)
        hit = [7, 8, 20, 21, 22]
        assert (got["status"][hit] == ca.SUBSET_BAD_POINT).all() and not sums[hit].any()
        assert not any(got[k][hit].any() for k in ("half", "n_pixels", "clipped", "sssig_x", "sigma_u"))
        assert (got["status"][30:33] != ca.SUBSET_BAD_POINT).all() and got["clipped"][30:33].all()
        keep = np.setdiff1d(np.arange(40), hit + [30, 31, 32])
        assert got[keep].tobytes() == want[keep].tobytes() and sums[keep].tobytes() == want_sums[keep].tobytes()
        # a point's record does not depend on the other points of the call
        for k in (0, 13, 39):
            alone, alone_sums = e.suggest_subset(pts[k:k + 1], 1e5, 2, 40, return_sums=True)
            assert alone[0].tobytes() == want[k].tobytes() and alone_sums[0].tobytes() == want_sums[k].tobytes()
        assert e.suggest_subset(pts[::-1], 1e5, 2, 40)[::-1].tobytes() == want.tobytes()


def test_arguments_and_refusals(pair):
    e = make_engine({ca.IMG_UND: pair[0]}, RECTS, commit=False)
    lib, h = e.lib, e._h
    out = np.full(4 * 64, 7, np.uint8).view(ca.PATTERN_DTYPE)
    sub = np.full(3 * 32, 7, np.uint8).view(ca.SUBSET_DTYPE)
    pts = np.float32([[40, 40], [100, 77], [250, 3]])

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def quality(cfg=(ca.IMG_UND, 0, 255, 1.0, 1.0), output=out, reserved=None):
        c = _ffi.LkPatternConfig(*cfg) if cfg is not None else None
        if reserved is not None:
            c.reserved[reserved] = 1
        rc = lib.lk_pattern_quality(h, C.byref(c) if c is not None else None, ptr(output), None, None)
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and msg.startswith("lk_pattern_quality: "), (rc, msg)
        return msg

    def suggest(cfg=(ca.IMG_UND, 2, 40, 1, 1e5, 1.0), n=3, points=pts, output=sub, reserved=None):
        c = _ffi.LkSubsetConfig(*cfg) if cfg is not None else None
        if reserved is not None:
            c.reserved[reserved] = 1
        rc = lib.lk_suggest_subset(h, C.byref(c) if c is not None else None, n, _ffi.fptr(points) if points is not None else None,
                                   ptr(output), None)
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and msg.startswith("lk_suggest_subset: "), (rc, msg)
        return msg

    assert "no committed sectors" in quality()
    e.commit_sectors()
    assert "configuration" in quality(None) and "configuration" in suggest(None)
    assert "output" in quality(output=None) and "output" in suggest(output=None)
    for slot in (-1, 3, 7):
        assert "unknown slot" in quality((slot, 0, 255, 1.0, 1.0)) and "unknown slot" in suggest((slot, 2, 40, 1, 1e5, 1.0))
    assert "not set" in quality((ca.IMG_DEF, 0, 255, 1.0, 1.0)) and "not set" in suggest((ca.IMG_NXT, 2, 40, 1, 1e5, 1.0))
    for k in range(3):
        assert "reserved" in quality(reserved=k)
    for k in range(2):
        assert "reserved" in suggest(reserved=k)
    for low, high in ((-1, 255), (256, 255), (0, -1), (0, 256)):
        assert "0 .. 255" in quality((ca.IMG_UND, low, high, 1.0, 1.0))
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert "finite" in quality((ca.IMG_UND, 0, 255, bad, 1.0)) and "finite" in quality((ca.IMG_UND, 0, 255, 1.0, bad))
        assert "noise_sigma" in suggest((ca.IMG_UND, 2, 40, 1, 1e5, bad))
        assert "sssig_min" in suggest((ca.IMG_UND, 2, 40, 1, bad, 1.0))
    assert "no points" in suggest(n=0) and "no points" in suggest(n=-3) and "no points" in suggest(points=None)
    for lo, hi, step in ((0, 40, 1), (5, 4, 1), (2, 129, 1), (2, 40, 0), (2, 40, -1), (-3, -1, 1)):
        assert "candidates" in suggest((ca.IMG_UND, lo, hi, step, 1e5, 1.0))
    for t in (0.0, -1.0, 2.0 ** 30):             # T = ceil(4 sssig_min) must lie in 1 .. 2^32 - 1
        assert "sssig_min" in suggest((ca.IMG_UND, 2, 40, 1, t, 1.0))
    assert (out.view(np.uint8) == 7).all() and (sub.view(np.uint8) == 7).all()          # the outputs are untouched
    assert lib.lk_pattern_quality(None, None, ptr(out), None, None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_suggest_subset(None, None, 3, _ffi.fptr(pts), ptr(sub), None) == ca.ERROR_BAD_DOMAIN
    # the largest threshold and the extreme ladder are accepted
    got = e.suggest_subset(pts, float(np.float32(2.0 ** 30 - 64)), 1, 128, 127)
    assert (got["status"] == ca.SUBSET_NONE).all() and (got["half"] == 128).all()
    assert (e.pattern_quality()["status"] == ca.PATTERN_OK).all()
    e.close()
