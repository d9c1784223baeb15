"""Camera noise on the GPU (lk_camera_noise, lk_sector_noise, include/lk_engine.h) against the numpy restatement of
noise_ref.py.  The device produces integers only, so every table, frame sum and sector sum is tested for equality, and a
record is byte for byte the host function of the device's own tables.

All frames are 151 x 233: neither dimension is a multiple of 4, so the rows start at every alignment and every row has a cut
head and tail.

The overflow guard: K = 16 frames that alternate 0 and 255 put every pixel into bin 128 with q = K s2 - s1^2 =
16 * 8 * 255^2 - (8 * 255)^2 = 4 161 600 (the largest q of sixteen frames, K^2 255^2 / 4), 1.46e11 over the frame and
about 1.5e10 > 2^32 in one workgroup: a 32-bit partial sum anywhere fails it."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import noise_ref as nr
import uncertainty_ref as ur

pytestmark = pytest.mark.gpu

ROWS, COLS = 151, 233
REGION = (3, 2, 229, 147)
FIT = dict(grey_low=8, grey_high=247, min_count=5)


@pytest.fixture(scope="module")
def frames():
    """16 static frames: one random scene, noise of a few grey levels, a small offset per frame"""
    rng = np.random.default_rng(42)
    base = rng.integers(0, 256, (ROWS, COLS)).astype(np.float64)
    return np.stack([np.clip(np.rint(base + 3.0 * rng.standard_normal(base.shape) + 0.3 * f), 0, 255).astype(np.uint8) for f in range(16)])


@pytest.fixture(scope="module")
def mask():
    rng = np.random.default_rng(43)
    m = (rng.random((ROWS, COLS)) < 0.7).astype(np.uint8) * rng.integers(1, 256, (ROWS, COLS)).astype(np.uint8)
    m[40:60, 100:180] = 0      # whole units without a pixel
    return m


def image_engine(px, slots, **kw):
    e = ca.HipCorrelationEngine(py_stop=2, **kw)
    for slot, p in zip(slots, px):
        e.set_image(slot, p)
    return e


def ring_engine(px, first, **kw):
    e = ca.HipCorrelationEngine(py_stop=2, **kw)
    e.sequence_reserve(first + len(px))
    for i, p in enumerate(px):
        e.sequence_set_frame(first + i, p)
    return e


def check_call(e, px, source, region=None, mask=None):
    """tables and frame sums equal numpy's, the record is the host function of them and the restatement's"""
    K = len(px)
    rec, bins, fs = e.camera_noise(region=region, mask=mask, return_tables=True, **source, **FIT)
    want_bins, want_fs = nr.tables(px, region, mask)
    assert bins.tolist() == want_bins.tolist(), np.argwhere(bins != want_bins)[:5]
    assert fs.tolist() == want_fs.tolist()
    assert rec.tobytes() == ca.noise_from_bins(K, bins, fs, **FIT).tobytes()
    nr.check_record(rec, nr.from_bins(K, want_bins, want_fs, **FIT), (source, region))
    assert e.camera_noise(region=region, mask=mask, **source, **FIT).tobytes() == rec.tobytes()      # without the tables
    return rec, bins, fs


SOURCES = {
    "images2": (2, dict(slots=(ca.IMG_UND, ca.IMG_DEF))),
    "images3": (3, dict(slots=(ca.IMG_NXT, ca.IMG_UND, ca.IMG_DEF))),
    "ring5": (5, dict(ring_first=1, n_frames=5)),
    "ring16": (16, dict(ring_first=0, n_frames=16)),
}


@pytest.mark.parametrize("name", list(SOURCES))
def test_tables_frame_sums_and_records_equal_numpy(frames, mask, name):
    K, source = SOURCES[name]
    px = frames[:K]
    e = image_engine(px, source["slots"]) if "slots" in source else ring_engine(px, source["ring_first"])
    with e:
        whole, _, _ = check_call(e, px, source)
        assert whole["status"] == ca.NOISE_OK and whole["n_pixels"] == ROWS * COLS and whole["bins_used"] > 200
        print(f"{name}: sigma {whole['sigma']:.4f} detrended {whole['sigma_detrended']:.4f} flicker {whole['flicker']:.4f} "
              f"a {whole['a']:.4f} b {whole['b']:.6f}")
        masked, _, _ = check_call(e, px, source, mask=mask)
        assert masked["n_pixels"] == int((mask != 0).sum())
        check_call(e, px, source, region=REGION)
        check_call(e, px, source, region=REGION, mask=mask)
        wide, _, fs = check_call(e, px, source, region=(100, 0, 100, ROWS - 1))      # one pixel wide
        assert wide["n_pixels"] == ROWS and fs[0] == int(px[0][:, 100].astype(np.int64).sum())
        high, _, _ = check_call(e, px, source, region=(0, 75, COLS - 1, 75), mask=mask)   # one pixel high
        assert high["n_pixels"] == int((mask[75] != 0).sum())
        check_call(e, px, source, region=(7, 9, 22, 9))                              # a row piece shorter than a unit or two
        none, bins, fs = check_call(e, px, source, mask=np.zeros((ROWS, COLS), np.uint8))
        assert none["status"] == ca.NOISE_TOO_FEW and not bins.any() and not fs.any()
        # the tables of a region are the sums of the tables of its parts
        parts = [(0, 0, COLS - 1, 70), (0, 71, 116, ROWS - 1), (117, 71, COLS - 1, ROWS - 1)]
        tabs = [e.camera_noise(region=r, return_tables=True, **source, **FIT)[1:] for r in parts]
        _, bins, fs = e.camera_noise(return_tables=True, **source, **FIT)
        assert (sum(t[0] for t in tabs) == bins).all() and (sum(t[1] for t in tabs) == fs).all()
        ms, workgroups = e.noise_last()
        assert ms > 0 and workgroups >= 1


def test_overflow_guard():
    K = 16
    px = np.stack([np.full((ROWS, COLS), 255 * (f % 2), np.uint8) for f in range(K)])
    with ring_engine(px, 0) as e:
        rec, bins, fs = e.camera_noise(ring_first=0, n_frames=K, return_tables=True)
        N = ROWS * COLS
        assert bins[128].tolist() == [N, N * 4161600] and N * 4161600 > 2 ** 32 * 30 and not np.delete(bins, 128, 0).any()
        assert fs.tolist() == [N * 255 * (f % 2) for f in range(K)]
        assert rec["status"] == ca.NOISE_NO_MODEL and rec["n_pixels"] == N and rec["var"] == 4161600 / 240
        want_bins, want_fs = nr.tables(px)
        assert bins.tolist() == want_bins.tolist() and fs.tolist() == want_fs.tolist()
        nr.check_record(rec, nr.from_bins(K, want_bins, want_fs), "overflow")


def test_one_hot_bin():
    px = np.full((2, ROWS, COLS), 77, np.uint8)
    with image_engine(px, (ca.IMG_UND, ca.IMG_DEF)) as e:
        rec, bins, fs = e.camera_noise(return_tables=True)
        assert bins[77].tolist() == [ROWS * COLS, 0] and not np.delete(bins, 77, 0).any() and fs.tolist() == [77 * ROWS * COLS] * 2
        assert rec["status"] == ca.NOISE_NO_MODEL and rec["bins_used"] == 1 and rec["var"] == 0 and rec["a"] == 0 and rec["b"] == 0
        assert rec["mean"] == 77 and rec["sigma"] == 0 and rec["flicker"] == 0
        nr.check_record(rec, nr.from_bins(2, bins, fs), "flat")


@pytest.mark.parametrize("K", [2, 3])
def test_same_bytes_again_and_from_ring_slots(frames, mask, K):
    px = frames[4:4 + K]
    slots = (ca.IMG_DEF, ca.IMG_NXT, ca.IMG_UND)[:K]
    with image_engine(px, slots) as e, ring_engine(px, 2) as r:
        for kw in (dict(), dict(region=REGION, mask=mask)):
            a = e.camera_noise(slots=slots, return_tables=True, **kw, **FIT)
            b = e.camera_noise(slots=slots, return_tables=True, **kw, **FIT)
            c = r.camera_noise(ring_first=2, n_frames=K, return_tables=True, **kw, **FIT)
            for x, y, z in zip(a, b, c):
                assert x.tobytes() == y.tobytes() == z.tobytes()


# ---- sectors -------------------------------------------------------------------------------------------------------------------
GRID = [(5 + 21 * i, 4 + 17 * j, 5 + 21 * i + 20, 4 + 17 * j + 16) for i in range(6) for j in range(5)]     # 21 x 17 each
BIG = [(140, 95, 169, 124), (131, 5, 230, 104)]        # 900 and 10 000 samples: the 64- and the 512-lane group
LIST = np.float32([[x, y] for y in range(100, 131, 3) for x in range(10, 120, 7)])
OUTSIDE = np.float32([[x, y] for y in range(-4, 7) for x in range(224, 241)])     # partly beyond the right and the top border


def sector_engine(px, py_start, ring):
    e = ca.HipCorrelationEngine(py_start=py_start, py_stop=2)
    if ring:
        e.sequence_reserve(len(px))
        for i, p in enumerate(px):
            e.sequence_set_frame(i, p)
    else:
        for slot, p in zip((ca.IMG_UND, ca.IMG_DEF, ca.IMG_NXT), px):
            e.set_image(slot, p)
    rects = GRID + BIG
    for s, r in enumerate(rects):
        e.resetPolygon_rect(s, *r)
    e.set_sector_points(len(rects), LIST)
    e.set_sector_points(len(rects) + 1, OUTSIDE)
    e.commit_sectors()
    return e, rects


def check_sectors(e, rects, level_px, level, source):
    K = len(level_px)
    out, sums = e.sector_noise(return_sums=True, **source)
    assert len(out) == len(rects) + 2
    for s in range(e.n_sectors):
        xy = ur.rect_rows(*ur.rect_level(rects[s], level)) if s < len(rects) else e.level_xy(level, s)
        want = nr.sector_sums(level_px, xy)
        assert sums[s].tolist() == want.tolist(), (s, sums[s], want)
        assert out[s].tobytes() == ca.noise_from_sums(K, sums[s]).tobytes()
        nr.check_sector_record(out[s], nr.from_sums(K, want), s)
    assert e.sector_noise(**source).tobytes() == out.tobytes()
    return out, sums


@pytest.mark.parametrize("K,ring", [(2, False), (5, True)])
def test_sector_noise(frames, K, ring):
    px = frames[:K]
    e, rects = sector_engine(px, 0, ring)
    with e:
        n0 = [e.sector_info(s)[0] for s in range(e.n_sectors)]
        assert n0[:30] == [357] * 30 and n0[30:32] == [900, 10000] and n0[32:] == [len(LIST), len(OUTSIDE)]
        source = dict(ring_first=0, n_frames=K) if ring else dict(slots=(ca.IMG_UND, ca.IMG_DEF))
        out, sums = check_sectors(e, rects, px, 0, source)
        assert out["n"][:32].tolist() == n0[:32] and out["n"][32] == len(LIST)
        inside = int(((OUTSIDE[:, 0] <= COLS - 1) & (OUTSIDE[:, 1] >= 0)).sum())
        assert 0 < inside < len(OUTSIDE) and out["n"][33] == inside                  # the samples beyond the border are not counted
        assert (out["status"] == ca.NOISE_OK).all() and (out["sigma"] > 1).all()
        ms, workgroups = e.noise_last()
        assert ms > 0 and workgroups == 0


def test_sector_noise_at_level_one(frames):
    px = frames[:3]
    e, rects = sector_engine(px, 1, False)
    with e:
        level_px = np.stack([e.get_pyramid_level(slot, 1) for slot in (ca.IMG_UND, ca.IMG_DEF, ca.IMG_NXT)])
        assert level_px.shape == (3, ROWS // 2, COLS // 2)
        out, sums = check_sectors(e, rects, level_px, 1, dict(slots=(ca.IMG_UND, ca.IMG_DEF, ca.IMG_NXT)))
        print(f"level 1: n {out['n'].tolist()}, list sizes {[len(e.level_xy(1, s)) for s in (32, 33)]}")
        assert out["n"][:32].tolist() == [len(ur.rect_rows(*ur.rect_level(r, 1))) for r in rects]
        # the frame call reads the same level
        rec, bins, fs = e.camera_noise(slots=(ca.IMG_UND, ca.IMG_DEF, ca.IMG_NXT), return_tables=True)
        want_bins, want_fs = nr.tables(level_px)
        assert bins.tolist() == want_bins.tolist() and fs.tolist() == want_fs.tolist() and rec["n_pixels"] == level_px[0].size


# ---- the engine around the calls -----------------------------------------------------------------------------------------------
def test_no_engine_state_changes():
    und, dfm = ur.experiment_pair()
    rects = ur.experiment_rects()[:36]
    g = np.zeros((len(rects), 6), np.float32)
    with ca.HipCorrelationEngine(precision=ur.EXP_PRECISION, py_stop=2) as e:
        e.set_image(ca.IMG_UND, und)
        e.set_image(ca.IMG_DEF, dfm)
        for s, r in enumerate(rects):
            e.resetPolygon_rect(s, *r)
        e.commit_sectors()
        first = e.correlate_all(g)
        assert (first["error_code"] == 0).all()
        report = e.launch_report()

        def state():
            return dict(guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(), stats=e.sector_stats())

        kept = state()
        rec = e.camera_noise(**FIT)
        sec = e.sector_noise()
        assert rec["status"] == ca.NOISE_OK and (sec["status"] == ca.NOISE_OK).all()
        # two frames of noise sigma 4 each on one scene: the pooled sigma is the camera's, less what clipping at 0 and 255 takes
        print(f"sigma {rec['sigma']:.4f} (the frames were made with {ur.EXP_NOISE}), at the mean grey {rec['sigma_at_mean']:.4f}")
        assert 0.5 * ur.EXP_NOISE < rec["sigma"] <= 1.02 * np.sqrt(ur.EXP_NOISE ** 2 + 1 / 12)
        assert e.launch_report() == report and len(report) > 0
        after = state()
        for k in kept:
            assert kept[k].tobytes() == after[k].tobytes(), k
        assert e.correlate_all(g).tobytes() == first.tobytes()
        assert e.launch_report() == report


def test_every_refusal(frames):
    und, dfm = frames[0], frames[1]
    e = ca.HipCorrelationEngine(py_stop=2)
    e.set_image(ca.IMG_UND, und)
    e.set_image(ca.IMG_DEF, dfm)
    e.sequence_reserve(4)
    e.sequence_set_frame(0, und)
    e.sequence_set_frame(1, dfm)
    e.sequence_set_frame(3, dfm[:-1])           # slot 2 stays empty, slot 3 is one row short
    e.resetPolygon_rect(0, 10, 10, 30, 30)
    lib, h = e.lib, e._h
    out = np.full(96, 7, np.uint8)
    sec = np.full(32, 7, np.uint8)
    bins = np.full((256, 2), 7, np.int64)
    fs = np.full(16, 7, np.int64)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def config(source=ca.NOISE_IMAGES, n_frames=2, slots=(ca.IMG_UND, ca.IMG_DEF, 0), first=0, region=(0, 0, 0, 0), low=0, high=255,
               count=2, reserved=None):
        c = _ffi.LkNoiseConfig(source, n_frames, (C.c_int32 * 3)(*slots), first, *region, low, high, count)
        if reserved is not None:
            c.reserved[reserved] = 1
        return c

    def frame(cfg=True, output=out, **kw):
        c = config(**kw) if cfg else None
        rc = lib.lk_camera_noise(h, C.byref(c) if c is not None else None, None, ptr(output), ptr(bins), ptr(fs))
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and msg.startswith("lk_camera_noise: "), (rc, msg)
        return msg

    def sector(cfg=True, output=sec, **kw):
        c = config(**kw) if cfg else None
        rc = lib.lk_sector_noise(h, C.byref(c) if c is not None else None, ptr(output), None)
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and msg.startswith("lk_sector_noise: "), (rc, msg)
        return msg

    assert "no committed sectors" in sector()
    e.commit_sectors()
    for call in (frame, sector):
        assert "configuration" in call(cfg=False) and "output" in call(output=None)
        for k in range(3):
            assert "reserved" in call(reserved=k)
        assert "source" in call(source=2) and "source" in call(source=-1)
        for n in (-1, 0, 1, 4):
            assert "n_frames" in call(n_frames=n)
        for n in (1, 17):
            assert "n_frames" in call(source=ca.NOISE_RING, n_frames=n)
        assert "twice" in call(slots=(ca.IMG_UND, ca.IMG_UND, 0)) and "twice" in call(n_frames=3, slots=(ca.IMG_UND, ca.IMG_DEF, ca.IMG_UND))
        assert "unknown slot" in call(slots=(ca.IMG_UND, 3, 0)) and "unknown slot" in call(slots=(-1, ca.IMG_DEF, 0))
        assert "not set" in call(slots=(ca.IMG_UND, ca.IMG_NXT, 0))
        assert "unknown ring slot" in call(source=ca.NOISE_RING, first=3) and "unknown ring slot" in call(source=ca.NOISE_RING, first=-1)
        assert "unknown ring slot" in call(source=ca.NOISE_RING, n_frames=5)
        assert "ring slot is empty" in call(source=ca.NOISE_RING, first=1)
    e.sequence_set_frame(2, und)
    e.set_image(ca.IMG_NXT, dfm[:-1])
    for call in (frame, sector):
        assert "same dimensions" in call(source=ca.NOISE_RING, first=2)
        assert "same dimensions" in call(n_frames=3, slots=(ca.IMG_UND, ca.IMG_DEF, ca.IMG_NXT))
    for region in ((5, 5, 4, 9), (5, 5, 9, 4)):
        assert "region is empty" in frame(region=region)
    for region in ((-1, 0, 9, 9), (0, -1, 9, 9), (0, 0, COLS, 9), (0, 0, 9, ROWS)):
        assert "leaves" in frame(region=region)
    for low, high in ((-1, 255), (256, 255), (0, -1), (0, 256)):
        assert "0 .. 255" in frame(low=low, high=high)
    for count in (1, 0, -3):
        assert "min_count" in frame(count=count)
    assert (out == 7).all() and (sec == 7).all() and (bins == 7).all() and (fs == 7).all()      # the outputs are untouched
    assert lib.lk_camera_noise(None, None, None, ptr(out), None, None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_sector_noise(None, None, ptr(sec), None) == ca.ERROR_BAD_DOMAIN
    # the accepted extremes: the largest region, the last ring slots
    assert e.camera_noise(region=(0, 0, COLS - 1, ROWS - 1))["n_pixels"] == ROWS * COLS
    assert e.camera_noise(ring_first=0, n_frames=3)["status"] == ca.NOISE_OK and len(e.sector_noise(ring_first=1, n_frames=2)) == 1
    e.close()
