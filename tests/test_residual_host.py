"""Host side of the photometry pass and the residual map (include/lk_engine.h): lk_photometry_from_sums - the kernel's own
record function compiled for the host - against the float64 restatement of residual_ref.py; lk_map_owner against the
brute-force owner rule; the struct sizes and prototypes; and the lighting experiment measured with the oracle alone, which
pins the constants the GPU test uses."""
import ctypes as C

import numpy as np

import correlation_amd as ca
from correlation_amd import _ffi, speckle

import residual_ref as rr

TRUTH = (1.3, -0.7, 0.002, 0.0, 0.0, -0.001)


def synthetic(n, a, b, noise, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, n).astype(np.float32)
    g = (np.float32(a) * f + np.float32(b)).astype(np.float32)
    if noise:
        g = (g + rng.normal(0.0, noise, n).astype(np.float32)).astype(np.float32)
    return f, g, (f - g).astype(np.float32)


def test_record_against_the_restatement():
    cases = [("noisy", synthetic(361, 0.8, 20.0, 3.0, 1)), ("noisy large", synthetic(10000, 1.1, -7.0, 6.0, 2)),
             ("darker", synthetic(899, 0.5, 32.0, 0.5, 3)), ("n = 2", synthetic(2, 0.9, 5.0, 1.0, 4)),
             ("n = 1", synthetic(1, 0.9, 5.0, 1.0, 5)), ("anticorrelated", synthetic(49, -0.7, 200.0, 2.0, 6))]
    for name, (f, g, V) in cases:
        sums = rr.sums_of(f, g, V)
        got = ca.photometry_from_sums(len(f), sums)
        worst = rr.check_record(got, f, g, V, sums, name)
        print(f"{name}: status {got['status']}, zncc {got['zncc']:.7f}, gain {got['gain']:.6f}, offset {got['offset']:.5f}, "
              f"rms {got['rms']:.5f}, rms_zn {got['rms_zn']:.5f}; worst error / tolerance {worst:.3g}, kappa {rr.kappa(len(f), sums):.3g}")
    assert ca.photometry_from_sums(1, rr.sums_of(*cases[4][1]))["status"] == ca.PHOTO_TOO_FEW
    assert ca.photometry_from_sums(2, rr.sums_of(*cases[3][1]))["status"] == ca.PHOTO_OK


def test_noise_free_gain_offset_and_zncc_come_back():
    for a, b, n in ((0.5, 32.0, 361), (0.75, 10.0, 10000), (1.0, 0.0, 49), (0.25, 100.0, 899)):
        f, g, V = synthetic(n, a, b, 0.0, 7)      # (a f + b is exact in float32 for these a, b and integer f)
        sums = rr.sums_of(f, g, V)
        got = ca.photometry_from_sums(n, sums)
        rr.check_record(got, f, g, V, sums, (a, b))
        tol = 2.0 ** -22 + 1e-12 * rr.kappa(n, sums)
        assert got["status"] == ca.PHOTO_OK
        assert abs(float(got["gain"]) - a) <= tol * abs(a), (a, b, got)
        assert abs(float(got["offset"]) - b) <= tol * abs(b) + 1e-12 * rr.kappa(n, sums) * (abs(float(got["mean_g"])) + a * float(got["mean_f"])), (a, b, got)
        assert abs(float(got["zncc"]) - 1.0) <= tol, (a, b, got)


def test_flat_patches_and_the_flagged_count():
    rng = np.random.default_rng(8)
    tex = rng.integers(0, 256, 361).astype(np.float32)
    flat = np.full(361, 128.0, np.float32)
    for name, f, g in (("flat f", flat, tex), ("flat g", tex, flat), ("both flat", flat, flat)):
        V = (f - g).astype(np.float32)
        got = ca.photometry_from_sums(361, rr.sums_of(f, g, V))
        assert got["status"] == ca.PHOTO_FLAT, (name, got)
        rr.check_record(got, f, g, V, None, name)
    # nearly flat, but with contrast far above the rule's 1e-12: evaluated (kappa decides what is compared)
    f = flat.copy()
    f[::2] += 1.0
    g = (f * np.float32(0.5)).astype(np.float32)
    assert ca.photometry_from_sums(361, rr.sums_of(f, g, f - g))["status"] == ca.PHOTO_OK
    s = rr.sums_of(tex, tex[::-1].copy(), tex - tex[::-1])
    s[6] = 3.0
    got = ca.photometry_from_sums(361, s)
    assert got["status"] == ca.PHOTO_OUT_OF_IMAGE and got["n_points"] == 361 and not any(got[k] for k in rr.FLOATS)


def test_map_owner_against_brute_force():
    rng = np.random.default_rng(9)
    centres = (rng.random((300, 2)) * 100).astype(np.float32)
    good = rng.random(300) > 0.25
    radius = np.float32(9.5)
    want = rr.brute_owner(centres, good, radius, 0, 0, 101, 101)
    got = np.array([[ca.map_owner(centres, x, y, radius, good) for x in range(101)] for y in range(101)], np.int32)
    assert np.array_equal(got, want)
    assert (want == -1).any() and (want >= 0).any()
    assert np.array_equal(rr.brute_owner(centres, np.ones(300, bool), radius, 10, 20, 7, 5),
                          np.array([[ca.map_owner(centres, x, y, radius) for x in range(10, 17)] for y in range(20, 25)]))
    # level 1: pixel (x, y) stands at (2 x, 2 y)
    want1 = rr.brute_owner(centres, good, radius, 3, 4, 20, 10, level=1)
    got1 = np.array([[ca.map_owner(centres, 2 * x, 2 * y, radius, good) for x in range(3, 23)] for y in range(4, 14)], np.int32)
    assert np.array_equal(got1, want1)


def test_map_owner_ties_radius_and_bad_neighbours():
    # two centres mirrored about the pixel (10, 10): the lower index wins, whatever the order
    c = np.float32([[13.0, 10.0], [7.0, 10.0], [10.0, 14.5]])
    assert ca.map_owner(c, 10.0, 10.0, 5.0) == 0
    assert ca.map_owner(c[::-1].copy(), 10.0, 10.0, 5.0) == 1      # (10, 14.5) is farther; the mirrored pair is now 1 and 2
    assert ca.map_owner(c, 10.0, 10.0, 5.0, good=[0, 1, 1]) == 1
    # a candidate exactly on the radius is included; just inside a smaller radius it is not
    assert ca.map_owner(np.float32([[13.0, 14.0]]), 10.0, 10.0, 5.0) == 0
    assert ca.map_owner(np.float32([[13.0, 14.0]]), 10.0, 10.0, np.nextafter(np.float32(5.0), np.float32(0.0))) == -1
    # the nearest neighbour is not good: skipped for the next one, or for nobody
    c = np.float32([[10.5, 10.0], [12.0, 10.0], [40.0, 40.0]])
    assert ca.map_owner(c, 10.0, 10.0, 4.0) == 0
    assert ca.map_owner(c, 10.0, 10.0, 4.0, good=[0, 1, 1]) == 1
    assert ca.map_owner(c, 10.0, 10.0, 4.0, good=[0, 0, 1]) == -1
    assert ca.map_owner(c, 10.0, 10.0, 1.0, good=[0, 1, 1]) == -1
    assert ca.map_owner(np.zeros((0, 2), np.float32), 1.0, 1.0, 3.0) == -1
    for bad in (0.0, -1.0, np.inf, np.nan):
        try:
            ca.map_owner(c, 10.0, 10.0, bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_struct_sizes_and_prototypes(engine_lib):
    assert ca.PHOTOMETRY_DTYPE.itemsize == 64 and ca.PHOTO_SUMS == 8
    assert [ca.PHOTOMETRY_DTYPE.fields[k][1] for k in ("n_points", "status", "mean_f", "zncc", "gain", "offset", "rms", "rms_zn",
                                                       "znssd", "max_abs", "reserved")] == [0, 4, 8, 24, 28, 32, 36, 40, 44, 48, 52]
    assert C.sizeof(_ffi.LkPhotometryConfig) == 16 and C.sizeof(_ffi.LkResidualMapConfig) == 32
    assert [ca.PHOTO_OK, ca.PHOTO_BAD_RECORD, ca.PHOTO_OUT_OF_IMAGE, ca.PHOTO_TOO_FEW, ca.PHOTO_FLAT] == list(range(5))
    for name in ("lk_photometry", "lk_photometry_from_sums", "lk_residual_map", "lk_map_owner"):
        assert name in _ffi.SYMBOLS and hasattr(engine_lib, name)
    assert hasattr(engine_lib, "lk_internal_residual_last")
    assert _ffi.SYMBOLS["lk_photometry"][1][1] == C.POINTER(_ffi.LkPhotometryConfig)
    assert _ffi.SYMBOLS["lk_residual_map"][1][1] == C.POINTER(_ffi.LkResidualMapConfig)
    # the library refuses what the header says it refuses, without an engine
    out = np.zeros(1, ca.PHOTOMETRY_DTYPE)
    assert engine_lib.lk_photometry_from_sums(3, None, out.ctypes.data_as(C.c_void_p)) == ca.ERROR_BAD_DOMAIN
    assert engine_lib.lk_photometry(None, None, None, None, None) == ca.ERROR_BAD_DOMAIN
    assert engine_lib.lk_residual_map(None, None, None, None, None, None) == ca.ERROR_BAD_DOMAIN


# the sectors of test_residual_gpu.py's lighting test, at its near-truth records
LIGHT_RECTS = [(8, 8, 26, 26), (40, 8, 46, 14), (8, 60, 38, 88), (140, 140, 239, 239)]
LIGHT_P = np.float32([1.25, -0.65, 0.001, 0.0005, -0.0005, -0.001])


def rect_rows(x0, y0, x1, y1):
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)


def rect_centre(x0, y0, x1, y1):
    pts = rect_rows(x0, y0, x1, y1).astype(np.float64)
    return np.float32(pts[:, 0].mean()), np.float32(pts[:, 1].mean())


def test_lighting_identities_with_the_oracle_alone(oracle):
    """zncc' = zncc, gain' = gain / 2, offset' = offset / 2 + 32, rms_zn' = rms_zn / 2 between the pairs (und, D) and
    (und, D / 2 + 32): the differences the sampler's float rounding leaves, from the oracle's floats and the host function.
    residual_ref.LIGHTING_MEASURED records them; the GPU test allows twice as much.  rms' > rms and rms' > rms_zn' hold."""
    und, dfm = speckle.speckle_pair(256, 256, p=TRUTH, seed=5)
    d, d2 = rr.lighting_frames(dfm)
    assert np.array_equal(d2.astype(np.int32) * 2 - 64, d.astype(np.int32))
    worst = {k: 0.0 for k in rr.LIGHTING_MEASURED}
    for r in LIGHT_RECTS:
        cx, cy = rect_centre(*r)
        recs = []
        for frame in (d, d2):
            f, g, V, bad = rr.sample_values(oracle, ca.IM_BICUBIC, ca.FM_UVUXUYVXVY, und, frame, rect_rows(*r), cx, cy, LIGHT_P)
            assert not bad
            got = ca.photometry_from_sums(len(f), rr.sums_of(f, g, V))
            assert got["status"] == ca.PHOTO_OK
            recs.append(got)
        a, b = recs
        for k, (left, right) in rr.lighting_sides(a, b).items():
            worst[k] = max(worst[k], abs(float(left) - float(right)))
        print(f"{r}: zncc {a['zncc']:.7f} / {b['zncc']:.7f}, gain {a['gain']:.6f} / {b['gain']:.6f}, offset {a['offset']:.4f} / "
              f"{b['offset']:.4f}, rms {a['rms']:.4f} / {b['rms']:.4f}, rms_zn {a['rms_zn']:.4f} / {b['rms_zn']:.4f}")
        assert b["rms"] > a["rms"] and b["rms"] > b["rms_zn"]
    print("largest difference per field:", {k: f"{v:.3g}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= rr.LIGHTING_MEASURED[k] * (1 + 1e-6), (k, v, rr.LIGHTING_MEASURED[k])
