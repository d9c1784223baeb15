"""The B-spline refinement on the GPU (lk_refine_spline, lk_spline_coefficients, lk_spline_sample; include/lk_engine.h):
the coefficient image against the float32 restatement byte for byte and against the float64 one, the sampler at the nodes,
at random points and at the edge of its validity rule, the interpolation bias beside lk_refine_znssd's, and the contract of
the pass - seeds, sums, batch and lane-group independence, the border, a bad record, the refusals, the engine's state.

Bounds.  Coefficients against float64: 2e-3 grey levels, 4 x the 5.2e-4 measured between the float32 recipe and a float64
filter at the border of a 33 x 29 image (the margin covers another image and a rounding that scales with |c|, up to about
560).  Sampler: W within 64 x 2^-24 x max|c| - 36 rounded products and sums of weights that sum to 1 - and the two
derivatives within twice that.  Bias: |mean (u - s)| of the spline pass at most half the bicubic's, for both orders at both
shifts; with 64 sectors the standard error of a mean is about 0.0005 px against a bicubic bias of 0.006 px."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi, speckle

import spline_ref as sr
import znssd_ref as zr

pytestmark = pytest.mark.gpu

ORDERS = [3, 5]
SLOTS = [ca.IMG_UND, ca.IMG_DEF, ca.IMG_NXT]
# 67 x 45, 33 x 29 and 9 x 8 (a line shorter than the 28 terms of the start-up sum); 45 x 67 and 20 x 129: rows of two and
# three 64-column tiles, the last of three elements and of one
SHAPES = [(67, 45), (33, 29), (9, 8), (45, 67), (20, 129)]


def image(shape, seed=3):
    """a small speckle image: blobs as speckle.blobs, denser so that a 9 x 8 image has some"""
    h, w = shape
    xs, ys, amps = speckle.blobs(h, w, seed, density=12)
    return speckle._render(h, w, xs, ys, amps, 1.5)


def image_engine(img, slots=SLOTS, **kw):
    e = ca.HipCorrelationEngine(py_start=0, py_stop=0, **kw)
    for slot in slots:
        e.set_image(slot, img)
    return e


# ---- 1. the coefficient image ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_coefficients_are_the_restatements_bytes(shape):
    img = image(shape)
    with image_engine(img) as e:
        for order in ORDERS:
            want = sr.prefilter(img, order)
            for slot in SLOTS:
                got = e.spline_coefficients(slot, order)
                assert got.shape == shape and got.dtype == np.float32
                diff = np.abs(got - want).max()
                assert got.tobytes() == want.tobytes(), (shape, order, slot, diff)
        assert e.spline_coefficients(ca.IMG_DEF, 0).tobytes() == sr.prefilter(img, 5).tobytes()   # order 0 is 5


def test_coefficients_after_an_unrelated_solve_and_against_float64():
    img = image((67, 45))
    with ca.HipCorrelationEngine(py_start=0, py_stop=0, fitting_model=ca.FM_UV) as e:
        e.set_undeformed_image(img)
        e.set_deformed_image(img)
        before = [e.spline_coefficients(ca.IMG_DEF, order) for order in ORDERS]
        e.resetPolygon_rect(0, 8, 8, 26, 26)
        e.commit_sectors()
        rec = e.correlate_all(np.zeros((1, 6), np.float32))
        assert rec["error_code"][0] == 0
        e.refine_spline(guesses=np.zeros((1, 6), np.float32), order=3)
        for order, kept in zip(ORDERS, before):
            got = e.spline_coefficients(ca.IMG_DEF, order)
            assert got.tobytes() == kept.tobytes() == sr.prefilter(img, order).tobytes(), order
            err = np.abs(got.astype(np.float64) - sr.prefilter(img, order, np.float64)).max()
            print(f"order {order}: max |float32 on the device - float64| = {err:.3g}, max |c| = {np.abs(got).max():.4g}")
            assert err <= 2e-3, (order, err)


# ---- 2. the sampler -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sampled():
    img = image((67, 45))
    return img, {order: sr.prefilter(img, order) for order in ORDERS}


@pytest.mark.parametrize("order", ORDERS)
def test_sampler_returns_the_pixels_at_the_nodes(sampled, order):
    img, _ = sampled
    rows, cols = img.shape
    L = 2 if order == 3 else 3   # two pixels or more inside; the quintic's rule begins a pixel further in
    ys, xs = np.mgrid[L:rows - L, L:cols - L]
    with image_engine(img, [ca.IMG_DEF]) as e:
        out = e.spline_sample(ca.IMG_DEF, np.stack([xs.ravel(), ys.ravel()], 1), order)
    assert (out[:, 3] == 1).all()
    err = np.abs(out[:, 0] - img[L:rows - L, L:cols - L].ravel()).max()
    print(f"order {order}: max |W - pixel| at {len(out)} nodes = {err:.3g}")
    assert err <= 1e-3, (order, err)


@pytest.mark.parametrize("order", ORDERS)
def test_sampler_at_random_points_and_at_the_edge_of_its_rule(sampled, order):
    img, coef = sampled
    rows, cols = img.shape
    L = order // 2
    rng = np.random.default_rng(17)
    pts = np.stack([rng.uniform(L, cols - L - 1, 2000), rng.uniform(L, rows - L - 1, 2000)], 1).astype(np.float32)
    # the edge: on it and one float inside, on all four sides
    lo, hi_x, hi_y, mid = np.float32(L), np.float32(cols - L - 1), np.float32(rows - L - 1), np.float32(10.5)
    up, down = (lambda v: np.nextafter(v, np.float32(np.inf))), (lambda v: np.nextafter(v, np.float32(-np.inf)))
    edge = np.float32([(lo, mid), (up(lo), mid), (hi_x, mid), (down(hi_x), mid), (mid, lo), (mid, up(lo)), (mid, hi_y), (mid, down(hi_y)),
                       (np.nan, mid), (mid, -1.0), (1e9, mid)])
    want_ok = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 0], bool)
    assert (sr.valid(order, edge, rows, cols) == want_ok).all()
    with image_engine(img, [ca.IMG_DEF]) as e:
        out = e.spline_sample(ca.IMG_DEF, np.concatenate([pts, edge]), order)
    ok = sr.valid(order, np.concatenate([pts, edge]), rows, cols)
    assert (out[:, 3] == ok).all() and not out[~ok].any()
    assert ok[:2000].sum() > 1900
    W, Wx, Wy = sr.sample64(coef[order], np.concatenate([pts, edge])[ok], order)
    bound = 64 * 2.0 ** -24 * float(np.abs(coef[order]).max())
    errs = [np.abs(out[ok][:, k] - ref).max() for k, ref in enumerate((W, Wx, Wy))]
    print(f"order {order}: max |W, Wx, Wy - float64| = {errs[0]:.3g}, {errs[1]:.3g}, {errs[2]:.3g}; bound {bound:.3g} (twice for the derivatives)")
    assert errs[0] <= bound and errs[1] <= 2 * bound and errs[2] <= 2 * bound, (errs, bound)


# ---- 3. the interpolation bias ----------------------------------------------------------------------------------------------------
BIAS_SIDE, BIAS_GRID = 21, 8
BIAS_RECTS = [(12 + BIAS_SIDE * i, 12 + BIAS_SIDE * j, 12 + BIAS_SIDE * i + BIAS_SIDE - 1, 12 + BIAS_SIDE * j + BIAS_SIDE - 1)
              for j in range(BIAS_GRID) for i in range(BIAS_GRID)]


def shifted_pair(s, size=192):
    xs, ys, amps = speckle.blobs(size, size, 7)
    return speckle._render(size, size, xs, ys, amps, 2.5), speckle._render(size, size, xs + np.float32(s), ys + np.float32(0.3), amps, 2.5)


@pytest.fixture(scope="module")
def bias():
    """mean over the sectors of u - s: {shift: {"bicubic" | 3 | 5: mean}}"""
    out = {}
    for s in (0.25, 0.75):
        und, dfm = shifted_pair(s)
        with ca.HipCorrelationEngine(interpolation=ca.IM_BICUBIC, fitting_model=ca.FM_UV, precision=1e-3, py_start=0, py_stop=2) as e:
            e.set_undeformed_image(und)
            e.set_deformed_image(dfm)
            for k, r in enumerate(BIAS_RECTS):
                e.resetPolygon_rect(k, *r)
            e.commit_sectors()
            g = np.zeros((e.n_sectors, 6), np.float32)
            g[:, 0], g[:, 1] = s + 0.2, 0.1
            runs = {"bicubic": e.refine_znssd(guesses=g), 3: e.refine_spline(guesses=g, order=3), 5: e.refine_spline(guesses=g, order=5)}
        out[s] = {}
        for name, (rec, info) in runs.items():
            assert (info["status"] == ca.ZN_CONVERGED).all(), (s, name, info["status"])
            out[s][name] = float((rec["p"][:, 0].astype(np.float64) - s).mean())
            print(f"shift {s}: {name}: mean u - s = {out[s][name]:+.5f} px, mean v - 0.3 = "
                  f"{float((rec['p'][:, 1].astype(np.float64) - 0.3).mean()):+.5f} px, rms of u about its mean "
                  f"{float(rec['p'][:, 0].astype(np.float64).std()):.5f} px")
    return out


def test_the_bicubic_bias_is_the_s_curve(bias):
    assert bias[0.25]["bicubic"] * bias[0.75]["bicubic"] < 0, bias


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shift", [0.25, 0.75])
def test_the_spline_halves_the_bias_at_least(bias, order, shift):
    assert abs(bias[shift][order]) <= 0.5 * abs(bias[shift]["bicubic"]), (shift, order, bias[shift])


# ---- 4. the contract of the pass ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    return zr.pair()


# 64 rectangles of 361 samples, then 49, 576 and 10 000 samples: 16-lane rows, a wavefront, the 512-lane group
RECTS = zr.GRID + [(170, 20, 176, 26), (180, 40, 203, 63), (150, 150, 249, 249)]
SMALL, WAVE, BIG = len(zr.GRID), len(zr.GRID) + 1, len(zr.GRID) + 2


def make_engine(und, dfm, rects=RECTS, model=ca.FM_UVUXUYVXVY, commit=True):
    e = ca.HipCorrelationEngine(interpolation=ca.IM_BICUBIC, fitting_model=model, precision=zr.PRECISION, py_start=0, py_stop=2)
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    for s, r in enumerate(rects):
        e.resetPolygon_rect(s, *r)
    if commit:
        e.commit_sectors()
    return e


@pytest.fixture(scope="module")
def batch(pair):
    with make_engine(*pair) as e:
        assert [e.sector_info(s)[0] for s in (0, SMALL, WAVE, BIG)] == [361, 49, 576, 10000]
        return {order: e.refine_spline(guesses=zr.zero_gradient_seeds(len(RECTS)), order=order, return_sums=True) for order in ORDERS}


@pytest.mark.parametrize("order", ORDERS)
def test_records_and_guesses_seed_alike_and_the_sums_give_the_info(pair, batch, order):
    rec, info, sums = batch[order]
    n = len(RECTS)
    print("order", order, "status histogram", np.bincount(info["status"], minlength=9), "trips", info["iterations"].min(), "..",
          info["iterations"].max())
    # (six parameters on the 49 samples of the 7 x 7 sector need not settle within 50 trips; its bytes are compared all the same)
    big = info["n_points"] >= 361
    assert (info["status"][big] == ca.ZN_CONVERGED).all() and (rec["error_code"][big] == 0).all(), info["status"]
    assert info["status"][SMALL] in (ca.ZN_CONVERGED, ca.ZN_MAX_ITERS)
    # against the analytic map at the centres of the 19 x 19 sectors: lk_refine_znssd's bound on the same sectors (1.5 x the
    # restatement's 0.0265 px, znssd_ref.py) plus the 0.01 px by which two samplers may differ (the size of the bicubic's bias)
    want = np.array([zr.analytic_uv(*(float(c) for c in zr.rect_centre(r))) for r in RECTS[:SMALL]])
    err = np.hypot(rec["p"][:SMALL, 0] - want[:, 0], rec["p"][:SMALL, 1] - want[:, 1])
    print(f"order {order}: max |(u, v) - analytic map| over the 19 x 19 sectors = {err.max():.4f} px")
    assert err.max() <= 1.5 * zr.ACCURACY + 0.01, err.max()
    seeds = np.zeros(n, ca.RESULT_DTYPE)
    seeds["p"][:] = zr.zero_gradient_seeds(n)
    with make_engine(*pair) as e:
        r, i, q = e.refine_spline(records=seeds, order=order, return_sums=True)
    assert r.tobytes() == rec.tobytes() and i.tobytes() == info.tobytes() and q.tobytes() == sums.tobytes()
    for s in (0, 37, SMALL, WAVE, BIG):
        status, _, crit, gain, offset = ca.znssd_step_from_sums(ca.FM_UVUXUYVXVY, int(info["n_points"][s]), sums[s], float(info["lambda"][s]))
        zncc = zr.criterion(ca.FM_UVUXUYVXVY, int(info["n_points"][s]), sums[s])[4]
        assert status == 0
        for name, want in (("gain", gain), ("offset", offset), ("znssd", crit), ("zncc", zncc)):
            assert info[name][s].tobytes() == np.float32(want).tobytes(), (s, name, info[name][s], want)


@pytest.mark.parametrize("order", ORDERS)
def test_a_sector_alone_gives_the_bytes_of_the_batch(pair, batch, order):
    rec, info, sums = batch[order]
    seeds = zr.zero_gradient_seeds(1)
    for k in (0, SMALL, WAVE, BIG):   # 16 lanes twice, 64 and 512
        with make_engine(*pair, [RECTS[k]]) as e:
            r, i, q = e.refine_spline(guesses=seeds, order=order, return_sums=True)
            assert r[0].tobytes() == rec[k].tobytes() and i[0].tobytes() == info[k].tobytes() and q[0].tobytes() == sums[k].tobytes(), k


def test_the_border_a_bad_record_and_the_orders(pair):
    # x + u = 252 + 1.3: the quintic's six nodes end at column 256, the cubic's four at 255
    rects = [(234, 100, 252, 118), (100, 100, 118, 118)]
    with make_engine(*pair, rects, model=ca.FM_UV) as e:
        g = zr.zero_gradient_seeds(2)
        (r3, i3), (r5, i5) = e.refine_spline(guesses=g, order=3), e.refine_spline(guesses=g, order=5)
        assert i3["status"].tolist() == [ca.ZN_CONVERGED, ca.ZN_CONVERGED], i3["status"]
        assert i5["status"].tolist() == [ca.ZN_OUT_OF_IMAGE, ca.ZN_CONVERGED], i5["status"]
        assert r5["error_code"][0] == ca.ERROR_INTERPOLATION_OUT_OF_IMAGE and r5["p"][0].tobytes() == g[0].tobytes() and r5["chi"][0] == 0
        assert i5["evaluations"][0] == 1 and i5["iterations"][0] == 0 and i5["zncc"][0] == 0
        assert r3["p"][1].tobytes() != r5["p"][1].tobytes()     # two samplers
        assert np.abs(r3["p"][1, :2] - r5["p"][1, :2]).max() < 0.01
        # records as seeds: a bad one passes through byte for byte
        seeds = np.zeros(2, ca.RESULT_DTYPE)
        seeds["p"][:] = g
        seeds["chi"] = 1.0
        seeds["error_code"][1] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        seeds["iterations"][1] = 50
        out, oi = e.refine_spline(records=seeds, order=3)
        assert oi["status"].tolist() == [ca.ZN_CONVERGED, ca.ZN_BAD_SEED]
        assert out[1].tobytes() == seeds[1].tobytes() and oi["evaluations"][1] == 0
        seeds["error_code"][1] = 0
        seeds["p"][1, 1] = np.nan
        assert e.refine_spline(records=seeds)[0][1].tobytes() == seeds[1].tobytes()
        seeds["p"][1, 1] = g[1, 1]
        seeds["chi"][1] = 5.0
        assert e.refine_spline(records=seeds, chi_max=2.0, order=3)[1]["status"].tolist() == [ca.ZN_CONVERGED, ca.ZN_BAD_SEED]
        # the engine's interpolation plays no part
        a = e.refine_spline(guesses=g, order=5)
    e2 = ca.HipCorrelationEngine(interpolation=ca.IM_BILINEAR, fitting_model=ca.FM_UV, precision=zr.PRECISION, py_start=0, py_stop=2)
    with e2:
        e2.set_undeformed_image(pair[0])
        e2.set_deformed_image(pair[1])
        for s, r in enumerate(rects):
            e2.resetPolygon_rect(s, *r)
        e2.commit_sectors()
        b = e2.refine_spline(guesses=g, order=5)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


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


def test_engine_state_is_untouched(pair):
    rects = zr.GRID[:16]
    seeds = zr.zero_gradient_seeds(16)
    seeds[9, 0] = 300.0
    with make_engine(*pair, rects) as e, make_engine(*pair, rects) as plain:
        first = e.correlate_all(seeds)
        plain.correlate_all(seeds)

        def state():
            return dict(records=device_records(e), guesses=e.get_guesses(), last_eval=e.last_evaluated_parameters(), stats=e.sector_stats())

        kept = state()
        a = e.refine_spline()
        b = e.refine_spline(records=first, order=5)
        c = e.refine_spline(guesses=zr.zero_gradient_seeds(16), order=3)
        e.spline_coefficients(ca.IMG_UND, 3)
        e.spline_sample(ca.IMG_DEF, [[20.5, 30.25]], 5)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert a[1]["status"][9] == ca.ZN_BAD_SEED and (c[1]["status"] == ca.ZN_CONVERGED).all()
        after = state()
        for k in kept:
            assert kept[k].tobytes() == after[k].tobytes(), k
        assert e.correlate_all(zr.zero_gradient_seeds(16)).tobytes() == plain.correlate_all(zr.zero_gradient_seeds(16)).tobytes()


def test_arguments_and_refusals(pair):
    rects = zr.GRID[:9]
    e = make_engine(*pair, rects, commit=False)
    lib, h = e.lib, e._h
    seeds = np.zeros(9, ca.RESULT_DTYPE)
    seeds["p"][:] = zr.zero_gradient_seeds(9)
    g = zr.zero_gradient_seeds(9)
    rec = np.full(9, 7, np.uint8).repeat(48).view(ca.RESULT_DTYPE)
    info = np.full(9, 7, np.uint8).repeat(64).view(ca.ZNSSD_DTYPE)
    sums = np.full((9, ca.ZN_SUMS), 7.0)
    kept = [rec.tobytes(), info.tobytes(), sums.tobytes()]

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def config(**kw):
        fields = dict(def_slot=-1, chi_max=0.0, max_iters=-1, precision=0.0, lambda0=0.0, order=0)
        fields.update(kw)
        return _ffi.LkSplineConfig(**fields)

    def refused(cfg="default", records=None, guesses=None, outputs=(rec, info), word=None, **kw):
        if cfg == "default":
            cfg = config(**kw)
        if word is not None:
            cfg.reserved[word] = 1
        rc = lib.lk_refine_spline(h, C.byref(cfg) if cfg is not None else None, ptr(records), _ffi.fptr(guesses) if guesses is not None else None,
                                  ptr(outputs[0]), ptr(outputs[1]), ptr(sums))
        msg = lib.lk_last_error_string(h).decode()
        assert rc == ca.ERROR_BAD_DOMAIN and msg.startswith("lk_refine_spline: "), (rc, msg)   # names the function called
        return msg

    assert "no committed sectors" in refused(guesses=g) and "no committed sectors" in refused(records=seeds)
    e.commit_sectors()
    assert "no solve" in refused()
    assert "no configuration" in refused(None, guesses=g)
    assert "no output" in refused(guesses=g, outputs=(None, None))
    for word in range(2):
        assert "reserved" in refused(guesses=g, word=word)
    for order in (4, 1, -3, 7):
        assert "order must be 3 or 5" in refused(guesses=g, order=order)
    assert "both given" in refused(records=seeds, guesses=g)
    assert "chi_max" in refused(records=seeds, chi_max=np.nan) and "chi_max" in refused(guesses=g, chi_max=np.inf)
    assert "precision" in refused(guesses=g, precision=np.nan) and "lambda0" in refused(guesses=g, lambda0=np.inf)
    assert "ring slot" in refused(guesses=g, def_slot=0) and "def_slot" in refused(guesses=g, def_slot=-2)
    assert [rec.tobytes(), info.tobytes(), sums.tobytes()] == kept       # every refusal left the outputs as they were
    # the two image calls: order, output, points, a slot that is not set
    out = np.full((256, 256), 7, np.float32)
    for call, args in (("lk_spline_coefficients", (ca.IMG_DEF, 4, _ffi.fptr(out))), ("lk_spline_coefficients", (ca.IMG_DEF, 5, None)),
                       ("lk_spline_coefficients", (ca.IMG_NXT, 5, _ffi.fptr(out))), ("lk_spline_sample", (ca.IMG_DEF, 2, _ffi.fptr(g), 9, _ffi.fptr(out))),
                       ("lk_spline_sample", (ca.IMG_DEF, 5, None, 9, _ffi.fptr(out))), ("lk_spline_sample", (ca.IMG_DEF, 5, _ffi.fptr(g), 0, _ffi.fptr(out))),
                       ("lk_spline_sample", (7, 5, _ffi.fptr(g), 9, _ffi.fptr(out)))):
        assert getattr(lib, call)(h, *args) == ca.ERROR_BAD_DOMAIN, (call, args)
        assert lib.lk_last_error_string(h).decode().startswith(call + ": "), (call, lib.lk_last_error_string(h))
    assert (out == 7).all()
    # either output alone; the defaults of the C configuration are lk_refine_znssd's; order 0 is the quintic
    cfg = config()
    assert lib.lk_refine_spline(h, C.byref(cfg), None, _ffi.fptr(g), ptr(rec), None, None) == 0
    assert lib.lk_refine_spline(h, C.byref(cfg), ptr(seeds), None, None, ptr(info), None) == 0
    both = e.refine_spline(guesses=g, order=5, max_iters=50, precision=1e-3, lambda0=1e-3)
    assert rec.tobytes() == both[0].tobytes() and info.tobytes() == both[1].tobytes() and (info["status"] == ca.ZN_CONVERGED).all()
    # a solve in flight refuses the engine-held records and finishes normally afterwards
    e.correlate_all_async()
    assert "waited for" in refused()
    solved = e.wait_results()
    assert e.refine_spline()[0].tobytes() == e.refine_spline(records=solved)[0].tobytes()
    e.close()
    # a level image with a side below 8
    tiny = image((20, 7))
    with image_engine(tiny, [ca.IMG_UND, ca.IMG_DEF], fitting_model=ca.FM_U) as t:
        out = np.zeros((20, 7), np.float32)
        assert t.lib.lk_spline_coefficients(t._h, ca.IMG_DEF, 3, _ffi.fptr(out)) == ca.ERROR_BAD_DOMAIN
        assert "lk_spline_coefficients: the level image has a side below 8" in t.lib.lk_last_error_string(t._h).decode()
        t.resetPolygon_rect(0, 2, 8, 4, 12)
        t.commit_sectors()
        with pytest.raises(ca.LkError, match="lk_refine_spline: the level image has a side below 8"):
            t.refine_spline(guesses=np.zeros((1, 6), np.float32))
