"""The weighted refinement without a GPU (include/lk_engine.h: lk_refine_weighted, lk_weight_window,
lk_weighted_step_from_sums): the window function against a double exponential and, bit for bit, against the restatement
with an exact fused multiply-add; the exported step with N = n against lk_znssd_step_from_sums bit for bit and with a
non-integer N against the numpy restatement; the layouts, the prototypes and the refusals that need no GPU; and the
experiments the GPU tests take their bounds from, run with the restatement alone: the edge sectors with and without the
mask, the border sector, and the Gaussian window on quadratic_ref's curved field.

Window: the float evaluation rounds t = r2 inv - a relative 2^-23 of t at the worst, which is t ln 2 2^-23 of the result - so
within 1e-6 relative over the subset the window is made for, |dx|, |dy| <= 3 sigma (t ln 2 <= 9).  Step: as
test_znssd_host.py, 1e-12 of the largest unknown of the unit-diagonal system."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import quadratic_ref as qr
import spline_ref as sr
import weighted_ref as wr
import znssd_ref as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
SIGMAS = [19 / 6, 31 / 6, 49 / 6, 2.0, 12.5]
REL = 1e-12


# ---- the window -------------------------------------------------------------------------------------------------------------------
def test_window_against_the_double_exponential(engine_lib):
    """over |dx|, |dy| <= 3 sigma on a grid of quarter pixels (every offset a sector's sample has from its centre at levels
    0 and 1) and on one of 0.37 px; the host export is the restatement on a sample of each grid"""
    rng = np.random.default_rng(2)
    worst = 0.0
    for sigma in SIGMAS:
        s32 = float(np.float32(sigma))
        inv = wr.inv_of(sigma)
        for pitch in (0.25, 0.37):
            half = np.arange(0.0, 3.0 * s32 + 1e-9, pitch)
            axis = np.concatenate([-half[:0:-1], half]).astype(np.float32)
            dx, dy = (t.ravel() for t in np.meshgrid(axis, axis))
            w = wr.window32(inv, dx, dy)
            ref = wr.window64(s32, dx, dy)
            rel = np.abs(w.astype(np.float64) - ref) / ref
            worst = max(worst, float(rel.max()))
            assert rel.max() <= 1e-6, (sigma, pitch, rel.max(), dx[rel.argmax()], dy[rel.argmax()])
            pick = rng.integers(0, len(dx), 100)
            got = np.array([ca.weight_window(inv, dx[j], dy[j]) for j in pick], np.float32)
            assert got.tobytes() == w[pick].tobytes(), (sigma, pitch)
    print(f"window: worst |w - exp| / exp over {len(SIGMAS)} sigmas, |d| <= 3 sigma: {worst:.3g} (allowed 1e-6)")


def test_window_bits_against_the_exact_restatement(engine_lib):
    # the vectorised fused multiply-add of the restatement is the exact one (fractions) on random operands
    rng = np.random.default_rng(1)
    a, b, c = (rng.normal(size=200).astype(np.float32) for _ in range(3))
    assert wr.fma32(a, b, c).tobytes() == np.array([sr.fma32(x, y, z) for x, y, z in zip(a, b, c)], np.float32).tobytes()
    inv = wr.inv_of(31 / 6)
    for dx, dy in ((0.0, 0.0), (1.0, 0.0), (0.5, -0.5), (15.0, 15.0), (-7.25, 3.5), (40.0, 0.0), (1.3, -0.7), (1e-3, 2e-3)):
        got, want = ca.weight_window(inv, dx, dy), wr.window32(inv, dx, dy)[0]
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (dx, dy, got, want)
    assert ca.weight_window(inv, 0.0, 0.0) == 1.0 and ca.weight_window(0.0, 5.0, 5.0) == 1.0
    # the cut: t >= 126 is 0, just below it the smallest values are normal floats
    r = np.sqrt(126.0 / float(inv))
    assert ca.weight_window(inv, np.float32(r * 1.001), 0.0) == 0.0 and ca.weight_window(inv, 1e6, 1e6) == 0.0
    small = ca.weight_window(inv, np.float32(r * 0.999), 0.0)
    assert small >= np.finfo(np.float32).tiny and small.tobytes() == wr.window32(inv, np.float32(r * 0.999), 0.0)[0].tobytes()
    # inv is the float of the double formula, per level
    assert wr.inv_of(3.0) == np.float32(wr.LOG2E / 18.0) and wr.inv_of(3.0, level=1) == np.float32(wr.LOG2E / 4.5)
    lib = engine_lib
    w = np.full(1, 7, np.float32)
    for bad in ((-1.0, 0.0, 0.0), (np.nan, 0.0, 0.0), (np.inf, 0.0, 0.0), (0.1, np.nan, 0.0), (0.1, 0.0, np.inf)):
        assert lib.lk_weight_window(*[C.c_float(t) for t in bad], _ffi.fptr(w)) == ca.ERROR_BAD_DOMAIN and w[0] == 7
    assert lib.lk_weight_window(C.c_float(0.1), C.c_float(0.0), C.c_float(0.0), None) == ca.ERROR_BAD_DOMAIN
    with pytest.raises(ValueError):
        ca.weight_window(-1.0, 0.0, 0.0)


# ---- the step -----------------------------------------------------------------------------------------------------------------------
def real_floats(oracle, model, rect=(46, 65, 64, 83), p=(1.1, -0.5, 0.001, 0.0005, -0.0005, 0.001)):
    und, dfm = zr.pair()
    xy = zr.rect_rows(*rect)
    cx, cy = zr.rect_centre(rect)
    f, g, H, bad = zr.sample_floats(oracle, ca.IM_BICUBIC, model, und, dfm, xy, cx, cy, np.float32(p))
    assert not bad.any()
    return xy, cx, cy, f, g, H, bad


@pytest.mark.parametrize("model", MODELS)
def test_step_with_unit_weights_is_the_znssd_step_bit_for_bit(oracle, engine_lib, model):
    xy, cx, cy, f, g, H, bad = real_floats(oracle, model)
    n, sums = len(xy), zr.sums_of(f, g, H, bad)
    assert wr.sums_of(f, g, H, bad, np.ones(n, np.float32)).tobytes() == sums.tobytes()
    for lam in (0.0, 1e-9, 1e-3, 0.1, 10.0, 1e6):
        a, b = ca.weighted_step_from_sums(model, n, float(n), sums, lam), ca.znssd_step_from_sums(model, n, sums, lam)
        assert a[0] == b[0] == 0 and a[1].tobytes() == b[1].tobytes(), (model, lam, a, b)
        assert np.float64(a[2:]).tobytes() == np.float64(b[2:]).tobytes(), (model, lam, a, b)
    P = _ffi.N_PARAMS[model]
    for k in (P + 1, P + 2):   # the too-few rule reads n_valid, whatever N is
        a, b = ca.weighted_step_from_sums(model, k, float(k), sums, 1e-3), ca.znssd_step_from_sums(model, k, sums, 1e-3)
        assert a[0] == b[0] and (a[0] == ca.ZN_TOO_FEW) == (k == P + 1) and a[1].tobytes() == b[1].tobytes()
    assert ca.weighted_step_from_sums(model, P + 1, float(n), sums, 1e-3)[0] == ca.ZN_TOO_FEW


@pytest.mark.parametrize("model", MODELS)
def test_step_with_a_non_integer_weight_sum_against_the_restatement(oracle, engine_lib, model):
    P = _ffi.N_PARAMS[model]
    worst = 0.0
    for rect, sigma, keep in (((46, 65, 64, 83), 19 / 6, 256), ((100, 30, 130, 60), 31 / 6, 256), ((100, 30, 130, 60), 0.0, 120),
                              ((100, 30, 130, 60), 31 / 6, 120)):
        xy, cx, cy, f, g, H, bad = real_floats(oracle, model, rect, p=(1.2, -0.6, 0.001, 0.0, 0.0, -0.001))
        w = wr.sample_weights(xy, cx, cy, wr.inv_of(sigma) if sigma else 0.0, wr.column_mask(keep))
        pro = wr.prologue(xy, cx, cy, w)
        assert (pro["sw"] != round(pro["sw"])) == bool(sigma) and 0 < pro["n_valid"] <= len(xy)
        sums = wr.sums_of(f, g, H, bad, w)
        for lam in (0.0, 1e-3, 10.0):
            got = ca.weighted_step_from_sums(model, pro["n_valid"], pro["sw"], sums, lam)
            want = wr.step(model, pro["n_valid"], pro["sw"], sums, float(np.float32(lam)))
            assert got[0] == want[0] == 0, (model, rect, sigma, keep, lam, got[0], want[0])
            for a, b, absolute in ((got[2], want[2], REL), (got[3], want[3], 0.0), (got[4], want[4], 0.0)):
                assert abs(a - b) <= REL * abs(b) + absolute, (model, lam, a, b)
            assert want[1][:P].all()
            root = want[6][:P] / want[1][:P]             # sqrt(diag A): the restatement's scaled unknowns over its delta
            tol = REL * np.abs(want[6][:P]).max()
            err = np.abs(got[1][:P] * root - want[6][:P]).max()
            assert err <= tol and not got[1][P:].any(), (model, lam, got[1], want[1], err, tol)
            worst = max(worst, err / tol)
        # with the plain count in place of the weight sum the step is another one
        if sigma:
            assert ca.weighted_step_from_sums(model, pro["n_valid"], float(pro["n_valid"]), sums, 1e-3)[3] != got[3]
    print(f"model {model}: worst error / tolerance {worst:.3g}")


@pytest.mark.parametrize("model", MODELS)
def test_restatements_agree_at_unit_weights(oracle, model):
    """weighted_ref's criterion, step and loop are znssd_ref's with (n_valid, N) for n: at N = n they give the same numbers"""
    und, dfm = zr.pair()
    xy, cx, cy, f, g, H, bad = real_floats(oracle, model)
    n, sums = len(xy), zr.sums_of(f, g, H, bad)
    assert wr.criterion(model, n, float(n), sums) == zr.criterion(model, n, sums)
    for lam in (0.0, 1e-3, 10.0):
        a, b = wr.step(model, n, float(n), sums, lam), zr.step(model, n, sums, lam)
        assert a[0] == b[0] == 0 and a[2:6] == b[2:6] and a[1].tobytes() == b[1].tobytes() and a[6].tobytes() == b[6].tobytes()
    P = _ffi.N_PARAMS[model]
    assert wr.step(model, P + 1, float(n), sums, 1e-3)[0] == zr.step(model, P + 1, sums, 1e-3)[0] == ca.ZN_TOO_FEW
    ones = np.ones(n, np.float32)
    seed = np.float32([1.25, -0.65, 0, 0, 0, 0])

    def plain(p):
        return zr.sums_of(*zr.sample_floats(oracle, ca.IM_BICUBIC, model, und, dfm, xy, cx, cy, p))

    def unit(p):
        return wr.sums_of(*zr.sample_floats(oracle, ca.IM_BICUBIC, model, und, dfm, xy, cx, cy, p), ones)
    a, b = wr.loop(unit, model, n, n, float(n), seed), zr.loop(plain, model, n, seed)
    assert a.keys() == b.keys() and a["status"] == ca.ZN_CONVERGED and a["iterations"] > 0
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (model, k, a[k], b[k])


# ---- layouts, prototypes, refusals --------------------------------------------------------------------------------------------------
def test_layouts_and_prototypes():
    d = ca.WEIGHTED_DTYPE
    assert d.itemsize == 80 and C.sizeof(_ffi.LkWeightedConfig) == 48
    offsets = {k: d.fields[k][1] for k in d.names}
    assert offsets == dict(n_points=0, status=4, iterations=8, evaluations=12, zncc=16, gain=20, offset=24, znssd=28, zncc_seed=32,
                           shift=36, last_step=44, n_valid=48, weight_sum=52, n_eff=56, centroid_dx=60, centroid_dy=64, reserved=68,
                           **{"lambda": 40})
    # the first 48 bytes are struct lk_znssd's
    for k in ca.ZNSSD_DTYPE.names[:-1]:
        assert ca.ZNSSD_DTYPE.fields[k] == d.fields[k], k
    text = open(os.path.join(ROOT, "include", "lk_engine.h")).read()
    body = re.search(r"typedef struct lk_weighted_config \{(.*?)\} lk_weighted_config;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n.strip()) for t, names in re.findall(r"^\s*(int|float)\s+([^;]+);", body, re.M) for n in names.split(",")]
    assert fields == [("int", "def_slot"), ("float", "chi_max"), ("int", "max_iters"), ("float", "precision"), ("float", "lambda0"),
                      ("float", "sigma"), ("float", "min_fraction"), ("int", "mask_rows"), ("int", "mask_cols"), ("int", "reserved[3]")]
    S = _ffi.LkWeightedConfig
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("def_slot", 0), ("chi_max", 4), ("max_iters", 8), ("precision", 12),
                                                                  ("lambda0", 16), ("sigma", 20), ("min_fraction", 24), ("mask_rows", 28),
                                                                  ("mask_cols", 32), ("reserved", 36)]
    for name, n_args in (("lk_refine_weighted", 8), ("lk_weight_window", 4), ("lk_weighted_step_from_sums", 9)):
        proto = re.search(r"^int " + name + r"\(([^;]*)\);", text, re.M)
        assert proto and len(proto.group(1).split(",")) == n_args, name
        restype, argtypes = _ffi.SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == n_args, name


def test_refusals_without_a_device(engine_lib):
    lib = engine_lib
    model = ca.FM_UVUXUYVXVY
    status = C.c_int32(77)
    buf = np.zeros(ca.ZN_SUMS)
    ptr = buf.ctypes.data_as(C.c_void_p)

    def call(m=model, n=100, N=100.0, sums=ptr, lam=0.0, st=C.byref(status)):
        return lib.lk_weighted_step_from_sums(m, n, C.c_double(N), sums, C.c_float(lam), None, None, None, st)

    for kw in (dict(m=9), dict(n=-1), dict(N=-1.0), dict(N=np.nan), dict(N=np.inf), dict(sums=None), dict(st=None), dict(lam=-1.0),
               dict(lam=np.nan)):
        assert call(**kw) == ca.ERROR_BAD_DOMAIN, kw
    assert status.value == 77
    assert call() == 0 and status.value == ca.ZN_FLAT
    assert call(N=0.0) == 0 and status.value == ca.ZN_FLAT            # no weight at all: refused, no NaN escapes
    with pytest.raises(ValueError):
        ca.weighted_step_from_sums(model, 10, -1.0, buf, 0.0)
    cfg = _ffi.LkWeightedConfig()
    assert lib.lk_refine_weighted(None, C.byref(cfg), None, None, None, None, None, None) == ca.ERROR_BAD_DOMAIN


# ---- the experiments behind the GPU tests' bounds --------------------------------------------------------------------------------
def test_edge_sectors_of_the_restatement(oracle):
    """EDGE_MASKED, EDGE_UNMASKED and the prologue of the edge sectors"""
    und, dfm = wr.edge_pair()
    mask = wr.column_mask(wr.EDGE_KEEP + 1)
    seed = zr.zero_gradient_seeds(1)[0]
    masked, plain = [], []
    for r in wr.EDGE_RECTS:
        xy = zr.rect_rows(*r)
        cx, cy = zr.rect_centre(r)
        u, v = zr.analytic_uv(float(cx), float(cy))
        a, w, pro = wr.refine(oracle, und, dfm, xy, cx, cy, seed, mask=mask)
        b = zr.loop(lambda p: zr.sums_of(*wr.affine_floats(oracle, und, dfm, xy, cx, cy, p)), ca.FM_UVUXUYVXVY, len(xy), seed)
        assert a["status"] == ca.ZN_CONVERGED and b["status"] == ca.ZN_CONVERGED, (r, a["status"], b["status"])
        assert (pro["n_valid"], pro["sw"], pro["n_eff"], pro["centroid"]) == (620, 620.0, 620.0, (-5.5, 0.0))
        masked.append(max(abs(float(a["p"][0]) - u), abs(float(a["p"][1]) - v)))
        plain.append(max(abs(float(b["p"][0]) - u), abs(float(b["p"][1]) - v)))
    print(f"edge: masked largest {max(masked):.6f} mean {np.mean(masked):.6f} px; unmasked mean {np.mean(plain):.6f} px "
          f"({np.mean(plain) / max(masked):.1f} times the masked largest)")
    assert 0.5 * wr.EDGE_MASKED <= max(masked) <= wr.EDGE_MASKED, "EDGE_MASKED is no longer the measured figure"
    assert 0.9 * wr.EDGE_UNMASKED <= np.mean(plain) <= 1.1 * wr.EDGE_UNMASKED, "EDGE_UNMASKED is no longer the measured figure"
    assert np.mean(plain) >= 4.0 * wr.EDGE_MASKED


def test_border_sector_of_the_restatement(oracle):
    und, dfm = zr.pair()
    xy = zr.rect_rows(*wr.BORDER_RECT)
    cx, cy = zr.rect_centre(wr.BORDER_RECT)
    seed = zr.zero_gradient_seeds(1)[0]
    u, v = zr.analytic_uv(float(cx), float(cy))
    plain = wr.refine(oracle, und, dfm, xy, cx, cy, seed)[0]
    assert plain["status"] == ca.ZN_OUT_OF_IMAGE and plain["evaluations"] == 1
    a, w, pro = wr.refine(oracle, und, dfm, xy, cx, cy, seed, mask=wr.column_mask(wr.BORDER_CUT))
    err = max(abs(float(a["p"][0]) - u), abs(float(a["p"][1]) - v))
    print(f"border: masked |(u, v) - analytic| = {err:.6f} px, n_valid {pro['n_valid']} of {len(xy)}")
    assert a["status"] == ca.ZN_CONVERGED and pro["n_valid"] == 27 * 31
    assert 0.5 * wr.BORDER <= err <= wr.BORDER <= 1.5 * zr.ACCURACY


def test_gaussian_window_of_the_restatement(oracle):
    """GAUSS[side] with sigma = side / 6 on the curved field, and that it is at most half of the unit-weight figure"""
    und, dfm = qr.pair()
    for side in (31, 49):
        errs, n_eff = [], 0.0
        for x, y in qr.CENTRES:
            r = qr.square(x, y, side)
            xy = zr.rect_rows(*r)
            cx, cy = zr.rect_centre(r)
            g, truth = qr.true_translation_seeds([(cx, cy)])
            a, w, pro = wr.refine(oracle, und, dfm, xy, cx, cy, g[0], sigma=side / 6)
            assert a["status"] == ca.ZN_CONVERGED, (side, x, y, a["status"])
            errs.append(max(abs(float(a["p"][0]) - truth[0][0]), abs(float(a["p"][1]) - truth[0][1])))
            n_eff = pro["n_eff"]
        mean = float(np.mean(errs))
        print(f"gaussian window, side {side}, sigma {side / 6:.3f}: mean error {mean:.6f} px (largest {max(errs):.6f}), "
              f"{mean / qr.AFFINE_BIAS[side]:.2f} of the unit-weight {qr.AFFINE_BIAS[side]}; n_eff {n_eff:.1f} of {side * side}")
        assert 0.5 * wr.GAUSS[side] <= mean <= wr.GAUSS[side], "GAUSS is no longer the measured figure"
        assert wr.GAUSS[side] <= 0.5 * qr.AFFINE_BIAS[side]
