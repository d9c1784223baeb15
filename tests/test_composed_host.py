"""The host side of the composed refinement (include/lk_engine.h: lk_refine_composed, lk_composed_step_from_sums), on the CPU:
the layout of the two records and the prototypes; lk_composed_step_from_sums against the steps it is made of, bit for bit,
and with a non-integer weight sum against composed_ref's float64 restatement (the unknowns of the unit-diagonal system
within 1e-12 of their largest, as test_quadratic_host.py and test_weighted_host.py); the refusals that need no device; that
composed_ref's copies agree with quadratic_ref at N = n; and the two experiments behind the GPU tests' pinned figures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import composed_ref as cr
import quadratic_ref as qr
import weighted_ref as wr
import znssd_ref as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
REL = 1e-12
SEED = np.float32([1.25, -0.65, 0.001, 0.0005, -0.0005, -0.001, 1e-4, -1e-4, 5e-5, -5e-5, 1e-4, -1e-4])


# ---- layouts and prototypes ---------------------------------------------------------------------------------------------------------
def test_layouts_and_prototypes():
    d, q, w = ca.COMPOSED_DTYPE, ca.QUADRATIC_DTYPE, ca.WEIGHTED_DTYPE
    assert d.itemsize == 128 == q.itemsize and C.sizeof(_ffi.LkComposedConfig) == 64
    for k in q.names[:-1]:     # struct lk_quadratic up to and including bend
        assert d.fields[k] == q.fields[k], k
    assert q.names[-2] == "bend" and d.fields["n_valid"][1] == q.fields["reserved"][1] == 100
    names = ("n_valid", "weight_sum", "n_eff", "centroid_dx", "centroid_dy")
    assert [d.fields[k][1] for k in names] == [100, 104, 108, 112, 116] and d.fields["reserved"][1] == 120
    assert all(d.fields[k][0] == w.fields[k][0] for k in names) and d.fields["reserved"][0].shape == (2,)
    text = open(os.path.join(ROOT, "include", "lk_engine.h")).read()
    body = re.search(r"typedef struct lk_composed_config \{(.*?)\} lk_composed_config;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n.strip()) for t, names_ in re.findall(r"^\s*(int|float)\s+([^;]+);", body, re.M) for n in names_.split(",")]
    assert fields == [("int", "def_slot"), ("float", "chi_max"), ("int", "max_iters"), ("float", "precision"), ("float", "lambda0"),
                      ("int", "order"), ("int", "sampler"), ("float", "sigma"), ("float", "min_fraction"), ("int", "mask_rows"),
                      ("int", "mask_cols"), ("int", "reserved[5]")]
    S = _ffi.LkComposedConfig
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [
        ("def_slot", 0), ("chi_max", 4), ("max_iters", 8), ("precision", 12), ("lambda0", 16), ("order", 20), ("sampler", 24),
        ("sigma", 28), ("min_fraction", 32), ("mask_rows", 36), ("mask_cols", 40), ("reserved", 44)]
    body = re.search(r"struct lk_composed \{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    words = [n.strip() for _, names_ in re.findall(r"^\s*(int32_t|float)\s+([^;]+);", body, re.M) for n in names_.split(",")]
    assert words == ["n_points", "status", "iterations", "evaluations", "p[12]", "zncc", "gain", "offset", "znssd", "zncc_seed", "shift",
                     "lambda", "last_step", "bend", "n_valid", "weight_sum", "n_eff", "centroid_dx", "centroid_dy", "reserved[2]"]
    for name, n_args in (("lk_refine_composed", 9), ("lk_composed_step_from_sums", 10)):
        proto = re.search(r"^int " + name + r"\(([^;]*)\);", text, re.M)
        assert proto and len(proto.group(1).split(",")) == n_args, name
        restype, argtypes = _ffi.SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == n_args, name
    assert hasattr(ca.HipCorrelationEngine, "refine_composed") and ca.composed_step_from_sums is _ffi.composed_step_from_sums


# ---- the step -------------------------------------------------------------------------------------------------------------------------
def first_order_floats(oracle, model, rect=(46, 65, 64, 83), p=(1.1, -0.5, 0.001, 0.0005, -0.0005, 0.001)):
    und, dfm = zr.pair()
    xy = zr.rect_rows(*rect)
    cx, cy = zr.rect_centre(rect)
    f, g, H, bad = zr.sample_floats(oracle, ca.IM_BICUBIC, model, und, dfm, xy, cx, cy, np.float32(p))
    assert not bad.any()
    return xy, cx, cy, f, g, H, bad


def second_order_floats(oracle, rect=(46, 65, 76, 95), p=SEED):
    und, dfm = qr.pair()
    xy = qr.rect_rows(*rect)
    cx, cy = zr.rect_centre(rect)
    out = qr.sample_floats(oracle, ca.IM_BICUBIC, und, dfm, xy, cx, cy, p)
    assert not out[6].any()
    return (xy, cx, cy) + out


@pytest.mark.parametrize("model", MODELS)
def test_order_1_is_the_znssd_step_bit_for_bit(oracle, engine_lib, model):
    xy, cx, cy, f, g, H, bad = first_order_floats(oracle, model)
    n, sums = len(xy), zr.sums_of(f, g, H, bad)
    P = _ffi.N_PARAMS[model]
    for lam in (0.0, 1e-9, 1e-3, 0.1, 10.0, 1e6):
        a, b = ca.composed_step_from_sums(1, model, n, float(n), sums, lam), ca.znssd_step_from_sums(model, n, sums, lam)
        assert a[0] == b[0] == 0 and a[1][:6].tobytes() == b[1].tobytes() and not a[1][P:].any(), (model, lam, a, b)
        assert np.float64(a[2:]).tobytes() == np.float64(b[2:]).tobytes(), (model, lam, a, b)
    for k in (P + 1, P + 2):   # the too-few rule reads n_valid, whatever N is
        a, b = ca.composed_step_from_sums(1, model, k, float(k), sums, 1e-3), ca.znssd_step_from_sums(model, k, sums, 1e-3)
        assert a[0] == b[0] and (a[0] == ca.ZN_TOO_FEW) == (k == P + 1)
    # a weight sum that is no integer: lk_weighted_step_from_sums, bit for bit
    w = wr.sample_weights(xy, cx, cy, wr.inv_of(19 / 6))
    pro, ws = wr.prologue(xy, cx, cy, w), wr.sums_of(f, g, H, bad, w)
    a, b = ca.composed_step_from_sums(1, model, pro["n_valid"], pro["sw"], ws, 1e-3), ca.weighted_step_from_sums(model, pro["n_valid"], pro["sw"], ws, 1e-3)
    assert a[0] == b[0] == 0 and a[1][:6].tobytes() == b[1].tobytes() and np.float64(a[2:]).tobytes() == np.float64(b[2:]).tobytes()


def test_order_2_is_the_quadratic_step_bit_for_bit(oracle, engine_lib):
    xy, cx, cy, f, g, gx, gy, dx, dy, bad = second_order_floats(oracle)
    n, sums = len(xy), qr.sums_of(f, g, gx, gy, dx, dy, bad)
    assert cr.sums_of(f, g, gx, gy, dx, dy, bad, np.ones(n, np.float32)).tobytes() == sums.tobytes()
    for model in MODELS + [77]:     # (the model plays no part)
        for lam in (0.0, 1e-9, 1e-3, 0.1, 10.0, 1e6):
            a, b = ca.composed_step_from_sums(2, model, n, float(n), sums, lam), ca.quadratic_step_from_sums(n, sums, lam)
            assert a[0] == b[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[1].all(), (model, lam, a, b)
            assert np.float64(a[2:]).tobytes() == np.float64(b[2:]).tobytes(), (model, lam, a, b)
    for k in (13, 14):
        a, b = ca.composed_step_from_sums(2, 0, k, float(k), sums, 1e-3), ca.quadratic_step_from_sums(k, sums, 1e-3)
        assert a[0] == b[0] and (a[0] == ca.ZN_TOO_FEW) == (k == 13) and a[1].tobytes() == b[1].tobytes()
    assert ca.composed_step_from_sums(2, 0, 13, float(n), sums, 1e-3)[0] == ca.ZN_TOO_FEW


def test_order_2_with_a_non_integer_weight_sum_against_the_restatement(oracle, engine_lib):
    worst = 0.0
    for rect, sigma, keep in (((46, 65, 76, 95), 31 / 6, 256), ((100, 30, 130, 60), 31 / 6, 256), ((100, 30, 130, 60), 0.0, 120),
                              ((100, 30, 130, 60), 31 / 6, 120)):
        xy, cx, cy, f, g, gx, gy, dx, dy, bad = second_order_floats(oracle, rect)
        w = wr.sample_weights(xy, cx, cy, wr.inv_of(sigma) if sigma else 0.0, wr.column_mask(keep))
        pro = wr.prologue(xy, cx, cy, w)
        assert (pro["sw"] != round(pro["sw"])) == bool(sigma) and 0 < pro["n_valid"] <= len(xy)
        sums = cr.sums_of(f, g, gx, gy, dx, dy, bad, w)
        for lam in (0.0, 1e-3, 10.0):
            got = ca.composed_step_from_sums(2, ca.FM_UVUXUYVXVY, pro["n_valid"], pro["sw"], sums, lam)
            want = cr.step(pro["n_valid"], pro["sw"], sums, float(np.float32(lam)))
            assert got[0] == want[0] == 0, (rect, sigma, keep, lam, got[0], want[0])
            for a, b in ((got[2], want[2]), (got[3], want[3]), (got[4], want[4])):
                assert abs(a - b) <= REL * abs(b) + (REL if b is want[2] else 0.0), (lam, a, b)
            assert want[1].all()
            root = want[6] / want[1]             # sqrt(diag A): the restatement's scaled unknowns over its delta
            tol = REL * np.abs(want[6]).max()
            err = np.abs(got[1] * root - want[6]).max()
            assert err <= tol, (lam, got[1], want[1], err, tol)
            worst = max(worst, err / tol)
        if sigma:   # with the plain count in place of the weight sum the step is another one
            assert ca.composed_step_from_sums(2, 0, pro["n_valid"], float(pro["n_valid"]), sums, 1e-3)[3] != got[3]
    print(f"order 2: worst error / tolerance {worst:.3g}")


def test_restatements_agree_at_unit_weights(oracle):
    """composed_ref's criterion, step and loop are quadratic_ref's with (n_valid, N) for n: at N = n they give the same numbers"""
    und, dfm = qr.pair()
    xy, cx, cy, f, g, gx, gy, dx, dy, bad = second_order_floats(oracle)
    n, sums = len(xy), qr.sums_of(f, g, gx, gy, dx, dy, bad)
    assert cr.criterion(n, float(n), sums) == qr.criterion(n, sums)
    for lam in (0.0, 1e-3, 10.0):
        a, b = cr.step(n, float(n), sums, lam), qr.step(n, sums, lam)
        assert a[0] == b[0] == 0 and a[2:6] == b[2:6] and a[1].tobytes() == b[1].tobytes() and a[6].tobytes() == b[6].tobytes()
    assert cr.step(13, float(n), sums, 1e-3)[0] == qr.step(13, sums, 1e-3)[0] == ca.ZN_TOO_FEW
    seed = np.zeros(12, np.float32)
    seed[:2] = (1.25, -0.65)
    a = cr.refine(oracle, und, dfm, xy, cx, cy, seed[:6])[0]
    b = qr.loop(qr.sector_evaluator(oracle, ca.IM_BICUBIC, und, dfm, xy, cx, cy), n, seed)
    assert a.keys() == b.keys() and a["status"] == ca.ZN_CONVERGED and a["iterations"] > 0
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (k, a[k], b[k])


def test_refusals_without_a_device(engine_lib):
    lib = engine_lib
    status = C.c_int32(77)
    buf = np.zeros(ca.QD_SUMS)
    delta = np.full(12, 7.0)
    ptr = buf.ctypes.data_as(C.c_void_p)

    def call(order=2, m=ca.FM_UVUXUYVXVY, n=100, N=100.0, sums=ptr, lam=0.0, st=C.byref(status)):
        return lib.lk_composed_step_from_sums(order, m, n, C.c_double(N), sums, C.c_float(lam), delta.ctypes.data_as(C.c_void_p), None, None, st)

    for kw in (dict(order=0), dict(order=3), dict(order=1, m=9), dict(n=-1), dict(N=-1.0), dict(N=np.nan), dict(N=np.inf), dict(sums=None),
               dict(st=None), dict(lam=-1.0), dict(lam=np.nan)):
        assert call(**kw) == ca.ERROR_BAD_DOMAIN, kw
    assert status.value == 77 and (delta == 7.0).all()       # outputs untouched
    assert call() == 0 and status.value == ca.ZN_FLAT and not delta.any()
    assert call(order=1) == 0 and status.value == ca.ZN_FLAT
    assert call(N=0.0) == 0 and status.value == ca.ZN_FLAT   # no weight at all: refused, no NaN escapes
    assert call(m=9) == 0                                    # order 2: the model plays no part
    with pytest.raises(ValueError):
        ca.composed_step_from_sums(3, 0, 10, 10.0, buf, 0.0)
    cfg = _ffi.LkComposedConfig()
    assert lib.lk_refine_composed(None, C.byref(cfg), None, None, None, None, None, None, None) == ca.ERROR_BAD_DOMAIN


# ---- the experiments behind the GPU tests' pinned figures ------------------------------------------------------------------------------
def test_rim_sectors_of_the_restatement(oracle):
    """The side of the rim test and its three figures (composed_ref.RIM_SIDE, RIM): all eight sectors CONVERGED under
    (order 2, mask) at RIM_SIDE, and the masked twelve-parameter mean below the two others."""
    runs = cr.rim_restated(oracle, cr.RIM_SIDE)
    for name, (statuses, err) in runs.items():
        print(f"rim, side {cr.RIM_SIDE}, {name}: largest |(u, v) - truth| = {err.max():.6f} px, mean {err.mean():.6f} px; statuses {statuses}")
    assert all(s == ca.ZN_CONVERGED for s in runs["composed"][0]), runs["composed"][0]
    for name, (statuses, err) in runs.items():
        largest, mean = cr.RIM[name]
        assert abs(err.max() - largest) <= 1e-4 and abs(err.mean() - mean) <= 1e-4, (name, err.max(), err.mean(), cr.RIM[name])
    assert cr.RIM["composed"][1] < cr.RIM["quadratic"][1] and cr.RIM["composed"][1] < cr.RIM["weighted"][1]
    print(f"mean ratios: quadratic / composed {cr.RIM['quadratic'][1] / cr.RIM['composed'][1]:.2f}, "
          f"weighted / composed {cr.RIM['weighted'][1] / cr.RIM['composed'][1]:.2f}")


@pytest.mark.parametrize("shift", cr.CURVE_SHIFTS)
def test_s_curve_of_the_restatement(oracle, shift):
    """composed_ref.CURVE: the mean u error of twelve parameters under the bicubic and under the quintic B-spline"""
    for sampler in (0, 5):
        statuses, bias = cr.curve_restated(oracle, shift, sampler)
        print(f"shift {shift}, sampler {sampler}: mean u - s = {bias.mean():+.6f} px; statuses {np.bincount(statuses, minlength=9)}")
        assert all(s == ca.ZN_CONVERGED for s in statuses)
        assert abs(bias.mean() - cr.CURVE[shift][sampler]) <= 1e-5, (shift, sampler, bias.mean(), cr.CURVE[shift][sampler])
    assert abs(cr.CURVE[shift][5]) < abs(cr.CURVE[shift][0])
