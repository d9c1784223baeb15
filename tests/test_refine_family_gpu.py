"""The five refinement passes as one family (lk_refine_znssd, _quadratic, _spline, _weighted, _composed): what their shared
host side (csrc/lk_refine.hpp) could break and the tests of each pass do not cross-check.  Every pass keeps the state and the
bench hook of its own slot when the passes alternate on one engine; a call with two faults is refused for the one the order of
the checks puts first; the defaults of a configuration left open are the documented ones for every pass.

A 256 x 256 pair (quadratic_ref's) with nine squares of sides 21 and 31 and the 96 x 96 square between them, so that all
three lane groups take sectors and the sectors of a group are not neighbours in the batch: an order pointer that is off by
one between two groups launches a sector twice and another never."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import quadratic_ref as qr

pytestmark = pytest.mark.gpu

RECTS = qr.RECTS[0:3] + qr.RECTS[25:27] + [qr.RECTS[qr.BIG]] + qr.RECTS[27:29] + qr.RECTS[3:5]   # sides 21, 31, 96, 31, 21
COUNT3 = (5, 4, 1)
S = len(RECTS)

# the pass: its entry point, configuration, info record and sums; whether it takes a mask, second-order seeds, the weights'
# words; the configuration's own words of a good call
PASSES = {
    "znssd": ("lk_refine_znssd", _ffi.LkZnssdConfig, ca.ZNSSD_DTYPE, ca.ZN_SUMS, False, False, False, {}),
    "quadratic": ("lk_refine_quadratic", _ffi.LkQuadraticConfig, ca.QUADRATIC_DTYPE, ca.QD_SUMS, False, True, False, {}),
    "spline": ("lk_refine_spline", _ffi.LkSplineConfig, ca.ZNSSD_DTYPE, ca.ZN_SUMS, False, False, False, {"order": 5}),
    "weighted": ("lk_refine_weighted", _ffi.LkWeightedConfig, ca.WEIGHTED_DTYPE, ca.ZN_SUMS, True, False, True, {}),
    "composed": ("lk_refine_composed", _ffi.LkComposedConfig, ca.COMPOSED_DTYPE, ca.QD_SUMS, True, True, True,
                 {"order": 2, "sampler": 0}),
}


def make_engine(pair, commit=True, rects=RECTS):
    e = ca.HipCorrelationEngine(interpolation=ca.IM_BICUBIC, fitting_model=ca.FM_UVUXUYVXVY, py_start=0, py_stop=2)
    e.set_undeformed_image(pair[0])
    e.set_deformed_image(pair[1])
    for s, r in enumerate(rects):
        e.resetPolygon_rect(s, *r)
    if commit:
        e.commit_sectors()
    return e


@pytest.fixture(scope="module")
def engine():
    with make_engine(qr.pair()) as e:
        yield e


@pytest.fixture(scope="module")
def guesses(engine):
    return qr.true_translation_seeds([engine.sector_info(s)[1:3] for s in range(S)])[0]


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def call(e, name, records=None, guesses=None, outputs=None, reserved=None, **words):
    """lk_refine_<name> through the C ABI -> (return code, message, records, info, sums); outputs: the three arrays to write"""
    fn, cfg_type, info_dtype, n_sums, has_mask, has_second, _, own = PASSES[name]
    fields = dict(def_slot=-1, chi_max=0.0, max_iters=-1, precision=0.0, lambda0=0.0, **own)
    fields.update(words)
    cfg = cfg_type(**fields)
    if reserved is not None:
        cfg.reserved[reserved] = 1
    rec, info, sums = outputs or (np.zeros(S, ca.RESULT_DTYPE), np.zeros(S, info_dtype), np.zeros((S, n_sums)))
    args = [None] * has_mask + [ptr(records), _ffi.fptr(guesses) if guesses is not None else None] + [None] * has_second
    rc = getattr(e.lib, fn)(e._h, C.byref(cfg), *args, ptr(rec), ptr(info), ptr(sums))
    return rc, e.lib.lk_last_error_string(e._h).decode(), rec, info, sums


# ---- 1. the passes alternate on one engine ---------------------------------------------------------------------------------------
def run_all(e, g):
    return {"znssd": e.refine_znssd(guesses=g, return_sums=True),
            "quadratic": e.refine_quadratic(guesses=g, return_sums=True),
            "spline": e.refine_spline(guesses=g, return_sums=True),
            "weighted": e.refine_weighted(guesses=g, sigma=6.0, return_sums=True),
            "composed": e.refine_composed(guesses=g, sampler=3, sigma=6.0, return_sums=True)}


def test_interleaved_passes_keep_their_own_state(engine, guesses):
    e = engine
    n0 = [e.sector_info(s)[0] for s in range(S)]
    assert sorted(n0) == [441] * 5 + [961] * 4 + [9216]        # 16, 64 and 512 lanes (csrc/lk_device.hpp: lk_bw_group)
    first = run_all(e, guesses)
    for name in first:                                         # after all five ran: every hook still reports its own call
        last = getattr(e, name + "_last")()
        assert last[1] == COUNT3 and last[0] > 0, (name, last)
        if name == "spline":
            assert 0 <= last[2] <= last[0], last
    again = run_all(e, guesses)
    for name in first:
        assert [a.tobytes() for a in first[name]] == [a.tobytes() for a in again[name]], name
    # A sector's result does not depend on its place in the batch (the tests of each pass).  With the batch reversed the
    # groups meet their sectors at other places of the order table: every sector was launched, once, by its own group.
    with make_engine(qr.pair(), rects=RECTS[::-1]) as r:
        turned = run_all(r, guesses[::-1])
    for name in first:
        assert [a.tobytes() for a in first[name]] == [a[::-1].tobytes() for a in turned[name]], name


# ---- 2. which refusal wins ------------------------------------------------------------------------------------------------------------
BOTH = "records and guesses are both given (seeds are one or the other)"
PRECISION = "precision and lambda0 must be finite (<= 0: the default)"
SIGMA = "sigma must be finite and >= 0 (0: no window)"
# (faults of the call, the refusal the order of the checks gives); "both": records and guesses; "bare": no committed sectors
TWO_FAULTS = [
    (dict(reserved=0, both=True), "reserved words must be 0"),
    (dict(both=True, chi_max=np.nan), BOTH),
    (dict(precision=np.nan, sigma=-1.0), PRECISION),
    (dict(sigma=-1.0, bare=True), SIGMA),
    (dict(precision=np.nan, bare=True), PRECISION),            # the same place for the passes without weights
]
OWN_WORDS = {
    "spline": (dict(order=4, both=True), "order must be 3 or 5 (0: 5)"),
    "composed": (dict(order=3, both=True), "order must be 1 (the engine's model) or 2 (twelve parameters)"),
}


@pytest.fixture(scope="module")
def bare():
    with make_engine(qr.pair(), commit=False) as e:
        yield e


@pytest.mark.parametrize("name", list(PASSES))
def test_the_first_check_in_order_refuses(engine, bare, guesses, name):
    fn, _, info_dtype, n_sums, _, _, has_weights, _ = PASSES[name]
    cases = [c for c in TWO_FAULTS if has_weights or "sigma" not in c[0]] + ([OWN_WORDS[name]] if name in OWN_WORDS else [])
    seeds = np.zeros(S, ca.RESULT_DTYPE)
    seeds["p"][:] = guesses
    outputs = (np.full(S, 7, np.uint8).repeat(48).view(ca.RESULT_DTYPE),
               np.full(S, 7, np.uint8).repeat(info_dtype.itemsize).view(info_dtype), np.full((S, n_sums), 7.0))
    kept = [a.tobytes() for a in outputs]
    for faults, text in cases:
        faults = dict(faults)
        e = bare if faults.pop("bare", False) else engine
        records = seeds if faults.pop("both", False) else None
        rc, msg, *_ = call(e, name, records=records, guesses=guesses, outputs=outputs, **faults)
        assert (rc, msg) == (ca.ERROR_BAD_DOMAIN, fn + ": " + text), faults
    assert [a.tobytes() for a in outputs] == kept              # every refusal left the outputs as they were


# ---- 3. the defaults of a configuration left open ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PASSES))
def test_open_words_take_the_documented_defaults(engine, guesses, name):
    rc0, msg0, rec0, info0, _ = call(engine, name, guesses=guesses, max_iters=-1, precision=0.0, lambda0=0.0)
    rc1, msg1, rec1, info1, _ = call(engine, name, guesses=guesses, max_iters=50, precision=1e-3, lambda0=1e-3)
    assert (rc0, rc1) == (0, 0), (msg0, msg1)
    assert rec0.tobytes() == rec1.tobytes() and info0.tobytes() == info1.tobytes()
    assert (info0["iterations"] > 0).all()                     # (max_iters was not read as 0: the loop ran)
