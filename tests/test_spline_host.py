"""The host side of the B-spline refinement (include/lk_engine.h: lk_spline_weights, lk_spline_config, the prototypes): the
kernel's weight function against the restatement bit for bit, the partition of unity, the derivative weights against a
central difference of the exact pieces, the node values, the struct layout and the refusals that need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import spline_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRACTIONS = [0.0, 2.0 ** -20, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -24]
ORDERS = [3, 5]


@pytest.mark.parametrize("order", ORDERS)
def test_weights_are_the_restatements_bits(engine_lib, order):
    for t in FRACTIONS:
        w, g = ca.spline_weights(order, t)
        rw, rg = sr.weights32(order, t)
        assert w.dtype == np.float32 and len(w) == order + 1 == len(g)
        assert w.tobytes() == rw.tobytes(), (order, t, w, rw)
        assert g.tobytes() == rg.tobytes(), (order, t, g, rg)


@pytest.mark.parametrize("order", ORDERS)
def test_weights_sum_to_one_and_derivative_weights_to_zero(engine_lib, order):
    for t in FRACTIONS + list(np.random.default_rng(3).uniform(0, 1, 50)):
        w, g = ca.spline_weights(order, t)
        assert abs(w.astype(np.float64).sum() - 1.0) <= 4 * 2.0 ** -24, (order, t, w)
        assert abs(g.astype(np.float64).sum()) <= 4 * 2.0 ** -24, (order, t, g)


@pytest.mark.parametrize("order", ORDERS)
def test_derivative_weights_against_a_central_difference(engine_lib, order):
    h = 1e-5
    for t in (0.1, 0.25, 0.5, 0.75, 0.9):
        t32 = float(np.float32(t))
        _, g = ca.spline_weights(order, t32)
        hi, lo = sr.weights64(order, t32 + h)[0], sr.weights64(order, t32 - h)[0]
        assert np.abs(g - (hi - lo) / (2 * h)).max() <= 1e-6, (order, t, g, (hi - lo) / (2 * h))


def test_node_values(engine_lib):
    w, g = ca.spline_weights(5, 0.0)
    assert w.tobytes() == np.float32([1 / 120, 26 / 120, 66 / 120, 26 / 120, 1 / 120, 0]).tobytes(), w
    assert g.tobytes() == np.float32([-1 / 24, -10 / 24, 0, 10 / 24, 1 / 24, 0]).tobytes(), g
    w, g = ca.spline_weights(3, 0.0)
    assert w.tobytes() == np.float32([1 / 6, 4 / 6, 1 / 6, 0]).tobytes(), w
    assert g.tobytes() == np.float32([-0.5, 0, 0.5, 0]).tobytes(), g
    # the pieces of the restatement are the B-spline: its values at the nodes
    assert [row[0] for row in sr.pieces(5)] == [sr.F(k, 120) for k in (1, 26, 66, 26, 1, 0)]
    assert sum(sum(row) for row in sr.pieces(5)) == 1 and sum(sum(row) for row in sr.pieces(3)) == 1


def test_zeros_behind_the_order_and_refusals(engine_lib):
    lib = engine_lib
    w, g = np.full(6, 7, np.float32), np.full(6, 7, np.float32)
    assert lib.lk_spline_weights(3, 0.3, _ffi.fptr(w), _ffi.fptr(g)) == 0
    assert not w[4:].any() and not g[4:].any() and w[:4].all()
    kept = w.tobytes()
    assert lib.lk_spline_weights(4, 0.3, _ffi.fptr(w), _ffi.fptr(g)) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_spline_weights(5, 0.3, None, _ffi.fptr(g)) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_spline_weights(5, 0.3, _ffi.fptr(w), None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_spline_weights(5, float("nan"), _ffi.fptr(w), _ffi.fptr(g)) == ca.ERROR_BAD_DOMAIN
    assert w.tobytes() == kept
    with pytest.raises(ValueError):
        ca.spline_weights(4, 0.5)
    # order 0 is the quintic, as in the configuration
    assert lib.lk_spline_weights(0, 0.3, _ffi.fptr(w), _ffi.fptr(g)) == 0
    assert w.tobytes() == ca.spline_weights(5, 0.3)[0].tobytes()
    # the entry points that take an engine refuse a null one
    cfg = _ffi.LkSplineConfig()
    assert lib.lk_refine_spline(None, C.byref(cfg), None, None, None, None, None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_spline_coefficients(None, 0, 5, None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_spline_sample(None, 0, 5, None, 0, None) == ca.ERROR_BAD_DOMAIN


def test_struct_layout_is_the_headers():
    text = open(os.path.join(ROOT, "include", "lk_engine.h")).read()
    body = re.search(r"typedef struct lk_spline_config \{(.*?)\} lk_spline_config;", text, re.S).group(1)
    fields = re.findall(r"^\s*(int|float)\s+(\w+)(?:\[(\d+)\])?;", body, re.M)
    assert [(t, n, k) for t, n, k in fields] == [("int", "def_slot", ""), ("float", "chi_max", ""), ("int", "max_iters", ""),
                                                 ("float", "precision", ""), ("float", "lambda0", ""), ("int", "order", ""),
                                                 ("int", "reserved", "2")]
    S = _ffi.LkSplineConfig
    assert C.sizeof(S) == 32
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("def_slot", 0), ("chi_max", 4), ("max_iters", 8), ("precision", 12),
                                                                  ("lambda0", 16), ("order", 20), ("reserved", 24)]
    for name in ("lk_refine_spline", "lk_spline_coefficients", "lk_spline_sample", "lk_spline_weights"):
        assert re.search(r"^int %s\(" % name, text, re.M), name


def test_the_float32_recipe_tracks_the_float64_one():
    """the restatements against each other, and the spline of the coefficients against the pixels"""
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (33, 29)).astype(np.uint8)
    for order in ORDERS:
        c32, c64 = sr.prefilter(img, order), sr.prefilter(img, order, np.float64)
        assert c32.dtype == np.float32 and np.abs(c32 - c64).max() <= 2e-3
        # re-convolving with the B-spline returns the pixels: the node values are the weights at t = 0
        w = np.array([float(r[0]) for r in sr.pieces(order)][:order])   # (the last weight is 0)
        L = order // 2
        back = sum(w[j] * w[i] * c64[j:33 - 2 * L + j, i:29 - 2 * L + i] for j in range(order) for i in range(order))
        inner = img[L:33 - L, L:29 - L].astype(np.float64)
        assert np.abs(back - inner)[4:-4, 4:-4].max() <= 1e-6, np.abs(back - inner)[4:-4, 4:-4].max()
