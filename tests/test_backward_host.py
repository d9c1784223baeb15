"""Backward update, host side: lk_compose_inverse (the kernel's own composition W(p) o W(q)^-1, compiled for the host)
against float64 numpy for the four models, and the Python constants against updateEnum (enums.hpp:39)."""
import numpy as np
import pytest

import correlation_amd as ca

P = {ca.FM_U: 1, ca.FM_UV: 2, ca.FM_UVQ: 3, ca.FM_UVUXUYVXVY: 6}


def as_map(model, p):
    """W(p): d -> t + A d, float64"""
    p = np.asarray(p, np.float64)
    t = np.array([p[0], p[1] if model != ca.FM_U else 0.0])
    if model in (ca.FM_U, ca.FM_UV):
        A = np.eye(2)
    elif model == ca.FM_UVQ:
        A = np.array([[1.0, -p[2]], [p[2], 1.0]])
    else:
        A = np.array([[1.0 + p[2], p[3]], [p[4], 1.0 + p[5]]])
    return t, A


def ref_compose(model, p, q):
    tp, Ap = as_map(model, p)
    tq, Aq = as_map(model, q)
    A = Ap @ np.linalg.inv(Aq)
    t = tp - A @ tq
    out = np.zeros(6)
    out[0] = t[0]
    if model == ca.FM_U:
        return out
    out[1] = t[1]
    if model == ca.FM_UVQ:
        out[2] = (A[1, 0] - A[0, 1]) / 2
    elif model == ca.FM_UVUXUYVXVY:
        out[2:6] = [A[0, 0] - 1, A[0, 1], A[1, 0], A[1, 1] - 1]
    return out


def rand_params(rng, model, scale_g=0.02):
    p = np.zeros(6, np.float32)
    p[:2] = rng.uniform(-5, 5, 2)
    if model == ca.FM_UVQ:
        p[2] = rng.uniform(-scale_g, scale_g)
    elif model == ca.FM_UVUXUYVXVY:
        p[2:] = rng.uniform(-scale_g, scale_g, 4)
    if model == ca.FM_U:
        p[1] = 0
    return p


def test_update_constants_match_update_enum():
    # enums.hpp:39: enum updateEnum {update_forward, update_backward}
    assert (ca.UPDATE_FORWARD, ca.UPDATE_BACKWARD) == (0, 1)
    assert "lk_set_update" in ca.SYMBOLS and "lk_evaluate_backward" in ca.SYMBOLS and "lk_compose_inverse" in ca.SYMBOLS


@pytest.mark.parametrize("model", [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY])
def test_compose_inverse_against_float64(model):
    rng = np.random.default_rng(11 + model)
    n = P[model]
    for _ in range(200):
        p, q = rand_params(rng, model), rand_params(rng, model)
        got = ca.compose_inverse(model, p[:n], q[:n])
        want = ref_compose(model, p, q)
        assert got is not None
        assert np.abs(got[:2] - want[:2]).max() < 2e-5, (got, want)
        if n > 2:
            assert np.abs(got[2:n] - want[2:n]).max() < 2e-7, (got, want)
        assert not got[n:].any()


@pytest.mark.parametrize("model", [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY])
def test_compose_identity(model):
    rng = np.random.default_rng(5)
    n = P[model]
    zero = np.zeros(6, np.float32)
    for _ in range(50):
        p = rand_params(rng, model)
        assert np.array_equal(ca.compose_inverse(model, p[:n], zero[:n])[:n], p[:n])   # p o id^-1 = p, bit for bit
        inv = ca.compose_inverse(model, zero[:n], p[:n])                              # id o p^-1
        if model != ca.FM_UVQ:  # p o (id o p^-1)^-1 = p
            back = ca.compose_inverse(model, zero[:n], inv[:n])
            assert np.abs(back[:n] - p[:n]).max() < 1e-5


@pytest.mark.parametrize("model", [ca.FM_U, ca.FM_UV, ca.FM_UVUXUYVXVY])
def test_compose_with_own_inverse_is_zero(model):
    rng = np.random.default_rng(9)
    n = P[model]
    for _ in range(100):
        p = rand_params(rng, model)
        got = ca.compose_inverse(model, p[:n], p[:n])
        assert np.abs(got[:n]).max() < 1e-6, got


def test_uvq_projection_rule():
    # a pure rotation composed with the inverse of another: the skew part of A - I, halved; translation of the composed map
    p = np.array([0.3, -0.2, 0.05], np.float32)
    q = np.array([-0.1, 0.4, -0.03], np.float32)
    got = ca.compose_inverse(ca.FM_UVQ, p, q)
    want = ref_compose(ca.FM_UVQ, np.r_[p, 0, 0, 0], np.r_[q, 0, 0, 0])
    assert np.abs(got[:3] - want[:3]).max() < 1e-6
    # not the sum of the angles: the composed map of two linearised rotations is not one
    assert abs(got[2] - (p[2] - q[2])) > 1e-6


def test_singular_step():
    lib = ca.load_library()
    from correlation_amd import _ffi
    p = np.array([1, 2, 0.01, 0.0, 0.0, 0.02], np.float32)
    for q in ([0, 0, -1, 0, 0, -1], [0, 0, -1, 0, 0, 0], [0, 0, 0, 1, 1, 0]):
        out = np.full(6, 7.0, np.float32)
        qq = np.asarray(q, np.float32)
        assert lib.lk_compose_inverse(ca.FM_UVUXUYVXVY, _ffi.fptr(p), _ffi.fptr(qq), _ffi.fptr(out)) == 1
        assert (out == 7.0).all()  # untouched
    # a NaN step is not singular: it composes to NaN (whose evaluation then fails, as in the forward mode)
    out = np.zeros(6, np.float32)
    qq = np.array([0, 0, np.nan, 0, 0, 0], np.float32)
    assert lib.lk_compose_inverse(ca.FM_UVUXUYVXVY, _ffi.fptr(p), _ffi.fptr(qq), _ffi.fptr(out)) == 0
    assert np.isnan(out).any()
    # |det| just above the bound: a step
    qq = np.array([0, 0, -1 + 2e-6, 0, 0, 0], np.float32)
    out = np.zeros(6, np.float32)
    assert lib.lk_compose_inverse(ca.FM_UVUXUYVXVY, _ffi.fptr(p), _ffi.fptr(qq), _ffi.fptr(out)) == 0
    assert lib.lk_compose_inverse(7, _ffi.fptr(p), _ffi.fptr(qq), _ffi.fptr(out)) == ca.ERROR_BAD_DOMAIN
    # UVQ: det = 1 + q^2 is never singular
    assert ca.compose_inverse(ca.FM_UVQ, [0, 0, 0], [0, 0, 1.0]) is not None
