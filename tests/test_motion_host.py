"""Global motion per frame, the host side (include/lk_engine.h: lk_motion_from_sums, lk_motion_apply, lk_motion_remove): the
kernel's own fit and removal compiled for the host, against the float64 restatement of tests/motion_ref.py; an exact rigid
motion recovered and taken out; every status; every refusal.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi
from motion_ref import FLOATS, fit_from_sums, remove_reference, sums_of_points

KINDS = [ca.MOTION_TRANSLATION, ca.MOTION_RIGID, ca.MOTION_SIMILARITY, ca.MOTION_AFFINE]
P = C.c_void_p


def lattice(n=12, pitch=19.0, first=17.0):
    g = first + pitch * np.arange(n)
    return np.float32([(x, y) for x in g for y in g])


def test_layout_and_symbols(engine_lib):
    assert ca.MOTION_DTYPE.itemsize == 64 and C.sizeof(_ffi.LkMotionConfig) == 32
    assert [ca.MOTION_DTYPE.fields[k][1] for k in ("cx", "tx", "axx", "theta", "rms", "n_fit", "status", "passes_run")] == \
        [0, 8, 16, 32, 40, 48, 56, 60]
    for name in ("lk_rigid_motion", "lk_motion_from_sums", "lk_motion_apply", "lk_motion_remove"):
        assert hasattr(engine_lib, name) and name in _ffi.SYMBOLS
    assert hasattr(engine_lib, "lk_internal_motion_last")
    assert (ca.MOTION_TRANSLATION, ca.MOTION_RIGID, ca.MOTION_SIMILARITY, ca.MOTION_AFFINE) == (0, 1, 2, 3)
    assert (ca.MOTION_OK, ca.MOTION_TOO_FEW, ca.MOTION_DEGENERATE) == (0, 1, 2)


@pytest.mark.parametrize("kind", KINDS)
def test_from_sums_matches_the_restatement(engine_lib, kind):
    rng = np.random.default_rng(10 + kind)
    cen = lattice().astype(np.float64)
    o = np.float64([121.5, 121.5])
    for trial in range(20):
        pick = rng.random(len(cen)) < rng.uniform(0.2, 1.0)
        pick[:3] = True
        x, y = (cen[pick] - o).T
        G = rng.uniform(-0.3, 0.3, (2, 2))
        uv = rng.uniform(-20, 20, 2) + (cen[pick] - o) @ G.T + rng.normal(0, 0.05, (pick.sum(), 2))
        uv = np.float32(uv).astype(np.float64)
        n, s = sums_of_points(x, y, uv[:, 0], uv[:, 1])
        got = ca.motion_from_sums(kind, n, s, o)
        status, c, t, A = fit_from_sums(kind, ca.MOTION_MIN_SECTORS[kind], n, s)
        assert status == ca.MOTION_OK == got["status"] and got["n_fit"] == n
        assert not got["rms"] and not got["max_residual"] and not got["n_rejected"] and not got["passes_run"]
        want = dict(cx=o[0] + c[0], cy=o[1] + c[1], tx=t[0], ty=t[1], axx=A[0, 0], axy=A[0, 1], ayx=A[1, 0], ayy=A[1, 1],
                    theta=np.arctan2(A[1, 0] - A[0, 1], A[0, 0] + A[1, 1]), scale=np.sqrt(abs(np.linalg.det(A))))
        # the same formulas in the same order: a few roundings of double apart, then one rounding to float
        for k, w in want.items():
            assert abs(float(got[k]) - w) <= 2.0 ** -23 * abs(w) + 1e-12, (trial, k, float(got[k]), w)
        if kind == ca.MOTION_TRANSLATION:
            assert (got["axx"], got["axy"], got["ayx"], got["ayy"], got["theta"], got["scale"]) == (1, 0, 0, 1, 0, 1)
        if kind == ca.MOTION_RIGID:
            assert abs(float(got["scale"]) - 1) <= 2.0 ** -22
        # the motion at its own centroid is t
        at_c = ca.motion_apply(got, [[got["cx"], got["cy"]]])
        assert at_c.dtype == np.float32 and at_c.tobytes() == np.float32([[got["tx"], got["ty"]]]).tobytes()


@pytest.mark.parametrize("model", [ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY])
def test_an_exact_rigid_motion_is_recovered_and_removed(engine_lib, model):
    th, t = np.deg2rad(30.0), np.float64([12.5, -7.25])
    Rm = np.float64([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    cen = lattice()
    X = cen.astype(np.float64)
    pivot = np.float64([100.0, 140.0])
    rec = np.zeros(len(cen), ca.RESULT_DTYPE)
    rec["p"][:, :2] = (X - pivot) @ Rm.T + pivot + t - X
    if model == ca.FM_UVQ:
        rec["p"][:, 2] = np.tan(th)          # F = [[1, -q], [q, 1]] is R / cos(theta) for q = tan(theta): no q is left
    elif model == ca.FM_UVUXUYVXVY:
        rec["p"][:, 2:6] = (Rm - np.eye(2)).ravel()
    rec["chi"], rec["n_points"], rec["iterations"], rec["und_cx"], rec["und_cy"] = 0.5, 361, 7, cen[:, 0], cen[:, 1]
    o = np.float64([121.5, 121.5])
    u, v = rec["p"][:, 0].astype(np.float64), rec["p"][:, 1].astype(np.float64)
    n, s = sums_of_points(X[:, 0] - o[0], X[:, 1] - o[1], u, v)
    m = ca.motion_from_sums(ca.MOTION_RIGID, n, s, o)
    Umax, Rmax = np.abs(rec["p"][:, :2]).max(), np.abs(X - o).max()
    # the inputs are floats: u and v carry 2^-24 Umax each, which the fit averages but does not remove
    tol_t, tol_A = 2.0 ** -23 * Umax, 2.0 ** -23 * Umax / Rmax + 2.0 ** -23
    assert m["status"] == ca.MOTION_OK and m["n_fit"] == 144
    assert abs(float(m["theta"]) - th) <= tol_A and abs(float(m["scale"]) - 1) <= tol_A
    assert np.abs(np.float64([[m["axx"], m["axy"]], [m["ayx"], m["ayy"]]]) - Rm).max() <= tol_A
    c = X.mean(axis=0)
    assert np.abs(np.float64([m["cx"], m["cy"]]) - c).max() <= 2.0 ** -23 * 256
    assert np.abs(np.float64([m["tx"], m["ty"]]) - ((c - pivot) @ Rm.T + pivot + t - c)).max() <= tol_t + 2.0 ** -23 * Umax
    # taken out again: displacements and gradients that are zero up to the float rounding of the inputs and of the motion
    out = ca.motion_remove(model, m, cen, rec)
    tol_u = 2.0 ** -23 * (Umax + 256 + Umax + 2 * Rmax) + 2 * Rmax * tol_A
    print(f"model {model}: largest |u''| {np.abs(out['p'][:, :2]).max():.3g} of {tol_u:.3g}, "
          f"largest |gradient''| {np.abs(out['p'][:, 2:]).max():.3g} of {4 * tol_A:.3g}")
    assert np.abs(out["p"][:, :2]).max() <= tol_u
    assert np.abs(out["p"][:, 2:]).max() <= 4 * tol_A
    for k in ("chi", "n_points", "iterations", "error_code", "und_cx", "und_cy"):
        assert out[k].tobytes() == rec[k].tobytes()
    # ... and it is the restatement's removal, each output rounded to float once
    want = remove_reference(model, m, cen, rec, np.ones(len(cen), bool))
    assert np.abs(out["p"].astype(np.float64) - want).max() <= 2.0 ** -23 * np.abs(want).max() + 1e-6 * 2.0 ** -20
    # good = ...: the others are copied; a motion that is not OK copies everything
    some = np.arange(len(cen)) % 3 == 0
    part = ca.motion_remove(model, m, cen, rec, good=some)
    assert part[some].tobytes() == out[some].tobytes() and part[~some].tobytes() == rec[~some].tobytes()
    dead = m.copy()
    dead["status"] = ca.MOTION_TOO_FEW
    assert ca.motion_remove(model, dead, cen, rec).tobytes() == rec.tobytes()
    assert not ca.motion_apply(dead, cen).any()


def test_translation_of_a_one_parameter_model(engine_lib):
    cen = lattice(4)
    rec = np.zeros(len(cen), ca.RESULT_DTYPE)
    rec["p"][:, 0] = 3.25 + 0.001 * np.arange(len(cen))
    rec["p"][:, 1:] = 77.0                      # not parameters of FM_U: never read, never written
    n, s = sums_of_points(cen[:, 0], cen[:, 1], rec["p"][:, 0], np.zeros(len(cen)))
    m = ca.motion_from_sums(ca.MOTION_TRANSLATION, n, s, [0.0, 0.0])
    out = ca.motion_remove(ca.FM_U, m, cen, rec)
    assert np.allclose(out["p"][:, 0], rec["p"][:, 0] - m["tx"], atol=2.0 ** -20) and (out["p"][:, 1:] == 77.0).all()
    rot = ca.motion_from_sums(ca.MOTION_RIGID, n, sums_of_points(cen[:, 0], cen[:, 1], -0.1 * cen[:, 1], 0.1 * cen[:, 0])[1], [0.0, 0.0])
    assert rot["status"] == ca.MOTION_OK
    with pytest.raises(ValueError):
        ca.motion_remove(ca.FM_U, rot, cen, rec)


def test_every_status_is_reached(engine_lib):
    o = [0.0, 0.0]
    line = sums_of_points([0, 1, 2, 3], [0, 0, 0, 0], [1, 1, 1, 1], [0, 0.1, 0.2, 0.3])
    point = sums_of_points([5, 5, 5], [7, 7, 7], [1, 2, 3], [0, 0, 0])
    spread = sums_of_points([0, 1, 0, 1], [0, 0, 1, 1], [1, 1, 1, 1], [2, 2, 2, 2])
    fold = sums_of_points([0, 1, 0, 1], [0, 0, 1, 1], [0, -1, 0, -1], [0, 0, 0, 0])     # u = -x: A = diag(0, 1)
    opposite = sums_of_points([-1, 1], [0, 0], [2, -2], [0, 0])                          # x' = -x ... and then h > 0
    for kind in KINDS:
        assert ca.motion_from_sums(kind, *spread, o)["status"] == ca.MOTION_OK
        few = ca.motion_from_sums(kind, 2, spread[1], o, min_sectors=3)
        assert few["status"] == ca.MOTION_TOO_FEW and few["n_fit"] == 2
        assert not any(few[k] for k in FLOATS)
        assert ca.motion_from_sums(kind, 0, np.zeros(11), o)["status"] == ca.MOTION_TOO_FEW
    assert ca.motion_from_sums(ca.MOTION_TRANSLATION, *point, o)["status"] == ca.MOTION_OK
    for kind in (ca.MOTION_RIGID, ca.MOTION_SIMILARITY, ca.MOTION_AFFINE):
        got = ca.motion_from_sums(kind, *point, o)
        assert got["status"] == ca.MOTION_DEGENERATE and not any(got[k] for k in FLOATS) and got["n_fit"] == 3
    # centres on a line carry a rotation but no plane
    assert ca.motion_from_sums(ca.MOTION_RIGID, *line, o)["status"] == ca.MOTION_OK
    assert ca.motion_from_sums(ca.MOTION_AFFINE, *line, o)["status"] == ca.MOTION_DEGENERATE
    assert ca.motion_from_sums(ca.MOTION_AFFINE, *fold, o)["status"] == ca.MOTION_DEGENERATE
    # h == 0: the scatter x' = 0 x has neither a direction nor a size (u = -x, v = -y)
    collapse = sums_of_points([0, 1, 0, 1], [0, 0, 1, 1], [0, -1, 0, -1], [0, 0, -1, -1])
    assert ca.motion_from_sums(ca.MOTION_RIGID, *collapse, o)["status"] == ca.MOTION_DEGENERATE
    assert ca.motion_from_sums(ca.MOTION_SIMILARITY, *collapse, o)["status"] == ca.MOTION_DEGENERATE
    half_turn = ca.motion_from_sums(ca.MOTION_RIGID, *opposite, o)
    assert half_turn["status"] == ca.MOTION_OK and half_turn["axx"] == -1 and abs(abs(float(half_turn["theta"])) - np.pi) < 1e-6


def test_every_refusal_of_the_host_functions(engine_lib):
    L = engine_lib
    s, o = np.zeros(11), np.zeros(2)
    out = np.full(1, 7, ca.MOTION_DTYPE)
    kept = out.tobytes()

    def from_sums(kind=1, min_sectors=2, n=4, sums=s, origin=o, output=out):
        return L.lk_motion_from_sums(kind, min_sectors, n, sums.ctypes.data_as(P) if sums is not None else None,
                                     origin.ctypes.data_as(P) if origin is not None else None,
                                     output.ctypes.data_as(P) if output is not None else None)

    assert from_sums() == 0
    out[:] = np.full(1, 7, ca.MOTION_DTYPE)
    for bad in (dict(kind=-1), dict(kind=4), dict(n=-1), dict(sums=None), dict(origin=None), dict(output=None),
                dict(kind=0, min_sectors=0), dict(kind=1, min_sectors=1), dict(kind=2, min_sectors=1), dict(kind=3, min_sectors=2)):
        assert from_sums(**bad) == ca.ERROR_BAD_DOMAIN, bad
        assert out.tobytes() == kept
    with pytest.raises(ValueError):
        ca.motion_from_sums(7, 4, s, o)
    # lk_motion_apply
    m = np.zeros(1, ca.MOTION_DTYPE)
    m["axx"] = m["ayy"] = 1
    xy, uv = np.zeros((2, 2), np.float32), np.full((2, 2), 7, np.float32)
    assert L.lk_motion_apply(m.ctypes.data_as(P), 2, _ffi.fptr(xy), _ffi.fptr(uv)) == 0 and not uv.any()
    uv[:] = 7
    for args in ((None, 2, _ffi.fptr(xy), _ffi.fptr(uv)), (m.ctypes.data_as(P), 0, _ffi.fptr(xy), _ffi.fptr(uv)),
                 (m.ctypes.data_as(P), -1, _ffi.fptr(xy), _ffi.fptr(uv)), (m.ctypes.data_as(P), 2, None, _ffi.fptr(uv)),
                 (m.ctypes.data_as(P), 2, _ffi.fptr(xy), None)):
        assert L.lk_motion_apply(*args) == ca.ERROR_BAD_DOMAIN
        assert (uv == 7).all()
    # lk_motion_remove
    rec, res = np.zeros(1, ca.RESULT_DTYPE), np.full(1, 7, ca.RESULT_DTYPE)
    kept = res.tobytes()

    def remove(model=ca.FM_UV, motion=m, a=rec, b=res):
        return L.lk_motion_remove(model, motion.ctypes.data_as(P) if motion is not None else None, 1.0, 2.0,
                                  a.ctypes.data_as(P) if a is not None else None, b.ctypes.data_as(P) if b is not None else None)

    assert remove() == 0 and res.tobytes() == rec.tobytes()
    res[:] = np.full(1, 7, ca.RESULT_DTYPE)
    singular, turned = m.copy(), m.copy()
    singular["ayy"] = 0
    turned["axy"], turned["ayx"] = -0.1, 0.1
    for bad in (dict(model=-1), dict(model=4), dict(motion=None), dict(a=None), dict(b=None), dict(motion=singular),
                dict(model=ca.FM_U, motion=turned)):
        assert remove(**bad) == ca.ERROR_BAD_DOMAIN, bad
        assert res.tobytes() == kept
    assert remove(model=ca.FM_U) == 0
