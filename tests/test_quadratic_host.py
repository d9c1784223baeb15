"""The second-order refinement without a GPU (include/lk_engine.h: lk_refine_quadratic, lk_quadratic_step_from_sums): the
record's layout and the prototypes, the exported step function against the numpy restatement on sums of real samples -
several dampings, every refusal - its agreement with the six-parameter step where the answer is affine, and the experiment
that the GPU tests take their bounds from, run with the restatement alone: twelve against six parameters on a pair with an
exactly quadratic field.

Step: as test_znssd_host.py - host function and restatement work from the same doubles by the same formulas and differ in
the rounding of a handful of double operations and in the solver (L D L^T against numpy's LU) on a matrix with a unit
diagonal.  The unknowns of that system, delta sqrt(diag A), agree within 1e-12 of their largest; crit, gain, offset within
1e-12 relative (crit, a difference from 1: 1e-12 absolute)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import quadratic_ref as qr
import znssd_ref as zr

REL = 1e-12
SEED = np.float32([1.1, -0.5, 0.001, 0.0005, -0.0005, 0.001, 2e-4, -1e-4, 1e-4, -2e-4, 1e-4, 3e-4])


def test_record_layout_and_prototypes():
    assert ca.QUADRATIC_DTYPE.itemsize == 128 and C.sizeof(_ffi.LkQuadraticConfig) == 32 and ca.QD_SUMS == 88 and ca.QD_PARAMS == 12
    offsets = {k: ca.QUADRATIC_DTYPE.fields[k][1] for k in ca.QUADRATIC_DTYPE.names}
    assert offsets == dict(n_points=0, status=4, iterations=8, evaluations=12, p=16, zncc=64, gain=68, offset=72, znssd=76,
                           zncc_seed=80, shift=84, last_step=92, bend=96, reserved=100, **{"lambda": 88})
    assert [f[0] for f in _ffi.LkQuadraticConfig._fields_] == [f[0] for f in _ffi.LkZnssdConfig._fields_]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_ffi.__file__))), "include", "lk_engine.h")).read()
    for name, n_args in (("lk_refine_quadratic", 8), ("lk_quadratic_step_from_sums", 7)):
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto and len(proto.group(1).split(",")) == n_args, name
        restype, argtypes = _ffi.SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == n_args, name
    assert hasattr(ca.HipCorrelationEngine, "refine_quadratic") and callable(ca.quadratic_step_from_sums)
    # the layout of the sums, and the expansion's table
    assert (qr.W0, qr.T0, qr.TF0, qr.TG0, qr.SPARE, qr.FLAGGED) == (5, 50, 62, 74, 86, 87) and len(qr.MONO) == 15
    assert qr.MONO[:6] == [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2)] and qr.MONO[10] == (4, 0) and qr.MONO[14] == (0, 4)


@pytest.fixture(scope="module")
def pair():
    return qr.pair()


def test_the_pair_is_the_issue_s(pair):
    und, dfm = pair
    assert und.shape == dfm.shape == (256, 256) and und.dtype == np.uint8
    sat = float((dfm == 255).mean())
    print(f"saturated pixels of the deformed image: {100 * sat:.2f} %")
    assert 0.03 < sat < 0.09
    t = qr.truth_at(128.0, 128.0)
    assert np.allclose(t, qr.FIELD, rtol=0, atol=1e-15)
    # the truth about another centre is the same field: w(c + d) from the expansion about c
    c, d = (88.0, 168.0), (7.0, -5.0)
    p = qr.truth_at(*c)
    wx = p[0] + p[2] * d[0] + p[3] * d[1] + 0.5 * p[6] * d[0] ** 2 + p[7] * d[0] * d[1] + 0.5 * p[8] * d[1] ** 2
    assert abs(wx - qr.field_at(c[0] + d[0], c[1] + d[1])[0]) < 1e-12


def real_sums(oracle, pair, rect=(46, 65, 76, 95), p=SEED, interp=ca.IM_BICUBIC):
    und, dfm = pair
    xy = qr.rect_rows(*rect)
    cx, cy = zr.rect_centre(rect)
    fl = qr.sample_floats(oracle, interp, und, dfm, xy, cx, cy, np.float32(p))
    assert not fl[6].any()
    return len(xy), qr.sums_of(*fl), fl


def compare_step(n, sums, lam):
    got = ca.quadratic_step_from_sums(n, sums, lam)
    want = qr.step(n, sums, float(np.float32(lam)))
    assert got[0] == want[0], (lam, got[0], want[0])
    worst = 0.0
    if want[0] in (0, ca.ZN_NEGATIVE, ca.ZN_SINGULAR):
        for g, w, absolute in ((got[2], want[2], REL), (got[3], want[3], 0.0), (got[4], want[4], 0.0)):
            tol = REL * abs(w) + absolute
            assert abs(g - w) <= tol, (lam, g, w)
            worst = max(worst, abs(g - w) / tol)
    else:
        assert got[2] == got[3] == got[4] == 0.0
    if want[0] == 0:
        A, _ = qr.normal_equations(n, sums, want[3])
        scaled = got[1] * np.sqrt(np.diag(A))
        tol = REL * np.abs(want[6]).max()
        err = np.abs(scaled - want[6]).max()
        assert err <= tol, (lam, got[1], want[1], err, tol)
        worst = max(worst, err / tol)
    else:
        assert not got[1].any()
    return worst


def test_expansion_is_the_generic_layout(oracle, pair):
    """SH, SHH, SHf, SHg expanded from the 88 sums are the sums of the twelve H themselves"""
    n, sums, (f, g, gx, gy, dx, dy, bad) = real_sums(oracle, pair)
    f, g, gx, gy, X, Y = (a.astype(np.float64) for a in (f, g, gx, gy, dx, dy))
    H = np.stack([gx, gy, gx * X, gx * Y, gy * X, gy * Y, 0.5 * gx * X * X, gx * X * Y, 0.5 * gx * Y * Y, 0.5 * gy * X * X,
                  gy * X * Y, 0.5 * gy * Y * Y], 1)
    SH, SHH, SHf, SHg = qr.expand(sums)
    for got, want in ((SH, H.sum(axis=0)), (SHH, H.T @ H), (SHf, H.T @ f), (SHg, H.T @ g)):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_step_against_the_restatement(oracle, pair):
    worst = 0.0
    for rect, p in (((46, 65, 76, 95), SEED), ((100, 30, 123, 53), np.float32([1.6, -0.9] + [0.0] * 10)),
                    ((8, 160, 20, 170), np.float32([0.7, 0.1, 0.004, 0.0, 0.0, -0.003] + [0.0] * 6))):
        n, sums, _ = real_sums(oracle, pair, rect, p)
        for lam in (0.0, 1e-9, 1e-3, 0.1, 10.0, 1e6):
            worst = max(worst, compare_step(n, sums, lam))
        status, delta, crit, gain, offset = ca.quadratic_step_from_sums(n, sums, 1e-3)
        assert status == 0 and 0.0 < crit < 1.0 and gain > 0.0 and np.isfinite(delta).all()   # (seeds a pixel or two off)
    print(f"worst error / tolerance {worst:.3g}")


def test_step_refusals(oracle, pair):
    und, dfm = pair
    n, sums, (f, g, gx, gy, dx, dy, bad) = real_sums(oracle, pair)
    assert ca.quadratic_step_from_sums(n, sums, 1e-3)[0] == 0
    # TOO_FEW: n < 14
    assert ca.quadratic_step_from_sums(13, sums, 1e-3)[0] == ca.ZN_TOO_FEW == qr.step(13, sums, 1e-3)[0]
    assert ca.quadratic_step_from_sums(14, sums, 1e-3)[0] != ca.ZN_TOO_FEW
    # FLAT: a constant f, a constant g
    for ff, gg in ((np.full_like(f, 128.0), g), (f, np.full_like(g, 77.0))):
        s = qr.sums_of(ff, gg, gx, gy, dx, dy, bad)
        assert compare_step(n, s, 1e-3) == 0.0 and ca.quadratic_step_from_sums(n, s, 1e-3)[0] == ca.ZN_FLAT
    # NEGATIVE: the inverted deformed patch; criterion, gain and offset are still reported
    s = qr.sums_of(f, np.float32(255.0) - g, -gx, -gy, dx, dy, bad)
    got = ca.quadratic_step_from_sums(n, s, 1e-3)
    assert got[0] == ca.ZN_NEGATIVE and got[3] < 0.0 and not got[1].any()
    compare_step(n, s, 1e-3)
    # SINGULAR: no texture along x - g_x = 0 in every sample, so A_00 = 0
    s = qr.sums_of(f, g, np.zeros_like(gx), gy, dx, dy, bad)
    for lam in (0.0, 1e-3, 100.0):
        assert ca.quadratic_step_from_sums(n, s, lam)[0] == ca.ZN_SINGULAR
        compare_step(n, s, lam)
    # samples on one row: Y = 0, so the columns of uy, uxy, uyy vanish
    row = np.abs(dy) == np.abs(dy).min()
    assert row.sum() >= 14
    s = qr.sums_of(f[row], g[row], gx[row], gy[row], dx[row], np.zeros_like(dy[row]), bad[row])
    assert ca.quadratic_step_from_sums(int(row.sum()), s, 1e-3)[0] == ca.ZN_SINGULAR == qr.step(int(row.sum()), s, 1e-3)[0]
    # arguments
    lib = _ffi.load_library()
    status = C.c_int32(77)
    buf = np.zeros(ca.QD_SUMS)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert lib.lk_quadratic_step_from_sums(-1, ptr, 0.0, None, None, None, C.byref(status)) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_quadratic_step_from_sums(100, None, 0.0, None, None, None, C.byref(status)) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_quadratic_step_from_sums(100, ptr, 0.0, None, None, None, None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_quadratic_step_from_sums(100, ptr, -1.0, None, None, None, C.byref(status)) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_quadratic_step_from_sums(100, ptr, float("nan"), None, None, None, C.byref(status)) == ca.ERROR_BAD_DOMAIN
    assert status.value == 77
    assert lib.lk_quadratic_step_from_sums(100, ptr, 0.0, None, None, None, C.byref(status)) == 0 and status.value == ca.ZN_FLAT


def test_an_affine_answer_is_the_six_parameter_step(oracle, pair):
    """Sums built from an affine-only H: f = g + sum_k c_k H_k over the six first-order H alone, with c chosen so that the
    perturbation does not correlate with g (the eliminated gain stays 1).  The Gauss-Newton step of both models is then c:
    the first six components of the twelve-parameter step equal lk_znssd_step_from_sums on the six-parameter sums of the
    same samples, and the six second-order rows are solved (no SINGULAR) to zero.  Both solves are exact up to rounding;
    the difference is bounded by 1e-12 of the largest scaled unknown, as compare_step bounds a solver."""
    _, _, (f32, g32, gx, gy, dx, dy, bad) = real_sums(oracle, pair)
    g, gx, gy, X, Y = (a.astype(np.float64) for a in (g32, gx, gy, dx, dy))
    n = len(g)
    H = np.stack([gx, gy, gx * X, gx * Y, gy * X, gy * Y], 1)
    Hc, gc = H - H.mean(axis=0), g - g.mean()
    rng = np.random.default_rng(24)
    c = rng.normal(size=6) * np.array([0.3, 0.3, 0.01, 0.01, 0.01, 0.01])
    k = Hc.T @ gc
    c = c - k * (k @ c) / (k @ k)                 # sum (H c)~ g~ = 0
    f = g + H @ c
    s88 = qr.sums_from_H(f, g, gx, gy, X, Y)
    s45 = np.zeros(ca.ZN_SUMS)
    iu = np.triu_indices(6)
    s45[:44] = np.concatenate([[f.sum(), g.sum(), (f * f).sum(), (g * g).sum(), (f * g).sum()], H.sum(axis=0), (H.T @ H)[iu], H.T @ f, H.T @ g])
    worst = 0.0
    for lam in (0.0, 1e-9):
        st6, d6, crit6, gain6, _ = ca.znssd_step_from_sums(ca.FM_UVUXUYVXVY, n, s45, lam)
        st12, d12, crit12, gain12, _ = ca.quadratic_step_from_sums(n, s88, lam)
        assert st6 == 0 and st12 == 0, (st6, st12)
        if lam == 0.0:
            A6 = zr.normal_equations(ca.FM_UVUXUYVXVY, n, s45, gain6)[0]
            A12 = qr.normal_equations(n, s88, gain12)[0]
            r6, r12 = np.sqrt(np.diag(A6)), np.sqrt(np.diag(A12))
            scale = np.abs(d6[:6] * r6).max()
            err = max(np.abs((d12[:6] - d6[:6]) * r6).max(), np.abs(d12[6:] * r12[6:]).max())
            worst = max(worst, err / (REL * scale))
            assert err <= REL * scale, (d12, d6, err, scale)
            assert np.abs(d6[:6] - c).max() <= 1e-9 * np.abs(c).max()      # (and both are the constructed answer)
        assert abs(gain12 - gain6) <= REL and abs(crit12 - crit6) <= REL
    print(f"affine answer: worst error / tolerance {worst:.3g}")


# ---- the experiment: twelve against six parameters on the quadratic field ---------------------------------------------------
@pytest.fixture(scope="module")
def refined(oracle, pair):
    """the restatement's loops over the test geometry from the zero-gradient seed at the true translation"""
    und, dfm = pair
    lists, centres = qr.sector_lists(oracle)
    seeds, truth = qr.true_translation_seeds(centres)
    quad, affine = [], []
    for s, (xy, (cx, cy)) in enumerate(zip(lists, centres)):
        p12 = np.zeros(12, np.float32)
        p12[:6] = seeds[s]
        quad.append(qr.loop(qr.sector_evaluator(oracle, ca.IM_BICUBIC, und, dfm, xy, cx, cy), len(xy), p12))
        affine.append(zr.loop(qr.affine_evaluator(oracle, ca.IM_BICUBIC, und, dfm, xy, cx, cy), ca.FM_UVUXUYVXVY, len(xy), seeds[s]))
    return dict(truth=truth, quad=quad, affine=affine)


def test_accuracy_of_the_restatement(refined):
    """ACCURACY_Q, SECOND_Q and AFFINE_BIAS of quadratic_ref.py, and the claim: at side 31 the twelve-parameter model's
    largest error is at most a quarter of the six-parameter model's mean error"""
    truth = refined["truth"]
    for side in qr.SIDES:
        idx = [s for s in range(qr.BIG) if qr.SIDE_OF[s] == side]
        assert len(idx) == 25
        eq, e2, ea = [], [], []
        for s in idx:
            q, a = refined["quad"][s], refined["affine"][s]
            assert q["status"] == ca.ZN_CONVERGED and a["status"] == ca.ZN_CONVERGED, (s, q["status"], a["status"])
            eq.append(np.abs(q["p"][:2].astype(np.float64) - truth[s][:2]).max())
            e2.append(np.abs(q["p"][6:].astype(np.float64) - truth[s][6:]).max())
            ea.append(np.abs(a["p"][:2].astype(np.float64) - truth[s][:2]).max())
        ev = [refined["quad"][s]["evaluations"] for s in idx]
        print(f"side {side}: twelve parameters max / mean {max(eq):.6f} / {np.mean(eq):.6f} px, second-order max {max(e2):.3g}, "
              f"evaluations {min(ev)}..{max(ev)}; six parameters max / mean {max(ea):.6f} / {np.mean(ea):.6f} px")
        for name, table, value in (("ACCURACY_Q", qr.ACCURACY_Q, max(eq)), ("SECOND_Q", qr.SECOND_Q, max(e2)),
                                   ("AFFINE_BIAS", qr.AFFINE_BIAS, float(np.mean(ea)))):
            assert value <= table[side], (name, side, value, table[side])
            assert value >= 0.5 * table[side], f"{name}[{side}] is no longer the measured figure"
    for name, s, pinned in (("ACCURACY_BIG", qr.BIG, qr.ACCURACY_BIG), ("ACCURACY_RING", qr.RING, qr.ACCURACY_RING)):
        q = refined["quad"][s]
        value = np.abs(q["p"][:2].astype(np.float64) - truth[s][:2]).max()
        print(f"{name}: {value:.6f} px, {len(q['sums'])} sums, evaluations {q['evaluations']}")
        assert q["status"] == ca.ZN_CONVERGED and 0.5 * pinned <= value <= pinned, (name, value, pinned)
    assert qr.ACCURACY_Q[31] <= qr.AFFINE_BIAS[31] / 4.0, "the pair does not show the claim"
