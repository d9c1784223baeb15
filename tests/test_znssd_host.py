"""The ZNSSD refinement without a GPU (include/lk_engine.h: lk_refine_znssd, lk_znssd_step_from_sums): the record's layout
and the prototypes, the exported step function against the numpy restatement on sums of real samples - every model, several
dampings, every refusal - and the two experiments that the GPU tests take their bounds from, run with the restatement
alone: the lighting identity (D against D' = D / 2 + 32) and the accuracy against the analytic map.

Step: the host function and the restatement work from the same doubles by the same formulas; they differ in the rounding
of a handful of double operations and in the solver (L D L^T against numpy's LU) on a matrix with a unit diagonal.  The
unknowns of that system, delta sqrt(diag A), agree within 1e-12 of their largest; crit, gain, offset within 1e-12
relative (crit, a difference from 1: 1e-12 absolute)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi

import znssd_ref as zr

MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
REL = 1e-12


def test_record_layout_and_prototypes():
    assert ca.ZNSSD_DTYPE.itemsize == 64 and C.sizeof(_ffi.LkZnssdConfig) == 32 and ca.ZN_SUMS == 45
    offsets = {k: ca.ZNSSD_DTYPE.fields[k][1] for k in ca.ZNSSD_DTYPE.names}
    assert offsets == dict(n_points=0, status=4, iterations=8, evaluations=12, zncc=16, gain=20, offset=24, znssd=28,
                           zncc_seed=32, shift=36, last_step=44, reserved=48, **{"lambda": 40})
    assert [f[0] for f in _ffi.LkZnssdConfig._fields_] == ["def_slot", "chi_max", "max_iters", "precision", "lambda0", "reserved"]
    assert (ca.ZN_CONVERGED, ca.ZN_MAX_ITERS, ca.ZN_STALLED, ca.ZN_BAD_SEED, ca.ZN_OUT_OF_IMAGE, ca.ZN_TOO_FEW, ca.ZN_FLAT,
            ca.ZN_NEGATIVE, ca.ZN_SINGULAR) == tuple(range(9))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_ffi.__file__))), "include", "lk_engine.h")).read()
    for name, n_args in (("lk_refine_znssd", 7), ("lk_znssd_step_from_sums", 8)):
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto and len(proto.group(1).split(",")) == n_args, name
        restype, argtypes = _ffi.SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == n_args, name
    for k, model in enumerate(MODELS):
        assert zr.layout(_ffi.N_PARAMS[model])[5] == (10, 15, 21, 45)[k]
    assert re.search(r"LK_ZN_CONVERGED = 0, LK_ZN_MAX_ITERS = 1, LK_ZN_STALLED = 2", header)
    assert re.search(r"LK_ZN_NEGATIVE = 7", header) and re.search(r"LK_ZN_SINGULAR = 8", header)


@pytest.fixture(scope="module")
def clean():
    return zr.pair()


def real_sums(oracle, pair, model, rect=(46, 65, 64, 83), interp=ca.IM_BICUBIC, p=(1.1, -0.5, 0.001, 0.0005, -0.0005, 0.001)):
    und, dfm = pair
    xy = zr.rect_rows(*rect)
    cx, cy = zr.rect_centre(rect)
    f, g, H, bad = zr.sample_floats(oracle, interp, model, und, dfm, xy, cx, cy, np.float32(p))
    assert not bad.any()
    return len(xy), zr.sums_of(f, g, H, bad)


def compare_step(model, n, sums, lam):
    got = ca.znssd_step_from_sums(model, n, sums, lam)
    want = zr.step(model, n, sums, float(np.float32(lam)))
    assert got[0] == want[0], (model, lam, got[0], want[0])
    P = _ffi.N_PARAMS[model]
    worst = 0.0
    if want[0] in (0, ca.ZN_NEGATIVE, ca.ZN_SINGULAR):
        for g, w, absolute in ((got[2], want[2], REL), (got[3], want[3], 0.0), (got[4], want[4], 0.0)):
            tol = REL * abs(w) + absolute
            assert abs(g - w) <= tol, (model, lam, g, w)
            worst = max(worst, abs(g - w) / tol)
    else:
        assert got[2] == got[3] == got[4] == 0.0
    if want[0] == 0:
        A, _ = zr.normal_equations(model, n, sums, want[3])
        root = np.sqrt(np.diag(A))
        scaled = got[1][:P] * root
        tol = REL * np.abs(want[6][:P]).max()
        err = np.abs(scaled - want[6][:P]).max()
        assert err <= tol and not got[1][P:].any(), (model, lam, got[1], want[1], err, tol)
        worst = max(worst, err / tol)
    else:
        assert not got[1].any()
    return worst


@pytest.mark.parametrize("model", MODELS)
def test_step_against_the_restatement(oracle, clean, model):
    worst = 0.0
    for rect, p in (((46, 65, 64, 83), (1.1, -0.5, 0.001, 0.0005, -0.0005, 0.001)), ((100, 30, 123, 53), (1.6, -0.9, 0.0, 0.0, 0.0, 0.0)),
                    ((8, 160, 20, 170), (0.7, 0.1, 0.004, 0.0, 0.0, -0.003))):
        n, sums = real_sums(oracle, clean, model, rect, p=p)
        for lam in (0.0, 1e-9, 1e-3, 0.1, 10.0, 1e6):
            worst = max(worst, compare_step(model, n, sums, lam))
        status, delta, crit, gain, offset = ca.znssd_step_from_sums(model, n, sums, 1e-3)
        assert status == 0 and 0.0 < crit < 0.5 and 0.8 < gain < 1.2 and np.abs(delta[:2]).max() < 2.0
    print(f"model {model}: worst error / tolerance {worst:.3g}")


def test_step_refusals(oracle, clean):
    model = ca.FM_UVUXUYVXVY
    n, sums = real_sums(oracle, clean, model)
    assert ca.znssd_step_from_sums(model, n, sums, 1e-3)[0] == 0
    # TOO_FEW: n < P + 2, for every model
    for m in MODELS:
        P = _ffi.N_PARAMS[m]
        k, s = real_sums(oracle, clean, m)
        assert ca.znssd_step_from_sums(m, P + 1, s, 1e-3)[0] == ca.ZN_TOO_FEW == zr.step(m, P + 1, s, 1e-3)[0]
        assert ca.znssd_step_from_sums(m, P + 2, s, 1e-3)[0] != ca.ZN_TOO_FEW
    # FLAT: a constant f, a constant g
    und, dfm = clean
    xy = zr.rect_rows(46, 65, 64, 83)
    f, g, H, bad = zr.sample_floats(oracle, ca.IM_BICUBIC, model, und, dfm, xy, 55.0, 74.0, np.zeros(6, np.float32))
    for ff, gg in ((np.full_like(f, 128.0), g), (f, np.full_like(g, 77.0))):
        s = zr.sums_of(ff, gg, H, bad)
        assert compare_step(model, len(xy), s, 1e-3) == 0.0 and ca.znssd_step_from_sums(model, len(xy), s, 1e-3)[0] == ca.ZN_FLAT
    # NEGATIVE: the inverted deformed patch; criterion, gain and offset are still reported
    s = zr.sums_of(f, np.float32(255.0) - g, -H, bad)
    got = ca.znssd_step_from_sums(model, len(xy), s, 1e-3)
    assert got[0] == ca.ZN_NEGATIVE and got[3] < 0.0 and not got[1].any()
    compare_step(model, len(xy), s, 1e-3)
    # SINGULAR: a deformed image without texture along x - g_x = 0 in every sample, so H_0 = 0 and A_00 = 0
    stripes = np.repeat((np.arange(256) * 37 % 200 + 20).astype(np.uint8)[:, None], 256, axis=1)
    for m in (ca.FM_UV, ca.FM_UVUXUYVXVY):
        fs, gs, Hs, bs = zr.sample_floats(oracle, ca.IM_BILINEAR, m, und, stripes, xy, 55.0, 74.0, np.float32([0.3, 0.4, 0, 0, 0, 0]))
        assert not bs.any() and not Hs[:, 0].any() and Hs[:, 1].any()
        s = zr.sums_of(fs, gs + np.float32(0.01) * fs, Hs, bs)   # (some correlation with f: c > 0)
        for lam in (0.0, 1e-3, 100.0):
            assert ca.znssd_step_from_sums(m, len(xy), s, lam)[0] == ca.ZN_SINGULAR
            compare_step(m, len(xy), s, lam)
    # collinear columns H_1 = 2 H_0: singular without damping, solvable with it
    Hc = H[:, :2].copy()
    Hc[:, 1] = np.float32(2.0) * Hc[:, 0]
    s = zr.sums_of(f, g, Hc, bad)
    assert ca.znssd_step_from_sums(ca.FM_UV, len(xy), s, 0.0)[0] == ca.ZN_SINGULAR == zr.step(ca.FM_UV, len(xy), s, 0.0)[0]
    assert ca.znssd_step_from_sums(ca.FM_UV, len(xy), s, 1e-3)[0] == 0
    # arguments
    lib = _ffi.load_library()
    status = C.c_int32(77)
    buf = np.zeros(ca.ZN_SUMS)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert lib.lk_znssd_step_from_sums(9, 100, ptr, 0.0, None, None, None, C.byref(status)) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_znssd_step_from_sums(model, -1, ptr, 0.0, None, None, None, C.byref(status)) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_znssd_step_from_sums(model, 100, None, 0.0, None, None, None, C.byref(status)) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_znssd_step_from_sums(model, 100, ptr, 0.0, None, None, None, None) == ca.ERROR_BAD_DOMAIN
    assert lib.lk_znssd_step_from_sums(model, 100, ptr, -1.0, None, None, None, C.byref(status)) == ca.ERROR_BAD_DOMAIN
    assert status.value == 77
    assert lib.lk_znssd_step_from_sums(model, 100, ptr, 0.0, None, None, None, C.byref(status)) == 0 and status.value == ca.ZN_FLAT


@pytest.fixture(scope="module")
def refined(oracle, clean):
    """the restatement's loop over the test geometry from the zero-gradient seeds, on the clean pair, on D and on D'"""
    und, dfm = clean
    lists, centres = zr.sector_lists(oracle)
    seeds = zr.zero_gradient_seeds(len(lists))
    d, d2 = zr.lighting_frames(dfm)
    return dict(lists=lists, centres=centres, clean=zr.refine_all(oracle, und, dfm, lists, centres, seeds),
                d=zr.refine_all(oracle, und, d, lists, centres, seeds), d2=zr.refine_all(oracle, und, d2, lists, centres, seeds))


def test_lighting_identity_of_the_restatement(refined):
    """(u, v) refined on D and on D' = D / 2 + 32 from the same seeds: the figure D_LIGHT of znssd_ref.py"""
    worst = worst_z = 0.0
    for s, (a, b) in enumerate(zip(refined["d"], refined["d2"])):
        assert a["status"] == ca.ZN_CONVERGED and b["status"] == ca.ZN_CONVERGED, (s, a["status"], b["status"])
        diff = float(np.abs(a["p"][:2].astype(np.float64) - b["p"][:2].astype(np.float64)).max())
        worst = max(worst, diff)
        worst_z = max(worst_z, abs(a["zncc"] - b["zncc"]))
    trips = [r["iterations"] for r in refined["d2"]]
    print(f"lighting: largest |(u, v) on D - (u, v) on D'| over {len(trips)} sectors = {worst:.6f} px; trips on D' {min(trips)}..{max(trips)}; "
          f"largest |zncc - zncc'| = {worst_z:.3g} (one float32 step at 1 is {np.spacing(np.float32(0.9999)):.3g})")
    assert worst <= zr.D_LIGHT, (worst, zr.D_LIGHT)
    assert worst >= 0.5 * zr.D_LIGHT, "D_LIGHT is no longer the measured figure"


def test_accuracy_of_the_restatement(refined):
    """(u, v) against the analytic map at the sector's centre on the clean pair: the figure ACCURACY of znssd_ref.py"""
    worst = 0.0
    for s, r in enumerate(refined["clean"]):
        assert r["status"] == ca.ZN_CONVERGED, (s, r["status"])
        cx, cy = (float(t) for t in refined["centres"][s])
        u, v = zr.analytic_uv(cx, cy)
        worst = max(worst, abs(float(r["p"][0]) - u), abs(float(r["p"][1]) - v))
    ev = [r["evaluations"] for r in refined["clean"]]
    print(f"accuracy: largest |(u, v) - analytic| over {len(ev)} sectors = {worst:.6f} px; evaluations {min(ev)}..{max(ev)}")
    assert worst <= zr.ACCURACY, (worst, zr.ACCURACY)
    assert worst >= 0.5 * zr.ACCURACY, "ACCURACY is no longer the measured figure"


def test_plain_least_squares_fails_where_the_refinement_does_not(oracle, clean, refined):
    """On D' the oracle's own solve (plain sum of squares, all pyramid levels) is farther from the analytic map than the
    restatement's refinement on at least 90 % of the sectors: the claim test_znssd_gpu.py makes for the engine's solve."""
    und, dfm = clean
    _, d2 = zr.lighting_frames(dfm)
    o = oracle.Oracle(model=oracle.FM_UVUXUYVXVY, precision=zr.PRECISION, py_stop=2)
    o.set_image(0, und)
    o.set_image(1, d2)
    lists, centres = refined["lists"], refined["centres"]
    rec = o.correlate_sectors(lists, centers=np.float32(centres), guesses=zr.zero_gradient_seeds(len(lists)))
    o.close()
    better = 0
    for s, r in enumerate(refined["d2"]):
        u, v = zr.analytic_uv(float(centres[s][0]), float(centres[s][1]))
        e_zn = np.hypot(float(r["p"][0]) - u, float(r["p"][1]) - v)
        e_ls = np.hypot(float(rec["p"][s][0]) - u, float(rec["p"][s][1]) - v)
        better += bool(not np.isfinite(e_ls) or e_ls > e_zn)
    print(f"on D': the plain solve is worse than the refinement on {better} of {len(lists)} sectors")
    assert better >= 0.9 * len(lists)
