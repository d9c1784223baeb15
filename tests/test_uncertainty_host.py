"""Per-sector uncertainty, host side (include/lk_engine.h: lk_uncertainty_from_sums - the kernel's own function compiled
for the host): against a float64 numpy restatement on sums restated from the oracle's per-sample values, the status
cases, arguments, symbols and the record layout, and whether the definition means something.  No GPU needed.

The consistency experiment (uncertainty_ref.py): one 256 x 256 speckle image twice, independent Gaussian noise of 4 grey
levels on both copies, 12 x 12 sectors of 19 x 19 solved by the oracle with LK_FM_UV.  Measured with the oracle alone:
R = std(u over the sectors) / mean(predicted sigma_u) = 1.3388 (uncertainty_ref.R_ORACLE).
144 sectors give about +-6 % statistical spread; outside 0.7 - 1.4 the definition would be in question (the s^2
estimator, the factor for noise in both images), not a kernel."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi, speckle

import uncertainty_ref as ur

MODELS = [ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY]
TRUTH = (1.3, -0.7, 0.002, 0.0, 0.0, -0.001)
P_AT = {ca.FM_U: [1.25], ca.FM_UV: [1.25, -0.65], ca.FM_UVQ: [1.25, -0.65, 0.001],
        ca.FM_UVUXUYVXVY: [1.25, -0.65, 0.002, 0.001, -0.001, -0.001]}
RECTS = [(8, 8, 26, 26), (30, 12, 48, 30), (20, 36, 26, 42), (9, 33, 19, 51)]   # 19 x 19 twice, 7 x 7, 11 x 19


@pytest.fixture(scope="module")
def pair64():
    return speckle.speckle_pair(64, 64, p=TRUTH, seed=3)


@pytest.fixture(scope="module")
def oracle_sums(oracle, pair64):
    """(model, rect) -> (n, sums [28]) from the oracle's per-sample values: computed once, read by every test"""
    und, dfm = pair64
    out = {}
    for model in MODELS:
        for r in RECTS:
            xy = ur.rect_rows(*r)
            cx, cy = xy.mean(axis=0)
            terms, bad = ur.sample_terms(oracle, ca.IM_BICUBIC, model, und, dfm, xy, cx, cy, P_AT[model])
            assert not bad
            out[model, r] = (len(xy), terms.sum(axis=0))
    return out


@pytest.mark.parametrize("model", MODELS)
def test_host_function_matches_numpy_restatement(engine_lib, oracle_sums, model):
    for r in RECTS:
        n, sums = oracle_sums[model, r]
        got = ca.uncertainty_from_sums(model, n, sums, 0)
        assert got["status"] == ca.UNC_OK
        worst = ur.check_record(got, model, n, sums, 0, (model, r))
        print(f"model {model} rect {r}: worst error / tolerance {worst:.3g}, sigma {got['sigma']}, noise {got['noise']:.3f}")
        P = _ffi.N_PARAMS[model]
        assert (got["sigma"][:P] > 0).all() and not got["sigma"][P:].any()
        if model == ca.FM_U:
            assert got["sigma_major"] == got["sigma"][0] and got["rho_uv"] == 0 and got["sigma_minor"] == 0 and got["theta"] == 0
            assert got["sssig_y"] == 0
        else:
            assert got["sigma_major"] >= max(got["sigma"][0], got["sigma"][1]) * (1 - 1e-6)
            assert got["sigma_minor"] <= min(got["sigma"][0], got["sigma"][1]) * (1 + 1e-6)
            assert abs(got["rho_uv"]) < 1


def test_too_few_samples(engine_lib, oracle_sums):
    for model in MODELS:
        P = _ffi.N_PARAMS[model]
        _, sums = oracle_sums[model, RECTS[0]]
        for n, want in ((P, ca.UNC_TOO_FEW), (0, ca.UNC_TOO_FEW), (P + 1, ca.UNC_OK)):
            got = ca.uncertainty_from_sums(model, n, sums, 0)
            assert got["status"] == want and got["n_points"] == n
            ur.check_record(got, model, n, sums, 0, (model, n))


def x_only_sums(oracle):
    """the sums of a pair that varies in x only, under LK_FM_UV: every dW/dy is exactly 0"""
    ramp = (np.arange(64)[None, :] * 37 % 251).astype(np.uint8)
    und = np.repeat(ramp, 64, axis=0)
    dfm = np.roll(und, 1, axis=1)
    xy = ur.rect_rows(20, 20, 38, 38)
    terms, bad = ur.sample_terms(oracle, ca.IM_BICUBIC, ca.FM_UV, und, dfm, xy, 29.0, 29.0, [0.75, 0.0])
    assert not bad
    return len(xy), terms.sum(axis=0)


def test_one_directional_texture_is_singular_for_uv_and_fine_for_u(engine_lib, oracle):
    n, sums = x_only_sums(oracle)
    A, _, chi = ur.unpack(ca.FM_UV, sums)
    assert A[0, 0] > 0 and A[1, 1] == 0 and A[0, 1] == 0 and chi > 0
    got = ca.uncertainty_from_sums(ca.FM_UV, n, sums, 0)
    assert got["status"] == ca.UNC_SINGULAR and got["n_points"] == n
    ur.check_record(got, ca.FM_UV, n, sums, 0, "x only, uv")
    as_u = np.zeros(28)
    as_u[:3] = A[0, 0], sums[3], chi                     # the same sums in LK_FM_U's layout: A00, b0, chi
    got = ca.uncertainty_from_sums(ca.FM_U, n, as_u, 0)
    assert got["status"] == ca.UNC_OK and got["sigma"][0] > 0
    ur.check_record(got, ca.FM_U, n, as_u, 0, "x only, u")
    # nearly one-directional: a pivot of C below the threshold, with every A_aa > 0
    near = np.zeros(28)
    near[:6] = 4.0, 2.0 * (1 - 1e-11), 1.0, 0.1, 0.1, 5.0
    got = ca.uncertainty_from_sums(ca.FM_UV, 100, near, 0)
    assert got["status"] == ca.UNC_SINGULAR
    ur.check_record(got, ca.FM_UV, 100, near, 0, "near singular")


@pytest.mark.parametrize("model", MODELS)
def test_level_scales_the_displacements_alone(engine_lib, oracle_sums, model):
    """sigma[0] and sigma[1] are carried to level-0 pixels (times 2^L), and with them the axes of the (u, v) ellipse, which
    are lengths in the same pixels (for LK_FM_U sigma_major IS sigma[0]); every other field is the same bytes."""
    n, sums = oracle_sums[model, RECTS[0]]
    a, b = ca.uncertainty_from_sums(model, n, sums, 0), ca.uncertainty_from_sums(model, n, sums, 1)
    P = _ffi.N_PARAMS[model]
    assert (b["sigma"][:min(P, 2)] == 2 * a["sigma"][:min(P, 2)]).all()
    assert b["sigma"][2:].tobytes() == a["sigma"][2:].tobytes()
    assert b["sigma_major"] == 2 * a["sigma_major"] and b["sigma_minor"] == 2 * a["sigma_minor"]
    for k in ("noise", "rho_uv", "theta", "sssig_x", "sssig_y", "n_points", "status", "reserved"):
        assert b[k] == a[k], k
    ur.check_record(b, model, n, sums, 1, (model, "level 1"))


def test_bad_arguments(engine_lib, oracle_sums):
    n, sums = oracle_sums[ca.FM_UV, RECTS[0]]
    sums = np.ascontiguousarray(sums)
    out = np.zeros(1, ca.UNCERTAINTY_DTYPE)
    out["n_points"] = 77
    ps, po = sums.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for model in (-1, 4, 99):
        assert engine_lib.lk_uncertainty_from_sums(model, n, ps, 0, po) == ca.ERROR_BAD_DOMAIN
    for level in (-1, 8):
        assert engine_lib.lk_uncertainty_from_sums(ca.FM_UV, n, ps, level, po) == ca.ERROR_BAD_DOMAIN
    assert engine_lib.lk_uncertainty_from_sums(ca.FM_UV, n, None, 0, po) == ca.ERROR_BAD_DOMAIN
    assert engine_lib.lk_uncertainty_from_sums(ca.FM_UV, n, ps, 0, None) == ca.ERROR_BAD_DOMAIN
    assert out["n_points"][0] == 77 and not out["sigma"].any()
    with pytest.raises(ValueError):
        ca.uncertainty_from_sums(7, n, sums)
    assert engine_lib.lk_parameter_uncertainty(None, None, None, None, None) == ca.ERROR_BAD_DOMAIN


def test_symbols_constants_and_record_layout(engine_lib):
    for name in ("lk_parameter_uncertainty", "lk_uncertainty_from_sums"):
        assert hasattr(engine_lib, name) and name in _ffi.SYMBOLS
    assert (ca.UNC_OK, ca.UNC_BAD_RECORD, ca.UNC_OUT_OF_IMAGE, ca.UNC_TOO_FEW, ca.UNC_SINGULAR) == (0, 1, 2, 3, 4)
    d = ca.UNCERTAINTY_DTYPE
    assert d.itemsize == 64 and ca.UNC_SUMS == 28
    names = ("sigma", "noise", "rho_uv", "sigma_major", "sigma_minor", "theta", "sssig_x", "sssig_y", "n_points", "status",
             "reserved")
    assert d.names == names
    assert [d.fields[k][1] for k in names] == [0] + [24 + 4 * i for i in range(10)]
    assert d.fields["sigma"][0] == np.dtype((np.float32, (6,)))
    assert all(d.fields[k][0] == np.float32 for k in names[1:8]) and all(d.fields[k][0] == np.int32 for k in names[8:])
    assert C.sizeof(_ffi.LkUncertaintyConfig) == 8
    assert [f for f, _ in _ffi.LkUncertaintyConfig._fields_] == ["def_slot", "reserved"]


def test_predicted_sigma_is_the_scatter_of_u(engine_lib, oracle):
    und, dfm = ur.experiment_pair()
    rects = ur.experiment_rects()
    o = oracle.Oracle(model=oracle.FM_UV, precision=ur.EXP_PRECISION, py_stop=2)
    o.set_image(0, und)
    o.set_image(1, dfm)
    rec = o.correlate_sectors([oracle.rect_points(*r) for r in rects], None, np.zeros((len(rects), 6), np.float32))
    assert (rec["error_code"] == 0).all()
    R, mean_sigma = ur.experiment_ratio(oracle, und, dfm, rec, np.zeros((len(rects), 2), np.float32))
    print(f"R = std(u) / mean(sigma_u) = {R:.4f}; std(u) = {rec['p'][:, 0].std():.5f} px, mean sigma_u = {mean_sigma:.5f} px, "
          f"mean(u) = {rec['p'][:, 0].mean():.5f} px")
    assert 0.7 <= R <= 1.4, R                      # outside: the definition is in question
    assert abs(R - ur.R_ORACLE) <= 0.005 * ur.R_ORACLE, (R, ur.R_ORACLE)   # the recorded value is this measurement
