"""The state the add-on passes keep on the engine (lk_pass.hpp: one table of slots, filled on first use, emptied by
lk_destroy): the bench hooks before and after every pass on one engine, an engine destroyed with every slot empty, and a pass
whose buffers are regrown for more sectors against a fresh engine.  Results and return codes only."""
import ctypes as C
import math

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi, speckle

import uncertainty_ref as ur

pytestmark = pytest.mark.gpu

TRUTH = (1.3, -0.7, 0.002, 0.0, 0.0, -0.001)
RADIUS = 40.0   # 2.1 pitches of the 19-pixel sectors: five neighbours for a corner of the block
# hook -> (its arguments after the engine and device_ms, its refusal before the pass has run)
HOOKS = {
    "strain": (3, "lk_internal_strain_last: no lk_strain_field yet"),
    "uncertainty": (1, "lk_internal_uncertainty_last: no lk_parameter_uncertainty yet"),
    "outlier": (3, "lk_internal_outlier_last: no lk_flag_outliers yet"),
    "track": (2, "lk_internal_track_last: no lk_track_points yet"),
    "residual": (2, "lk_internal_residual_last: no lk_photometry or lk_residual_map yet"),
}


@pytest.fixture(scope="module")
def pair():
    return speckle.speckle_pair(256, 256, p=TRUTH, seed=5)


def block(n):
    """n x n neighbouring sectors of the 12 x 12 experiment grid"""
    rects = ur.experiment_rects()
    return [rects[i * ur.EXP_N + j] for i in range(n) for j in range(n)]


def make_engine(pair, rects):
    e = ca.HipCorrelationEngine(precision=ur.EXP_PRECISION, py_stop=2)
    e.set_undeformed_image(pair[0])
    e.set_deformed_image(pair[1])
    for s, r in enumerate(rects):
        e.resetPolygon_rect(s, *r)
    e.commit_sectors()
    return e


def last(e, name):
    """(return code, message, device ms) of lk_internal_<name>_last; the values beyond the time are not asked for"""
    fn = getattr(e.lib, f"lk_internal_{name}_last")
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float)] + [C.c_void_p] * HOOKS[name][0]
    ms = C.c_float(float("nan"))
    rc = fn(e._h, C.byref(ms), *[None] * HOOKS[name][0])
    return rc, e.lib.lk_last_error_string(e._h).decode(), ms.value


def timed(e, name):
    rc, msg, ms = last(e, name)
    assert rc == 0, (name, rc, msg)
    assert math.isfinite(ms) and ms >= 0.0, (name, ms)


def solve(e):
    rec = e.correlate_all(np.float32([TRUTH[0], TRUTH[1], 0, 0, 0, 0]))
    assert (rec["error_code"] == 0).all(), rec["error_code"]
    return rec


def test_every_pass_on_one_engine(pair):
    e = make_engine(pair, block(3))
    for name, (_, refusal) in HOOKS.items():
        rc, msg, _ = last(e, name)
        assert rc == ca.ERROR_BAD_DOMAIN and msg == refusal, (name, rc, msg)
    solve(e)
    assert len(e.strain_field(RADIUS)) == 9
    timed(e, "strain")
    assert len(e.parameter_uncertainty()) == 9
    timed(e, "uncertainty")
    assert len(e.flag_outliers(RADIUS)[0]) == 9
    timed(e, "outlier")
    assert e.track_points(np.float32([[40.0, 40.0]]), RADIUS, source=_ffi.TRACK_RECORDS_ENGINE)[0].shape == (1, 1)
    timed(e, "track")
    assert len(e.photometry()) == 9
    timed(e, "residual")
    assert e.residual_map(RADIUS, (20, 20, 4, 4))[2].shape == (4, 4)
    timed(e, "residual")
    assert e.reseed_failed(RADIUS)[0].shape == (9,)
    for name in HOOKS:   # the recovery pass took the last empty slot; the others still hold their last call
        timed(e, name)
    e.close()


def test_engine_without_a_pass(pair):
    e = make_engine(pair, block(3))
    solve(e)
    e.close()
    assert not e._h.value


def test_buffers_regrown_for_more_sectors(pair):
    e = make_engine(pair, block(3))
    solve(e)
    assert len(e.strain_field(RADIUS)) == 9
    for s, r in enumerate(block(4)):
        e.resetPolygon_rect(s, *r)
    e.commit_sectors()
    rec = solve(e)
    regrown = e.strain_field(RADIUS)
    e.close()
    fresh = make_engine(pair, block(4))
    assert solve(fresh).tobytes() == rec.tobytes()
    want = fresh.strain_field(RADIUS)
    fresh.close()
    assert len(want) == 16 and (want["status"] == ca.STRAIN_OK).all(), want["status"]
    assert regrown.tobytes() == want.tobytes()
