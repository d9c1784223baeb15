"""Material-point tracks, host side (include/lk_engine.h): lk_track_step - the kernel's per-frame function compiled for the
host - against the float64 restatement of tests/track_ref.py, lk_gauges_from_tracks on known answers, bad arguments, and
the layout of the record.  No GPU is needed: both functions are host code of the library.

Tolerances: the C function and the restatement evaluate the same double expressions in the same order, so the double state
agrees within 1e-12 relative (in fact to the bit on an IEEE machine) and every float output within one float ulp of the
restatement's double value (the rounding to float itself is half an ulp)."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi
from track_ref import FLOATS, step_reference

MODES = (ca.TRACK_TOTAL, ca.TRACK_INCREMENTAL)
TENSORS = (ca.STRAIN_GREEN_LAGRANGE, ca.STRAIN_SMALL)


def random_window(rng, n, line=False, row=False):
    """the 11 sums of n sectors around a position: offsets of a few pitches, displacements of a few pixels"""
    x, y = rng.uniform(-50, 50, n), rng.uniform(-50, 50, n)
    if line:
        y = 0.5 * x + 3.0
    if row:
        y = np.full(n, 33.2337)       # a row of centres seen from a point off their lattice: Cyy is rounding noise, not 0
    u = 2.0 + 0.01 * x - 0.02 * y + rng.normal(0, 0.05, n)
    v = -1.0 + 0.015 * x + 0.005 * y + rng.normal(0, 0.05, n)
    return np.float64([x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum(), u.sum(), (x * u).sum(), (y * u).sum(),
                       v.sum(), (x * v).sum(), (y * v).sum()])


def random_state(rng):
    X, Y = rng.uniform(0, 256, 2)
    F = np.eye(2) + rng.normal(0, 0.02, (2, 2))
    return np.float64([X, Y, X + rng.normal(0, 3), Y + rng.normal(0, 3), F[0, 0], F[0, 1], F[1, 0], F[1, 1]])


def ulp32(x):
    return np.spacing(np.abs(np.float32(x))).astype(np.float64)


def check_step(mode, min_nb, n, sums, state, tensor, want_status=None):
    got, got_state = ca.track_step(mode, min_nb, n, sums, state, tensor)
    vals, nbrs, status, ref_state = step_reference(mode, min_nb, n, sums, state, tensor)
    assert got["status"] == status and got["neighbours"] == nbrs, (got, status, nbrs)
    if want_status is not None:
        assert status == want_status
    assert got_state[:2].tobytes() == np.float64(state)[:2].tobytes()
    if status == ca.TRACK_OK:
        for k, name in enumerate(FLOATS):
            assert abs(float(got[name]) - vals[k]) <= ulp32(vals[k]), (name, got[name], vals[k])
        assert np.allclose(got_state, ref_state, rtol=1e-12, atol=0)
    else:
        assert not any(got[name] for name in FLOATS)
        assert np.isnan(got_state[2:]).all() and np.isnan(ref_state[2:]).all()
    return status


@pytest.mark.parametrize("mode", MODES)
def test_step_matches_the_float64_restatement(mode):
    rng = np.random.default_rng(11 + mode)
    seen = set()
    for trial in range(200):
        n = int(rng.integers(3, 60))
        seen.add(check_step(mode, 3, n, random_window(rng, n), random_state(rng), TENSORS[trial % 2]))
    assert seen == {ca.TRACK_OK}
    # TOO_FEW: fewer sectors than asked for, an empty window included
    for n, min_nb in ((4, 5), (0, 3), (2, 3)):
        check_step(mode, min_nb, n, random_window(rng, n), random_state(rng), 0, ca.TRACK_TOO_FEW)
    # DEGENERATE: the window's centres on a line, and all in one place
    check_step(mode, 3, 12, random_window(rng, 12, line=True), random_state(rng), 0, ca.TRACK_DEGENERATE)
    for n in (3, 4, 7, 12):
        sums = random_window(rng, n, row=True)
        check_step(mode, 3, n, sums, random_state(rng), 0, ca.TRACK_DEGENERATE)
        check_step(mode, 3, n, sums[[1, 0, 4, 3, 2, 5, 7, 6, 8, 10, 9]], random_state(rng), 0, ca.TRACK_DEGENERATE)   # ... a column
    same = np.float64([5 * 3.0, 5 * 4.0, 5 * 9.0, 5 * 12.0, 5 * 16.0, 1, 3, 4, 2, 6, 8])
    check_step(mode, 3, 5, same, random_state(rng), 0, ca.TRACK_DEGENERATE)
    # BAD_POINT goes first, whatever the window
    for bad in (np.nan, np.inf):
        st = random_state(rng)
        st[1] = bad
        check_step(mode, 3, 20, random_window(rng, 20), st, 0, ca.TRACK_BAD_POINT)


def test_lost_from_a_state_that_is_not_finite():
    rng = np.random.default_rng(5)
    for k in range(2, 8):
        st = random_state(rng)
        st[k] = np.nan if k % 2 else np.inf
        sums = random_window(rng, 20)
        check_step(ca.TRACK_INCREMENTAL, 3, 20, sums, st, 0, ca.TRACK_LOST)
        # TOTAL mode does not read x, y or F of the state: the frame is fitted as if nothing had happened
        check_step(ca.TRACK_TOTAL, 3, 20, sums, st, 0, ca.TRACK_OK)
    # a chain: OK, TOO_FEW, then LOST for good
    st = random_state(rng)
    rec, st = ca.track_step(ca.TRACK_INCREMENTAL, 3, 20, random_window(rng, 20), st)
    assert rec["status"] == ca.TRACK_OK and np.isfinite(st).all()
    rec, st = ca.track_step(ca.TRACK_INCREMENTAL, 3, 2, random_window(rng, 2), st)
    assert rec["status"] == ca.TRACK_TOO_FEW and rec["neighbours"] == 2 and np.isnan(st[2:]).all()
    for _ in range(2):
        rec, st = ca.track_step(ca.TRACK_INCREMENTAL, 3, 20, random_window(rng, 20), st)
        assert rec["status"] == ca.TRACK_LOST and rec["neighbours"] == 0 and np.isnan(st[2:]).all()


def test_incremental_step_composes_the_gradient():
    """two exact affine increments: F = (I + G2)(I + G1), x = x1 + a2 + G2 (x1 - x0) - from sums of exact samples"""
    rng = np.random.default_rng(9)
    pts = rng.uniform(-40, 40, (30, 2))
    X = np.float64([100.0, 120.0])
    st = np.float64([X[0], X[1], X[0], X[1], 1, 0, 0, 1])
    x, Ftot = X.copy(), np.eye(2)
    for a, G in ((np.float64([2.0, -1.0]), np.float64([[0.01, -0.02], [0.015, 0.005]])),
                 (np.float64([-0.5, 3.0]), np.float64([[-0.01, 0.004], [0.0, 0.02]]))):
        c = x + pts                                    # sector centres around the current position
        uv = a + (c - X) @ G.T                         # the increment field, affine about X
        d = c - x
        sums = np.float64([d[:, 0].sum(), d[:, 1].sum(), (d[:, 0] ** 2).sum(), (d[:, 0] * d[:, 1]).sum(), (d[:, 1] ** 2).sum(),
                           uv[:, 0].sum(), (d[:, 0] * uv[:, 0]).sum(), (d[:, 1] * uv[:, 0]).sum(),
                           uv[:, 1].sum(), (d[:, 0] * uv[:, 1]).sum(), (d[:, 1] * uv[:, 1]).sum()])
        rec, st = ca.track_step(ca.TRACK_INCREMENTAL, 3, len(pts), sums, st)
        x = x + a + G @ (x - X)
        Ftot = (np.eye(2) + G) @ Ftot
        assert rec["status"] == ca.TRACK_OK
        assert np.allclose(st[2:4], x, rtol=0, atol=1e-9) and np.allclose(st[4:].reshape(2, 2), Ftot, rtol=0, atol=1e-11)
        assert abs(rec["x"] - x[0]) <= ulp32(x[0]) and abs(rec["u"] - (x[0] - X[0])) <= ulp32(x[0] - X[0]) + 1e-9
        assert abs(rec["vy"] - (Ftot[1, 1] - 1)) <= ulp32(Ftot[1, 1] - 1) + 1e-11


def make_tracks(positions, reference):
    """[F][Q][2] positions and [Q][2] reference positions -> TRACK_DTYPE [F][Q], all OK"""
    p = np.asarray(positions, np.float64)
    t = np.zeros(p.shape[:2], ca.TRACK_DTYPE)
    t["x"], t["y"] = p[..., 0], p[..., 1]
    t["u"], t["v"] = p[..., 0] - np.float64(reference)[:, 0], p[..., 1] - np.float64(reference)[:, 1]
    return t


def test_gauges_known_answers():
    ref = [[10.0, 20.0], [110.0, 20.0], [10.0, 70.0]]
    ang = np.deg2rad(30.0)
    frames = [ref,
              [[10.0, 20.0], [120.0, 20.0], [10.0, 70.0]],                                    # gauge 0-1 stretched by 10 %
              [[10.0, 20.0], [10.0 + 100 * np.cos(ang), 20.0 + 100 * np.sin(ang)], [10.0, 70.0]]]   # ... rotated by 30 degrees
    t = make_tracks(frames, ref)
    g = ca.gauges_from_tracks(t, [[0, 1], [0, 2], [1, 0]])
    assert g.shape == (3, 3, 4)
    assert np.array_equal(g[0, 0], np.float32([100.0, 0.0, 0.0, 0.0]))
    assert np.allclose(g[1, 0], [110.0, 0.1, np.log(1.1), 0.0], rtol=3e-7, atol=1e-7)
    assert np.allclose(g[2, 0], [100.0, 0.0, 0.0, ang], rtol=3e-7, atol=2e-7)
    assert np.allclose(g[2, 2], [100.0, 0.0, 0.0, ang], rtol=3e-7, atol=2e-7)             # the reversed pair turns alike
    assert np.array_equal(g[:, 1], np.float32([[50.0, 0.0, 0.0, 0.0]] * 3))
    # an end that is not OK: zeros in that frame for every gauge it belongs to, and for a gauge of length zero
    for status in (ca.TRACK_TOO_FEW, ca.TRACK_DEGENERATE, ca.TRACK_LOST, ca.TRACK_BAD_POINT):
        bad = t.copy()
        bad["status"][1, 1] = status
        gb = ca.gauges_from_tracks(bad, [[0, 1], [0, 2], [1, 0], [2, 2]])
        assert not gb[1, 0].any() and not gb[1, 2].any() and gb[1, 1].any() and gb[0, 0].any() and gb[2, 0].any()
        assert not gb[:, 3].any()
    # the object's method is the same function
    assert np.array_equal(ca.HipCorrelationEngine.gauges_from_tracks(t, [[0, 1]]), g[:, :1])


def test_bad_arguments(engine_lib):
    lib = engine_lib
    sums = np.zeros(11)
    st = np.float64([1, 2, 1, 2, 1, 0, 0, 1])
    out = np.zeros(1, ca.TRACK_DTYPE)
    out["x"] = 7.0
    P = C.c_void_p

    def step(mode=0, min_nb=3, n=5, s=sums, state=st, tensor=0, o=out):
        return lib.lk_track_step(mode, min_nb, n, s.ctypes.data_as(P) if s is not None else None,
                                 state.ctypes.data_as(P) if state is not None else None, tensor,
                                 o.ctypes.data_as(P) if o is not None else None)

    for kw in (dict(mode=2), dict(mode=-1), dict(min_nb=2), dict(n=-1), dict(tensor=2), dict(tensor=-1), dict(s=None),
               dict(state=None), dict(o=None)):
        assert step(**kw) == ca.ERROR_BAD_DOMAIN, kw
    assert out["x"][0] == 7.0 and np.array_equal(st, [1, 2, 1, 2, 1, 0, 0, 1])
    assert step() == 0 and out["status"][0] == ca.TRACK_DEGENERATE and out["neighbours"][0] == 5   # (five sectors in one place)
    with pytest.raises(ValueError):
        ca.track_step(5, 3, 4, sums, st)

    t = np.zeros((2, 3), ca.TRACK_DTYPE)
    g = np.full((2, 1, 4), 7.0, np.float32)

    def gauges(F=2, Q=3, tr=t, G=1, pairs=(0, 1), o=g):
        ij = np.int32(pairs) if pairs is not None else None
        return lib.lk_gauges_from_tracks(F, Q, tr.ctypes.data_as(P) if tr is not None else None, G,
                                         ij.ctypes.data_as(P) if ij is not None else None,
                                         _ffi.fptr(o) if o is not None else None)

    for kw in (dict(pairs=(0, 3)), dict(pairs=(-1, 1)), dict(pairs=(3, 0)), dict(F=0), dict(Q=0), dict(G=0), dict(tr=None),
               dict(pairs=None), dict(o=None)):
        assert gauges(**kw) == ca.ERROR_BAD_DOMAIN, kw
    assert (g == 7.0).all()
    assert gauges() == 0 and not g.any()          # two points at the origin: L0 = 0
    with pytest.raises(ValueError):
        ca.gauges_from_tracks(t, [[0, 3]])


def test_record_layout():
    d = ca.TRACK_DTYPE
    assert d.itemsize == 64
    assert d.names == FLOATS + ("neighbours", "status")
    assert [d.fields[n][1] for n in d.names] == list(range(0, 64, 4))
    assert all(d.fields[n][0] == np.float32 for n in FLOATS) and d.fields["neighbours"][0] == np.int32
    assert C.sizeof(_ffi.LkTrackConfig) == 24
    assert [getattr(_ffi.LkTrackConfig, f).offset for f, _ in _ffi.LkTrackConfig._fields_] == [0, 4, 8, 12, 16, 20]
    assert (ca.TRACK_OK, ca.TRACK_TOO_FEW, ca.TRACK_DEGENERATE, ca.TRACK_LOST, ca.TRACK_BAD_POINT) == (0, 1, 2, 3, 4)
    assert (ca.TRACK_TOTAL, ca.TRACK_INCREMENTAL) == (0, 1)
    assert (ca.TRACK_RECORDS_CALLER, ca.TRACK_RECORDS_ENGINE, ca.TRACK_RECORDS_WINDOW) == (0, 1, 2)
