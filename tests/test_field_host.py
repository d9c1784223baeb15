"""Field map, host side (include/lk_engine.h): lk_field_from_sums - the kernel's fit of one node compiled for the host -
against the float64 restatement of tests/field_ref.py on random weighted sums and on every status branch; UNIFORM sums
against lk_track_step in TOTAL mode; bad arguments; the layout of the configuration and the constants.  No GPU is needed.

The C function and the restatement evaluate the same correctly rounded double operations in the same order (no fused
multiply-add on either side), so the six plane coefficients and the five tensor fields that need +, x, / and sqrt only are
compared bit for bit; theta (atan2) within one float ulp."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi
from field_ref import fit_reference

TENSORS = (ca.STRAIN_GREEN_LAGRANGE, ca.STRAIN_SMALL)
HEADER = Path(__file__).resolve().parents[1] / "include" / "lk_engine.h"


def weighted_sums(x, y, u, v, w):
    """the header's `sums` paragraph, member after member"""
    s, W = np.zeros(11), 0.0
    for xi, yi, ui, vi, wi in zip(x, y, u, v, w):
        wx, wy = wi * xi, wi * yi
        W += wi
        s += np.float64([wx, wy, wx * xi, wx * yi, wy * yi, wi * ui, wx * ui, wy * ui, wi * vi, wx * vi, wy * vi])
    return W, s


def random_window(rng, n, bisquare, line=False, row=False, r=60.0):
    ang, rad = rng.uniform(0, 2 * np.pi, n), r * np.sqrt(rng.uniform(0, 1, n))
    x, y = rad * np.cos(ang), rad * np.sin(ang)
    if line:
        y = 0.5 * x + 3.0
    if row:
        y = np.full(n, 33.2337)       # a row of centres seen from a node off their lattice: Cyy is rounding noise, not 0
    u = 2.0 + 0.01 * x - 0.02 * y + rng.normal(0, 0.05, n)
    v = -1.0 + 0.015 * x + 0.005 * y + rng.normal(0, 0.05, n)
    d2 = x * x + y * y
    w = (1.0 - np.minimum(d2, r * r) / (r * r)) ** 2 if bisquare else np.ones(n)
    return (x, y, u, v, w)


def check(min_nb, n, W, sums, tensor, want=None):
    status, got = ca.field_from_sums(min_nb, n, W, sums, tensor)
    ref_status, plane, tens, _ = fit_reference(min_nb, [n], [W], sums, tensor)
    assert status == ref_status[0], (status, ref_status)
    if want is not None:
        assert status == want, (status, want)
    if status != ca.FIELD_OK:
        assert np.isnan(got).all()
        return status
    ref = np.concatenate([plane[0], tens[0]]).astype(np.float32)
    assert got[:11].tobytes() == ref[:11].tobytes(), (got, ref)
    assert abs(float(got[11]) - float(ref[11])) <= np.spacing(np.abs(ref[11])), (got[11], ref[11])
    return status


@pytest.mark.parametrize("bisquare", [False, True])
def test_fit_matches_the_float64_restatement(bisquare):
    rng = np.random.default_rng(31 + bisquare)
    for trial in range(200):
        n = int(rng.integers(3, 60))
        W, s = weighted_sums(*random_window(rng, n, bisquare))
        assert check(3, n, W, s, TENSORS[trial % 2]) == ca.FIELD_OK
    # TOO_FEW: fewer members than asked for, an empty window included; it goes first, whatever the sums
    for n, min_nb in ((4, 5), (0, 3), (2, 3)):
        W, s = weighted_sums(*random_window(rng, n, bisquare))
        check(min_nb, n, W, s, 0, ca.FIELD_TOO_FEW)
    check(5, 4, 0.0, np.zeros(11), 0, ca.FIELD_TOO_FEW)
    # DEGENERATE: no weight at all (every member on the rim), a weight sum that is not a number
    check(3, 5, 0.0, np.zeros(11), 0, ca.FIELD_DEGENERATE)
    check(3, 5, float("nan"), np.ones(11), 0, ca.FIELD_DEGENERATE)
    check(3, 5, -1.0, np.ones(11), 0, ca.FIELD_DEGENERATE)
    # ... the members on a line (D <= 1e-6 CC), in a row or a column off the lattice (the noise rule), all in one place (CC == 0)
    W, s = weighted_sums(*random_window(rng, 12, bisquare, line=True))
    check(3, 12, W, s, 0, ca.FIELD_DEGENERATE)
    for n in (3, 4, 7, 12):
        W, s = weighted_sums(*random_window(rng, n, bisquare, row=True))
        check(3, n, W, s, 0, ca.FIELD_DEGENERATE)
        check(3, n, W, s[[1, 0, 4, 3, 2, 5, 7, 6, 8, 10, 9]], 0, ca.FIELD_DEGENERATE)
    same = np.float64([5 * 3.0, 5 * 4.0, 5 * 9.0, 5 * 12.0, 5 * 16.0, 1, 3, 4, 2, 6, 8])
    check(3, 5, 5.0, same, 0, ca.FIELD_DEGENERATE)


def test_every_degenerate_rule_fires_alone():
    """each clause of the rule on moments built for it: the others hold"""
    base = dict(Sx=0.0, Sy=0.0, Sxx=1000.0, Sxy=0.0, Syy=1000.0)

    def sums(**kw):
        d = dict(base, **kw)
        return np.float64([d["Sx"], d["Sy"], d["Sxx"], d["Sxy"], d["Syy"], 1, 2, 3, 4, 5, 6])
    check(3, 10, 10.0, sums(), 0, ca.FIELD_OK)
    check(3, 10, 10.0, sums(Sxx=0.0), 0, ca.FIELD_DEGENERATE)                                    # CC == 0
    check(3, 10, 10.0, sums(Sx=100.0, Sxx=1000.0 * (1 + 2.0 ** -41)), 0, ca.FIELD_DEGENERATE)    # Cxx <= 2^-40 Sxx
    check(3, 10, 10.0, sums(Sy=100.0, Syy=1000.0 * (1 + 2.0 ** -41)), 0, ca.FIELD_DEGENERATE)    # Cyy <= 2^-40 Syy
    check(3, 10, 10.0, sums(Sxy=1000.0 * (1 - 4e-7)), 0, ca.FIELD_DEGENERATE)                    # D <= 1e-6 CC
    check(3, 10, 10.0, sums(Sxy=1000.0 * (1 - 6e-7)), 0, ca.FIELD_OK)


def test_uniform_sums_give_the_floats_of_the_track_step():
    """With w = 1 the weight sum is the count and the sums are lk_track_points': the fit at a point whose reference
    position is the origin (so that x - X is du itself) has lk_track_step's floats in TOTAL mode.  The gradients of the
    track are (float)((1 + g) - 1), those of the map (float)g: the same float unless g lies within 2^-53 of a rounding
    boundary of float, which for gradients of 1e-2 has a probability of 1e-7 per value - none among these."""
    rng = np.random.default_rng(5)
    names = ("u", "v", "ux", "uy", "vx", "vy", "exx", "eyy", "exy", "e1", "e2", "theta")
    for trial in range(200):
        n = int(rng.integers(3, 60))
        x, y, u, v, w = random_window(rng, n, False)
        W, s = weighted_sums(x, y, u, v, w)
        assert W == n
        tensor = TENSORS[trial % 2]
        status, got = ca.field_from_sums(3, n, W, s, tensor)
        track, _ = ca.track_step(ca.TRACK_TOTAL, 3, n, s, [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0], tensor)
        assert status == ca.FIELD_OK and track["status"] == ca.TRACK_OK and track["neighbours"] == n
        assert got.tobytes() == np.float32([track[k] for k in names]).tobytes(), (trial, got, track)
    # the status sets agree too
    for n, min_nb, row in ((2, 3, False), (0, 3, False), (7, 3, True)):
        x, y, u, v, w = random_window(rng, n, False, row=row)
        W, s = weighted_sums(x, y, u, v, w)
        status, got = ca.field_from_sums(min_nb, n, W, s)
        track, _ = ca.track_step(ca.TRACK_TOTAL, min_nb, n, s, [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0])
        assert (status, int(track["status"])) in ((ca.FIELD_TOO_FEW, ca.TRACK_TOO_FEW), (ca.FIELD_DEGENERATE, ca.TRACK_DEGENERATE))
        assert np.isnan(got).all()


def test_bad_arguments():
    lib = ca.load_library()
    s = np.ones(11)
    out = np.full(12, 7.0, np.float32)
    status = C.c_int(-5)
    P = C.c_void_p

    def call(min_nb=3, n=5, sums=s, tensor=0, o=out, st=status):
        return lib.lk_field_from_sums(min_nb, n, 5.0, sums.ctypes.data_as(P) if sums is not None else None, tensor,
                                      _ffi.fptr(o) if o is not None else None, C.byref(st) if st is not None else None)
    for kw in (dict(min_nb=2), dict(n=-1), dict(sums=None), dict(tensor=2), dict(tensor=-1), dict(o=None), dict(st=None)):
        assert call(**kw) == ca.ERROR_BAD_DOMAIN, kw
        assert (out == 7.0).all() and status.value == -5
    assert call() == 0 and status.value in (ca.FIELD_OK, ca.FIELD_DEGENERATE)
    with pytest.raises(ValueError):
        ca.field_from_sums(2, 5, 5.0, s)


def test_layout_and_constants():
    cfg = _ffi.LkFieldMapConfig
    assert C.sizeof(cfg) == 64
    want = ["radius", "chi_max", "min_neighbours", "tensor", "weight", "frame", "iterations", "x0", "y0", "nx", "ny", "stride",
            "channels", "reserved"]
    assert [f[0] for f in cfg._fields_] == want
    assert [getattr(cfg, k).offset for k in want] == [4 * i for i in range(14)]
    text = HEADER.read_text()
    enums = {}
    for block in re.findall(r"enum \{([^}]*LK_FIELD_[^}]*)\}", text):
        for item in block.split(","):
            name, expr = item.split("=")
            assert re.fullmatch(r"[0-9<() -]+", expr.strip()), expr
            enums[name.strip()] = int(eval(expr))
    for name in ("OK", "TOO_FEW", "DEGENERATE", "UNIFORM", "BISQUARE", "REFERENCE", "DEFORMED", "ALL"):
        assert enums["LK_FIELD_" + name] == getattr(ca, "FIELD_" + name), name
    for i, name in enumerate(ca.FIELD_CHANNELS):
        assert enums["LK_FIELD_" + name.upper()] == 1 << i == getattr(ca, "FIELD_" + name.upper()), name
    assert ca.FIELD_ALL == (1 << len(ca.FIELD_CHANNELS)) - 1
    # the members of the struct in the header, in order
    body = re.search(r"typedef struct lk_field_map_config \{(.*?)\} lk_field_map_config;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.strip().split("[")[0] for decl in body.split(";") for m in re.sub(r"^\s*(float|int|uint32_t)\s", "", decl.strip()).split(",")
               if m.strip()]
    assert members == want, members
