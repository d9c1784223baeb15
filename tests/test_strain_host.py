"""Strain field, host side (include/lk_engine.h: lk_strain_from_gradient - the kernel's own tensor function compiled for
the host): against a float64 restatement, a pure rotation, arguments, symbols and the record layout.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import _ffi


def tensor_reference(tensor, g):
    """float64 restatement of the header's formulas; g [..., 4] float32 = ux, uy, vx, vy -> [..., 6] float64 and the radicand"""
    g = np.asarray(g, np.float32).astype(np.float64)
    ux, uy, vx, vy = g[..., 0], g[..., 1], g[..., 2], g[..., 3]
    if tensor == ca.STRAIN_GREEN_LAGRANGE:
        exx = ux + 0.5 * (ux * ux + vx * vx)
        eyy = vy + 0.5 * (uy * uy + vy * vy)
        exy = 0.5 * (uy + vx) + 0.5 * (ux * uy + vx * vy)
    else:
        exx, eyy, exy = ux, vy, 0.5 * (uy + vx)
    rad2 = ((exx - eyy) / 2) ** 2 + exy ** 2
    rad = np.sqrt(rad2)
    return np.stack([exx, eyy, exy, (exx + eyy) / 2 + rad, (exx + eyy) / 2 - rad, 0.5 * np.arctan2(2 * exy, exx - eyy)], -1), rad2


def within_one_ulp(got, want):
    want = np.asarray(want, np.float64)
    ulp = np.spacing(np.maximum(np.abs(want), np.float64(np.finfo(np.float32).tiny)).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want) <= ulp


@pytest.mark.parametrize("tensor", [ca.STRAIN_GREEN_LAGRANGE, ca.STRAIN_SMALL])
def test_tensor_matches_float64_restatement(engine_lib, tensor):
    rng = np.random.default_rng(7 + tensor)
    grads = np.concatenate([np.zeros((1, 4)), rng.uniform(-0.2, 0.2, (400, 4))]).astype(np.float32)
    got = np.stack([ca.strain_from_gradient(tensor, g) for g in grads])
    want, rad2 = tensor_reference(tensor, grads)
    assert got.dtype == np.float32
    assert within_one_ulp(got[:, :5], want[:, :5]).all()
    sure = rad2 > 1e-6                       # theta is only defined where the principal directions are
    assert sure.sum() > 300
    assert within_one_ulp(got[sure, 5], want[sure, 5]).all()
    assert (got[:, 3] >= got[:, 4]).all()
    assert not got[0].any()                  # the zero gradient: no strain


def test_pure_rotation_has_no_green_lagrange_strain(engine_lib):
    for deg in (1.0, 10.0, 30.0, -75.0):
        a = np.deg2rad(deg)
        g = np.float32([np.cos(a) - 1, -np.sin(a), np.sin(a), np.cos(a) - 1])      # F = R(a): grad u = R - I
        gl = ca.strain_from_gradient(ca.STRAIN_GREEN_LAGRANGE, g)
        assert np.abs(gl[:5]).max() <= 1e-7, (deg, gl)
        sm = ca.strain_from_gradient(ca.STRAIN_SMALL, g)
        assert abs(sm[0] - (np.cos(a) - 1)) < 1e-7 and abs(sm[1] - (np.cos(a) - 1)) < 1e-7 and sm[0] < 0, (deg, sm)


def test_known_tensor_values(engine_lib):
    # uniaxial stretch along x by 10 %: e1 = exx along theta = 0; simple shear: principal directions at +-45 degrees (small)
    gl = ca.strain_from_gradient(ca.STRAIN_GREEN_LAGRANGE, [0.1, 0, 0, 0])
    assert np.allclose(gl, [0.105, 0, 0, 0.105, 0, 0], atol=1e-7)
    sm = ca.strain_from_gradient(ca.STRAIN_SMALL, [0, 0.02, 0, 0])
    assert np.allclose(sm, [0, 0, 0.01, 0.01, -0.01, np.pi / 4], atol=1e-7)
    sm = ca.strain_from_gradient(ca.STRAIN_SMALL, [0, 0, 0, 0.05])         # stretch along y: e1 points along y
    assert np.allclose(sm, [0, 0.05, 0, 0.05, 0, np.pi / 2], atol=1e-6)


def test_bad_arguments(engine_lib):
    g = np.zeros(4, np.float32)
    out = np.full(6, 7.0, np.float32)
    for tensor in (-1, 2, 99):
        assert engine_lib.lk_strain_from_gradient(tensor, _ffi.fptr(g), _ffi.fptr(out)) == ca.ERROR_BAD_DOMAIN
        assert (out == 7.0).all()
    assert engine_lib.lk_strain_from_gradient(0, None, _ffi.fptr(out)) == ca.ERROR_BAD_DOMAIN
    assert engine_lib.lk_strain_from_gradient(0, _ffi.fptr(g), None) == ca.ERROR_BAD_DOMAIN
    with pytest.raises(ValueError):
        ca.strain_from_gradient(5, g)
    assert engine_lib.lk_strain_field(None, None, None, None) == ca.ERROR_BAD_DOMAIN


def test_symbols_constants_and_record_layout(engine_lib):
    for name in ("lk_strain_field", "lk_strain_from_gradient"):
        assert hasattr(engine_lib, name) and name in _ffi.SYMBOLS
    assert (ca.STRAIN_OK, ca.STRAIN_FILLED, ca.STRAIN_TOO_FEW, ca.STRAIN_DEGENERATE) == (0, 1, 2, 3)
    assert (ca.STRAIN_GREEN_LAGRANGE, ca.STRAIN_SMALL) == (0, 1)
    d = ca.STRAIN_DTYPE
    assert d.itemsize == 64
    names = ("u", "v", "ux", "uy", "vx", "vy", "exx", "eyy", "exy", "e1", "e2", "theta", "residual", "neighbours", "status",
             "reserved")
    assert d.names == names
    assert [d.fields[k][1] for k in names] == [4 * i for i in range(16)]
    assert all(d.fields[k][0] == np.float32 for k in names[:13]) and all(d.fields[k][0] == np.int32 for k in names[13:])
    assert C.sizeof(_ffi.LkStrainConfig) == 16
    assert [getattr(_ffi.LkStrainConfig, f).offset for f, _ in _ffi.LkStrainConfig._fields_] == [0, 4, 8, 12]
    assert [f for f, _ in _ffi.LkStrainConfig._fields_] == ["radius", "chi_max", "min_neighbours", "tensor"]
