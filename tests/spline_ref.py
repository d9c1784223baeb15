"""Restatements behind the B-spline refinement tests (include/lk_engine.h: lk_refine_spline, lk_spline_coefficients,
lk_spline_sample, lk_spline_weights): the recursive prefilter in float32 - the header's recipe, operation by operation -
and in float64, the sampler's weights with an exact fused multiply-add, the B-spline pieces as fractions, a float64
sampler.  numpy only.  Shared by test_spline_host.py and test_spline_gpu.py."""
from fractions import Fraction as F
from math import comb, factorial, sqrt

import numpy as np

START = 28     # terms of the causal start-up sum
POLES = {3: [sqrt(3.0) - 2.0],
         5: [sqrt(67.5 - sqrt(4436.25)) + sqrt(26.25) - 6.5, sqrt(67.5 + sqrt(4436.25)) - sqrt(26.25) - 6.5]}


def gain(order):
    lam = 1.0
    for z in POLES[order]:
        lam *= (1.0 - z) * (1.0 - 1.0 / z)
    return lam


# ---- the prefilter ------------------------------------------------------------------------------------------------------------
def _filter_lines(c, order, T):
    """c [lines][N] of type T, filtered along the last axis in place: every product and every sum rounded to T"""
    N = c.shape[1]
    c *= T(gain(order))
    for zd in POLES[order]:
        z = T(zd)
        acc, zp = c[:, 0].copy(), z
        for k in range(1, min(N, START)):
            acc = acc + zp * c[:, k]
            zp = T(zp * z)
        c[:, 0] = acc
        for k in range(1, N):
            c[:, k] = c[:, k] + z * c[:, k - 1]
        a = T(z / T(T(z * z) - T(1.0)))
        c[:, N - 1] = a * (z * c[:, N - 2] + c[:, N - 1])
        for k in range(N - 2, -1, -1):
            c[:, k] = z * (c[:, k + 1] - c[:, k])
    return c


def prefilter(img, order, T=np.float32):
    """the coefficient image [rows][cols] of type T: along every row, then along every column"""
    c = np.ascontiguousarray(img, dtype=T).copy()
    c = _filter_lines(c, order, T)
    return np.ascontiguousarray(_filter_lines(np.ascontiguousarray(c.T), order, T).T)


# ---- the pieces of the uniform B-spline ----------------------------------------------------------------------------------------
def pieces(order):
    """a[i][k]: the coefficient of t^k of the weight of node i - order // 2, i = 0 .. order, at the fraction t, as fractions:
    beta_n(x) = 1 / n! sum_k (-1)^k C(n + 1, k) (x + (n + 1) / 2 - k)_+^n at x = t + order // 2 - i"""
    n, L = order, order // 2
    out = []
    for i in range(n + 1):
        acc = [F(0)] * (n + 1)
        for k in range(n + 2):
            shift = F(L - i) + F(n + 1, 2) - k
            if shift >= 0:     # (t + shift)_+ on [0, 1)
                for j in range(n + 1):
                    acc[j] += (-1) ** k * comb(n + 1, k) * comb(n, j) * shift ** (n - j)
        out.append([a / factorial(n) for a in acc])
    return out


def derivative_pieces(order):
    return [[k * row[k] for k in range(1, len(row))] for row in pieces(order)]


def round32(fr):
    """the float32 nearest the fraction, ties to even"""
    f = np.float32(float(fr))
    near = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    return min(near, key=lambda c: (abs(F(float(c)) - fr), int(np.float32(c).view(np.uint32)) & 1))


def fma32(a, b, c):
    """fmaf: a b + c rounded once"""
    return round32(F(float(a)) * F(float(b)) + F(float(c)))


def weights32(order, t):
    """(w, g) float32 [order + 1] as the kernel forms them: every coefficient the float nearest the fraction, Horner's rule
    with one fused multiply-add per power"""
    t = np.float32(t)
    out = []
    for table in (pieces(order), derivative_pieces(order)):
        col = []
        for row in table:
            v = round32(row[-1])
            for a in row[-2::-1]:
                v = fma32(v, t, round32(a))
            col.append(v)
        out.append(np.array(col, np.float32))
    return out


def weights64(order, t):
    """(w, g) float64 [..., order + 1] of the exact pieces"""
    t = np.asarray(t, np.float64)
    out = []
    for table in (pieces(order), derivative_pieces(order)):
        out.append(np.stack([sum(float(a) * t ** k for k, a in enumerate(row)) + 0.0 * t for row in table], -1))
    return out


# ---- the sampler --------------------------------------------------------------------------------------------------------------
def valid(order, xy, rows, cols):
    """the sampler's rule, in float32 as the kernel evaluates it"""
    x, y = np.asarray(xy, np.float32)[:, 0], np.asarray(xy, np.float32)[:, 1]
    L = np.float32(order // 2)
    return (x > L) & (y > L) & (x < np.float32(cols) - (L + np.float32(1))) & (y < np.float32(rows) - (L + np.float32(1)))


def sample64(coef, xy, order):
    """W, Wx, Wy float64 [n] of the spline with the coefficients `coef` at the valid points xy [n][2]"""
    xy = np.asarray(xy, np.float32)
    c = np.asarray(coef, np.float64)
    ix, iy = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
    wx, gx = weights64(order, xy[:, 0].astype(np.float64) - ix)
    wy, gy = weights64(order, xy[:, 1].astype(np.float64) - iy)
    L = order // 2
    W, Wx, Wy = np.zeros(len(xy)), np.zeros(len(xy)), np.zeros(len(xy))
    for j in range(order + 1):
        for i in range(order + 1):
            v = c[iy - L + j, ix - L + i]
            W += wy[:, j] * wx[:, i] * v
            Wx += wy[:, j] * gx[:, i] * v
            Wy += gy[:, j] * wx[:, i] * v
    return W, Wx, Wy
