"""Restatements behind the speckle-quality tests (include/lk_engine.h: lk_pattern_quality, lk_suggest_subset), in numpy
int64 / float64: the doubled central differences with clamped neighbours, a sector's nine integer sums and the terms of its
gradient-magnitude sum, the record of lk_pattern_from_sums, the summed-area tables in int64 (which do not wrap), and the
suggestion by a linear scan over the candidates.  Shared by test_pattern_host.py and test_pattern_gpu.py."""
import math

import numpy as np

import correlation_amd as ca

FLOATS = ("mean", "std", "frac_low", "frac_high", "sssig_x", "sssig_y", "mig", "sigma_u", "sigma_v", "sigma_major", "theta")
SIGMAS = ("sigma_u", "sigma_v", "sigma_major", "theta")
APERTURE = 1e-6


def gradients(img):
    """(gx2, gy2) of a u8 image as int64 [rows][cols]: I(min(x + 1, cols - 1), y) - I(max(x - 1, 0), y), and alike in y"""
    a = np.asarray(img, np.int64)
    rows, cols = a.shape
    xs, ys = np.arange(cols), np.arange(rows)
    gx2 = a[:, np.minimum(xs + 1, cols - 1)] - a[:, np.maximum(xs - 1, 0)]
    gy2 = a[np.minimum(ys + 1, rows - 1), :] - a[np.maximum(ys - 1, 0), :]
    return gx2, gy2


def nodes(xy, rows, cols):
    """the nodes (int)(q + 0.5f) of float32 positions [n][2], clamped to the image -> (ix, iy)"""
    q = (np.asarray(xy, np.float32).reshape(-1, 2) + np.float32(0.5)).astype(np.int32)
    return np.clip(q[:, 0], 0, cols - 1), np.clip(q[:, 1], 0, rows - 1)


def sector_sums(img, xy, grey_low=0, grey_high=255):
    """-> (the nine int64 sums, the float64 terms sqrt(gx2^2 + gy2^2) of the samples) of the sample list xy [n][2]"""
    a = np.asarray(img, np.int64)
    gx2, gy2 = gradients(img)
    ix, iy = nodes(xy, *a.shape)
    I, gx, gy = a[iy, ix], gx2[iy, ix], gy2[iy, ix]
    sums = np.array([I.sum(), (I * I).sum(), (gx * gx).sum(), (gy * gy).sum(), (gx * gy).sum(), (I <= grey_low).sum(),
                     (I >= grey_high).sum(), I.min() if len(I) else 0, I.max() if len(I) else 0], np.int64)
    return sums, np.sqrt((gx * gx + gy * gy).astype(np.float64))


def record(n, sums, mig_sum, noise_sigma=1.0, max_saturated=1.0):
    """float64 restatement of lk_pattern_from_sums, the header's operations in the header's order -> (status, dict of the
    float fields as float64 and grey_min / grey_max)"""
    out = {k: 0.0 for k in FLOATS}
    out.update(grey_min=0, grey_max=0)
    if n < 2:
        return ca.PATTERN_TOO_FEW, out
    N = float(n)
    S1, S2, Gxx, Gyy, Gxy, low, high = (float(int(v)) for v in sums[:7])
    var = N * S2 - S1 * S1
    out.update(mean=S1 / N, std=math.sqrt(var if var > 0.0 else 0.0) / N, grey_min=int(sums[7]), grey_max=int(sums[8]),
               frac_low=low / N, frac_high=high / N, sssig_x=Gxx / 4.0, sssig_y=Gyy / 4.0, mig=float(mig_sum) / (2.0 * N))
    if int(sums[2]) + int(sums[3]) == 0:
        return ca.PATTERN_FLAT, out
    prod = Gxx * Gyy
    det = prod - Gxy * Gxy
    if det <= APERTURE * prod:
        return ca.PATTERN_APERTURE, out
    sg = float(np.float32(noise_sigma)) if np.float32(noise_sigma) > 0 else 1.0
    s2 = sg * sg
    c00, c11, c01 = s2 * (8.0 * Gyy / det), s2 * (8.0 * Gxx / det), s2 * (-8.0 * Gxy / det)
    mean, half = (c00 + c11) * 0.5, (c00 - c11) * 0.5
    rad = math.sqrt(half * half + c01 * c01)
    out.update(sigma_u=sg * math.sqrt(8.0 * Gyy / det), sigma_v=sg * math.sqrt(8.0 * Gxx / det), sigma_major=math.sqrt(mean + rad),
               theta=0.5 * math.atan2(2.0 * c01, c00 - c11))
    if low + high > float(np.float32(max_saturated)) * N:
        return ca.PATTERN_SATURATED, out
    return ca.PATTERN_OK, out


def check_record(got, n, sums, mig_sum, noise_sigma=1.0, max_saturated=1.0, tag=None):
    """got: one PATTERN_DTYPE record of the sums.  Status, counts and grey levels exactly.  Every float field but theta is
    the float32 rounding of the restatement's double - the restatement performs the same IEEE double operations (+, -, *, /,
    sqrt: all correctly rounded) in the same order - so those are compared bit for bit.  theta goes through atan2, which no
    library promises to round correctly: it is compared within 1 ulp of float."""
    status, want = record(n, sums, mig_sum, noise_sigma, max_saturated)
    assert got["status"] == status and got["n_points"] == n and got["reserved"] == 0, (tag, got, status)
    assert got["grey_min"] == want["grey_min"] and got["grey_max"] == want["grey_max"], (tag, got, want)
    for k in FLOATS:
        w = np.float32(want[k])
        if k == "theta":
            assert abs(float(got[k]) - want[k]) <= float(np.spacing(np.abs(w))), (tag, k, got[k], want[k])
        else:
            assert np.float32(got[k]).tobytes() == w.tobytes(), (tag, k, got[k], want[k])
    return status


# ---- the tables and the suggestion -------------------------------------------------------------------------------------------
def tables(img):
    """int64 summed-area tables of gx2^2 and gy2^2 with a leading zero row and column: T[y + 1][x + 1] = the sum over
    [0, x] x [0, y].  They do not wrap."""
    gx2, gy2 = gradients(img)
    out = []
    for g in (gx2, gy2):
        t = np.zeros((g.shape[0] + 1, g.shape[1] + 1), np.int64)
        t[1:, 1:] = (g * g).cumsum(0).cumsum(1)
        out.append(t)
    return out


def box(t, x0, y0, x1, y1):
    """the sums over the boxes [x0, x1] x [y0, y1] (arrays, inside the image) of one int64 table"""
    return t[y1 + 1, x1 + 1] - t[y0, x1 + 1] - t[y1 + 1, x0] + t[y0, x0]


def threshold(sssig_min):
    return int(math.ceil(4.0 * float(np.float32(sssig_min))))


def suggest(img, points, sssig_min, half_min, half_max, half_step=1, noise_sigma=1.0, tabs=None):
    """-> (SUBSET_DTYPE records [Q], int64 sums [Q][n_cand][2]) by a linear scan over every candidate of every point"""
    rows, cols = np.asarray(img).shape
    tx, ty = tabs if tabs is not None else tables(img)
    pts = np.asarray(points, np.float32).reshape(-1, 2)
    halves = np.arange(half_min, half_max + 1, half_step)
    T = threshold(sssig_min)
    sg = float(np.float32(noise_sigma)) if np.float32(noise_sigma) > 0 else 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        f = pts + np.float32(0.5)
        ok = np.isfinite(pts).all(axis=1) & (f[:, 0] > -1) & (f[:, 0] < cols) & (f[:, 1] > -1) & (f[:, 1] < rows)
        node = np.where(ok[:, None], f, 0).astype(np.int64)
    nx, ny = node[:, 0:1], node[:, 1:2]
    h = halves[None, :]
    x0, x1 = np.maximum(nx - h, 0), np.minimum(nx + h, cols - 1)
    y0, y1 = np.maximum(ny - h, 0), np.minimum(ny + h, rows - 1)
    sums = np.stack([box(tx, x0, y0, x1, y1), box(ty, x0, y0, x1, y1)], axis=2)
    sums[~ok] = 0
    passes = (sums[:, :, 0] >= T) & (sums[:, :, 1] >= T)
    first = np.where(passes.any(axis=1), passes.argmax(axis=1), len(halves) - 1)
    q = np.arange(len(pts))
    rec = np.zeros(len(pts), ca.SUBSET_DTYPE)
    rec["half"] = halves[first]
    rec["status"] = np.where(passes.any(axis=1), ca.SUBSET_OK, ca.SUBSET_NONE)
    rec["n_pixels"] = ((x1 - x0 + 1) * (y1 - y0 + 1))[q, first]
    rec["clipped"] = ((nx - h < 0) | (ny - h < 0) | (nx + h > cols - 1) | (ny + h > rows - 1))[q, first]
    g = sums[q, first].astype(np.float64)
    s = g / 4.0
    rec["sssig_x"], rec["sssig_y"] = s[:, 0], s[:, 1]
    with np.errstate(divide="ignore"):
        sigma = np.where(g > 0, sg * np.sqrt(2.0 / s), 0.0)
    rec["sigma_u"], rec["sigma_v"] = sigma[:, 0], sigma[:, 1]
    bad = np.zeros(1, ca.SUBSET_DTYPE)
    bad["status"] = ca.SUBSET_BAD_POINT
    rec[~ok] = bad[0]
    return rec, sums
