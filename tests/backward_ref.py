"""Restatements behind the backward-update tests (lk_set_update(LK_UPDATE_BACKWARD), lk_evaluate_backward; include/lk_engine.h
and DESIGN.md section 13) on the oracle alone: the pyramid by oracle.pyramid_level, the level lists by oracle.decimate, the
float32 level centres, the template (the undeformed node and the sampler's gradient there) and the deformed value by
oracle.interpolate_many, float64 sums, and a numpy restatement of the loop around them.  The composition is
ca.compose_inverse, the kernel's function compiled for the host (pinned by test_backward_host.py).

LK_IM_BICUBIC_SEPARABLE is not in the oracle: the GPU tests pass the engine's lk_sample through `sampler`
(test_separable_bicubic_extension pins it).

A second mode accumulates H, b and chi in float32 and changes nothing else.  It is a yardstick only: a sector whose float64
and float32 runs end alike (settled()) is one whose result does not hang on the last bits of the sums, so the kernel - whose
sums are float32 in yet another order - may be held to the float64 run's parameters.  The rule reads nothing from the GPU.

Shared by test_backward_gpu.py, test_frame_shapes_gpu.py, test_pass_instances_host.py and test_pass_instances_gpu.py."""
import numpy as np

import correlation_amd as ca

P = {ca.FM_U: 1, ca.FM_UV: 2, ca.FM_UVQ: 3, ca.FM_UVUXUYVXVY: 6}
F32 = np.float32
ORACLE_INTERPS = (ca.IM_NEAREST, ca.IM_BILINEAR, ca.IM_BICUBIC)


def round_like_host(v):
    return np.trunc(np.asarray(v, F32) + F32(0.5)).astype(np.int64)


def level_center(c0, level):
    """the centre of a sector at a level from its level-0 centre: float32, times 1 / 2^level above level 0"""
    cx, cy = c0
    if level == 0:
        return F32(cx), F32(cy)
    inv = F32(1.0) / F32(1 << level)
    return F32(cx) * inv, F32(cy) * inv


def warp(model, x, y, cx, cy, p):
    """Warp<MODEL>::apply in float32, left to right"""
    p = np.asarray(p, F32)
    dx, dy = x - cx, y - cy
    if model == ca.FM_U:
        return x + p[0], y.copy(), dx, dy
    if model == ca.FM_UV:
        return x + p[0], y + p[1], dx, dy
    if model == ca.FM_UVQ:
        return (x + p[0]) - p[2] * dy, (y + p[1]) + p[2] * dx, dx, dy
    return ((x + p[0]) + p[2] * dx) + p[3] * dy, ((y + p[1]) + p[4] * dx) + p[5] * dy, dx, dy


def jac(model, gx, gy, dx, dy):
    gx, gy, dx, dy = [np.asarray(t, np.float64) for t in (gx, gy, dx, dy)]
    if model == ca.FM_U:
        return gx[:, None]
    if model == ca.FM_UV:
        return np.stack([gx, gy], 1)
    if model == ca.FM_UVQ:
        return np.stack([gx, gy, gx * (-dy) + gy * dx], 1)
    return np.stack([gx, gy, gx * dx, gx * dy, gy * dx, gy * dy], 1)


def close(got, want, rtol=2e-5, atol=1e-3):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() <= rtol * max(np.abs(want).max(), 1.0) + atol


class Frames:
    """the pyramids of a pair by the oracle, and the sampler of a (slot, level): interpolate_many, or `sampler(slot, level,
    points [n][2] float32) -> [n][4] = W, dW/dx, dW/dy, flag` where the oracle has none"""

    def __init__(self, oracle, interp, und, dfm, levels=3, sampler=None):
        assert sampler is not None or interp in ORACLE_INTERPS, "the oracle has no such sampler: pass one"
        self.oracle, self.interp, self.sampler = oracle, interp, sampler
        self.img = {ca.IMG_UND: [np.ascontiguousarray(und, np.uint8)], ca.IMG_DEF: [np.ascontiguousarray(dfm, np.uint8)]}
        for pyr in self.img.values():
            for _ in range(levels - 1):
                pyr.append(oracle.pyramid_level(pyr[-1]))

    def sample(self, slot, level, pts):
        pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
        if not len(pts):
            return np.zeros((0, 4), F32)
        if self.sampler is not None:
            return np.asarray(self.sampler(slot, level, pts), F32)
        return self.oracle.interpolate_many(self.interp, self.img[slot][level], pts)


def level_lists(oracle, pts0, levels=3):
    """the sample lists of a sector at every level: level l + 1 from level l by oracle.decimate"""
    out = [np.ascontiguousarray(pts0, F32).reshape(-1, 2)]
    for _ in range(levels - 1):
        out.append(oracle.decimate(out[-1], 1))
    return out


def _sum(terms, acc):
    """the sum over the samples (axis 0): float64 terms added in float64, or rounded to float32 and added in float32 - every
    column on its own and contiguous, which numpy adds pairwise: a tree, as the kernel's lanes and reduction are, not a chain"""
    if acc == np.float64:
        return terms.sum(axis=0)
    cols = np.ascontiguousarray(terms.astype(F32).reshape(len(terms), -1).T)
    return cols.sum(axis=1, dtype=F32).astype(np.float64).reshape(terms.shape[1:])


class RefSector:
    """the template of one sector at one level, from the oracle's pieces (float64 sums; acc=np.float32: float32 sums)"""

    def __init__(self, frames, model, pts, c0, level, acc=np.float64):
        self.frames, self.model, self.level, self.acc = frames, model, level, acc
        pts = np.asarray(pts, F32).reshape(-1, 2)
        self.x, self.y = pts[:, 0].copy(), pts[:, 1].copy()
        self.cx, self.cy = level_center(c0, level)
        und = frames.img[ca.IMG_UND][level]
        ux = np.clip(round_like_host(self.x), 0, und.shape[1] - 1)
        uy = np.clip(round_like_host(self.y), 0, und.shape[0] - 1)
        self.T = und[uy, ux].astype(np.float64)
        g = frames.sample(ca.IMG_UND, level, np.stack([ux, uy], 1).astype(F32))
        self.tbad = bool(g[:, 3].any())
        self.G = jac(model, g[:, 1], g[:, 2], self.x - self.cx, self.y - self.cy)
        n = P[model]
        self.H = _sum((self.G[:, :, None] * self.G[:, None, :]).reshape(len(pts), n * n), acc).reshape(n, n)
        self.n = len(self.x)
        self._values = {}

    def with_acc(self, acc):
        """the same sector with the other accumulation: the samples and the cached deformed values are shared"""
        other = RefSector.__new__(RefSector)
        other.__dict__.update(self.__dict__)
        other.acc = acc
        n = P[self.model]
        other.H = _sum((self.G[:, :, None] * self.G[:, None, :]).reshape(self.n, n * n), acc).reshape(n, n)
        return other

    def evaluate(self, p):
        """-> b [P], chi, whether a sample left the deformed image"""
        key = np.asarray(p, F32).tobytes()
        if key not in self._values:
            xd, yd, _, _ = warp(self.model, self.x, self.y, self.cx, self.cy, p)
            self._values[key] = self.frames.sample(ca.IMG_DEF, self.level, np.stack([xd, yd], 1))
        w = self._values[key]
        V = self.T - w[:, 0].astype(np.float64)
        return _sum(self.G * V[:, None], self.acc), float(_sum(V * V, self.acc)), bool(w[:, 3].any())


class Problem:
    """one sector of a pair for solve_ref: its lists and templates at every level, built once and shared by the float64 and
    the float32 run"""

    def __init__(self, frames, model, pts0, c0, lists=None):
        self.frames, self.model, self.c0 = frames, model, (F32(c0[0]), F32(c0[1]))
        self.lists = lists if lists is not None else level_lists(frames.oracle, pts0, len(frames.img[ca.IMG_UND]))
        self._sectors = {}

    def sector(self, level, acc=np.float64):
        if level not in self._sectors:
            self._sectors[level] = RefSector(self.frames, self.model, self.lists[level], self.c0, level)
        base = self._sectors[level]
        return base if acc == np.float64 else base.with_acc(acc)


def starved_step(oracle, H, b, lam, n_samples):
    """The step of a starved level (at most 2 P samples): the engine takes the reference's solver there, as include/lk_engine.h
    says ("QR on starved levels") - compute_model_parameters' scaling and damping and the column-pivoted QR, in float32.  With
    nine samples for six parameters a float64 solve of the same system lands 1e-5 from it in the gradient terms.
    Scaled and damped here, operation by operation as lko_damped_solve does it: that entry takes whichever solver the oracle's
    last solve was configured with, colpiv_qr_solve is the QR whatever ran before (test_pass_instances_host.py ties the two)."""
    n = len(b)
    scaling = F32(1.0) / F32(n_samples)
    A32 = np.triu(np.asarray(H).astype(F32) * scaling)
    A32 = A32 + np.triu(A32, 1).T
    A32[np.diag_indices(n)] *= F32(1.0) + F32(lam)
    assert A32.dtype == F32
    return oracle.colpiv_qr_solve(A32, np.asarray(b, F32) * scaling)


def solve_ref(problem, guess, precision=1e-3, max_iters=50, py=(0, 1, 2), acc=np.float64):
    """numpy restatement of the backward loop of include/lk_engine.h (float64 sums and solve - the reference's float32 QR on a
    starved level -, the oracle's sampler, the host copy of the kernel's composition) -> p float32 [6], chi, iterations, error code.  acc=np.float32: the sums in float32."""
    model = problem.model
    n = P[model]
    py_start, py_step, py_stop = py
    p = np.zeros(6, F32)
    p[:n] = guess[:n]
    reached, error, lg_chi, level_old = 0, 0, F32(np.finfo(F32).max), 0
    min_l, max_l = F32(1e-9), F32(1e9)

    def translate(p, src, dst):
        mag = F32(1.0) / F32(1 << (dst - src)) if dst - src > 0 else F32(1 << (src - dst))
        p[:min(n, 2)] = (p[:min(n, 2)] * mag).astype(F32)

    def step(ref, b, lam, p_from):
        if ref.n <= 2 * n:   # a starved level
            return ca.compose_inverse(model, p_from[:n], -starved_step(problem.frames.oracle, ref.H, b, lam, ref.n))
        A = ref.H / ref.n
        A[np.diag_indices(n)] *= (1.0 + float(lam))
        try:
            delta = np.linalg.solve(A, b / ref.n).astype(F32)
        except np.linalg.LinAlgError:   # an exactly singular system: no step (the kernel's singular step)
            return None
        return ca.compose_inverse(model, p_from[:n], -delta)

    early = False
    for level in range(py_stop, py_start - 1, -py_step):
        translate(p, level_old, level)
        error, lam, lg_chi = 0, F32(1e-4), F32(np.finfo(F32).max)
        ref = problem.sector(level, acc)
        if ref.tbad:
            error, early = ca.ERROR_INTERPOLATION_OUT_OF_IMAGE, True
            translate(p, level, 0)
            break
        lg_p = p.copy()
        first, use_saved, saved, it, kb = True, True, None, 0, None
        while True:
            ok, tent = True, None
            if first:
                tent = p.copy()
            else:
                it += 1
                if it > max_iters or lam >= max_l:
                    error = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
                    break
                reached = it
                if use_saved:
                    tent, ok = saved, saved is not None
                else:
                    p = lg_p.copy()
                    tent = step(ref, kb, lam, lg_p)
                    ok = tent is not None
            chi = F32(np.inf)
            if ok:
                p = tent.copy()
                b, chi64, bad = ref.evaluate(tent)
                if bad:
                    error, early = ca.ERROR_INTERPOLATION_OUT_OF_IMAGE, first
                    break
                chi = F32(chi64) * F32(1.0 / ref.n)
                la = lam
                if not first:
                    la = lam * F32(0.4)
                    la = la if la > min_l else min_l
                saved = step(ref, b, la, tent)
                if saved is not None:
                    p = saved.copy()
            if first:
                lg_chi, kb, first = chi, b, False
                continue
            mx = chi if lg_chi < chi else lg_chi
            with np.errstate(invalid="ignore"):
                delta_chi = abs((lg_chi - chi) / (mx + F32(precision)))
            if chi <= lg_chi:
                lg_chi, lg_p, kb, use_saved = chi, tent.copy(), b, True
                lam = max(lam * F32(0.4), min_l)
            else:
                lam, use_saved = min(lam * F32(10.0), max_l), False
            if delta_chi < precision:
                break
        if early:
            translate(p, level, 0)
            break
        level_old = level
    if not early:
        translate(p, level_old, 0)
    return p, lg_chi, reached, error


# ---- the settled rule --------------------------------------------------------------------------------------------------------
# the bounds the whole-solve comparison holds the kernel to (test_whole_solves_against_restatement): |d(u, v)| < 1e-4, the
# other parameters within 1e-6
BOUND_UV, BOUND_REST = 1e-4, 1e-6


def settled(model, run64, run32):
    """a sector is settled when its float64 and float32 runs give the same error code, the same iteration count and
    parameters within one tenth of the comparison bounds"""
    n = P[model]
    (p64, _, it64, err64), (p32, _, it32, err32) = run64, run32
    if err64 != err32 or it64 != it32:
        return False
    d = np.abs(p64.astype(np.float64) - p32.astype(np.float64))
    if not np.isfinite(d[:n]).all():
        return False
    return bool(d[:min(n, 2)].max() < 0.1 * BOUND_UV and (n <= 2 or d[2:n].max() < 0.1 * BOUND_REST))
