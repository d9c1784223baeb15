"""The fast 32-lane solve instance of the six-parameter models keeps the 28 sums of an evaluation spread over the lanes
of a 16-lane row (reduce-scatter) and solves from there (damped_step_scattered).  Both halves are checked here against
the code they replace, bit for bit, inside one launch each (include/lk_engine.h: lk_step_compare, lk_reduce_compare):
the register damped_step<6, false> against the scattered step on the same sums, and the all-reduce of evaluate<>
(four DPP stages, partner row, solo: partner half) against the reduce-scatter on the same lane values.  Ordinary
launches on valid memory; nothing here is a tolerance - every comparison is of bit patterns."""
import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd.workload import C2

pytestmark = pytest.mark.gpu

NA, N = 21, 28
DIAG = [0, 6, 11, 15, 18, 20]   # the diagonal in the row-major upper triangle
SCALING = {0: np.float32(1.0 / 361.0), 1: np.float32(1.0 / 100.0), 2: np.float32(1.0 / 25.0)}   # 1 / samples of a 19 x 19 sector's levels


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pack(sums, lam, scaling, p):
    """[n][40] records of lk_step_compare."""
    sums = np.asarray(sums, np.float32).reshape(-1, N)
    rec = np.zeros((sums.shape[0], 40), np.float32)
    rec[:, :N] = sums
    rec[:, 28] = lam
    rec[:, 29] = scaling
    rec[:, 30:36] = p
    return rec


def sums_of(A, b, chi):
    iu = np.triu_indices(6)
    return np.concatenate([np.asarray(A, np.float32)[iu], np.asarray(b, np.float32), [np.float32(chi)]]).astype(np.float32)


def check_same(out, what):
    reg, sc = out[:, 0], out[:, 1]
    assert np.all(sc[:, 13] == 1.0), f"{what}: the lanes of a wavefront disagree in {np.flatnonzero(sc[:, 13] != 1.0)[:8]}"
    for name, lo, hi in (("x", 0, 6), ("p", 6, 12), ("flag", 12, 13)):
        diff = np.flatnonzero((bits(reg[:, lo:hi]) != bits(sc[:, lo:hi])).any(axis=1))
        assert diff.size == 0, f"{what}: {name} differs in {diff.size} systems, first {diff[:8]}: {reg[diff[0]]} vs {sc[diff[0]]}"


@pytest.fixture(scope="module")
def engine():
    und, dfm = ca.speckle.speckle_pair(C2.size, C2.size, p=C2.truth, seed=7)
    e = ca.HipCorrelationEngine(fitting_model=C2.model, py_stop=C2.py_stop)
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    e.set_rect_grid(C2.x_begin, C2.x_begin, C2.x_end, C2.x_end, C2.hs, C2.vs)
    e.commit_sectors()
    yield e
    e.close()


@pytest.fixture(scope="module")
def c2_systems(engine):
    """28-sum vectors of real C2 evaluations: 400 sectors, the three levels, at the zero guess and near the answer."""
    rng = np.random.default_rng(5)
    rec = []
    for s in rng.choice(C2.hs * C2.vs, 400, replace=False):
        for level in (2, 1, 0):
            mag = np.float32(1.0 / (1 << level))
            for p in (np.zeros(6, np.float32), np.array(C2.truth, np.float32) * np.array([mag, mag, 1, 1, 1, 1], np.float32)):
                A, b, chi, err = engine.evaluate(int(s), level, p)
                if err:
                    continue
                rec.append((sums_of(A, b, chi), p, SCALING[level]))
    return rec


def test_healthy_c2_systems(engine, c2_systems):
    rng = np.random.default_rng(6)
    sums = np.array([r[0] for r in c2_systems])
    p = np.array([r[1] for r in c2_systems])
    assert len(sums) > 2000
    lam = np.float32(1e-4) * np.float32(0.4) ** rng.integers(0, 6, len(sums))   # the damping of the first trips
    out = engine.step_compare(pack(sums, lam, np.array([r[2] for r in c2_systems]), p))
    assert np.all(out[:, 0, 12] == 1.0), "real C2 systems are well conditioned"
    assert np.abs(out[:, 0, :6]).max() > 0
    check_same(out, "C2 evaluations")


def test_damped_near_singular_systems(engine):
    """Rank-deficient H H^T (rank 1 to 5) plus rounding: the damping alone keeps the pivots up, lambda from 1e-3 to 1e3."""
    rng = np.random.default_rng(7)
    rec = []
    for lam in (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3):
        for rank in range(1, 6):
            for _ in range(40):
                H = (rng.standard_normal((361, rank)) @ rng.standard_normal((rank, 6)) * 10.0 ** rng.uniform(-2, 2, 6)).astype(np.float32)
                V = rng.standard_normal(361).astype(np.float32) * 20
                rec.append(pack(sums_of(H.T @ H, H.T @ V, V @ V), lam, 1.0 / 361.0, rng.standard_normal(6).astype(np.float32)))
    out = engine.step_compare(np.concatenate(rec))
    assert out[:, 0, 12].sum() > 0, "the damping carries some of these systems through the pivot test"
    check_same(out, "damped near-singular systems")


def test_small_and_bad_pivots(engine, c2_systems):
    """Pivots below LK_FAST_PIVOT (1e-6 of the diagonal entry) and below 1e-7 of the largest: a duplicated parameter with
    no damping to speak of, a zero, negative or tiny diagonal at each position, a huge one next to ordinary ones."""
    rng = np.random.default_rng(8)
    rec = []
    base = [r[0] for r in c2_systems[:60]]
    iu = np.triu_indices(6)
    for s in base:
        A = np.zeros((6, 6), np.float32)
        A[iu] = s[:NA]
        A = A + np.triu(A, 1).T
        b = s[NA:NA + 6].copy()
        for j in range(6):
            for k in range(6):
                if k == j:
                    continue
                B, c = A.copy(), b.copy()   # parameter j becomes a copy of parameter k: an exactly singular system
                B[j, :], B[:, j] = B[k, :], B[:, k]
                B[j, j] = B[k, k]
                c[j] = c[k]
                rec.append(pack(sums_of(B, c, s[-1]), 10.0 ** rng.uniform(-9, -6), 1.0 / 361.0, np.zeros(6, np.float32)))
            for d in (0.0, -1.0, 1e-12, 1e12):
                t = s.copy()
                t[DIAG[j]] = np.float32(d) if d <= 0 else t[DIAG[j]] * np.float32(d)
                rec.append(pack(t, 1e-4, 1.0 / 361.0, rng.standard_normal(6).astype(np.float32)))
    out = engine.step_compare(np.concatenate(rec))
    assert (out[:, 0, 12] == 0.0).sum() > len(out) // 10, "these systems are meant to fail the pivot test"
    zeroed = (out[:, 0, 12] == 0.0) & (out[:, 0, :6] == 0.0).any(axis=1)
    assert zeroed.any(), "a bad pivot zeroes that parameter's step"
    check_same(out, "bad pivots")


def test_nan_zero_and_extremes(engine, c2_systems):
    s = c2_systems[0][0]
    rec = [pack(np.zeros(N, np.float32), 1e-4, 1.0 / 361.0, np.ones(6, np.float32))]
    for v in range(N):   # a NaN, an infinity in every place
        for bad in (np.nan, np.inf, -np.inf):
            t = s.copy()
            t[v] = bad
            rec.append(pack(t, 1e-4, 1.0 / 361.0, np.ones(6, np.float32)))
    rec.append(pack(s, np.nan, 1.0 / 361.0, np.ones(6, np.float32)))
    rec.append(pack(s, 1e-4, np.inf, np.ones(6, np.float32)))       # scaling of an empty level (1 / 0)
    rec.append(pack(s * np.float32(1e-30), 1e-4, 1e-10, np.ones(6, np.float32)))   # denormal products
    rec.append(pack(s * np.float32(1e25), 1e9, 1.0, np.ones(6, np.float32)))       # overflow under the damping
    out = engine.step_compare(np.concatenate(rec))
    assert np.isnan(out[:, 0, :6]).any() and (out[0, 0, :6] == 0).all() and out[0, 0, 12] == 0.0
    check_same(out, "NaN, zeros and extremes")


@pytest.mark.parametrize("wide", [False, True], ids=["two-sectors", "solo"])
def test_reduce_scatter_keeps_the_association(engine, wide):
    """Lane values whose sum depends on the association in the last bits (mixed signs, twelve binades, near-cancelling
    pairs): a different tree would show in most of the 28 x 256 totals.  Every lane must read back, for every sum, the
    bits the all-reduce leaves there."""
    rng = np.random.default_rng(9 + wide)
    n = 256
    v = (rng.standard_normal((n, 64, N)) * 2.0 ** rng.integers(-6, 7, (n, 64, N))).astype(np.float32)
    pair = rng.random((n, 32, N)) < 0.3   # near-cancelling neighbours
    v[:, 1::2][pair] = -v[:, 0::2][pair] * np.float32(1 + 2.0 ** -12)
    v[0] = 0.0
    v[1, :, 3] = np.nan
    v[2, 17, :] = np.inf
    out = engine.reduce_compare(v, wide=wide)
    ref, got = out[:, 0], out[:, 1]
    # the yardstick itself: every lane of a group holds the same bits, and they are not those of another association
    group = 64 if wide else 32
    r = bits(ref).reshape(n, 64 // group, group, N)
    assert (r == r[:, :, :1]).all()
    lanes = v[3:].reshape(n - 3, 64 // group, group, N).astype(np.float32)
    seq = np.zeros_like(lanes[:, :, 0])
    for i in range(group):
        seq = seq + lanes[:, :, i]
    assert (bits(seq) != bits(ref[3:].reshape(n - 3, 64 // group, group, N)[:, :, 0])).mean() > 0.3, "inputs do not expose the association"
    diff = np.argwhere(bits(ref) != bits(got))
    assert diff.size == 0, f"{len(diff)} totals differ, first (wavefront, lane, sum): {diff[:6].tolist()}"
