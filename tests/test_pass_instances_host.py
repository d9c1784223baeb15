"""What the pass-instance tests (test_pass_instances_gpu.py) rest on, without a GPU: the geometry of pass_instances_ref.py, the
backward restatement (backward_ref.py) on it - its float64 and float32 runs under the settled rule and its accuracy against the
analytic map - and the convergence of znssd_ref's loop on it."""
import numpy as np
import pytest

import correlation_amd as ca

import backward_ref as br
import pass_instances_ref as pi
import weighted_ref as wr
import znssd_ref as zr

S = pi.N_SECTORS


@pytest.fixture(scope="module")
def pair():
    return zr.pair()


def test_geometry_counts_and_groups(oracle):
    n0 = pi.counts()
    assert n0[:6] == [9, 513, 361, 9216, 512, 8192] and n0[7] == 8193
    assert 0 < n0[pi.RING] <= 512 and n0[pi.RING] % 16
    assert [n for (_, _, n) in pi.SECTORS if n is not None] == [n for k, n in enumerate(n0) if k != pi.RING]
    assert pi.groups() == [16, 64, 16, 512, 16, 64, 16, 512]
    # lk_bw_group restated: both sides of both thresholds
    assert [wr.group_of(n) for n in (512, 513, 8192, 8193)] == [16, 64, 64, 512]
    assert pi.count3() == (4, 2, 2)
    assert all(a != b for a, b in zip(pi.groups(), pi.groups()[1:]))     # no two sectors of a group are neighbours
    # every group as an implicit rectangle and as a list
    kinds = {(g, k == "rect") for g, (k, _, _) in zip(pi.groups(), pi.SECTORS)}
    assert {(16, True), (16, False), (64, True), (512, True), (512, False)} <= kinds
    # the point list: the 8192 nodes of the wide rectangle moved, and one more
    pts = pi.point_list()
    assert len(np.unique(pts, axis=0)) == 8193 and np.array_equal(pts[:8192] - np.float32([0, pi.SHIFT_Y]), zr.rect_rows(*pi.WIDE))
    # the levels: the 3 x 3 sector is starved at both coarser levels, the boundary sectors stay on their side of a wavefront
    per_level = [[len(l) for l in br.level_lists(oracle, xy)] for xy in pi.lists()]
    assert per_level[pi.TINY] == [9, 4, 1] and per_level[1] == [513, 140, 35] and per_level[3] == [9216, 2304, 576]
    print("samples per level", per_level)


@pytest.mark.parametrize("seed", ["near", "truth", "zero"])
def test_nothing_leaves_the_image(oracle, pair, seed):
    """the bicubic sampler - the one with the longest reach - flags no template node and no warped sample of any sector at any
    level, under each seed the tests use and under the six-parameter model, which moves the samples farthest"""
    p = {"near": pi.NEAR, "truth": np.float32(zr.TRUTH), "zero": np.zeros(6, np.float32)}[seed]
    frames = br.Frames(oracle, ca.IM_BICUBIC, *pair)
    for s, (xy0, c0) in enumerate(zip(pi.lists(), pi.centres())):
        for level, xy in enumerate(br.level_lists(oracle, xy0)):
            cx, cy = br.level_center(c0, level)
            pl = p.copy()
            pl[:2] *= np.float32(1.0 / (1 << level))
            xd, yd, _, _ = br.warp(ca.FM_UVUXUYVXVY, xy[:, 0], xy[:, 1], cx, cy, pl)
            assert not frames.sample(ca.IMG_DEF, level, np.stack([xd, yd], 1))[:, 3].any(), (s, level)
            assert not frames.sample(ca.IMG_UND, level, xy)[:, 3].any(), (s, level)


@pytest.fixture(scope="module")
def backward_cases(oracle, pair):
    out = {}
    for case in pi.ORACLE_CASES:
        problems = pi.backward_problems(oracle, case[0], case[1], *pair)
        out[case] = pi.backward_runs(problems, *case)
    return out


@pytest.mark.parametrize("case", pi.ORACLE_CASES, ids=pi.case_id)
def test_backward_reference_settles(backward_cases, case):
    """the float64 and the float32 run of the restatement under the settled rule: none unsettled for bilinear and bicubic, at
    most two of the eight sectors for nearest - the cap test_pass_instances_gpu.py asserts before it compares the kernel"""
    r64, r32, settled = backward_cases[case]
    yes, no = [s for s in range(S) if settled[s]], [s for s in range(S) if not settled[s]]
    print(f"{pi.case_id(case)}: settled {yes} unsettled {no}; iterations {[r[2] for r in r64]}; error codes {[r[3] for r in r64]}")
    assert len(no) <= pi.UNSETTLED_CAP[case[1]], no


def test_backward_reference_finds_the_map(backward_cases):
    """bicubic, six parameters: every sector but the 3 x 3 one within 0.1 px of the analytic map at its centre - the bound
    test_accuracy_full_size_pair holds the kernel to"""
    r64 = backward_cases[(ca.FM_UVUXUYVXVY, ca.IM_BICUBIC)][0]
    for s, (cx, cy) in enumerate(pi.centres()):
        if s == pi.TINY:
            continue
        p, _, _, err = r64[s]
        u, v = zr.analytic_uv(float(cx), float(cy))
        d = max(abs(float(p[0]) - u), abs(float(p[1]) - v))
        print(f"sector {s}: |(u, v) - analytic| = {d:.4f} px")
        assert err == ca.ERROR_NONE and d < 0.1, (s, p, u, v)


def test_float32_mode_changes_the_sums_only(oracle, pair):
    """the float32 mode shares the samples, the template and the loop with the float64 mode: its sums are the float64 ones to
    float32 precision, and the two modes differ"""
    pb = pi.backward_problems(oracle, ca.FM_UVUXUYVXVY, ca.IM_BICUBIC, *pair)[3]
    a, b = pb.sector(0), pb.sector(0, np.float32)
    assert a.G is b.G and a.T is b.T
    n = a.n
    assert np.abs(a.H - b.H).max() <= 16 * 2.0 ** -24 * np.abs(a.H).max() and not np.array_equal(a.H, b.H)
    (b64, chi64, _), (b32, chi32, _) = a.evaluate(pi.NEAR), b.evaluate(pi.NEAR)
    terms = np.abs(a.G * (a.T - pb.frames.sample(ca.IMG_DEF, 0, np.stack(br.warp(pb.model, a.x, a.y, a.cx, a.cy, pi.NEAR)[:2], 1))[:, 0])[:, None])
    assert (np.abs(b64 - b32) <= np.log2(n) * 2.0 ** -23 * terms.sum(axis=0)).all() and abs(chi64 - chi32) <= np.log2(n) * 2.0 ** -23 * chi64


def test_starved_step_is_the_oracles_damped_solve(oracle, pair):
    """backward_ref.starved_step against a reference of its own: lko_damped_solve - the oracle's restatement of
    compute_model_parameters and the solve, pinned by test_oracle_pins.py - with the column-pivoted QR selected (an oracle
    solve with solver 0 selects it), bit for bit, on the template matrices of the 3 x 3 sector and of a 32-sample level; and
    that it is the float64 solve of the same system to float32 precision times its condition number"""
    from oracle import lk_oracle as lo
    o = lo.Oracle(solver=0)
    o.set_image(0, pair[0])
    o.set_image(1, pair[1])
    o.newton_raphson(np.zeros(6, np.float32), lo.rect_points(30, 30, 48, 48))     # (leaves the QR selected)
    o.close()
    for model in pi.MODELS:
        problems = pi.backward_problems(oracle, model, ca.IM_BICUBIC, *pair)
        for s, level in ((pi.TINY, 0), (pi.TINY, 1), (4, 2)):
            ref = problems[s].sector(level)
            b = ref.evaluate(pi.NEAR * np.float32([1, 1, 1, 1, 1, 1]))[0]
            for lam in (1e-4, 4e-5, 1e-2, 10.0):
                got = br.starved_step(oracle, ref.H, b, lam, ref.n)
                want = oracle.damped_solve(ref.H.astype(np.float32), np.asarray(b, np.float32), np.float32(lam), np.float32(1.0) / np.float32(ref.n))
                assert got.tobytes() == want.tobytes(), (model, s, level, lam, got, want)
                A = ref.H / ref.n
                A[np.diag_indices(len(b))] *= 1.0 + lam
                if np.linalg.matrix_rank(A) == len(b):
                    exact = np.linalg.solve(A, b / ref.n)
                    assert np.abs(got - exact).max() <= 64 * 2.0 ** -24 * np.linalg.cond(A) * max(np.abs(exact).max(), 1e-30), (model, s, level, lam)


@pytest.mark.parametrize("interp", [ca.IM_BILINEAR, ca.IM_BICUBIC], ids=["bilinear", "bicubic"])
@pytest.mark.parametrize("model", pi.MODELS, ids=[pi.MODEL_NAME[m] for m in pi.MODELS])
def test_znssd_reference_converges(oracle, pair, model, interp):
    """znssd_ref.loop from the zero-gradient seeds converges on every sector but the 3 x 3 one"""
    und, dfm = pair
    seeds = pi.truth_seeds()
    status = []
    for s, (xy, (cx, cy)) in enumerate(zip(pi.lists(), pi.centres())):
        out = zr.loop(zr.sector_evaluator(oracle, interp, model, und, dfm, xy, cx, cy), model, len(xy), seeds[s])
        status.append(out["status"])
    print(f"{pi.MODEL_NAME[model]}-{pi.INTERP_NAME[interp]}: status {status}")
    assert all(st == ca.ZN_CONVERGED for s, st in enumerate(status) if s != pi.TINY), status
