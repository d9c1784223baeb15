"""The fixture of tests/test_solve_instances_gpu.py and tests/tools/solve_instances_report.py: one small non-square pair, seven
sectors that between them load every lane group of the solve kernel unevenly, the CPU oracle's records on them for the 12
(model, interpolator) cases it covers, what the launch report of a run has to show, and the float terms of one evaluation
from the oracle's own sampler.  Plain numpy and the oracle: nothing here touches a GPU, and everything the oracle gives on
this fixture is asserted (assert_oracle_facts) before a GPU result is compared with it.

  #  sector                                             samples  why
  0  rect (20,20)-(28,28)                                    81  fewer samples than lanes from 256 lanes up, at most one per
                                                                 lane of a wavefront at level 1, a thin top level (9 samples)
  1  rect (40,20)-(58,38)                                   361  the benchmark's size; fewer samples than a 512-lane group
  2  rect (70,20)-(102,52)                                 1089  wider than a 32-lane group
  3  rect (120,20)-(180,80)                                3721  232 samples per lane when forced into 16 lanes
  4  annular_points(25, 25, -0.5f, 1.0f, 40, 125, 4)        934  registered by description, centre = the float mean
  5  every other sample of rect (110,100)-(150,140)         841  an explicit list from the host, centre (130, 120)
  6  rect (186,140)-(206,170)                               651  leaves the image: the error path of every instance
"""
import functools
import os

import numpy as np

import correlation_amd as ca

ROWS, COLS = 176, 208
TRUTH = (0.6, -0.4, 0.001, 0.0, 0.0, -0.0005)
MODELS = (ca.FM_U, ca.FM_UV, ca.FM_UVQ, ca.FM_UVUXUYVXVY)
INTERPS = (ca.IM_NEAREST, ca.IM_BILINEAR, ca.IM_BICUBIC)
MODEL_NAME = {ca.FM_U: "u", ca.FM_UV: "uv", ca.FM_UVQ: "uvq", ca.FM_UVUXUYVXVY: "affine"}
INTERP_NAME = {ca.IM_NEAREST: "nearest", ca.IM_BILINEAR: "bilinear", ca.IM_BICUBIC: "bicubic", ca.IM_BICUBIC_SEPARABLE: "separable"}
CASES = [(m, i) for m in MODELS for i in INTERPS]          # the 12 cases the oracle covers
CASE_IDS = [f"{MODEL_NAME[m]}_{INTERP_NAME[i]}" for m, i in CASES]
OUT_OF_IMAGE = ca.ERROR_INTERPOLATION_OUT_OF_IMAGE
RECTS = {0: (20, 20, 28, 28), 1: (40, 20, 58, 38), 2: (70, 20, 102, 52), 3: (120, 20, 180, 80), 6: (186, 140, 206, 170)}
ANNULAR = (25.0, 25.0, np.float32(-0.5), np.float32(1.0), 40.0, 125.0, 4)      # sector 4
LIST_RECT, LIST_CENTER = (110, 100, 150, 140), (130.0, 120.0)                  # sector 5
COUNTS = (81, 361, 1089, 3721, 934, 841, 651)
S = len(COUNTS)
LEAVES = 6                                                  # the sector that leaves the image
# lk_engine_state.hpp: size_class / kGroupOfClass for these counts - the lane group of each sector's own size class ...
NATURAL_GROUPS = (16, 16, 32, 64, 32, 32, 32)
# ... and a 16-lane row (class 0) or a wavefront in reference-order mode
REFERENCE_GROUPS = (16, 16, 64, 64, 64, 64, 64)
FLOORS = {"p01": 5e-3, "p25": 5e-5, "chi": 5e-3}           # compare_results' floors (tests/test_parity_gpu.py)
WINDOW_FRAMES = 4
WINDOW_SECTORS = (0, 1, 2, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def frames():
    und, dfm = ca.speckle.speckle_pair(ROWS, COLS, p=TRUTH, seed=7)
    for a in (und, dfm):
        a.setflags(write=False)
    return und, dfm


@functools.lru_cache(maxsize=None)
def window_frames():
    """[undeformed, the same blobs deformed by 1, 2, 3 and 4 times the truth]"""
    out = [frames()[0]]
    for k in range(1, WINDOW_FRAMES + 1):
        out.append(ca.speckle.speckle_pair(ROWS, COLS, p=tuple(k * t for t in TRUTH), seed=7)[1])
        out[-1].setflags(write=False)
    assert np.array_equal(out[1], frames()[1])
    return out


@functools.lru_cache(maxsize=None)
def lists(oracle):
    """the level-0 sample list of every sector"""
    out = [None] * S
    for s, r in RECTS.items():
        out[s] = oracle.rect_points(*r)
    out[4] = oracle.annular_points(*ANNULAR)
    out[5] = oracle.rect_points(*LIST_RECT)[::2].copy()
    assert tuple(len(x) for x in out) == COUNTS, [len(x) for x in out]
    for x in out:
        x.setflags(write=False)
    return tuple(out)


def given_center(s):
    """the centre the engine gives an implicit rectangle, the one registered with the list; None: the float mean"""
    if s in RECTS:
        x0, y0, x1, y1 = RECTS[s]
        return ((x0 + x1) * 0.5, (y0 + y1) * 0.5)
    return LIST_CENTER if s == 5 else None


def register(e, oracle, sectors=range(S)):
    """sectors `sectors` of the fixture as sectors 0, 1, ... of `e`, each by the entry point of its kind; commits"""
    for k, s in enumerate(sectors):
        if s in RECTS:
            e.resetPolygon_rect(k, *RECTS[s])
        elif s == 4:
            e.resetPolygon_annular(k, *[float(v) if i < 6 else v for i, v in enumerate(ANNULAR)])
        else:
            e.set_sector_points(k, lists(oracle)[s], center=LIST_CENTER)
    e.commit_sectors()


def make_engine(oracle, model, interp, mode="default", sectors=range(S), pair=None):
    e = ca.HipCorrelationEngine(interpolation=interp, fitting_model=model)
    if mode == "batch_invariant":
        e.set_batch_invariant(True)
    elif mode.startswith("reference_order"):
        e.set_reference_order(int(mode.split(":")[1]))
    und, dfm = pair if pair is not None else frames()
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    register(e, oracle, sectors)
    return e


def oracle_solve(oracle, o, guesses=None, sectors=range(S)):
    """one pair on the oracle `o`: the sectors with a given centre in one call, the annular one (float mean) in its own"""
    sectors = list(sectors)
    out = np.zeros(len(sectors), oracle.RESULT_DTYPE)
    given = [k for k, s in enumerate(sectors) if given_center(s) is not None]
    mean = [k for k, s in enumerate(sectors) if given_center(s) is None]
    g = None if guesses is None else np.asarray(guesses, np.float32)
    if given:
        out[given] = o.correlate_sectors([lists(oracle)[sectors[k]] for k in given],
                                         centers=np.array([given_center(sectors[k]) for k in given], np.float32),
                                         guesses=None if g is None else g[given])
    if mean:
        out[mean] = o.correlate_sectors([lists(oracle)[sectors[k]] for k in mean], guesses=None if g is None else g[mean])
    return out


@functools.lru_cache(maxsize=None)
def oracle_records(oracle, model, interp, threads=1, solver=0):
    """the oracle's records of the seven sectors (zero guess, pyramid 0 / 1 / 2): once per case, read-only"""
    und, dfm = frames()
    o = oracle.Oracle(interp=interp, model=model, n_threads=threads, solver=solver)
    o.set_image(0, und)
    o.set_image(1, dfm)
    want = oracle_solve(oracle, o)
    o.close()
    want.setflags(write=False)
    return want


def yardsticks(oracle, model, interp):
    """compare_results' three runs: T = 1 (the target), T = 8 and the exact solver (the yardsticks)"""
    return tuple(oracle_records(oracle, model, interp, threads=t, solver=s) for t, s in ((1, 0), (8, 0), (1, 2)))


def yardstick_maxima(oracle, model, interp):
    """the yardsticks' own largest deviations from the target on the sectors with error 0: {"p01", "p25", "chi", "it"}"""
    want, self8, exact = yardsticks(oracle, model, interp)
    ok = want["error_code"] == 0
    out = {"p01": 0.0, "p25": 0.0, "chi": 0.0, "it": 0}
    for y in (self8, exact):
        dp = np.abs(y["p"][ok] - want["p"][ok])
        out["p01"] = max(out["p01"], float(dp[:, :2].max()))
        out["p25"] = max(out["p25"], float(dp[:, 2:].max()))
        out["chi"] = max(out["chi"], float((np.abs(y["chi"][ok] - want["chi"][ok]) / np.maximum(np.abs(want["chi"][ok]), 1e-30)).max()))
        out["it"] = max(out["it"], int(np.count_nonzero(np.abs(y["iterations"][ok] - want["iterations"][ok]) > 1)))
    return out


_asserted = set()


def assert_oracle_facts(oracle, model, interp):
    """What the oracle gives on this fixture, asserted before anything is compared with it (once per case): the sample
    counts; error 0 on sectors 0 to 5 and the out-of-image code on sector 6, in the target and in both yardsticks; 1 to 3
    iterations with the bilinear and the bicubic sampler (but up to 11 for the six-parameter model on the 81 samples of
    sector 0), up to 17 on the nearest sampler's staircase; and yardsticks so close to the target - below 3e-6 px, 4e-7 in
    the gradients, 1.4e-5 relative in chi - that three times their maxima stay below compare_results' floors: on this
    fixture the floors are the active bounds, and no yardstick run moves an iteration count by more than 1."""
    if (oracle, model, interp) in _asserted:
        return oracle_records(oracle, model, interp)
    label = f"{MODEL_NAME[model]} {INTERP_NAME[interp]}"
    for want in yardsticks(oracle, model, interp):
        assert np.array_equal(want["n_points"], COUNTS), (label, want["n_points"])
        expect = [0] * S
        expect[LEAVES] = OUT_OF_IMAGE
        assert want["error_code"].tolist() == expect, (label, want["error_code"])
    want = oracle_records(oracle, model, interp)
    it = want["iterations"][:LEAVES]
    if interp == ca.IM_NEAREST:
        assert 1 <= it.min() and it.max() <= 17, (label, it)
    else:
        rest = it[1:] if model == ca.FM_UVUXUYVXVY else it
        assert 1 <= it.min() and rest.max() <= 3 and it[0] <= 11, (label, it)
    y = yardstick_maxima(oracle, model, interp)
    print(f"oracle facts {label}: iterations {it.tolist()}, yardstick maxima |d(u, v)| {y['p01']:.2e} px, "
          f"|d gradients| {y['p25']:.2e}, chi rel {y['chi']:.2e}, iteration counts off by > 1: {y['it']}")
    assert y["p01"] < 3e-6 and y["p25"] < 4e-7 and y["chi"] < 1.4e-5 and y["it"] == 0, (label, y)
    for k, floor in FLOORS.items():
        assert 3 * y[k] <= floor, (label, k, y[k], floor)
    _asserted.add((oracle, model, interp))
    return want


ZERO = np.zeros(6, np.float32)
# (label, hooks read by the commit, lanes per sector, team width the launch report shows): the lane groups a hook can force
FORCED = (("16", {"LK_FORCE_GROUP": 16}, 16, 0), ("32", {"LK_FORCE_GROUP": 32}, 32, 0), ("64", {"LK_FORCE_GROUP": 64}, 64, 0),
          ("256", {"LK_FORCE_GROUP": 256}, 256, 0), ("512", {"LK_FORCE_TEAM": 1}, 512, 0), ("team of 2 x 512", {"LK_FORCE_TEAM": 2}, 512, 2))


class Hooks:
    """environment hooks for the engines built inside the block: set on entry through `patch` (pytest's monkeypatch), removed
    on exit.  patch = None (a child process or a tool of its own process, where no monkeypatch exists): os.environ itself.
    A hook that is already set is somebody else's and is left alone: the block refuses to run under it."""

    def __init__(self, patch, env):
        self.patch, self.env = patch, {k: str(v) for k, v in (env or {}).items()}

    def __enter__(self):
        taken = [k for k in self.env if k in os.environ]
        if taken:
            raise RuntimeError(f"hooks already set in the environment: {taken}")
        for k, v in self.env.items():
            if self.patch is None:
                os.environ[k] = v
            else:
                self.patch.setenv(k, v)

    def __exit__(self, *exc):
        for k in self.env:
            if self.patch is None:
                os.environ.pop(k, None)
            else:
                self.patch.delenv(k, raising=False)


def run_batch(oracle, model, interp, mode="default", env=None, patch=None, alone=()):
    """one batch solve of the seven sectors from the zero guess: dict(records, report, groups, team, top = samples of every
    sector at level 2, alone = [(sector, record, report)] of the sectors in `alone` solved again by lk_correlate)"""
    with Hooks(patch, env):
        e = make_engine(oracle, model, interp, mode)
        groups, team = e.sector_groups()
        out = dict(groups=groups.tolist(), team=team.tolist(), top=[e.sector_level_count(s, 2) for s in range(S)])
        out["records"] = e.correlate_all(ZERO)
        out["report"] = e.launch_report()
        out["alone"] = []
        for s in alone:
            one, _ = e.correlate(s, np.zeros(ca.N_PARAMS[model], np.float32))
            out["alone"].append((s, one, e.launch_report()))
        e.close()
    return out


def deviations(got, want):
    """largest |d(u, v)|, |d gradients| and relative d chi on the sectors the oracle solved"""
    ok = want["error_code"] == 0
    dp = np.abs(got["p"][ok] - want["p"][ok])
    chi = np.abs(got["chi"][ok] - want["chi"][ok]) / np.maximum(np.abs(want["chi"][ok]), 1e-30)
    return float(dp[:, :2].max()), float(dp[:, 2:].max()), float(chi.max())


# ---- windows: the oracle's frame loop over sectors 0 to 5 -------------------------------------------------------------------
WINDOW_CENTER = (COLS / 2.0, ROWS / 2.0)      # the centre the guess rule is given (its global guess is zero: unused)


@functools.lru_cache(maxsize=None)
def oracle_window(oracle, model, interp, threads=1):
    """[WINDOW_FRAMES][6] records of the reference's frame loop (constant-velocity guess rule) on window_frames()"""
    fr = window_frames()
    o = oracle.Oracle(interp=interp, model=model, n_threads=threads)
    o.set_image(0, fr[0])
    n = len(WINDOW_SECTORS)
    res, prev = np.zeros((n, 6), np.float32), np.zeros((n, 6), np.float32)
    zero = np.zeros(6, np.float32)
    first = oracle_solve(oracle, o, sectors=WINDOW_SECTORS)      # (for the centres alone)
    out = []
    for k in range(WINDOW_FRAMES):
        o.set_image(1, fr[k + 1])
        g = np.zeros((n, 6), np.float32)
        for s in range(n):
            g[s], prev[s] = oracle.adjust_initial_guess(model, k, True, zero, first["und_cx"][s], first["und_cy"][s],
                                                        WINDOW_CENTER[0], WINDOW_CENTER[1], res[s], prev[s])
        r = oracle_solve(oracle, o, guesses=g, sectors=WINDOW_SECTORS)
        res = r["p"].copy()
        out.append(r)
    o.close()
    out = np.stack(out)
    out.setflags(write=False)
    return out


# ---- the launch report ------------------------------------------------------------------------------------------------------
ROLE_NAME = {ca.LAUNCH_MAIN: "main", ca.LAUNCH_STARVED: "starved", ca.LAUNCH_FINISHER: "finisher", ca.LAUNCH_SAFE_PASS: "safe pass",
             ca.LAUNCH_EVAL: "eval"}
FLAVOUR_NAME = {ca.FLAVOUR_FAST: "fast", ca.FLAVOUR_SAFE: "SAFE", ca.FLAVOUR_REFERENCE: "reference order"}
SEEN = set()      # (kind, model, interp, group, flavour) of every instance a checked report named in this process
MEASURED = {}     # (model, interp, group label, flavour) -> deviations() of a one-pair run from the oracle, for the profile
EVAL_WORST = {}   # (model, interp, group) -> worst |sum - float64 sum| / bound of the evaluation sums


def describe(report):
    return "; ".join(f"{ROLE_NAME[r['role']]}: {'SEQ ' if r['seq'] else ''}{MODEL_NAME[r['model']]} {INTERP_NAME[r['interp']]} "
                     f"{r['group']} lanes x{r['threads']} {FLAVOUR_NAME[r['flavour']]}, {r['sectors']} sectors, team {r['team_w']}, "
                     f"persistent {r['persistent']}, grid {r['grid']}" for r in report)


def check_report(report, model, interp, mains, flavour, seq=0, safe_pass=None, persistent=None, team_w=None, label=""):
    """The launch report of one solving call shows the intended instances: every record has the model and interpolator;
    the main launches are, in order, `mains` = [(lanes per sector, sectors)] of `flavour`, SEQ or not; safe_pass
    True / False: a SAFE pass follows every main launch / there is none (None: not checked).  Starved-level launches
    (one lane per sector, then the 16-lane SAFE finisher) may stand in front of a main launch: returns whether one does."""
    text = f"{label}: launch report [{describe(report)}]"
    print(text)
    assert report, text
    for r in report:
        assert (r["model"], r["interp"]) == (model, interp), text
        assert r["threads"] == {1: 64, 16: 64, 32: 64, 64: 64, 256: 256, 512: 512}[r["group"]], text
        assert r["grid"] >= 1 and r["sectors"] >= 1, text
        SEEN.add(("seq" if r["seq"] else "solve", r["model"], r["interp"], r["group"], r["flavour"]))
    main = [r for r in report if r["role"] == ca.LAUNCH_MAIN]
    assert [(r["group"], r["sectors"]) for r in main] == list(mains), text
    for r in main:
        assert r["flavour"] == flavour and r["seq"] == seq, text
        assert persistent is None or r["persistent"] == persistent, text
        assert team_w is None or r["team_w"] == team_w, text
    passes = [r for r in report if r["role"] == ca.LAUNCH_SAFE_PASS]
    if safe_pass is not None:
        assert len(passes) == (len(main) if safe_pass else 0), text
    for r in passes:
        assert r["flavour"] == ca.FLAVOUR_SAFE and r["seq"] == seq and (seq or r["group"] == 16), text
    starved = [r for r in report if r["role"] == ca.LAUNCH_STARVED]
    finishers = [r for r in report if r["role"] == ca.LAUNCH_FINISHER]
    assert len(finishers) <= len(starved) and not (seq and starved), text
    for r in starved:
        assert (r["group"], r["flavour"], r["persistent"]) == (1, ca.FLAVOUR_FAST, 0), text
    for r in finishers:
        assert (r["group"], r["flavour"]) == (16, ca.FLAVOUR_SAFE), text
    assert len(report) == len(main) + len(passes) + len(starved) + len(finishers), text
    return bool(starved)


def classes_of(groups, sectors=range(S)):
    """[(lanes per sector, sectors)] of the launches a batch of these sectors makes: one per lane group, narrowest first"""
    g = [groups[s] for s in sectors]
    return [(w, g.count(w)) for w in sorted(set(g))]


# ---- one evaluation: the float terms from the oracle's sampler --------------------------------------------------------------
def eval_parameters(model, level):
    """test_evaluation_sums' parameters, the displacement scaled to the level"""
    P = ca.N_PARAMS[model]
    p = np.array([1.1, -0.6, 0.003, -0.002, 0.001, 0.002], np.float32)[:P]
    if model == ca.FM_UVQ:
        p[2] = 0.002
    p[:min(P, 2)] /= (1 << level)
    return p


def eval_terms(oracle, interp, model, und, dfm, xy, cx, cy, p, sampler=None):
    """The terms of one evaluation as the reference forms them in float (correlation_class.cpp:131-300: V = f - W,
    H_k = Wx dTx[k] + Wy dTy[k]; chi += V V, b_k += H_k V, A_kl += H_k H_l): [n][44] float32 in the layout of evaluate()'s
    sums (A row-major 6 x 6, upper triangle; b at 36; chi at 42), and whether the sampler flagged a sample.  Every factor
    is the oracle's (model_point, interpolate_many - or `sampler` for the separable bicubic extension)."""
    import znssd_ref
    P = ca.N_PARAMS[model]
    f, g, H, bad = znssd_ref.sample_floats(oracle, interp, model, und, dfm, xy, cx, cy, p, sampler=sampler)
    V = (f - g).astype(np.float32)
    t = np.zeros((len(f), 44), np.float32)
    t[:, 42] = V * V
    for k in range(P):
        t[:, 36 + k] = H[:, k] * V
        for l in range(k, P):
            t[:, 6 * k + l] = H[:, k] * H[:, l]
    assert t.dtype == np.float32
    return t, bool(bad.any())


def sum_bound(terms, lanes):
    """(float64 sum of the float terms, bound on |a float sum of them - that|) for `lanes` lanes that each add their share
    in a chain and then meet in a tree: every addition rounds once, relative 2^-24, and a term passes through at most
    c = samples per lane + log2(lanes) + 2 of them (the 2: the product's own rounding on whichever side forms it fused or
    not, and the chain's first step), so the error is at most c 2^-24 sum |term| to first order.  lanes = 0: one
    sequential chain over all samples (the oracle's own sum)."""
    n = len(terms)
    t = terms.astype(np.float64)
    depth = (n if lanes == 0 else -(-n // lanes) + int(np.log2(lanes))) + 2
    return t.sum(0), depth * 2.0 ** -24 * np.abs(t).sum(0)


def pack_sums(A, b, chi):
    out = np.zeros(44, np.float64)
    out[:36] = np.asarray(A, np.float64).ravel()
    out[36:42] = b
    out[42] = chi
    return out
