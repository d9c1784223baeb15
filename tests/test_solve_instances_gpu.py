"""Every compiled instance of the solve kernel and of the evaluation kernel against the CPU oracle.

lk_solve_kernel is one template compiled for 4 models x 4 interpolators x 6 lane groups x 3 flavours, plus the
frame-pipelined SEQ instances; lk_eval_kernel for 4 x 4 x 4.  The rest of the suite covers the models and interpolators in
the lane group the classifier picks, and the lane groups with the six-parameter model and the bicubic sampler: an error
that lives in one (model, group) pair passes it.  Here the 12 (model, interpolator) cases the oracle covers are crossed with
every lane group and flavour a hook or a mode can select, on one small non-square fixture (tests/solve_instances_ref.py).

Every run first shows from the engine's launch report (lk_get_launch_report) that the intended instance ran: a run whose
report names another instance fails.  No tolerance of this module's own for whole solves: reference-order and
batch-invariant runs are compared by bytes, default-mode runs with compare_results, whose floors are the active bounds on
this fixture (solve_instances_ref.assert_oracle_facts).  The tight check in default mode is the evaluation: every sum
against the float64 sum of the float terms, within the rounding of the group's own addition chain.
profiles/solve_instances.txt (tests/tools/solve_instances_report.py) holds the measured deviations."""
import os
import subprocess
import sys

import numpy as np
import pytest

import correlation_amd as ca

import frame_shapes_ref as fs
import solve_instances_ref as si

pytestmark = pytest.mark.gpu

PARITY = fs.module("test_parity_gpu")             # compare_results
REFORDER = fs.module("test_reference_order_gpu")  # assert_same_bytes, canonical
CASES = pytest.mark.parametrize("model,interp", si.CASES, ids=si.CASE_IDS)
FAST, SAFE, REF = ca.FLAVOUR_FAST, ca.FLAVOUR_SAFE, ca.FLAVOUR_REFERENCE


def label_of(model, interp, *more):
    return " ".join([si.MODEL_NAME[model], si.INTERP_NAME[interp]] + [str(m) for m in more])


# ---- 1. one-pair solves -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", [FAST, SAFE], ids=["fast", "safe"])
@CASES
def test_default_mode_in_every_forced_lane_group(oracle, monkeypatch, model, interp, flavour):
    """16, 32, 64 and 256 lanes per sector, one 512-thread workgroup and a team of two, in the fast flavour (with its SAFE
    pass behind it) and with LK_FORCE_SAFE=1 (the QR inside the kernel, no separate pass): compare_results against the
    oracle and its two yardsticks, the out-of-image code of sector 6 exactly.  The one-lane kernel of starved levels stands
    in front of the launch exactly where a sector's top level has at most 2 P samples: the 9 samples of sector 0 under the
    six-parameter model."""
    si.assert_oracle_facts(oracle, model, interp)
    yard = si.yardsticks(oracle, model, interp)
    P = ca.N_PARAMS[model]
    for name, env, group, team_w in si.FORCED:
        if flavour == SAFE:
            env = dict(env, LK_FORCE_SAFE=1)
        label = label_of(model, interp, name, si.FLAVOUR_NAME[flavour])
        run = si.run_batch(oracle, model, interp, "default", env, monkeypatch)
        assert run["groups"] == [group] * si.S, (label, run["groups"])
        assert run["team"] == [env.get("LK_FORCE_TEAM", 0)] * si.S, (label, run["team"])
        starved = si.check_report(run["report"], model, interp, [(group, si.S)], flavour, safe_pass=flavour == FAST, persistent=0,
                                  team_w=team_w, label=label)
        assert starved == (min(run["top"]) <= 2 * P) == (model == ca.FM_UVUXUYVXVY), (label, run["top"])
        print(f"{label}: one-lane starved-level launch {'ran' if starved else 'did not run'} (top-level samples {run['top']}, P = {P})")
        PARITY.compare_results(run["records"], yard, label)
        assert run["records"]["error_code"][si.LEAVES] == si.OUT_OF_IMAGE
        si.MEASURED[model, interp, name, flavour] = si.deviations(run["records"], yard[0])
        print(f"{label}: max |d(u, v)| %.2e, |d gradients| %.2e, chi rel %.2e" % si.MEASURED[model, interp, name, flavour])


@CASES
def test_batch_invariant_mode_alone_and_in_the_batch(oracle, monkeypatch, model, interp):
    """every sector in the lane group of its own size class (16, 32 and 64 lanes), SAFE flavour: compare_results, and each
    of the seven sectors solved alone by lk_correlate has the bytes it has in the batch"""
    si.assert_oracle_facts(oracle, model, interp)
    label = label_of(model, interp, "batch invariant")
    run = si.run_batch(oracle, model, interp, "batch_invariant", None, monkeypatch, alone=range(si.S))
    assert run["groups"] == list(si.NATURAL_GROUPS) and run["team"] == [0] * si.S, (label, run["groups"])
    starved = si.check_report(run["report"], model, interp, si.classes_of(si.NATURAL_GROUPS), SAFE, safe_pass=False, persistent=0,
                              label=label)
    assert starved == (model == ca.FM_UVUXUYVXVY)
    PARITY.compare_results(run["records"], si.yardsticks(oracle, model, interp), label)
    si.MEASURED[model, interp, "16 / 32 / 64 by class", SAFE] = si.deviations(run["records"], si.oracle_records(oracle, model, interp))
    for s, one, report in run["alone"]:
        si.check_report(report, model, interp, [(si.NATURAL_GROUPS[s], 1)], SAFE, safe_pass=False, label=f"{label} sector {s} alone")
        assert one.tobytes() == run["records"][s].tobytes(), (label, s, one, run["records"][s])


@pytest.mark.parametrize("threads", [1, 20])
@CASES
def test_reference_order_mode_is_the_oracles_bytes(oracle, monkeypatch, model, interp, threads):
    """the 16-lane row instance for sectors 0 and 1, the wavefront instance for the rest; the records of the batch and of
    every sector solved alone are the oracle's bytes for the same number of threads"""
    si.assert_oracle_facts(oracle, model, interp)
    want = si.oracle_records(oracle, model, interp, threads=threads)
    label = label_of(model, interp, f"reference order T={threads}")
    run = si.run_batch(oracle, model, interp, f"reference_order:{threads}", None, monkeypatch, alone=range(si.S))
    assert run["groups"] == list(si.REFERENCE_GROUPS) and run["team"] == [0] * si.S, (label, run["groups"])
    # (classes: sectors 0, 1 - sectors 2, 4, 5, 6 - sector 3; the last two both take a wavefront per sector)
    starved = si.check_report(run["report"], model, interp, [(16, 2), (64, 4), (64, 1)], REF, safe_pass=False, persistent=0, label=label)
    assert not starved          # (the ordered kernel is its own starved-level kernel below 131072 sectors)
    REFORDER.assert_same_bytes(run["records"], want, label)
    for s, one, report in run["alone"]:
        si.check_report(report, model, interp, [(si.REFERENCE_GROUPS[s], 1)], REF, safe_pass=False, label=f"{label} sector {s} alone")
        REFORDER.assert_same_bytes(one, want[s], f"{label} sector {s} alone")


@pytest.fixture(scope="module")
def blob768(oracle):
    return big_blob(oracle)


def big_blob(oracle):
    """test_reference_order_team_with_thread_chunks_of_a_sample_or_none's pair and blob: 65536 to 262144 samples, the
    one-workgroup class - a team of T workgroups in reference-order mode"""
    pair = ca.speckle.speckle_pair(768, 768, p=(0.9, 0.4, 0.001, 0.0005, -0.0005, 0.0015), seed=21)
    t = 2 * np.pi * np.arange(24) / 24
    rad = np.where(np.arange(24) % 2 == 0, 190.0, 130.0)
    contour = np.stack([384 + rad * np.cos(t), 384 + rad * np.sin(t)], 1).astype(np.float32)
    pts = oracle.blob_points(contour)
    assert 65536 < len(pts) < 262144
    return pair, contour, pts


@CASES
def test_reference_order_team_of_512_thread_workgroups(oracle, blob768, model, interp):
    """the reference-order instance of the 512-thread workgroup, as a team of T = 64 workgroups with one thread chunk of
    the reference each (pyramid 0 to 3): the oracle's bytes"""
    pair, contour, pts = blob768
    threads = 64
    e, o = REFORDER.engine_and_oracle(oracle, pair, model=model, interp=interp, threads=threads, py_stop=3)
    e.resetPolygon_blob(0, contour)
    e.commit_sectors()
    groups, team = e.sector_groups()
    assert groups.tolist() == [512] and team.tolist() == [threads], (groups, team)
    got = e.correlate_all(si.ZERO)
    label = label_of(model, interp, f"reference-order team T={threads}")
    si.check_report(e.launch_report(), model, interp, [(512, 1)], REF, safe_pass=False, persistent=0, team_w=threads, label=label)
    e.close()
    want = o.correlate_sectors([pts])
    o.close()
    REFORDER.assert_same_bytes(got, want, label)
    assert got["error_code"][0] == 0


# ---- the persistent sector queue: LK_FORCE_PERSISTENT is read once per process ----------------------------------------------
CHILD = r"""
import sys
import numpy as np
import correlation_amd as ca
from oracle import lk_oracle as oracle
import solve_instances_ref as si

oracle.lib()
KEYS = ("model", "interp", "group", "threads", "flavour", "seq", "role", "sectors", "team_w", "persistent", "grid")
out = {}
for (model, interp), case in zip(si.CASES, si.CASE_IDS):
    runs = [("batch_invariant", "batch_invariant", None), ("reference_order", "reference_order:1", None)]
    runs += [("default_" + name, "default", env) for name, env, group, team_w in si.FORCED[:3]]
    for name, mode, env in runs:
        run = si.run_batch(oracle, model, interp, mode, env)
        out[case + "_" + name + "_records"] = run["records"]
        out[case + "_" + name + "_report"] = np.int32([[r[k] for k in KEYS] for r in run["report"]])
np.savez(sys.argv[1], **out)
"""
REPORT_KEYS = ("model", "interp", "group", "threads", "flavour", "seq", "role", "sectors", "team_w", "persistent", "grid")
_child = {}


def persistent_child(tmp_path_factory):
    """all 12 cases in batch-invariant and reference-order mode (natural groups) and in default mode with 16, 32 and 64 lanes
    forced, by ONE child process with LK_FORCE_PERSISTENT=1"""
    if not _child:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests")]), LK_FORCE_PERSISTENT="1")
        for k in ("LK_FORCE_GROUP", "LK_FORCE_TEAM", "LK_FORCE_SAFE"):
            env.pop(k, None)
        out = tmp_path_factory.mktemp("solve_instances") / "persistent.npz"
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", CHILD, str(out)]
        try:      # the child runs ONCE: a failure is kept and fails the other cases from here, no second child is started
            done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            _child["failure"] = None if done.returncode == 0 else f"exit status {done.returncode}\n{done.stdout}{done.stderr}"
        except subprocess.TimeoutExpired as ex:
            _child["failure"] = f"no result after {ex.timeout} s"
        if _child["failure"] is None:
            _child.update(np.load(out))
    assert _child["failure"] is None, "the child process with LK_FORCE_PERSISTENT=1 failed: " + _child["failure"]
    return _child


@CASES
def test_persistent_sector_queue(oracle, monkeypatch, tmp_path_factory, model, interp):
    """workgroups that draw their sectors from the queue instead of taking them by position: in the two invariant modes the
    bytes of this process's non-persistent launches, in default mode within compare_results; every main launch of the
    child reports persistent = 1"""
    si.assert_oracle_facts(oracle, model, interp)
    child = persistent_child(tmp_path_factory)
    case = si.CASE_IDS[si.CASES.index((model, interp))]

    def child_run(name, mains, flavour):
        report = [dict(zip(REPORT_KEYS, (int(v) for v in row))) for row in child[f"{case}_{name}_report"]]
        si.check_report(report, model, interp, mains, flavour, safe_pass=flavour == FAST, persistent=1, label=f"{case} {name} persistent")
        return child[f"{case}_{name}_records"]

    for name, mode, mains, flavour in (("batch_invariant", "batch_invariant", si.classes_of(si.NATURAL_GROUPS), SAFE),
                                       ("reference_order", "reference_order:1", [(16, 2), (64, 4), (64, 1)], REF)):
        got = child_run(name, mains, flavour)
        here = si.run_batch(oracle, model, interp, mode, None, monkeypatch)
        si.check_report(here["report"], model, interp, mains, flavour, safe_pass=False, persistent=0, label=f"{case} {name} by position")
        assert REFORDER.canonical(got).tobytes() == REFORDER.canonical(here["records"]).tobytes(), (case, name)
    yard = si.yardsticks(oracle, model, interp)
    for name, env, group, team_w in si.FORCED[:3]:
        got = child_run("default_" + name, [(group, si.S)], FAST)
        PARITY.compare_results(got, yard, f"{case} {name} lanes persistent")
        assert got["error_code"][si.LEAVES] == si.OUT_OF_IMAGE


# ---- 2. the evaluation kernel -----------------------------------------------------------------------------------------------
EVAL_GROUPS = (16, 32, 64, 256)


def level_inputs(oracle, o, want, s, lvl):
    """(undeformed level, deformed level, the sector's samples and centre at that level) as the oracle has them"""
    xy = si.lists(oracle)[s]
    lxy = xy if lvl == 0 else oracle.decimate(xy, lvl)
    inv = np.float32(1.0 / (1 << lvl))
    return o.get_level(0, lvl), o.get_level(1, lvl), lxy, np.float32(want["und_cx"][s]) * inv, np.float32(want["und_cy"][s]) * inv


def check_evaluations(oracle, monkeypatch, model, interp, reference, label):
    """every sector at every level in the four lane groups of lk_eval_kernel.  reference(s, lvl, engine) -> (terms [n][44]
    or None where the sector leaves the image, expected error flag).  Returns {group: worst error / bound}."""
    worst = {}
    cache = {}
    for group in EVAL_GROUPS:
        with si.Hooks(monkeypatch, {"LK_FORCE_GROUP": group}):
            e = si.make_engine(oracle, model, interp)
        assert e.sector_groups()[0].tolist() == [group] * si.S
        worst[group] = 0.0
        for s in range(si.S):
            for lvl in (0, 1, 2):
                if (s, lvl) not in cache:
                    cache[s, lvl] = reference(s, lvl, e)
                terms, flag = cache[s, lvl]
                A, b, chi, err = e.evaluate(s, lvl, si.eval_parameters(model, lvl))
                report = e.launch_report()
                assert len(report) == 1 and report[0]["role"] == ca.LAUNCH_EVAL, report
                r = report[0]
                assert (r["model"], r["interp"], r["group"], r["threads"], r["seq"], r["flavour"]) == (model, interp, group, 256, 0, FAST), \
                    (label, group, r)
                si.SEEN.add(("eval", model, interp, group, FAST))
                assert terms is None or e.sector_level_count(s, lvl) == len(terms), (label, s, lvl)
                assert bool(err) == flag, (label, group, s, lvl, err, flag)
                if terms is None:
                    continue
                total, bound = si.sum_bound(terms, group)
                off = np.abs(si.pack_sums(A, b, chi) - total)
                assert (off <= bound).all(), (label, group, s, lvl, np.flatnonzero(off > bound), off[off > bound], bound[off > bound])
                worst[group] = max(worst[group], float((off[bound > 0] / bound[bound > 0]).max()))
        e.close()
    print(f"{label}: evaluation sums, worst error over bound per lane group {worst}")
    for group, w in worst.items():
        si.EVAL_WORST[model, interp, group] = w
    return worst


@CASES
def test_evaluation_sums_in_every_lane_group(oracle, monkeypatch, model, interp):
    """A, b and chi of evaluate(sector, level, p) for sectors 0 to 5 at the three levels, 16, 32, 64 and 256 lanes: each sum
    within c 2^-24 sum |term| of the float64 sum of the float terms (c: the group's longest addition chain,
    solve_instances_ref.sum_bound), the terms from the oracle's sampler - and oracle.evaluate's own sequential float sums
    within the same bound for one chain over all samples.  Sector 6: the error flag is the oracle's at every level."""
    want = si.assert_oracle_facts(oracle, model, interp)
    und, dfm = si.frames()
    o = oracle.Oracle(interp=interp, model=model)
    o.set_image(0, und)
    o.set_image(1, dfm)

    def reference(s, lvl, e):
        ul, dl, lxy, cx, cy = level_inputs(oracle, o, want, s, lvl)
        p = si.eval_parameters(model, lvl)
        Ao, bo, chio, erro = oracle.evaluate(interp, model, ul, dl, lxy, cx, cy, p)
        if s == si.LEAVES:
            if lvl == 2:
                assert erro != 0
            return None, bool(erro)
        terms, flagged = si.eval_terms(oracle, interp, model, ul, dl, lxy, cx, cy, p)
        assert not flagged and erro == 0, (s, lvl)
        total, bound = si.sum_bound(terms, 0)
        assert (np.abs(si.pack_sums(Ao, bo, chio) - total) <= bound).all(), (s, lvl)
        return terms, False

    check_evaluations(oracle, monkeypatch, model, interp, reference, label_of(model, interp))
    o.close()


@pytest.mark.parametrize("model", si.MODELS, ids=[si.MODEL_NAME[m] for m in si.MODELS])
def test_evaluation_sums_with_the_separable_bicubic(oracle, monkeypatch, model):
    """the extension the oracle has no sampler for: value and gradient from e.sample (test_separable_bicubic_extension pins
    it), the same sums, bound and groups"""
    interp = ca.IM_BICUBIC_SEPARABLE
    want = si.assert_oracle_facts(oracle, model, ca.IM_BICUBIC)      # (for the centres)
    und, dfm = si.frames()
    o = oracle.Oracle(interp=ca.IM_BICUBIC, model=model)
    o.set_image(0, und)
    o.set_image(1, dfm)

    def reference(s, lvl, e):
        ul, dl, lxy, cx, cy = level_inputs(oracle, o, want, s, lvl)
        terms, flagged = si.eval_terms(oracle, interp, model, ul, dl, lxy, cx, cy, si.eval_parameters(model, lvl),
                                       sampler=lambda pts: e.sample(ca.IMG_DEF, lvl, pts))
        assert flagged if (s == si.LEAVES and lvl == 2) else (not flagged or s == si.LEAVES), (s, lvl, flagged)
        return (None if flagged else terms), flagged

    check_evaluations(oracle, monkeypatch, model, interp, reference, label_of(model, interp))
    o.close()


# ---- 3. windows: the SEQ instances ------------------------------------------------------------------------------------------
def window_engine(oracle, model, interp, mode):
    return si.make_engine(oracle, model, interp, mode, sectors=si.WINDOW_SECTORS, pair=si.window_frames()[:2])


def run_window(oracle, model, interp, mode, env, monkeypatch):
    """(records [4][6] of one frame-pipelined window, its launch report, windows solved again SAFE)"""
    fr = si.window_frames()
    with si.Hooks(monkeypatch, env):
        e = window_engine(oracle, model, interp, mode)
        e.sequence_reserve(si.WINDOW_FRAMES)
        for i in range(si.WINDOW_FRAMES):
            e.sequence_set_frame(i, fr[i + 1])
        e.adjust_initial_guess(0, True, si.ZERO, si.WINDOW_CENTER)
        rec = e.correlate_sequence(si.WINDOW_FRAMES, first_slot=0, constant_velocity=True)
        assert e.sequence_is_pipelined
        report, reruns = e.launch_report(), e.stats()["window_safe_reruns"]
        e.close()
    return rec, report, reruns


def run_loop(oracle, model, interp, mode, env, monkeypatch):
    """the same frames one pair at a time on an engine of the same mode and hooks"""
    fr = si.window_frames()
    with si.Hooks(monkeypatch, env):
        e = window_engine(oracle, model, interp, mode)
        rec = []
        for k in range(si.WINDOW_FRAMES):
            e.set_deformed_image(fr[k + 1])
            e.adjust_initial_guess(k, True, si.ZERO, si.WINDOW_CENTER)
            rec.append(e.correlate_all(None))
        e.close()
    return np.stack(rec)


def window_hooks(model, group):
    """Sector 0's top level (9 samples) is starved under the six-parameter model, and a class with such a sector runs a window
    on the 16-lane rows in the SAFE flavour whatever its group: LK_STARVED_MAX=none (no level is starved; read by the commit)
    lets that model reach the other SEQ instances on the same sectors."""
    env = {"LK_FORCE_GROUP": group} if group else {}
    if model == ca.FM_UVUXUYVXVY:
        env["LK_STARVED_MAX"] = "none"
    return env


@CASES
def test_reference_order_window_is_the_oracles_frame_loop(oracle, monkeypatch, model, interp):
    """four frames at 1, 2, 3 and 4 times the truth over sectors 0 to 5 in one window: the SEQ reference-order instances of
    16 and 64 lanes, every frame the bytes of the oracle's frame loop"""
    want = si.oracle_window(oracle, model, interp)
    assert (want["error_code"] == 0).all()
    label = label_of(model, interp, "reference-order window")
    got, report, reruns = run_window(oracle, model, interp, "reference_order:1", None, monkeypatch)
    si.check_report(report, model, interp, [(16, 2), (64, 3), (64, 1)], REF, seq=1, safe_pass=False, persistent=1, label=label)
    assert reruns == 0
    for f in range(si.WINDOW_FRAMES):
        REFORDER.assert_same_bytes(got[f], want[f], f"{label} frame {f}")


@CASES
def test_batch_invariant_window_is_the_one_pair_loops_bytes(oracle, monkeypatch, model, interp):
    """the SEQ SAFE instances: the lane group of every sector's own class, then 16, 32 and 64 lanes forced - every frame the
    bytes of the one-pair loop of an engine with the same hooks"""
    for group in (0, 16, 32, 64):
        env = window_hooks(model, group) if group else {}
        label = label_of(model, interp, f"batch-invariant window, {group or 'natural'} lanes")
        got, report, reruns = run_window(oracle, model, interp, "batch_invariant", env, monkeypatch)
        mains = [(group, 6)] if group else si.classes_of(si.NATURAL_GROUPS, si.WINDOW_SECTORS)
        si.check_report(report, model, interp, mains, SAFE, seq=1, safe_pass=False, persistent=1, label=label)
        assert reruns == 0
        loop = run_loop(oracle, model, interp, "batch_invariant", env, monkeypatch)
        assert (loop["error_code"] == 0).all()
        for f in range(si.WINDOW_FRAMES):
            assert got[f].tobytes() == loop[f].tobytes(), f"{label}: records of frame {f}"


@CASES
def test_default_mode_window_stays_with_the_loop(oracle, monkeypatch, model, interp):
    """the SEQ fast instances with 16, 32 and 64 lanes forced (their gated SAFE pass is launched behind them and leaves at once:
    no window is solved again): test_sequence_window_gpu's comparison of the same name with the one-pair loop"""
    for group in (16, 32, 64):
        env = window_hooks(model, group)
        label = label_of(model, interp, f"default-mode window, {group} lanes")
        r_win, report, reruns = run_window(oracle, model, interp, "default", env, monkeypatch)
        si.check_report(report, model, interp, [(group, 6)], FAST, seq=1, safe_pass=True, persistent=1, label=label)
        assert reruns == 0
        r_loop = run_loop(oracle, model, interp, "default", env, monkeypatch)
        assert np.array_equal(r_win["error_code"], r_loop["error_code"])
        ok = r_loop["error_code"] == 0
        assert ok.all()
        assert np.abs(r_win["p"] - r_loop["p"])[ok][:, :2].max() < 2e-3
        assert (np.abs(r_win["iterations"] - r_loop["iterations"])[ok] <= 1).mean() > 0.99
