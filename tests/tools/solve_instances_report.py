"""What tests/test_solve_instances_gpu.py measures, written down: the module's own checks run once in this process (same
fixture, same assertions - a failing check ends the script), then
  - the instances of lk_launch_solve, lk_launch_solve_seq and lk_launch_eval that the engine's launch reports named,
    counted against the instances compiled for the 12 (model, interpolator) cases the oracle covers, with the ones no run
    reached by name;
  - per (model, interpolator, lane group, flavour) of the one-pair solves the largest |d(u, v)| (px), |d gradients| and
    relative d chi against oracle(T = 1) on the sectors it solved - next to compare_results' floors of 5e-3 / 5e-5 / 5e-3,
    which nobody has measured against before;
  - per (model, interpolator, lane group) of the evaluation kernel the worst |sum - float64 sum of the float terms| over its
    rounding bound (solve_instances_ref.sum_bound).
Writes --out (default profiles/solve_instances.txt) unless --no-write.
(Under tests/tools/ like the other oracle-backed tools: nothing under scripts/ may touch the oracle.)
Usage: python tests/tools/solve_instances_report.py [--out PATH] [--commit TEXT] [--no-write]"""
import argparse
import datetime
import importlib.util
import io
import os
import contextlib
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import correlation_amd as ca  # noqa: E402
from oracle import lk_oracle as oracle  # noqa: E402
import solve_instances_ref as si  # noqa: E402


def load_tests():
    spec = importlib.util.spec_from_file_location("solve_instances_tests", os.path.join(ROOT, "tests", "test_solve_instances_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compiled():
    """the instances of the launchers for the oracle's 12 cases (lk_kernels.hip: launch_solve_mi / launch_solve_g,
    launch_solve_seq_mi) and every instance of launch_eval_m"""
    F, S, R = ca.FLAVOUR_FAST, ca.FLAVOUR_SAFE, ca.FLAVOUR_REFERENCE
    solve = [(1, F)] + [(g, f) for g in (16, 32, 64, 256, 512) for f in (F, S)] + [(g, R) for g in (16, 64, 512)]
    seq = [(g, f) for f in (F, S) for g in (16, 32, 64)] + [(g, R) for g in (16, 64)]
    out = {("solve", m, i, g, f) for m, i in si.CASES for g, f in solve}
    out |= {("seq", m, i, g, f) for m, i in si.CASES for g, f in seq}
    out |= {("eval", m, i, g, F) for m in si.MODELS for i in si.INTERPS + (ca.IM_BICUBIC_SEPARABLE,) for g in (16, 32, 64, 256)}
    return out


def name_of(key):
    kind, m, i, g, f = key
    return f"{kind} {si.MODEL_NAME[m]} {si.INTERP_NAME[i]} {g} lanes {si.FLAVOUR_NAME[f]}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_instances.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    oracle.lib()
    T = load_tests()
    log = io.StringIO()
    with contextlib.redirect_stdout(log):      # (the checks print every launch report: kept out of the way)
        blob = T.big_blob(oracle)
        for model, interp in si.CASES:
            for flavour in (ca.FLAVOUR_FAST, ca.FLAVOUR_SAFE):
                T.test_default_mode_in_every_forced_lane_group(oracle, None, model, interp, flavour)
            T.test_batch_invariant_mode_alone_and_in_the_batch(oracle, None, model, interp)
            for threads in (1, 20):
                T.test_reference_order_mode_is_the_oracles_bytes(oracle, None, model, interp, threads)
            T.test_reference_order_team_of_512_thread_workgroups(oracle, blob, model, interp)
            T.test_evaluation_sums_in_every_lane_group(oracle, None, model, interp)
            T.test_reference_order_window_is_the_oracles_frame_loop(oracle, None, model, interp)
            T.test_batch_invariant_window_is_the_one_pair_loops_bytes(oracle, None, model, interp)
            T.test_default_mode_window_stays_with_the_loop(oracle, None, model, interp)
        for model in si.MODELS:
            T.test_evaluation_sums_with_the_separable_bicubic(oracle, None, model)
    commit = args.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    want, seen = compiled(), si.SEEN
    lines = [f"# solve_instances_report.py, {datetime.date.today().isoformat()}, commit {commit or 'unknown'}",
             f"# fixture: {si.ROWS} x {si.COLS} speckle pair, truth {si.TRUTH}, sectors of {si.COUNTS} samples, pyramid 0 / 1 / 2"]
    for kind, what in (("solve", "lk_launch_solve"), ("seq", "lk_launch_solve_seq"), ("eval", "lk_launch_eval")):
        w = {k for k in want if k[0] == kind}
        lines.append(f"instances named by a launch report, {what}: {len(w & seen)} of {len(w)} compiled for these cases")
        for k in sorted(w - seen):
            lines.append(f"  not reached: {name_of(k)}")
        assert not {k for k in seen if k[0] == kind} - w, sorted({k for k in seen if k[0] == kind} - w)
    lines.append("")
    lines.append("one-pair solves against oracle(T = 1), largest over the six sectors it solves (floors: 5e-3 px, 5e-5, 5e-3)")
    lines.append(f"{'model':8s}{'interpolator':14s}{'lanes per sector':24s}{'flavour':8s}{'|d(u, v)| px':>14s}{'|d gradients|':>15s}{'chi rel':>11s}")
    for (m, i, group, f), (d01, d25, chi) in sorted(si.MEASURED.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][3], str(kv[0][2]).zfill(24))):
        lines.append(f"{si.MODEL_NAME[m]:8s}{si.INTERP_NAME[i]:14s}{group:24s}{si.FLAVOUR_NAME[f]:8s}{d01:14.2e}{d25:15.2e}{chi:11.2e}")
    worst = tuple(max(v[k] for v in si.MEASURED.values()) for k in range(3))
    lines.append(f"largest of all: |d(u, v)| {worst[0]:.2e} px, |d gradients| {worst[1]:.2e}, chi rel {worst[2]:.2e}")
    lines.append("")
    lines.append("evaluation sums: worst |sum - float64 sum of the float terms| / (c 2^-24 sum |term|), sectors 0-5, levels 0-2")
    lines.append(f"{'model':8s}{'interpolator':14s}" + "".join(f"{str(g) + ' lanes':>12s}" for g in T.EVAL_GROUPS))
    for m in si.MODELS:
        for i in si.INTERPS + (ca.IM_BICUBIC_SEPARABLE,):
            lines.append(f"{si.MODEL_NAME[m]:8s}{si.INTERP_NAME[i]:14s}" + "".join(f"{si.EVAL_WORST[m, i, g]:12.3f}" for g in T.EVAL_GROUPS))
    lines.append(f"largest of all: {max(si.EVAL_WORST.values()):.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if not args.no_write:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
