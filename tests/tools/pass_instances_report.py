"""What tests/test_pass_instances_gpu.py measures, written down: the module's own checks run once in this process (same
geometry, same assertions - a failing check is named in the output and its figures are those measured up to it), then
  - the instances of lk_launch_backward and lk_launch_backward_eval that the engine's launch reports named, counted against
    the 4 x 4 x 3 compiled of each;
  - one line per (pass, model, interpolator, lane group): the worst measured deviation as a fraction of its bound - for the
    backward solves |d(u, v)| (px), |d other parameters| and d chi against backward_ref's float64 run next to their bounds,
    the sectors the restatement settles and the iteration counts that differ;
  - per (model, interpolator) the largest restated step at the state a refinement returned, over its bound.
Writes --out (default profiles/pass_instances.txt) unless --no-write.
(Under tests/tools/ like the other oracle-backed tools: nothing under scripts/ may touch the oracle.)
Usage: python tests/tools/pass_instances_report.py [--out PATH] [--commit TEXT] [--no-write]"""
import argparse
import contextlib
import datetime
import importlib.util
import io
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import lk_oracle as oracle  # noqa: E402
import pass_instances_ref as pi  # noqa: E402
import znssd_ref as zr  # noqa: E402

GROUPS = (16, 64, 512)


def load_tests():
    spec = importlib.util.spec_from_file_location("pass_instances_tests", os.path.join(ROOT, "tests", "test_pass_instances_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pass_instances.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    oracle.lib()
    T = load_tests()
    pair = zr.pair()
    log, failed = io.StringIO(), []
    with contextlib.redirect_stdout(log):      # (the checks print every sector: kept out of the way)
        runs = [(test, (case,), pi.case_id(case)) for case in pi.CASES
                for test in (T.test_backward_evaluation, T.test_backward_whole_solves, T.test_backward_three_levels_from_zero,
                             T.test_uncertainty_and_photometry, T.test_znssd, T.test_weighted)]
        runs += [(test, c, str(c)) for c in T.SPLINE_CASES for test in (T.test_spline, T.test_composed_first)]
        runs += [(T.test_composed_second, c, str(c)) for c in T.SECOND_CASES]
        for test, a, label in runs:
            try:
                test(oracle, pair, *a)
            except AssertionError as err:
                failed.append(f"FAILED {test.__name__}[{label}]: {(str(err).splitlines() or [''])[0][:160]}")
    commit = args.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    name = lambda m, i: f"{pi.MODEL_NAME[m]:8s}{pi.INTERP_NAME[i]:11s}"  # noqa: E731
    lines = [f"# pass_instances_report.py, {datetime.date.today().isoformat()}, commit {commit or 'unknown'}",
             f"# geometry: 256 x 256 speckle pair, truth {zr.TRUTH}; sectors of {pi.counts()} level-0 samples, lane groups {pi.groups()}",
             f"# backward solves: levels {pi.BW_PY[2]} .. {pi.BW_PY[0]} from the seed {pi.NEAR.tolist()}"]
    lines += failed
    for what, launcher in (("backward solve", "lk_launch_backward"), ("backward eval", "lk_launch_backward_eval")):
        want = {(what, m, i, g) for m, i in pi.CASES for g in GROUPS}
        seen = {k for k in pi.SEEN if k[0] == what}
        lines.append(f"instances named by a launch report, {launcher}: {len(want & seen)} of {len(want)} compiled")
        assert seen == want, sorted(want ^ seen)
    lines.append("")
    lines.append("backward solves against backward_ref's float64 run on the settled sectors (bounds: 1e-4 px, 1e-6, 5e-5 chi + 1e-6)")
    lines.append(f"{'model':8s}{'interpolator':11s}{'lanes':>7s}{'|d(u, v)| px':>14s}{'|d others|':>12s}{'d chi / bound':>15s}{'settled':>9s}{'iterations differ':>19s}")
    for m, i in pi.CASES:
        for g in GROUPS:
            r = pi.MEASURED.get(("backward solve", m, i, g))
            if r is None:      # (the check failed before it noted the figures: its message is above)
                lines.append(f"{name(m, i)}{g:7d}   see the failed check above")
                continue
            lines.append(f"{name(m, i)}{g:7d}{r['duv']:14.2e}{r['rest']:12.2e}{r['chi']:15.3f}{r['settled']:5d} / {r['sectors']}{r['it_diff']:19d}")
    solves = [pi.MEASURED["backward solve", m, i, g] for m, i in pi.CASES for g in GROUPS if ("backward solve", m, i, g) in pi.MEASURED]
    lines.append(f"largest of all: |d(u, v)| {max(r['duv'] for r in solves):.2e} px, |d others| {max(r['rest'] for r in solves):.2e}, "
                 f"d chi / bound {max(r['chi'] for r in solves):.3f}; unsettled sectors {sum(r['sectors'] - r['settled'] for r in solves)}")
    lines.append("")
    lines.append("backward solves from a zero guess over the levels 2, 1, 0: the sectors the restatement settles (each compared, same bounds)")
    for m, i in pi.CASES:
        lines.append(f"{name(m, i)}{pi.MEASURED.get(('three levels settled', m, i, 0), 'see the failed check above')}")
    nan = float("nan")
    titles = (("backward eval", "backward evaluation: worst |H, b, chi - float64 sums| / (2e-5 max|ref| + 1e-3; 1e-2 for chi), levels 0-2"),
              ("uncertainty", "uncertainty sums: worst |sum - float64 sum of the float terms| / (64 n 2^-53 sum|term|)"),
              ("photometry", "photometry sums: the same"), ("znssd sums", "ZNSSD seed evaluation sums: the same"),
              ("weighted sums", "weighted seed evaluation sums (mask and Gaussian window): the same"))
    for what, title in titles:   # (nan: the check failed before it noted the figure; its message is above)
        lines.append("")
        lines.append(title)
        lines.append(f"{'model':8s}{'interpolator':11s}" + "".join(f"{str(g) + ' lanes':>12s}" for g in GROUPS))
        for m, i in pi.CASES:
            lines.append(name(m, i) + "".join(f"{pi.MEASURED.get((what, m, i, g), nan):12.4f}" for g in GROUPS))
        lines.append(f"largest of all: {max(v for k, v in pi.MEASURED.items() if k[0] == what):.4f}")
    lines.append("")
    lines.append("refinement loops: largest restated step at the returned state of a converged sector / (4 x precision)")
    lines.append(f"{'model':8s}{'interpolator':11s}{'ZNSSD':>12s}{'weighted':>12s}")
    for m, i in pi.CASES:
        lines.append(name(m, i) + f"{pi.MEASURED.get(('znssd fixed point', m, i, 0), nan):12.4f}"
                     f"{pi.MEASURED.get(('weighted fixed point', m, i, 0), nan):12.4f}")
    lines.append("")
    lines.append("spline and composed kernels, seed evaluation sums: worst |sum - float64 sum of the float terms| / (64 n 2^-53 sum|term|);")
    lines.append("the last column: largest restated step at the returned state of a converged sector / (4 x precision)")
    lines.append(f"{'kernel':17s}{'case':20s}" + "".join(f"{str(g) + ' lanes':>12s}" for g in GROUPS) + f"{'step':>12s}")
    for what, cases, first in (("spline", T.SPLINE_CASES, pi.MODEL_NAME), ("composed first", T.SPLINE_CASES, pi.MODEL_NAME),
                               ("composed second", T.SECOND_CASES, pi.INTERP_NAME)):
        for a, b in cases:
            label = f"{first[a]}, " + (f"order {b}" if what == "spline" else f"sampler {b}")
            lines.append(f"{what:17s}{label:20s}" + "".join(f"{pi.MEASURED.get((what + ' sums', a, b, g), nan):12.4f}" for g in GROUPS)
                         + f"{pi.MEASURED.get((what + ' fixed point', a, b, 0), nan):12.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if not args.no_write:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
