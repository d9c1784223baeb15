"""Backward (inverse-compositional) against forward update on the bench configurations, one pair at a time, on the same
pair, the two modes alternated within one process: C2, C4 and (correctness and time) C3.  Per mode: HIP-event solve ms
(median of --reps), mean iterations / evaluations / sample evaluations per sector, point-iterations/s, the largest
parameter difference between the modes and against the speckle ground truth.  Writes profiles/backward_bench.txt (one
JSON line per case) unless --no-write.  --only CASE --mode forward|backward --reps K runs one mode of one case (the
kernel-time run under rocprofv3 --kernel-trace --stats).  Usage: python scripts/backward_bench.py"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import correlation_amd as ca  # noqa: E402
from correlation_amd.workload import C2, C4  # noqa: E402

C3_TRUTH = (1.1, 0.6, 0.0008, 0.0004, -0.0004, 0.0012)


def rect_case(w):
    und, dfm = ca.speckle.speckle_pair(w.size, w.size, p=w.truth, seed=7, device="cuda")
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    return e, w.truth, w.size / 2.0


def c3_case():
    und, dfm = ca.speckle.speckle_pair(4096, 4096, p=C3_TRUTH, seed=11, device="cuda")
    e = ca.HipCorrelationEngine(fitting_model=ca.FM_UVUXUYVXVY)
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    rs, as_, ri, ro = 8, 32, 600.0, 1800.0
    dr, da = np.float32((ro - ri) / rs), np.float32(2 * np.pi) / np.float32(as_)
    e.set_sectors_annular(0, np.float32([[np.float32(ri + i * dr), dr, np.float32(j) * da, da, 2048.0, 2048.0]
                                         for i in range(rs) for j in range(as_)]), as_)
    t = 2 * np.pi * np.arange(64) / 64
    rad = np.where(np.arange(64) % 2 == 0, 1500.0, 900.0)
    e.resetPolygon_blob(rs * as_, np.stack([2048 + rad * np.cos(t), 2048 + rad * np.sin(t)], 1).astype(np.float32))
    e.commit_sectors()
    return e, C3_TRUTH, 2048.0


CASES = {"C2": lambda: rect_case(C2), "C4": lambda: rect_case(C4), "C3": c3_case}


def run(e, mode, zero):
    e.set_update(mode)
    r = e.correlate_all(zero)
    st = e.stats()
    return r, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None)
    ap.add_argument("--mode", default=None, choices=[None, "forward", "backward"])
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    modes = {"forward": ca.UPDATE_FORWARD, "backward": ca.UPDATE_BACKWARD}
    lines = []
    for name in ([args.only] if args.only else ["C2", "C4", "C3"]):
        e, truth, c0 = CASES[name]()
        zero = np.zeros((e.n_sectors, 6), np.float32)
        if args.mode:  # one mode only (kernel-time runs)
            for _ in range(args.reps):
                run(e, modes[args.mode], zero)
            e.close()
            continue
        ms = {"forward": [], "backward": []}
        rec, st = {}, {}
        for k in range(args.reps + 1):   # alternated: forward, backward, forward, ... (the first round warms up)
            for m in ("forward", "backward"):
                r, s = run(e, modes[m], zero)
                if k > 0:
                    ms[m].append(s["solve_ms"])
                rec[m], st[m] = r, s
        out = {"case": name, "sectors": e.n_sectors, "reps": args.reps}
        for m in ("forward", "backward"):
            r, s = rec[m], st[m]
            ok = r["error_code"] == 0
            u = truth[0] + truth[2] * (r["und_cx"] - c0) + truth[3] * (r["und_cy"] - c0)
            v = truth[1] + truth[4] * (r["und_cx"] - c0) + truth[5] * (r["und_cy"] - c0)
            med = float(np.median(ms[m]))
            out[m] = {"solve_ms_median": med, "solve_ms_min": float(np.min(ms[m])),
                      "mean_iterations": float(r["iterations"].mean()),
                      "evaluations_per_sector": s["evaluations"] / e.n_sectors,
                      "sample_evaluations_per_sector": s["sample_evaluations"] / e.n_sectors,
                      "point_iterations_per_s": s["point_iterations"] / (med * 1e-3),
                      "error_counts": np.bincount(r["error_code"], minlength=6).tolist(),
                      "max_abs_uv_minus_truth": float(max(np.abs(r["p"][ok, 0] - u[ok]).max(),
                                                          np.abs(r["p"][ok, 1] - v[ok]).max()))}
        both = (rec["forward"]["error_code"] == 0) & (rec["backward"]["error_code"] == 0)
        d = np.abs(rec["forward"]["p"][both] - rec["backward"]["p"][both])
        out["max_abs_duv_backward_vs_forward"] = float(d[:, :2].max())
        out["max_abs_dgrad_backward_vs_forward"] = float(d[:, 2:].max())
        out["p99_abs_duv_backward_vs_forward"] = float(np.quantile(d[:, :2].max(1), 0.99))
        out["speedup_backward"] = out["forward"]["solve_ms_median"] / out["backward"]["solve_ms_median"]
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))
        e.close()
    if lines and not args.no_write:
        with open(os.path.join(ROOT, "profiles", "backward_bench.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
