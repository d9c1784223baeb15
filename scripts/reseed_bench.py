"""Recovery pass (lk_reseed_failed) on config 4 at full size, forward and backward mode: failed sectors before and after,
rounds, HIP-event time of the whole call next to the one-pair solve time of the same engine in the same run; and the
planning step alone (lk_reseed_plan) on a config-5-sized grid with 5 % of the records marked failed at random.  Writes
profiles/reseed_bench.txt (one JSON line per case) unless --no-write.  Kernel times of the planning kernels come from a
run of their own:  rocprofv3 --kernel-trace --stats -- python scripts/reseed_bench.py --only plan --no-write
Usage: python scripts/reseed_bench.py [--reps K]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import correlation_amd as ca  # noqa: E402
from correlation_amd.workload import C4, C5  # noqa: E402


def timed(e, stream, fn):
    """HIP-event time (ms) of fn() on the engine's stream, and its result"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e.synchronize()
    t0.record(stream)
    out = fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1), out


def solve_case(mode, reps):
    w = C4
    und, dfm = ca.speckle.speckle_pair(w.size, w.size, p=w.truth, seed=7, device="cuda")
    stream = torch.cuda.Stream()
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    e.set_stream(stream.cuda_stream)
    e.set_update(ca.UPDATE_BACKWARD if mode == "backward" else ca.UPDATE_FORWARD)
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    S = e.n_sectors
    zero = np.zeros((S, 6), np.float32)
    pitch = (w.x_end - w.x_begin) / w.hs
    radius = 2.5 * pitch
    solve_ms, call_ms = [], []
    for k in range(reps + 1):   # (the first round warms up)
        before = e.correlate_all(zero)
        s_ms = e.stats()["solve_ms"]
        ms, (after, n) = timed(e, stream, lambda: e.reseed_failed(radius, chi_max=0.0, min_neighbours=3, max_rounds=8))
        if k:
            solve_ms.append(s_ms)
            call_ms.append(ms)
    info = e.reseed_info()
    st = e.stats()
    out = {"case": "C4 " + mode, "sectors": S, "radius_px": radius, "min_neighbours": 3, "max_rounds": 8, "reps": reps,
           "failed_before": int((before["error_code"] != 0).sum()), "failed_after": int((after["error_code"] != 0).sum()),
           "recovered": int(n), "rounds_used": int(info["round"].max() + 1),
           "status_counts": np.bincount(info["status"], minlength=5).tolist(), "retry_solves": int(st["sectors"]),
           "one_pair_solve_ms_median": float(np.median(solve_ms)), "reseed_call_ms_median": float(np.median(call_ms)),
           "reseed_call_ms_min": float(np.min(call_ms))}
    e.close()
    return out


def plan_case(reps):
    w = C5
    stream = torch.cuda.Stream()
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    e.set_stream(stream.cuda_stream)
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    S = e.n_sectors
    rng = np.random.default_rng(3)
    rec = np.zeros(S, ca.RESULT_DTYPE)
    rec["p"] = rng.normal(0, 1, (S, 6)).astype(np.float32)
    rec["chi"] = 1.0
    rec["error_code"][rng.permutation(S)[:S // 20]] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
    pitch = (w.x_end - w.x_begin) / w.hs
    ms = []
    for k in range(reps + 1):
        t, (g, info) = timed(e, stream, lambda: e.reseed_plan(rec, 2.5 * pitch, min_neighbours=3))
        if k:
            ms.append(t)
    out = {"case": "C5-sized grid, plan alone (records up, classify, cell grid, plan, guesses and info down)", "sectors": S,
           "failed": int(S // 20), "planned": int((info["status"] == ca.RESEED_PLANNED).sum()),
           "mean_neighbours": float(info["neighbours"][info["status"] == ca.RESEED_PLANNED].mean()), "reps": reps,
           "plan_call_ms_median": float(np.median(ms)), "plan_call_ms_min": float(np.min(ms))}
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, choices=[None, "forward", "backward", "plan"])
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    lines = []
    for name in ([args.only] if args.only else ["forward", "backward", "plan"]):
        out = plan_case(args.reps) if name == "plan" else solve_case(name, args.reps)
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))
    if lines and not args.no_write:
        with open(os.path.join(ROOT, "profiles", "reseed_bench.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
