"""Per-sector uncertainty (lk_parameter_uncertainty) next to the one-pair solve it follows: config 2's grid (10 000 sectors
of 19 x 19) and config 4's grid (224 x 224 sectors of 7 x 7), records of a real solve, engine-held.  Per case: the median
of `reps` HIP-event times of the call's kernels, the median host time of the whole synchronous call (transfers included),
with and without the 28 sums copied out, the one-pair solve time of the same engine in the same process (lk_stats.solve_ms)
and its counters.  The yardstick is one evaluation's share of the solve, solve_ms * sectors / evaluations: the pass is one
evaluation per sector, with double sums; the ratio of its device time to that share is `device_over_one_evaluation`.
Writes profiles/uncertainty_bench.txt (one JSON line per run) unless --no-write.
Usage: python scripts/uncertainty_bench.py [--reps K] [--only c2|c4]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import correlation_amd as ca  # noqa: E402
from correlation_amd.workload import C2, C4  # noqa: E402


def last_call(e):
    ms, count = C.c_float(), (C.c_int * 3)()
    fn = e.lib.lk_internal_uncertainty_last   # (not part of the C ABI: the bench's window into the last call)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    assert fn(e._h, C.byref(ms), count) == 0
    return ms.value, list(count)


def make_engine(w):
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    und, dfm = ca.speckle.speckle_pair(w.size, w.size, p=w.truth, seed=7, device="cuda")
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    return e


def solve_of(e, reps):
    zero = np.zeros((e.n_sectors, 6), np.float32)
    ms = []
    for k in range(reps + 1):   # (the first warms up)
        e.correlate_all(zero)
        if k:
            ms.append(e.stats()["solve_ms"])
    return float(np.median(ms)), e.stats()


def runs(e, w, reps, solve_ms, stats):
    S = e.n_sectors
    share = solve_ms * stats["sectors"] / stats["evaluations"]
    lines, first = [], None
    for with_sums in (False, True):
        dev, call = [], []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            out = e.parameter_uncertainty(return_sums=with_sums)   # synchronous: ends in a stream synchronise
            t1 = time.perf_counter()
            ms, count = last_call(e)
            if k:
                dev.append(ms)
                call.append((t1 - t0) * 1e3)
        out = out[0] if with_sums else out
        if first is None:
            first = out
        assert out.tobytes() == first.tobytes()
        ok = out["status"] == ca.UNC_OK
        d = float(np.median(dev))
        line = {"case": w.name, "sectors": S, "sums_copied_out": with_sums, "reps": reps, "sectors_per_lane_group_16_64_512": count,
                "device_ms_median": d, "device_ms_min": float(np.min(dev)), "call_ms_median": float(np.median(call)),
                "status_counts": np.bincount(out["status"], minlength=5).tolist(),
                "sigma_u_median_px": float(np.median(out["sigma"][ok, 0])) if ok.any() else None,
                "noise_median": float(np.median(out["noise"][ok])) if ok.any() else None,
                "one_pair_solve_ms_median": solve_ms, "solve_evaluations": int(stats["evaluations"]),
                "solve_sectors": int(stats["sectors"]), "one_evaluation_share_ms": share,
                "device_over_one_evaluation": d / share, "device_over_solve": d / solve_ms,
                "call_over_solve": float(np.median(call)) / solve_ms}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None, choices=[None, "c2", "c4"])
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    lines = []
    for key, w in (("c2", C2), ("c4", C4)):
        if args.only in (None, key):
            e = make_engine(w)
            solve_ms, stats = solve_of(e, 5)
            lines += runs(e, w, args.reps, solve_ms, stats)
            e.close()
    if lines and not args.no_write:
        with open(os.path.join(ROOT, "profiles", "uncertainty_bench.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
