"""The ZNSSD refinement (lk_refine_znssd) next to the one-pair solve on config 2's pair: 2048 x 2048, 10 000 sectors of
19 x 19, six parameters, bicubic.  Two cases: seeds = the engine-held records of a converged solve, and seeds = the guesses
of lk_search_guesses (radius 4 at level py_start about zero guesses; no solve needed).  Per case: the median of `reps`
HIP-event times of the call's kernels (lk_internal_znssd_last), the median host time of the whole synchronous call, the
mean trips and evaluations per sector, the status histogram, and beside them the forward solve's solve_ms on the same pair.
No time is asserted.

    python scripts/znssd_bench.py [--reps K]        on the GPU: the timing lines
    python scripts/znssd_bench.py --resources       anywhere: VGPRs, LDS and scratch of every instance of the kernel, from
                                                    a compile of csrc/lk_znssd.hip with the resource remarks through
                                                    scripts/resource_usage.py

Each mode rewrites its own section of profiles/znssd_bench.txt (unless --no-write) and keeps the other."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "znssd_bench.txt")
HEADS = {"timing": "# timing (python scripts/znssd_bench.py)", "resources": "# resources (python scripts/znssd_bench.py --resources)"}


def write_section(name, lines):
    sections = {"timing": [], "resources": []}
    if os.path.exists(OUT):
        cur = None
        for line in open(OUT).read().splitlines():
            if line in HEADS.values():
                cur = [k for k, v in HEADS.items() if v == line][0]
            elif cur:
                sections[cur].append(line)
    sections[name] = lines
    with open(OUT, "w") as f:
        for k in ("timing", "resources"):
            if sections[k]:
                f.write("\n".join([HEADS[k]] + sections[k]) + "\n")


def resources():
    from correlation_amd import build
    csrc = build.CSRC
    with tempfile.TemporaryDirectory() as tmp:
        log = os.path.join(tmp, "usage.log")
        flags = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
                 "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage"]
        with open(log, "w") as f:
            subprocess.run([build.hipcc_path()] + flags + ["-c", "lk_znssd.hip", "-o", os.path.join(tmp, "lk_znssd.o")], cwd=csrc,
                           stderr=f, check=True)
        table = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "resource_usage.py"), log, "lk_znssd_kernel"],
                               capture_output=True, text=True, check=True).stdout
    return ["# MODEL (0 u, 1 uv, 2 uvq, 3 six parameters), INTERP (0 nearest, 1 bilinear, 2 bicubic, 3 separable bicubic), GROUP"] + \
        table.splitlines()


def timing(reps):
    import torch
    import correlation_amd as ca
    from correlation_amd.workload import C2 as w
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    und, dfm = ca.speckle.speckle_pair(w.size, w.size, p=w.truth, seed=7, device="cuda")
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    S = e.n_sectors
    zero = np.zeros((S, 6), np.float32)
    guesses = e.search_guesses(4, level=0, guesses=zero)   # (before any solve: the pipeline without one)
    solve = []
    for k in range(6):   # (the first warms up)
        e.correlate_all(zero)
        if k:
            solve.append(e.stats()["solve_ms"])
    stats = e.stats()
    lines = []
    for case, kw in (("records of the converged solve", dict()), ("guesses of lk_search_guesses", dict(guesses=guesses))):
        dev, call = [], []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            rec, info = e.refine_znssd(**kw)   # synchronous: ends in a stream synchronise
            t1 = time.perf_counter()
            ms, count = e.znssd_last()
            if k:
                dev.append(ms)
                call.append((t1 - t0) * 1e3)
        ran = info["evaluations"] > 0
        line = {"case": w.name, "seeds": case, "sectors": S, "reps": reps, "sectors_per_lane_group_16_64_512": list(count),
                "device_ms_median": float(np.median(dev)), "device_ms_min": float(np.min(dev)), "call_ms_median": float(np.median(call)),
                "status_counts": np.bincount(info["status"], minlength=9).tolist(),
                "mean_trips": float(info["iterations"][ran].mean()), "mean_evaluations": float(info["evaluations"][ran].mean()),
                "zncc_median": float(np.median(info["zncc"][ran])), "shift_median_px": float(np.median(info["shift"][ran])),
                "one_pair_solve_ms_median": float(np.median(solve)), "solve_evaluations": int(stats["evaluations"]),
                "solve_sectors": int(stats["sectors"]), "device_over_solve": float(np.median(dev)) / float(np.median(solve))}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
    e.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    name = "resources" if args.resources else "timing"
    lines = resources() if args.resources else timing(args.reps)
    if args.resources:
        print("\n".join(lines))
    if not args.no_write:
        write_section(name, lines)


if __name__ == "__main__":
    main()
