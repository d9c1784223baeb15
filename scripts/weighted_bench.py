"""The weighted refinement (lk_refine_weighted) beside lk_refine_znssd on the scene of
scripts/znssd_bench.py: config 2's pair, 2048 x 2048, 10 000 sectors of 19 x 19, six parameters.  Four passes run on one
engine from the same seeds - the engine-held records of a converged solve - with the calls alternating: lk_refine_znssd, and
lk_refine_weighted with sigma = 0 (every weight 1: the cost of the policy alone), with sigma = 19 / 6, and with a mask that
drops every fourth column of the image and no window.  Per pass the median of `reps` HIP-event times of the device part
(lk_internal_*_last), the median host time of the synchronous call (the mask's upload is part of it), trips and evaluations
per sector, the status histogram and the ratio to lk_refine_znssd.  No time is asserted.

    python scripts/weighted_bench.py [--reps K]     on the GPU: writes profiles/weighted_bench.txt
    python scripts/weighted_bench.py --resources    anywhere: VGPRs, LDS and scratch of every instance of lk_weighted_kernel,
                                                    from a compile of csrc/lk_weighted.hip with the resource remarks through
                                                    scripts/resource_usage.py; asserts that no instance uses scratch: writes
                                                    profiles/weighted_resources.txt"""
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
OUT = os.path.join(ROOT, "profiles", "weighted_bench.txt")
OUT_RESOURCES = os.path.join(ROOT, "profiles", "weighted_resources.txt")


def resources():
    from correlation_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        log = os.path.join(tmp, "usage.log")
        flags = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
                 "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage"]
        with open(log, "w") as f:
            subprocess.run([build.hipcc_path()] + flags + ["-c", "lk_weighted.hip", "-o", os.path.join(tmp, "lk_weighted.o")],
                           cwd=build.CSRC, stderr=f, check=True)
        mine = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "resource_usage.py"), log, "lk_weighted_kernel"],
                              capture_output=True, text=True, check=True).stdout.splitlines()
    # a row: "<template arguments>  VGPRs SGPRs (spill) scratch waves/SIMD LDS AGPRs VGPR-spill"
    scratch = [int(r.split()[-5]) for r in mine[1:]]
    lines = ["# python scripts/weighted_bench.py --resources",
             "# MODEL (0 u, 1 uv, 2 uvq, 3 six parameters), INTERP (0 nearest, 1 bilinear, 2 bicubic, 3 separable bicubic), GROUP"] + mine
    lines += ["# scratch, bytes per lane: at most %d over the %d instances" % (max(scratch), len(scratch))]
    assert len(mine) == 49 and max(scratch) == 0, lines[-1]
    return lines


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
    zero = np.zeros((e.n_sectors, 6), np.float32)
    for _ in range(3):
        e.correlate_all(zero)
    mask = np.ones((w.size, w.size), np.uint8)
    mask[:, 3::4] = 0
    passes = {"lk_refine_znssd": (lambda: e.refine_znssd(), e.znssd_last),
              "lk_refine_weighted sigma 0": (lambda: e.refine_weighted(), e.weighted_last),
              "lk_refine_weighted sigma 19/6": (lambda: e.refine_weighted(sigma=19.0 / 6.0), e.weighted_last),
              "lk_refine_weighted mask": (lambda: e.refine_weighted(mask=mask), e.weighted_last)}
    dev, call, last = ({k: [] for k in passes} for _ in range(3))
    for k in range(reps + 2):   # (the first two warm up; the passes alternate)
        for name, (run, hook) in passes.items():
            t0 = time.perf_counter()
            rec, info = run()   # synchronous: ends in a stream synchronise; seeds: the engine-held records
            t1 = time.perf_counter()
            ms, count = hook()
            last[name] = (info, count)
            if k >= 2:
                dev[name].append(ms)
                call[name].append((t1 - t0) * 1e3)
    lines = []
    base = float(np.median(dev["lk_refine_znssd"]))
    for name in passes:
        info, count = last[name]
        ran = info["evaluations"] > 0
        line = {"case": w.name, "pass": name, "seeds": "records of the converged solve", "sectors": e.n_sectors, "reps": reps,
                "sectors_per_lane_group_16_64_512": list(count), "device_ms_median": float(np.median(dev[name])),
                "device_ms_min": float(np.min(dev[name])), "call_ms_median": float(np.median(call[name])),
                "status_counts": np.bincount(info["status"], minlength=9).tolist(),
                "mean_trips": float(info["iterations"][ran].mean()), "mean_evaluations": float(info["evaluations"][ran].mean()),
                "zncc_median": float(np.median(info["zncc"][ran])), "device_over_znssd": float(np.median(dev[name])) / base}
        if "n_eff" in info.dtype.names:
            line["n_eff_median"] = float(np.median(info["n_eff"]))
            line["n_valid_median"] = float(np.median(info["n_valid"]))
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
    e.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    lines = resources() if args.resources else ["# python scripts/weighted_bench.py --reps %d" % args.reps] + timing(args.reps)
    if args.resources:
        print("\n".join(lines), flush=True)
    if not args.no_write:
        with open(OUT_RESOURCES if args.resources else OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
