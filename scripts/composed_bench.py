"""The composed refinement (lk_refine_composed) beside the four passes it combines, on the scene of
scripts/znssd_bench.py: config 2's pair, 2048 x 2048, 10 000 sectors of 19 x 19, six parameters.  All passes run on one
engine from the same seeds - the engine-held records of a converged solve - with the calls alternating.  Rows: the four
existing passes, then lk_refine_composed (order, sampler, weights) for the combinations no other pass has; `weights` is
sigma = 19 / 6 under a mask that drops every fourth column.  Per row the median of `reps` HIP-event times of the device part
(lk_internal_*_last; the coefficient image of a spline sampler is part of it), trips and evaluations per sector and the
status histogram.  Recorded figures: no time and no ratio is asserted.

    python scripts/composed_bench.py [--reps K]     on the GPU: writes profiles/composed_bench.txt
    python scripts/composed_bench.py --resources    anywhere: VGPRs, LDS and scratch of every instance of the kernels of
                                                    csrc/lk_composed.hip, from a compile with the resource remarks through
                                                    scripts/resource_usage.py; asserts that no instance uses scratch: writes
                                                    profiles/composed_resources.txt"""
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
OUT = os.path.join(ROOT, "profiles", "composed_bench.txt")
OUT_RESOURCES = os.path.join(ROOT, "profiles", "composed_resources.txt")
KERNELS = (("lk_composed_first_kernel", 24, "MODEL (0 u, 1 uv, 2 uvq, 3 six parameters), spline ORDER, GROUP"),
           ("lk_composed_second_kernel", 18,
            "SAMPLER (0 nearest, 1 bilinear, 2 bicubic, 3 separable bicubic, 11 cubic B-spline, 13 quintic B-spline), GROUP"))
# (lk_composed_info_kernel, a thread per sector that copies two records into one, is not a template and not listed)


def resources():
    from correlation_amd import build
    lines = ["# python scripts/composed_bench.py --resources"]
    worst, total = 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        log = os.path.join(tmp, "usage.log")
        flags = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
                 "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage"]
        with open(log, "w") as f:
            subprocess.run([build.hipcc_path()] + flags + ["-c", "lk_composed.hip", "-o", os.path.join(tmp, "lk_composed.o")],
                           cwd=build.CSRC, stderr=f, check=True)
        for kernel, instances, legend in KERNELS:
            mine = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "resource_usage.py"), log, kernel],
                                  capture_output=True, text=True, check=True).stdout.splitlines()
            # a row: "<template arguments>  VGPRs SGPRs (spill) scratch waves/SIMD LDS AGPRs VGPR-spill"
            scratch = [int(r.split()[-5]) for r in mine[1:]]
            assert len(scratch) == instances, (kernel, len(scratch), instances)
            worst, total = max([worst] + scratch), total + len(scratch)
            lines += ["# " + legend] + mine
    lines += ["# scratch, bytes per lane: at most %d over the %d instances" % (worst, total)]
    if worst != 0:
        print("\n".join(lines), flush=True)
    assert worst == 0, lines[-1]
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
    wt = dict(sigma=19.0 / 6.0, mask=mask)
    passes = {"lk_refine_znssd": (lambda: e.refine_znssd(), e.znssd_last),
              "lk_refine_quadratic": (lambda: e.refine_quadratic(), e.quadratic_last),
              "lk_refine_spline 5": (lambda: e.refine_spline(order=5), lambda: e.spline_last()[:2]),
              "lk_refine_weighted weights": (lambda: e.refine_weighted(**wt), e.weighted_last)}
    for order, sampler, weights in ((1, 5, True), (2, 0, False), (2, 0, True), (2, 3, False), (2, 5, False), (2, 5, True)):
        kw = dict(order=order, sampler=sampler, **(wt if weights else {}))
        passes["lk_refine_composed (%d, %d, %s)" % (order, sampler, "weights" if weights else "unit")] = (
            (lambda kw=kw: e.refine_composed(**kw)), e.composed_last)
    dev, last = ({k: [] for k in passes} for _ in range(2))
    for k in range(reps + 2):   # (the first two warm up; the passes alternate)
        for name, (run, hook) in passes.items():
            t0 = time.perf_counter()
            rec, info = run()   # synchronous: ends in a stream synchronise; seeds: the engine-held records
            t1 = time.perf_counter()
            ms, count = hook()
            last[name] = (info, count, (t1 - t0) * 1e3)
            if k >= 2:
                dev[name].append(ms)
    lines = []
    for name in passes:
        info, count, call_ms = last[name]
        ran = info["evaluations"] > 0
        line = {"case": w.name, "pass": name, "seeds": "records of the converged solve", "sectors": e.n_sectors, "reps": reps,
                "sectors_per_lane_group_16_64_512": list(count), "device_ms_median": float(np.median(dev[name])),
                "device_ms_min": float(np.min(dev[name])), "last_call_ms": call_ms,
                "status_counts": np.bincount(info["status"], minlength=9).tolist(),
                "mean_trips": float(info["iterations"][ran].mean()), "mean_evaluations": float(info["evaluations"][ran].mean())}
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
    lines = resources() if args.resources else ["# python scripts/composed_bench.py --reps %d" % args.reps] + timing(args.reps)
    if args.resources:
        print("\n".join(lines), flush=True)
    if not args.no_write:
        with open(OUT_RESOURCES if args.resources else OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
