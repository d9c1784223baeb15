"""The second-order refinement (lk_refine_quadratic) next to the ZNSSD refinement (lk_refine_znssd) on config 2's pair:
2048 x 2048, 10 000 sectors of 19 x 19, bicubic, the seeds the engine-held records of a converged solve.  Both passes run
on the same engine in the same process, their calls alternating; per pass: the median of `reps` HIP-event times of the
call's kernels (lk_internal_*_last), the median host time of the whole synchronous call, the mean trips and evaluations
per sector and the status histogram; then the ratios of the two, per call and per evaluation.  No time is asserted.

    python scripts/quadratic_bench.py [--reps K]    on the GPU: writes profiles/quadratic_bench.txt
    python scripts/quadratic_bench.py --resources   anywhere: VGPRs, LDS and scratch of every instance of the kernel, from a
                                                    compile of csrc/lk_quadratic.hip with the resource remarks through
                                                    scripts/resource_usage.py, and the worst scratch of lk_znssd_kernel's
                                                    512-lane instances beside them: writes profiles/quadratic_resources.txt"""
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
OUT = os.path.join(ROOT, "profiles", "quadratic_bench.txt")
OUT_RESOURCES = os.path.join(ROOT, "profiles", "quadratic_resources.txt")


def usage_table(source, kernel):
    from correlation_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        log = os.path.join(tmp, "usage.log")
        flags = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
                 "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage"]
        with open(log, "w") as f:
            subprocess.run([build.hipcc_path()] + flags + ["-c", source, "-o", os.path.join(tmp, source + ".o")], cwd=build.CSRC,
                           stderr=f, check=True)
        return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "resource_usage.py"), log, kernel],
                              capture_output=True, text=True, check=True).stdout.splitlines()


def resources():
    mine = usage_table("lk_quadratic.hip", "lk_quadratic_kernel")
    theirs = usage_table("lk_znssd.hip", "lk_znssd_kernel")

    def scratch(rows, group):   # a row: "<template arguments, GROUP last>  VGPRs SGPRs (spill) scratch waves/SIMD LDS AGPRs VGPR-spill"
        return [int(r.split()[-5]) for r in rows[1:] if r.split()[-9] == str(group)]
    worst = max(scratch(theirs, 512))
    lines = ["# python scripts/quadratic_bench.py --resources",
             "# INTERP (0 nearest, 1 bilinear, 2 bicubic, 3 separable bicubic), GROUP"] + mine
    lines += ["# scratch, bytes per lane: 16-lane instances at most %d, 64-lane at most %d, 512-lane at most %d; the worst 512-lane "
              "instance of lk_znssd_kernel: %d" % (max(scratch(mine, 16)), max(scratch(mine, 64)), max(scratch(mine, 512)), worst)]
    assert max(scratch(mine, 16)) == 0 and max(scratch(mine, 64)) == 0 and max(scratch(mine, 512)) <= worst, lines[-1]
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
    S = e.n_sectors
    zero = np.zeros((S, 6), np.float32)
    for _ in range(3):
        e.correlate_all(zero)
    passes = {"lk_refine_znssd": (e.refine_znssd, e.znssd_last), "lk_refine_quadratic": (e.refine_quadratic, e.quadratic_last)}
    dev, call, last = {k: [] for k in passes}, {k: [] for k in passes}, {}
    seed_only = {k: [] for k in passes}   # max_iters = 0: one evaluation per sector and no step
    for k in range(reps + 2):   # (the first two warm up; the passes alternate)
        for name, (run, hook) in passes.items():
            t0 = time.perf_counter()
            rec, info = run()   # synchronous: ends in a stream synchronise; seeds: the engine-held records
            t1 = time.perf_counter()
            ms, count = hook()
            last[name] = (info, count)
            run(max_iters=0)
            if k >= 2:
                dev[name].append(ms)
                call[name].append((t1 - t0) * 1e3)
                seed_only[name].append(hook()[0])
    lines, per = [], {}
    for name in passes:
        info, count = last[name]
        ran = info["evaluations"] > 0
        per[name] = (float(np.median(dev[name])), float(info["evaluations"][ran].mean()))
        line = {"pass": name, "case": w.name, "seeds": "records of the converged solve", "sectors": S, "reps": reps,
                "sectors_per_lane_group_16_64_512": list(count), "device_ms_median": per[name][0], "device_ms_min": float(np.min(dev[name])),
                "device_ms_max": float(np.max(dev[name])), "call_ms_median": float(np.median(call[name])),
                "status_counts": np.bincount(info["status"], minlength=9).tolist(), "mean_trips": float(info["iterations"][ran].mean()),
                "mean_evaluations": per[name][1], "zncc_median": float(np.median(info["zncc"][ran])),
                "shift_median_px": float(np.median(info["shift"][ran]))}
        # one evaluation of every sector alone, and what a trip costs beyond its evaluation: the step on lane 0 and the hand-over
        ev_ms = float(np.median(seed_only[name]))
        line["seed_evaluation_only_device_ms_median"] = ev_ms
        line["per_trip_beyond_its_evaluation_ms"] = (per[name][0] - per[name][1] * ev_ms) / float(info["iterations"][ran].mean())
        if name == "lk_refine_quadratic":
            line["bend_median_px"] = float(np.median(info["bend"][ran]))
        lines.append(json.dumps(line))
    (zn_ms, zn_ev), (qd_ms, qd_ev) = per["lk_refine_znssd"], per["lk_refine_quadratic"]
    lines.append(json.dumps({"quadratic_over_znssd_device": qd_ms / zn_ms, "quadratic_over_znssd_device_per_evaluation": (qd_ms / qd_ev) / (zn_ms / zn_ev),
                             "quadratic_over_znssd_seed_evaluation_only": float(np.median(seed_only["lk_refine_quadratic"])) /
                             float(np.median(seed_only["lk_refine_znssd"]))}))
    e.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    lines = resources() if args.resources else ["# python scripts/quadratic_bench.py --reps %d" % args.reps] + timing(args.reps)
    print("\n".join(lines), flush=True)
    if not args.no_write:
        with open(OUT_RESOURCES if args.resources else OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
