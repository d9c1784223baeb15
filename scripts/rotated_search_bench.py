"""HIP-event times of the rotation-aware automatic guess (lk_search_rotated) on the bench configurations - C2 at level 2,
R 16 and C4 at level 1, R 8, with 1, 13 and 37 angles - each beside lk_search_guesses at the same level and radius on the
same box, with the status counts.  One JSON line per case (median of --reps timed calls after a warm-up).

    python scripts/rotated_search_bench.py                on the GPU: writes profiles/rotated_search_bench.txt
    python scripts/rotated_search_bench.py --resources    anywhere: VGPRs, LDS and scratch of the kernels of
                                                          csrc/lk_rotated_search.hip and csrc/lk_guess_search.hip, from a
                                                          compile with the resource remarks; asserts that
                                                          none uses scratch: writes
                                                          profiles/rotated_search_resources.txt"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "rotated_search_bench.txt")
OUT_RESOURCES = os.path.join(ROOT, "profiles", "rotated_search_resources.txt")
ANGLE_STEP = np.deg2rad(5.0)
N_HALF = (0, 6, 18)   # 1, 13, 37 angles


def kernel_usage(log):
    """{kernel: {remark: value}} of a -Rpass-analysis=kernel-resource-usage log (plain, not templated, kernels)"""
    usage, cur = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][\w \[\]/]*): (\w+) \[", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return usage


def resources():
    from correlation_amd import build
    lines = ["# python scripts/rotated_search_bench.py --resources",
             "kernel: VGPRs SGPRs(spill) scratch waves/SIMD LDS AGPRs VGPR-spill"]
    scratch = []
    flags = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage"]
    with tempfile.TemporaryDirectory() as tmp:
        for src, kernels in (("lk_rotated_search.hip", ("lk_rotated_search_kernel", "lk_rotated_reduce_kernel")),
                             ("lk_guess_search.hip", ("lk_guess_search_kernel",))):
            log = os.path.join(tmp, src + ".log")
            with open(log, "w") as f:
                subprocess.run([build.hipcc_path()] + flags + ["-c", src, "-o", os.path.join(tmp, src + ".o")], cwd=build.CSRC,
                               stderr=f, check=True)
            usage = kernel_usage(log)
            for kernel in kernels:
                u = next(v for k, v in usage.items() if kernel in k)   # (the log has the mangled names)
                scratch.append(int(u["ScratchSize [bytes/lane]"]))
                lines.append("%-28s %s %s (%s) %s %s %s %s %s" % (kernel, u["VGPRs"], u["TotalSGPRs"], u["SGPRs Spill"],
                                                                u["ScratchSize [bytes/lane]"], u["Occupancy [waves/SIMD]"],
                                                                u["LDS Size [bytes/block]"], u["AGPRs"], u["VGPRs Spill"]))
    lines += ["# LDS above is the static part (the reduction arrays); the two search kernels add, per launch, 8 (2R+1)^2 bytes of",
              "# scores, 5120 bytes of template chunk and the staged window (up to 64 KB in all)",
              "# scratch, bytes per lane: at most %d over the %d kernels" % (max(scratch), len(scratch))]
    assert max(scratch) == 0, lines[-1]
    return lines


def timing(reps):
    import torch
    import correlation_amd as ca
    from correlation_amd.workload import C2, C4
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    stream = torch.cuda.Stream()   # the engine runs on it, the events are recorded on it
    lines = []
    for w, level, radius in ((C2, 2, 16), (C4, 1, 8)):
        und, dfm = ca.speckle.speckle_pair(w.size, w.size, p=w.truth, seed=7, device="cuda")
        e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
        e.set_stream(stream.cuda_stream)
        e.set_undeformed_image(und)
        e.set_deformed_image(dfm)
        e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
        e.commit_sectors()
        zero = np.zeros((e.n_sectors, 6), np.float32)

        def timed(upload, run):
            times = []
            for r in range(reps + 2):
                upload()   # (uploads the centres: every call searches the same)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                run()
                t1.record(stream)
                e.synchronize()
                torch.cuda.synchronize()
                if r >= 2:
                    times.append(t0.elapsed_time(t1))
            return float(np.median(times)), float(np.min(times))

        plain = timed(lambda: e.search_guesses(radius, level=level, guesses=zero), lambda: e.search_guesses(radius, level=level))
        info = e.guess_search_info()
        row = {"case": w.name.split(":")[0], "level": level, "radius": radius, "sectors": e.n_sectors, "pass": "lk_search_guesses",
               "ms_median": plain[0], "ms_min": plain[1], "status_counts": np.bincount(info["status"], minlength=6).tolist()}
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        for n_half in N_HALF:
            rot = timed(lambda: e.search_rotated(radius, ANGLE_STEP, n_half, level=level, guesses=zero),
                        lambda: e.search_rotated(radius, ANGLE_STEP, n_half, level=level))
            info = e.rotated_search_info()
            row = {"case": w.name.split(":")[0], "level": level, "radius": radius, "sectors": e.n_sectors, "pass": "lk_search_rotated",
                   "angles": 2 * n_half + 1, "ms_median": rot[0], "ms_min": rot[1], "times_plain": rot[0] / plain[0],
                   "status_counts": np.bincount(info["status"], minlength=6).tolist(),
                   "angle_index_counts": np.bincount(info["angle_index"] + n_half, minlength=2 * n_half + 1).tolist()}
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        e.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    if args.resources:
        lines = resources()
        print("\n".join(lines), flush=True)
    else:
        lines = ["# python scripts/rotated_search_bench.py --reps %d: HIP events on the engine's stream, median of the timed calls (ms);"
                 % args.reps, "# angle step 5 degrees about 0; status_counts: OK, TEXTURELESS, NO_CANDIDATE, TOO_FEW, TOO_LARGE, WEAK"]
        lines += timing(args.reps)
    if not args.no_write:
        with open(OUT_RESOURCES if args.resources else OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
