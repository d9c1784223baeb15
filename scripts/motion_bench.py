"""Global motion per frame (lk_rigid_motion) on config 2's geometry (10 000 sectors, the engine-held
records of one solved pair) and on config 4's (50 176 sectors, a solved 64-frame window read in place on the device).  Per
case LK_MOTION_RIGID, one pass, with and without records_out: the median of `reps` HIP-event times of the device part
(lk_internal_motion_last: pack, the four kernels of the pass, the removal - not the bounding box's round trip before it and
not the copies of the outputs) and of the whole synchronous call; beside it the same answer the long way round: the records
fetched to the host (hipMemcpy from the device pointer) and fitted in numpy.  From the byte count, how far the sums kernel's
share is from the HBM bound: the pass reads the 16-byte pack twice (sums, residuals) and the keep byte, after the pack
kernel has read the 48-byte records once.  Recorded figures: no time and no ratio is asserted.

    python scripts/motion_bench.py [--reps K] [--frames N]   on the GPU: writes profiles/motion_bench.txt
    python scripts/motion_bench.py --resources               anywhere: VGPRs, LDS and scratch of the kernels of csrc/lk_motion.hip
                                                             from a compile with the resource remarks; asserts that none uses
                                                             scratch; writes profiles/motion_resources.txt"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "motion_bench.txt")
OUT_RESOURCES = os.path.join(ROOT, "profiles", "motion_resources.txt")
HBM_GBS = 8000.0   # MI355X peak HBM3E bandwidth, GB/s: the bound the byte counts are held against


def resources():
    from correlation_amd import build
    lines = ["# python scripts/motion_bench.py --resources"]
    with tempfile.TemporaryDirectory() as tmp:
        log = os.path.join(tmp, "usage.log")
        flags = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
                 "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage"]
        with open(log, "w") as f:
            subprocess.run([build.hipcc_path()] + flags + ["-c", "lk_motion.hip", "-o", os.path.join(tmp, "lk_motion.o")],
                           cwd=build.CSRC, stderr=f, check=True)
        scratch = []
        for kernel, legend in (("lk_motion_sums_kernel", "RESIDUAL"), ("lk_motion_fit_kernel", "RESIDUAL")):
            mine = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "resource_usage.py"), log, kernel],
                                  capture_output=True, text=True, check=True).stdout.splitlines()
            assert len(mine) == 3, mine
            scratch += [int(r.split()[-5]) for r in mine[1:]]
            lines += ["# " + legend] + mine
        # lk_motion_remove_kernel is not a template: its remarks read directly
        text = open(log).read()
        block = text[text.index("lk_motion_remove_kernel"):]
        block = block[:block.index("Function Name", 1)] if "Function Name" in block[1:] else block
        got = dict(re.findall(r"remark:\s+([A-Za-z][\w \[\]/]*): (\w+) \[", block))
        lines += ["lk_motion_remove_kernel: VGPRs SGPRs(spill) scratch waves/SIMD LDS AGPRs VGPR-spill",
                  "%s %s %s (%s) %s %s %s %s %s" % ("".ljust(44), got["VGPRs"], got["TotalSGPRs"], got["SGPRs Spill"],
                                                    got["ScratchSize [bytes/lane]"], got["Occupancy [waves/SIMD]"],
                                                    got["LDS Size [bytes/block]"], got["AGPRs"], got["VGPRs Spill"])]
        scratch.append(int(got["ScratchSize [bytes/lane]"]))
    lines += ["# scratch, bytes per lane: at most %d over the %d kernels" % (max(scratch), len(scratch))]
    if max(scratch) != 0:
        print("\n".join(lines), flush=True)
    assert max(scratch) == 0, lines[-1]
    return lines


def numpy_fit(cen, rec):
    """the rigid fit of every frame from host records, vectorised over the sectors"""
    out = []
    c = cen.astype(np.float64)
    o = (c.min(axis=0) + c.max(axis=0)) / 2
    for r in rec:
        good = (r["error_code"] == 0) & np.isfinite(r["chi"]) & np.isfinite(r["p"]).all(axis=1)
        x, y = (c[good] - o).T
        u, v = r["p"][good, 0].astype(np.float64), r["p"][good, 1].astype(np.float64)
        n = len(x)
        xm, ym, um, vm = x.mean(), y.mean(), u.mean(), v.mean()
        dx, dy, du, dv = x - xm, y - ym, u - um, v - vm
        num = (dx * dv).sum() - (dy * du).sum()
        den = (dx * dx).sum() + (dx * du).sum() + (dy * dy).sum() + (dy * dv).sum()
        out.append((n, np.arctan2(num, den), um, vm))
    return out


def timing(reps, n_frames):
    import torch
    import correlation_amd as ca
    from correlation_amd.workload import C2, C4
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    dev = torch.device("cuda", 0)
    lines = []

    def measure(e, w, F, source, d_ptr):
        S = e.n_sectors
        cen = np.float32([e.sector_info(s)[1:] for s in range(S)])
        row = {"case": w.name, "sectors": S, "frames": F, "kind": "rigid", "passes": 1, "reps": reps,
               "source": "window, read in place" if source == ca.TRACK_RECORDS_WINDOW else "engine-held records"}
        for with_records in (False, True):
            dms, call = [], []
            for k in range(reps + 2):   # (the first two warm up)
                t0 = time.perf_counter()
                got = e.rigid_motion(ca.MOTION_RIGID, source=source, return_records=with_records)
                t1 = time.perf_counter()
                if k >= 2:
                    dms.append(e.motion_last()[0])
                    call.append((t1 - t0) * 1e3)
            m = got[0] if with_records else got
            tag = "with_records_out" if with_records else "motion_only"
            row[tag + "_device_ms_median"], row[tag + "_device_ms_min"] = float(np.median(dms)), float(np.min(dms))
            row[tag + "_call_ms_median"] = float(np.median(call))
        _, row["chunk"], row["chunks_per_frame"] = e.motion_last()
        # the long way round
        host = np.zeros((F, S), ca.RESULT_DTYPE)
        fetch, fit = [], []
        for k in range(3):
            t0 = time.perf_counter()
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), d_ptr, host.nbytes, 2) == 0
            t1 = time.perf_counter()
            ref = numpy_fit(cen, host)
            t2 = time.perf_counter()
            fetch.append((t1 - t0) * 1e3)
            fit.append((t2 - t1) * 1e3)
        row["numpy_fetch_ms_median"], row["numpy_fit_ms_median"] = float(np.median(fetch)), float(np.median(fit))
        row["theta_device_minus_numpy_max"] = float(max(abs(float(m["theta"][f]) - ref[f][1]) for f in range(F)))
        assert all(int(m["n_fit"][f]) == ref[f][0] for f in range(F))
        # bytes: pack kernel 48 read + 16 written; sums 16 + 1 written; residuals 16 + 1; the removal 48 + 16 + 48 written
        n = F * S
        row["bytes_motion_only"] = n * (48 + 16 + 17 + 17)
        row["bytes_sums_kernel"] = n * 17
        row["hbm_bound_ms_motion_only"] = row["bytes_motion_only"] / (HBM_GBS * 1e6)
        row["hbm_bound_ms_sums_kernel"] = row["bytes_sums_kernel"] / (HBM_GBS * 1e6)
        row["device_over_hbm_bound_motion_only"] = row["motion_only_device_ms_median"] / row["hbm_bound_ms_motion_only"]
        row["status_counts"] = np.bincount(m["status"], minlength=3).tolist()
        row["theta_first_frame"], row["rms_first_frame"] = float(m["theta"][0]), float(m["rms"][0])
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))

    # config 2: one solved pair
    w = C2
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    und, dfm = ca.speckle.speckle_pair(w.size, w.size, p=w.truth, seed=7, device="cuda")
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    e.correlate_all(np.zeros((e.n_sectors, 6), np.float32))
    d = C.c_void_p()
    assert e.lib.lk_get_results_device(e._h, C.byref(d)) == 0
    measure(e, w, 1, ca.TRACK_RECORDS_ENGINE, d)
    e.close()
    # config 4: a 64-frame window, its device records read in place
    w = C4
    frames = ca.speckle.speckle_sequence(w.size, w.size, n_frames + 1, velocity=(0.8, -0.4), dilation=1e-4, seed=7, device="cuda")
    d_frames = torch.from_numpy(np.stack(frames)).to(dev)
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    e.set_image_device(ca.IMG_UND, d_frames[0].data_ptr(), w.size, w.size)
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    e.sequence_reserve(n_frames)
    for i in range(n_frames):
        e.sequence_set_frame_device(i, d_frames[i + 1].data_ptr(), w.size, w.size)
    e.adjust_initial_guess(0, True, np.zeros(6, np.float32), (w.size / 2 - 0.5, w.size / 2 - 0.5))
    e.correlate_sequence(n_frames, constant_velocity=True)
    d = C.c_void_p()
    assert e.lib.lk_get_sequence_results_device(e._h, C.byref(d), None) == 0
    measure(e, w, n_frames, ca.TRACK_RECORDS_WINDOW, d)
    e.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    lines = resources() if args.resources else (["# python scripts/motion_bench.py --reps %d --frames %d" % (args.reps, args.frames)]
                                                + timing(args.reps, args.frames))
    if args.resources:
        print("\n".join(lines), flush=True)
    if not args.no_write:
        with open(OUT_RESOURCES if args.resources else OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
