"""Lens distortion (lk_lens_fit, lk_lens_correct) on config 2's grid (10 000 sectors) with one and with
16 frames of synthetic records of a shifted specimen seen through a lens, and on config 4's (50 176 sectors), a solved 64-frame
window read in place on the device.  Per case the medians of `reps`: the HIP-event time of one evaluation of the fit (the
chunk sums and their join, lk_internal_lens_last), of the whole fit's device part with the host steps between the
evaluations, and of the correction; the byte counts held against the HBM bound; lk_rigid_motion's pass on the same data as
the yardstick; and the long way round: the records fetched to the host and one evaluation by the numpy restatement of
tests/lens_ref.py.  Recorded figures: no time and no ratio is asserted.

    python scripts/lens_bench.py [--reps K] [--frames N]   on the GPU: writes profiles/lens_bench.txt
    python scripts/lens_bench.py --resources               anywhere: VGPRs, LDS and scratch of the kernels of csrc/lk_lens.hip
                                                           from a compile with the resource remarks; asserts that none uses
                                                           scratch; writes profiles/lens_resources.txt"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "lens_bench.txt")
OUT_RESOURCES = os.path.join(ROOT, "profiles", "lens_resources.txt")
HBM_GBS = 8000.0   # MI355X peak HBM3E bandwidth, GB/s: the bound the byte counts are held against


def resources():
    from correlation_amd import build
    lines = ["# python scripts/lens_bench.py --resources",
             "kernel: VGPRs AGPRs SGPRs scratch[bytes/lane] waves/SIMD LDS[bytes/block]"]
    with tempfile.TemporaryDirectory() as tmp:
        flags = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
                 "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run([build.hipcc_path()] + flags + ["-c", "lk_lens.hip", "-o", os.path.join(tmp, "lk_lens.o")], cwd=build.CSRC,
                           capture_output=True, text=True, check=True)
    scratch = []
    for block in r.stderr.split("Function Name: ")[1:]:
        mangled = block.split()[0]
        got = dict(re.findall(r"remark:\s+([A-Za-z][\w \[\]/]*): (\w+) \[", block))
        name = re.search(r"lk_lens_\w+?_kernel", mangled).group(0)
        q = re.search(r"kernelILi(\d)E", mangled)
        lines.append("%-28s %s %s %s %s %s %s" % (name + ("<Q = %s>" % q.group(1) if q else ""), got["VGPRs"], got["AGPRs"], got["TotalSGPRs"],
                                                  got["ScratchSize [bytes/lane]"], got["Occupancy [waves/SIMD]"], got["LDS Size [bytes/block]"]))
        scratch.append(int(got["ScratchSize [bytes/lane]"]))
    lines.append("# scratch, bytes per lane: at most %d over the %d kernels" % (max(scratch), len(scratch)))
    assert len(scratch) == 5 and max(scratch) == 0, lines
    return lines


def synthetic_records(ca, cen, lens, n_frames):
    """records u = D(U(X) + t_f) - X of a specimen shifted by t_f (a circle of 12 px), all good"""
    X = cen.astype(np.float64)
    Xu = ca.lens_undistort(lens, X)
    rec = np.zeros((n_frames, len(X)), ca.RESULT_DTYPE)
    for f in range(n_frames):
        phi = 2 * np.pi * (f + 0.25) / max(n_frames, 4)
        rec[f]["p"][:, :2] = ca.lens_distort(lens, Xu + 12.0 * np.float64([np.cos(phi), np.sin(phi)])) - X
    rec["chi"], rec["n_points"], rec["iterations"] = 0.5, 361, 5
    return rec


def timing(reps, n_frames):
    import torch
    import correlation_amd as ca
    import lens_ref
    from correlation_amd.workload import C2, C4
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    dev = torch.device("cuda", 0)
    lines = []

    def measure(e, name, F, source, records, d_ptr, free, nuisance, init):
        S = e.n_sectors
        cen = np.float32([e.sector_info(s)[1:] for s in range(S)])
        kw = dict(source=source, records=records)
        row = {"case": name, "sectors": S, "frames": F, "reps": reps, "free": free, "nuisance": nuisance,
               "source": "window, read in place" if source == ca.TRACK_RECORDS_WINDOW else "caller records, uploaded"}
        fit_ms, eval_ms, call_ms, corr_ms, corr_call, motion_ms = [], [], [], [], [], []
        for k in range(reps + 2):   # (the first two warm up)
            t0 = time.perf_counter()
            got = e.lens_fit(free, nuisance, init=init, **kw)
            t1 = time.perf_counter()
            last = e.lens_last()
            t2 = time.perf_counter()
            e.lens_correct(got["lens"], **kw)
            t3 = time.perf_counter()
            corr = e.lens_last()[0]
            e.rigid_motion(ca.MOTION_RIGID, **kw)
            if k >= 2:
                fit_ms.append(last[0]), eval_ms.append(last[4]), call_ms.append((t1 - t0) * 1e3)
                corr_ms.append(corr), corr_call.append((t3 - t2) * 1e3), motion_ms.append(e.motion_last()[0])
        row.update(status=int(got["status"]), iterations=int(got["iterations"]), evaluations=last[3], chunk=last[1], chunks_per_frame=last[2],
                   k1=float(got["lens"]["k1"]), rms_before=float(got["rms_before"]), rms=float(got["rms"]),
                   evaluation_device_ms_median=float(np.median(eval_ms)), evaluation_device_ms_min=float(np.min(eval_ms)),
                   fit_device_ms_median=float(np.median(fit_ms)), fit_call_ms_median=float(np.median(call_ms)),
                   correct_device_ms_median=float(np.median(corr_ms)), correct_call_ms_median=float(np.median(corr_call)),
                   rigid_motion_device_ms_median=float(np.median(motion_ms)))
        # bytes: an evaluation reads the 16-byte pack; the pack kernel (once per call) reads the 48-byte records and writes the
        # pack; the correction reads records and pack and writes records and a status byte
        n = F * S
        row["bytes_evaluation"], row["bytes_correct"] = n * 16, n * (48 + 16 + 48 + 16 + 48 + 1)
        row["hbm_bound_ms_evaluation"] = row["bytes_evaluation"] / (HBM_GBS * 1e6)
        row["hbm_bound_ms_correct"] = row["bytes_correct"] / (HBM_GBS * 1e6)
        row["evaluation_over_hbm_bound"] = row["evaluation_device_ms_median"] / row["hbm_bound_ms_evaluation"]
        row["correct_over_hbm_bound"] = row["correct_device_ms_median"] / row["hbm_bound_ms_correct"]
        # the long way round: the records to the host, one evaluation in numpy
        host = np.zeros((F, S), ca.RESULT_DTYPE)
        t0 = time.perf_counter()
        if d_ptr is not None:
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), d_ptr, host.nbytes, 2) == 0
        else:
            host[:] = records
        t1 = time.perf_counter()
        sums, _, _ = lens_ref.all_sums(lens_ref.as_dict(init), nuisance, np.zeros((F, 6)), cen, host, ca.FM_UVUXUYVXVY)
        t2 = time.perf_counter()
        row["numpy_fetch_ms"], row["numpy_evaluation_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
        first = e.lens_fit(free, nuisance, init=init, max_iters=1, return_sums=True, **kw)[1][0]
        assert (first[:, 0] == sums[:, 0]).all()
        row["sums_device_minus_numpy_relative_max"] = float((np.abs(first - sums) / np.maximum(np.abs(sums), 1e-300)).max())
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))

    four = ca.LENS_FREE_K1 | ca.LENS_FREE_K2 | ca.LENS_FREE_CENTRE
    # config 2's grid: synthetic records of a shifted specimen, one frame and 16
    w = C2
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    blank = np.zeros((w.size, w.size), np.uint8)
    e.set_undeformed_image(blank)
    e.set_deformed_image(blank)
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    start = e.lens_default()
    true = ca.make_lens(start["cx"] + 5.0, start["cy"] - 4.0, start["rn"], -0.03, 0.008)
    cen = np.float32([e.sector_info(s)[1:] for s in range(e.n_sectors)])
    measure(e, w.name + ", 1 frame", 1, ca.TRACK_RECORDS_CALLER, synthetic_records(ca, cen, true, 1), None, ca.LENS_FREE_K1, ca.LENS_TRANSLATION, start)
    measure(e, w.name + ", 16 frames", 16, ca.TRACK_RECORDS_CALLER, synthetic_records(ca, cen, true, 16), None, four, ca.LENS_TRANSLATION, start)
    e.close()
    # config 4: a solved window, its device records read in place (a specimen that drifts and dilates: a similarity per frame)
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
    measure(e, w.name + ", window", n_frames, ca.TRACK_RECORDS_WINDOW, None, d, ca.LENS_FREE_K1, ca.LENS_SIMILARITY, e.lens_default())
    e.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    lines = resources() if args.resources else (["# python scripts/lens_bench.py --reps %d --frames %d" % (args.reps, args.frames)]
                                                + timing(args.reps, args.frames))
    if args.resources:
        print("\n".join(lines), flush=True)
    if not args.no_write:
        with open(OUT_RESOURCES if args.resources else OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
