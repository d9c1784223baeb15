"""Strain field (lk_strain_field) next to the one-pair solve it follows: config 4's grid at a strain window of 2.5 and 7.5
pitches, config 2's grid at 2.5 pitches (records of a real solve, engine-held), and a config-5-sized grid at 2.5 pitches on
synthetic records (passed in).  Every case runs both lane-group widths, with and without the packed neighbour array
(LK_STRAIN_GROUP / LK_STRAIN_PACKED, read by the library per call), and the library's own choice.  Per run: the median of
`reps` HIP-event times of the device part (bounding box with its round trip, grid kernels, prep, strain kernel), the median
host time of the whole synchronous call (transfers included), mean neighbours per sector, neighbour visits per second of
the device part, and the ratio to the one-pair solve time of the same engine in the same process.
Writes profiles/strain_bench.txt (one JSON line per run) unless --no-write.
Usage: python scripts/strain_bench.py [--reps K] [--only c4|c2|c5] [--no-c5-solve]"""
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
from correlation_amd.workload import C2, C4, C5  # noqa: E402

VARIANTS = [("16", "1"), ("64", "1"), ("16", "0"), ("64", "0"), (None, None)]   # (group, packed); None: the library's choice


def last_call(e):
    ms, group, packed, members = C.c_float(), C.c_int(), C.c_int(), C.c_double()
    fn = e.lib.lk_internal_strain_last   # (not part of the C ABI: the bench's window into the last call)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
    assert fn(e._h, C.byref(ms), C.byref(group), C.byref(packed), C.byref(members)) == 0
    return ms.value, group.value, packed.value, members.value


def make_engine(w, images):
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    if images:
        und, dfm = ca.speckle.speckle_pair(w.size, w.size, p=w.truth, seed=7, device="cuda")
        e.set_undeformed_image(und)
        e.set_deformed_image(dfm)
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    return e


def solve_ms_of(e, reps):
    zero = np.zeros((e.n_sectors, 6), np.float32)
    ms = []
    for k in range(reps + 1):   # (the first warms up)
        e.correlate_all(zero)
        if k:
            ms.append(e.stats()["solve_ms"])
    return float(np.median(ms))


def strain_runs(e, name, w, pitches, reps, solve_ms, records=None):
    radius = pitches * (w.x_end - w.x_begin) / w.hs
    S = e.n_sectors
    lines, first = [], None
    for group, packed in VARIANTS:
        for key, val in (("LK_STRAIN_GROUP", group), ("LK_STRAIN_PACKED", packed)):
            os.environ.pop(key, None)
            if val is not None:
                os.environ[key] = val
        dev, call = [], []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            out = e.strain_field(radius, min_neighbours=3, records=records)   # synchronous: ends in a stream synchronise
            t1 = time.perf_counter()
            ms, g, p, members = last_call(e)
            if k:
                dev.append(ms)
                call.append((t1 - t0) * 1e3)
        if first is None:
            first = out
        assert np.array_equal(out["status"], first["status"]) and np.array_equal(out["neighbours"], first["neighbours"])
        nb = float(out["neighbours"].mean())
        d = float(np.median(dev))
        line = {"case": name, "sectors": S, "radius_pitches": pitches, "radius_px": radius, "group": g, "packed": p,
                "chosen_by": "library" if group is None else "override", "members_per_3x3_cells": members, "reps": reps,
                "records": "engine-held" if records is None else "passed in (upload included in the call)",
                "device_ms_median": d, "device_ms_min": float(np.min(dev)), "call_ms_median": float(np.median(call)),
                "mean_neighbours": nb, "neighbour_visits_per_s": S * nb / (d * 1e-3),
                "status_counts": np.bincount(out["status"], minlength=4).tolist(),
                "one_pair_solve_ms_median": solve_ms,
                "device_over_solve": d / solve_ms if solve_ms else None,
                "call_over_solve": float(np.median(call)) / solve_ms if solve_ms else None}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
    for key in ("LK_STRAIN_GROUP", "LK_STRAIN_PACKED"):
        os.environ.pop(key, None)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None, choices=[None, "c4", "c2", "c5"])
    ap.add_argument("--no-c5-solve", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    lines = []
    for key, w in (("c4", C4), ("c2", C2)):
        if args.only in (None, key):
            e = make_engine(w, True)
            solve = solve_ms_of(e, 5)
            for pitches in ((2.5, 7.5) if key == "c4" else (2.5,)):
                lines += strain_runs(e, w.name, w, pitches, args.reps, solve)
            e.close()
    if args.only in (None, "c5"):
        w = C5
        solve = None
        if not args.no_c5_solve:
            e = make_engine(w, True)
            solve = solve_ms_of(e, 2)
            e.close()
            torch.cuda.empty_cache()
        e = make_engine(w, False)
        S = e.n_sectors
        rng = np.random.default_rng(3)
        rec = np.zeros(S, ca.RESULT_DTYPE)
        rec["p"] = rng.normal(0, 1, (S, 6)).astype(np.float32)
        rec["chi"] = 1.0
        rec["error_code"][rng.permutation(S)[:S // 20]] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
        lines += strain_runs(e, w.name + " (synthetic records, 5 % failed)", w, 2.5, args.reps, solve, records=rec)
        e.close()
    if lines and not args.no_write:
        with open(os.path.join(ROOT, "profiles", "strain_bench.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
