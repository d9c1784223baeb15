"""Outlier flags (lk_flag_outliers) next to the strain field at the same radius and the one-pair solve they follow: config 4's
and config 2's grids at windows of 1.5, 2.5 and 7.5 pitches, detrend on and off, passes 1 and 2, on the engine-held records
of a real solve.  Per run: the median of `reps` HIP-event times of the device part (bounding box with its round trip, grid
kernels, prep, every pass), the median host time of the whole synchronous call, the lane group and LDS rows the library
chose, mean neighbours per sector; lk_strain_field's device part at the same radius and lk_stats.solve_ms of the same engine
are taken in the same process, and the ratios to both are reported.  --paths adds the forced variants (LK_OUTLIER_GROUP,
LK_OUTLIER_LDS_CAP = 0: every window re-walked).  Expectation, written down before any measurement: a device part within
a small multiple of the strain field's at the same radius - the two plane walks are the strain field's, the 66 counting
rounds read LDS.
Writes profiles/outlier_bench.txt (one JSON line per run) unless --no-write.
Usage: python scripts/outlier_bench.py [--reps K] [--only c4|c2] [--paths]"""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import correlation_amd as ca  # noqa: E402
from correlation_amd.workload import C2, C4  # noqa: E402
from strain_bench import last_call as strain_last_call, make_engine, solve_ms_of  # noqa: E402

HOOKS = ("LK_OUTLIER_GROUP", "LK_OUTLIER_LDS_CAP")


def last_call(e):
    ms, group, rows, members = C.c_float(), C.c_int(), C.c_int(), C.c_double()
    fn = e.lib.lk_internal_outlier_last   # (not part of the C ABI: the bench's window into the last call)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
    assert fn(e._h, C.byref(ms), C.byref(group), C.byref(rows), C.byref(members)) == 0
    return ms.value, group.value, rows.value, members.value


def strain_device_ms(e, radius, reps):
    ms = []
    for k in range(reps + 1):
        e.strain_field(radius, min_neighbours=3)
        if k:
            ms.append(strain_last_call(e)[0])
    return float(np.median(ms))


def outlier_runs(e, name, w, pitches, reps, solve_ms, paths):
    radius = pitches * (w.x_end - w.x_begin) / w.hs
    S = e.n_sectors
    strain_ms = strain_device_ms(e, radius, reps)
    variants = [(None, None)] + ([("16", None), ("64", None), ("16", "0"), ("64", "0")] if paths else [])
    lines = []
    for detrend in (1, 0):
        for passes in (1, 2):
            for group, cap in variants:
                for key, val in zip(HOOKS, (group, cap)):
                    os.environ.pop(key, None)
                    if val is not None:
                        os.environ[key] = val
                dev, call = [], []
                for k in range(reps + 1):
                    t0 = time.perf_counter()
                    out, n = e.flag_outliers(radius, detrend=detrend, passes=passes)   # synchronous
                    t1 = time.perf_counter()
                    ms, g, rows, members = last_call(e)
                    if k:
                        dev.append(ms)
                        call.append((t1 - t0) * 1e3)
                d = float(np.median(dev))
                line = {"case": name, "sectors": S, "radius_pitches": pitches, "radius_px": radius, "detrend": detrend,
                        "passes": passes, "group": g, "lds_rows": rows, "chosen_by": "library" if group is None and cap is None else "override",
                        "members_per_3x3_cells": members, "reps": reps, "device_ms_median": d, "device_ms_min": float(np.min(dev)),
                        "call_ms_median": float(np.median(call)), "mean_neighbours": float(out["neighbours"].mean()),
                        "flagged": n, "status_counts": np.bincount(out["status"], minlength=5).tolist(),
                        "strain_device_ms_median": strain_ms, "device_over_strain": d / strain_ms,
                        "one_pair_solve_ms_median": solve_ms, "device_over_solve": d / solve_ms,
                        "call_over_solve": float(np.median(call)) / solve_ms}
                print(json.dumps(line), flush=True)
                lines.append(json.dumps(line))
    for key in HOOKS:
        os.environ.pop(key, None)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None, choices=[None, "c4", "c2"])
    ap.add_argument("--paths", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    lines = []
    for key, w in (("c4", C4), ("c2", C2)):
        if args.only in (None, key):
            e = make_engine(w, True)
            solve = solve_ms_of(e, 5)
            for pitches in (1.5, 2.5, 7.5):
                lines += outlier_runs(e, w.name, w, pitches, args.reps, solve, args.paths)
            e.close()
    if lines and not args.no_write:
        with open(os.path.join(ROOT, "profiles", "outlier_bench.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
