"""Material-point tracks (lk_track_points) next to the strain field it shares its fit with: config 2's grid (100 x 100
sectors) and config 4's (224 x 224), Q = S random points inside the hull of the centres, synthetic records passed in
(smooth displacements, 5 % of the sectors failed), F = 1, 16 and 64 frames, windows of 1.5, 2.5 and 7.5 pitches, INCREMENTAL
mode (the chain through the frames is the serial one).  Every case runs both lane-group widths (LK_TRACK_GROUP, read by the
library per call) and the library's own choice.  Per run: the median of `reps` HIP-event times of the device part
(bounding box with its round trip, grid kernels, prep over F x S records, the one track launch), the time per fit
(device time / (F Q)), the median host time of the whole synchronous call (upload of the records included), and beside it
lk_strain_field's device time per fit on the same domain, radius and first frame - the yardstick: one launch, S fits, a
residual pass in addition.
Writes profiles/track_bench.txt (one JSON line per run) unless --no-write; --out names another file.
Usage: python scripts/track_bench.py [--reps K] [--only c2|c4] [--frames 1,16,64] [--out FILE]"""
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

GROUPS = ["16", "64", None]   # None: the library's choice
PITCHES = (1.5, 2.5, 7.5)


def track_last(e):
    ms, group, members = C.c_float(), C.c_int(), C.c_double()
    fn = e.lib.lk_internal_track_last   # (not part of the C ABI: the bench's window into the last call)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double)]
    assert fn(e._h, C.byref(ms), C.byref(group), C.byref(members)) == 0
    return ms.value, group.value, members.value


def strain_last(e):
    ms, group, packed, members = C.c_float(), C.c_int(), C.c_int(), C.c_double()
    fn = e.lib.lk_internal_strain_last
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
    assert fn(e._h, C.byref(ms), C.byref(group), C.byref(packed), C.byref(members)) == 0
    return ms.value, group.value


def make_engine(w):
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    return e


def synthetic(cen, n_frames, rng):
    """smooth increments of about a pixel per frame; 5 % of the sectors of every frame failed"""
    S = len(cen)
    c = cen.astype(np.float64)
    rec = np.zeros((n_frames, S), ca.RESULT_DTYPE)
    rec["chi"], rec["n_points"] = 1.0, 49
    mid = c.mean(axis=0)
    for f in range(n_frames):
        a, G = rng.uniform(-1, 1, 2), rng.uniform(-1e-3, 1e-3, (2, 2))
        uv = a + (c - mid) @ G.T
        rec["p"][f, :, 0], rec["p"][f, :, 1] = uv[:, 0], uv[:, 1]
        rec["error_code"][f, rng.permutation(S)[:S // 20]] = ca.ERROR_CORRELATION_MAX_ITERS_REACHED
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, choices=[None, "c2", "c4"])
    ap.add_argument("--frames", default="1,16,64")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    frames = [int(t) for t in args.frames.split(",")]
    lines = []
    for key, w in (("c2", C2), ("c4", C4)):
        if args.only not in (None, key):
            continue
        e = make_engine(w)
        S = e.n_sectors
        pitch = (w.x_end - w.x_begin) / w.hs
        cen = np.float32([e.sector_info(s)[1:] for s in range(S)])
        rng = np.random.default_rng(3)
        rec = synthetic(cen, max(frames), rng)
        lo, hi = cen.min(axis=0).astype(np.float64), cen.max(axis=0).astype(np.float64)
        pts = np.float32(rng.uniform(lo + 8 * pitch, hi - 8 * pitch, (S, 2)))   # (64 frames of a pixel each stay inside)
        for pitches in PITCHES:
            radius = pitches * pitch
            dev = []
            for k in range(args.reps + 1):   # (the first warms up)
                e.strain_field(radius, records=rec[0])
                if k:
                    dev.append(strain_last(e)[0])
            strain_ms, strain_group = float(np.median(dev)), strain_last(e)[1]
            for F in frames:
                first = None
                for group in GROUPS:
                    os.environ.pop("LK_TRACK_GROUP", None)
                    if group is not None:
                        os.environ["LK_TRACK_GROUP"] = group
                    dev, call = [], []
                    for k in range(args.reps + 1):
                        t0 = time.perf_counter()
                        out, _ = e.track_points(pts, radius, records=rec[:F], mode=ca.TRACK_INCREMENTAL)   # synchronous
                        t1 = time.perf_counter()
                        ms, g, members = track_last(e)
                        if k:
                            dev.append(ms)
                            call.append((t1 - t0) * 1e3)
                    if first is None:
                        first = out
                    assert np.array_equal(out["status"], first["status"]) and np.array_equal(out["neighbours"], first["neighbours"])
                    d = float(np.median(dev))
                    line = {"case": w.name, "sectors": S, "points": S, "frames": F, "radius_pitches": pitches, "radius_px": radius,
                            "group": g, "chosen_by": "library" if group is None else "override", "members_per_3x3_cells": members,
                            "reps": args.reps, "device_ms_median": d, "device_ms_min": float(np.min(dev)),
                            "call_ms_median": float(np.median(call)), "ns_per_fit": d * 1e6 / (F * S),
                            "mean_neighbours": float(out["neighbours"].mean()),
                            "status_counts": np.bincount(out["status"].ravel(), minlength=5).tolist(),
                            "strain_field_device_ms_median": strain_ms, "strain_field_group": strain_group,
                            "strain_field_ns_per_fit": strain_ms * 1e6 / S}
                    print(json.dumps(line), flush=True)
                    lines.append(json.dumps(line))
        os.environ.pop("LK_TRACK_GROUP", None)
        e.close()
    if lines and not args.no_write:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
