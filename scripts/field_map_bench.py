"""The field map (lk_field_map) on config 2's geometry: the 10 000 sectors of 19 x 19, synthetic records (smooth
displacements, 5 % of the sectors failed), windows of 2.5 pitches.  Per case the median and minimum of `reps` HIP-event
times of the device part (lk_internal_field_last: bounding box with its round trip, grid kernels, pack, the one map launch)
and the median host time of the synchronous call, which includes the copy of the planes to the host:
  the reference frame at 2048 x 2048 nodes (every pixel), UNIFORM against BISQUARE, U | V against all 15 channels, the
  staged tiles against LK_FIELD_WALK=1 (every node walks its 3 x 3 cells in global memory), the deformed frame with K = 4.
The yardstick is the only earlier route to such a map: lk_track_points with the nodes of a 512 x 512 window passed as
points (TOTAL mode, one frame; lk_internal_track_last), against the map of the same window - time per node against time
per point.
Writes one header line (date, commit, device) and one JSON line per case to --out (default profiles/field_map_bench.txt)
unless --no-write.
Usage: python scripts/field_map_bench.py [--reps K] [--out PATH] [--commit TEXT]"""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import correlation_amd as ca  # noqa: E402
from correlation_amd.workload import C2  # noqa: E402
from track_bench import synthetic, track_last  # noqa: E402  (scripts/ is the script's own directory)


def commit_text():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_map_bench.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--only", default=None, help="run the one case of this name (for a profiler)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    w = C2
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    S = e.n_sectors
    pitch = (w.x_end - w.x_begin) / w.hs
    radius = 2.5 * pitch
    cen = np.float32([e.sector_info(s)[1:] for s in range(S)])
    rec = synthetic(cen, 1, np.random.default_rng(3))[0]
    rec["p"][:, :2] *= 3.0           # displacements of a few pixels, gradients of 3e-3: the deformed frame has something to invert
    full, small = (0, 0, w.size, w.size), (768, 768, 512, 512)
    uv = ca.FIELD_U | ca.FIELD_V
    cases = [("reference_uniform_uv", full, dict(channels=uv), None),
             ("reference_bisquare_uv", full, dict(channels=uv, weight=ca.FIELD_BISQUARE), None),
             ("reference_uniform_all", full, dict(channels=ca.FIELD_ALL), None),
             ("reference_uniform_uv_walk", full, dict(channels=uv), "1"),
             ("reference_bisquare_uv_walk", full, dict(channels=uv, weight=ca.FIELD_BISQUARE), "1"),
             ("deformed_bisquare_uv_k4", full, dict(channels=uv, weight=ca.FIELD_BISQUARE, frame=ca.FIELD_DEFORMED, iterations=4), None),
             ("deformed_bisquare_uv_k4_walk", full, dict(channels=uv, weight=ca.FIELD_BISQUARE, frame=ca.FIELD_DEFORMED, iterations=4), "1"),
             ("window512_uniform_uv", small, dict(channels=uv), None)]
    common = {"case": w.name, "sectors": S, "radius_px": radius, "reps": args.reps}
    lines = []
    for name, window, kw, walk in cases:
        if args.only not in (None, name):
            continue
        os.environ.pop("LK_FIELD_WALK", None)
        if walk is not None:
            os.environ["LK_FIELD_WALK"] = walk
        dev, call = [], []
        for k in range(args.reps + 1):   # (the first warms up)
            t0 = time.perf_counter()
            out = e.field_map(radius, window, records=rec, want=(), **kw)
            t1 = time.perf_counter()
            ms, tiles, fallback = e.field_last()
            if k:
                dev.append(ms)
                call.append((t1 - t0) * 1e3)
        os.environ.pop("LK_FIELD_WALK", None)
        nodes = window[2] * window[3]
        d = float(np.median(dev))
        lines.append(dict(common, **{"pass": "field_map", "name": name, "nodes": [window[2], window[3]], "planes": len(out),
                                     "tiles": tiles, "fallback_tiles": fallback, "device_ms_median": d,
                                     "device_ms_min": float(np.min(dev)), "call_ms_median": float(np.median(call)),
                                     "ns_per_node": d * 1e6 / nodes, "fitted_share": float(np.isfinite(out["u"]).mean())}))
        print(json.dumps(lines[-1]), flush=True)
    if args.only in (None, "track_points_512"):
        jj, ii = np.meshgrid(np.arange(small[3]), np.arange(small[2]), indexing="ij")
        pts = np.float32(np.stack([small[0] + ii.ravel(), small[1] + jj.ravel()], 1))
        dev, call = [], []
        for k in range(args.reps + 1):
            t0 = time.perf_counter()
            tr, _ = e.track_points(pts, radius, records=rec[None], mode=ca.TRACK_TOTAL)
            t1 = time.perf_counter()
            ms, group, members = track_last(e)
            if k:
                dev.append(ms)
                call.append((t1 - t0) * 1e3)
        d = float(np.median(dev))
        lines.append(dict(common, **{"pass": "track_points", "name": "track_points_512", "points": len(pts), "group": group,
                                     "members_per_3x3_cells": members, "device_ms_median": d, "device_ms_min": float(np.min(dev)),
                                     "call_ms_median": float(np.median(call)), "ns_per_point": d * 1e6 / len(pts),
                                     "fitted_share": float((tr["status"] == ca.TRACK_OK).mean())}))
        print(json.dumps(lines[-1]), flush=True)
        same = [ln for ln in lines if ln["name"] == "window512_uniform_uv"]
        if same:
            ratio = {"name": "yardstick", "map_ns_per_node": same[0]["ns_per_node"], "track_ns_per_point": lines[-1]["ns_per_point"],
                     "track_over_map": lines[-1]["ns_per_point"] / same[0]["ns_per_node"]}
            lines.append(ratio)
            print(json.dumps(ratio), flush=True)
    e.close()
    head = json.dumps({"date": datetime.date.today().isoformat(), "commit": args.commit or commit_text(),
                       "device": torch.cuda.get_device_name(0)})
    if not args.no_write and args.only is None:
        with open(args.out, "w") as f:
            f.write("\n".join([head] + [json.dumps(line) for line in lines]) + "\n")


if __name__ == "__main__":
    main()
