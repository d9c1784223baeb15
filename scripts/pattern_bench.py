"""Speckle quality (lk_pattern_quality, lk_suggest_subset) on config 2's image: 2048 x 2048, the 10 000 sectors of 19 x 19
for the sector pass, and 10 000 points - the sector centres - with half-widths 5 .. 40 for the suggestion.  Per call the
median and minimum of `reps` HIP-event times (lk_internal_pattern_last): the sector pass, and of the suggestion the table
build and the query apart.  There is no earlier implementation to compare with, so the yardstick of the table build is the
bytes it moves by design over the time:
  row step     reads the u8 image once (the rows y - 1 and y + 1 come from cache) and writes the two u32 planes;
  column step  reads the planes for the band totals, and reads and writes them once more for the seeded band scans (the
               band totals themselves are 1 / band_rows of a plane);
so rows x cols x (1 + 4 x 2 x 4) bytes, as a fraction of the measured HBM rate of MI355X_MICROARCH (6.29 TB/s; 8.0 by the data
sheet).  At this size the image and both planes (4 + 32 MiB) fit the 256 MiB Infinity Cache: the fraction says how far the
build is from a streaming kernel, not what the HBM carried.
Writes one header line (date, commit) and one JSON line per pass to --out (default profiles/pattern_bench.txt) unless
--no-write.
Usage: python scripts/pattern_bench.py [--reps K] [--out PATH] [--commit TEXT]"""
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

HBM_MEASURED = 6.29e12   # bytes / s, float4 copy (MI355X_MICROARCH, chip-level parameters)
HBM_SPEC = 8.0e12


def timed(call, e, reps):
    """-> (the last result, per rep (device ms, build ms, query ms), median host ms of the synchronous call)"""
    times, host, out = [], [], None
    for k in range(reps + 1):   # (the first warms up)
        t0 = time.perf_counter()
        out = call()
        t1 = time.perf_counter()
        ms, _, _, build, query = e.pattern_last()
        if k:
            times.append((ms, build, query))
            host.append((t1 - t0) * 1e3)
    return out, np.array(times), float(np.median(host))


def commit_text():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pattern_bench.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    w = C2
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    und, _ = ca.speckle.speckle_pair(w.size, w.size, p=w.truth, seed=7, device="cuda")
    e.set_undeformed_image(und)             # the one slot both calls read
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    S = e.n_sectors
    common = {"case": w.name, "image": [w.size, w.size], "reps": args.reps}
    out, t, call = timed(lambda: e.pattern_quality(grey_low=5, grey_high=250, max_saturated=0.05), e, args.reps)
    lines = [dict(common, **{"pass": "pattern_quality", "sectors": S, "samples": int(out["n_points"].sum()),
                             "device_ms_median": float(np.median(t[:, 0])), "device_ms_min": float(t[:, 0].min()),
                             "call_ms_median": call, "status_counts": np.bincount(out["status"], minlength=5).tolist(),
                             "sssig_x_median": float(np.median(out["sssig_x"])), "mig_median": float(np.median(out["mig"])),
                             "sigma_u_median": float(np.median(out["sigma_u"]))})]
    pts = np.float32([e.sector_info(s)[1:] for s in range(S)])
    sssig_min = float(np.median(out["sssig_x"]))    # the SSSIG the committed 19 x 19 sectors have: suggestions around half = 9
    sub, t, call = timed(lambda: e.suggest_subset(pts, sssig_min, 5, 40), e, args.reps)
    _, row_tile, band_rows, _, _ = e.pattern_last()
    moved = w.size * w.size * (1 + 4 * 2 * 4)
    build = float(np.median(t[:, 1]))
    ok = sub["status"] == ca.SUBSET_OK
    lines.append(dict(common, **{"pass": "suggest_subset", "points": len(pts), "halves": [5, 40, 1], "sssig_min": sssig_min,
                                 "row_tile": row_tile, "band_rows": band_rows,
                                 "device_ms_median": float(np.median(t[:, 0])), "device_ms_min": float(t[:, 0].min()),
                                 "table_build_ms_median": build, "table_build_ms_min": float(t[:, 1].min()),
                                 "query_ms_median": float(np.median(t[:, 2])), "query_ms_min": float(t[:, 2].min()),
                                 "call_ms_median": call,
                                 "build_bytes_by_design": moved,
                                 "build_bytes": {"u8_rows_read": w.size * w.size, "u32_planes_written_row_step": 8 * w.size * w.size,
                                                 "u32_planes_read_band_totals": 8 * w.size * w.size,
                                                 "u32_planes_read_and_written_band_scans": 16 * w.size * w.size},
                                 "build_GB_per_s": moved / (build * 1e-3) / 1e9,
                                 "fraction_of_measured_hbm_rate": moved / (build * 1e-3) / HBM_MEASURED,
                                 "fraction_of_spec_hbm_rate": moved / (build * 1e-3) / HBM_SPEC,
                                 "status_counts": np.bincount(sub["status"], minlength=3).tolist(),
                                 "half_median": float(np.median(sub["half"][ok])) if ok.any() else None}))
    e.close()
    head = json.dumps({"date": datetime.date.today().isoformat(), "commit": args.commit or commit_text(),
                       "device": torch.cuda.get_device_name(0)})
    for line in lines:
        print(json.dumps(line), flush=True)
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write("\n".join([head] + [json.dumps(line) for line in lines]) + "\n")


if __name__ == "__main__":
    main()
