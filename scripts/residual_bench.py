"""Photometry (lk_photometry) and the back-warped residual map (lk_residual_map) next to the one-pair solve they follow:
config 2's grid (10 000 sectors of 19 x 19) and config 4's grid (224 x 224 sectors of 7 x 7) at 2048 x 2048, records of a real
solve, engine-held.  Per case the median of `reps` HIP-event times of each call's device part (lk_internal_residual_last), the
median host time of the whole synchronous call (transfers included), and the one-pair solve time of the same engine in the
same process (lk_stats.solve_ms) with its counters.
  photometry  the yardstick is one evaluation's share of the solve, solve_ms * sectors / evaluations, as for the uncertainty
              pass: the pass is one evaluation per sector; `device_over_one_evaluation` is the ratio.
  map         the whole level-0 image, radius = 1.5 sector pitches: ms, pixels / s, and the bytes the kernel must move - one
              undeformed byte read and 12 bytes written per pixel - divided by the time.  That is an HBM-side figure for
              orientation; the kernel's work is the owner search and the sampler's arithmetic.
Writes one header line (date, commit) and one JSON line per run to --out (default profiles/residual_bench.txt) unless
--no-write.
Usage: python scripts/residual_bench.py [--reps K] [--only c2|c4] [--out PATH] [--commit TEXT]"""
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
from correlation_amd.workload import C2, C4  # noqa: E402


def make_engine(w):
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    und, dfm = ca.speckle.speckle_pair(w.size, w.size, p=w.truth, seed=7, device="cuda")
    e.set_undeformed_image(und)
    e.set_deformed_image(dfm)
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    return e


def solve_of(e, reps):
    zero = np.zeros((e.n_sectors, 6), np.float32)
    ms = []
    for k in range(reps + 1):   # (the first warms up)
        e.correlate_all(zero)
        if k:
            ms.append(e.stats()["solve_ms"])
    return float(np.median(ms)), e.stats()


def timed(call, e, reps):
    dev, host, out, last = [], [], None, None
    for k in range(reps + 1):
        t0 = time.perf_counter()
        out = call()   # synchronous: ends in a stream synchronise
        t1 = time.perf_counter()
        last = e.residual_last()
        if k:
            dev.append(last[0])
            host.append((t1 - t0) * 1e3)
    return out, last, float(np.median(dev)), float(np.min(dev)), float(np.median(host))


def runs(e, w, reps, solve_ms, stats):
    S = e.n_sectors
    share = solve_ms * stats["sectors"] / stats["evaluations"]
    common = {"case": w.name, "sectors": S, "reps": reps, "one_pair_solve_ms_median": solve_ms,
              "solve_evaluations": int(stats["evaluations"]), "solve_sectors": int(stats["sectors"])}
    out, _, d, dmin, call = timed(lambda: e.photometry(), e, reps)
    ok = out["status"] == ca.PHOTO_OK
    lines = [dict(common, **{"pass": "photometry", "device_ms_median": d, "device_ms_min": dmin, "call_ms_median": call,
                             "status_counts": np.bincount(out["status"], minlength=5).tolist(),
                             "zncc_median": float(np.median(out["zncc"][ok])) if ok.any() else None,
                             "rms_median": float(np.median(out["rms"][ok])) if ok.any() else None,
                             "one_evaluation_share_ms": share, "device_over_one_evaluation": d / share,
                             "device_over_solve": d / solve_ms})]
    radius = 1.5 * (w.x_end - w.x_begin) / w.hs
    maps, last, d, dmin, call = timed(lambda: e.residual_map(radius), e, reps)
    owner = maps[2]
    pixels = owner.size
    lines.append(dict(common, **{"pass": "residual_map", "radius_px": radius, "pixels": int(pixels), "tiles": last[1],
                                 "fallback_tiles": last[2], "device_ms_median": d, "device_ms_min": dmin, "call_ms_median": call,
                                 "pixels_per_s": pixels / (d * 1e-3), "must_move_bytes": 13 * int(pixels),
                                 "must_move_GB_per_s": 13 * pixels / (d * 1e-3) / 1e9,
                                 "owned_fraction": float((owner >= 0).mean()), "ownerless_fraction": float((owner == -1).mean()),
                                 "device_over_solve": d / solve_ms}))
    for line in lines:
        print(json.dumps(line), flush=True)
    return [json.dumps(line) for line in lines]


def commit_text():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None, choices=[None, "c2", "c4"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_bench.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    head = json.dumps({"date": datetime.date.today().isoformat(), "commit": args.commit or commit_text(),
                       "device": torch.cuda.get_device_name(0)})
    lines = [head]
    for key, w in (("c2", C2), ("c4", C4)):
        if args.only in (None, key):
            e = make_engine(w)
            solve_ms, stats = solve_of(e, 5)
            lines += runs(e, w, args.reps, solve_ms, stats)
            e.close()
    if len(lines) > 1 and not args.no_write:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
