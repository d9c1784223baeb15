"""HIP-event times of the automatic initial guess (lk_search_guesses) on the bench configurations: C2 at level 2, R 16 and
at level 0, R 32; C4 at level 0, R 8; C5 at level 3, R 8.  One JSON line per case (median of --reps timed calls after a
warm-up), the search's status counts, and the C2 one-pair solve for scale.  Usage: python scripts/guess_search_bench.py"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import correlation_amd as ca  # noqa: E402
from correlation_amd.workload import C2, C4, C5  # noqa: E402

CASES = [(C2, 2, 16), (C2, 0, 32), (C4, 0, 8), (C5, 3, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream()   # the engine runs on it, the events are recorded on it
    images = {}
    for w, level, radius in CASES:
        if w.name not in images:
            images[w.name] = ca.speckle.speckle_pair(w.size, w.size, p=w.truth, seed=7, device="cuda")
        und, dfm = images[w.name]
        e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
        e.set_stream(stream.cuda_stream)   # the events below bracket the engine's work
        e.set_undeformed_image(und)
        e.set_deformed_image(dfm)
        e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
        e.commit_sectors()
        zero = np.zeros((e.n_sectors, 6), np.float32)
        solve_ms = None
        if level == 2 and radius == 16:
            e.correlate_all(zero)
            e.correlate_all(zero)
            solve_ms = e.stats()["solve_ms"]
        times = []
        for r in range(args.reps + 2):
            e.search_guesses(radius, level=level, guesses=zero)   # (uploads the centres: every call searches the same)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            e.search_guesses(radius, level=level)
            t1.record(stream)
            e.synchronize()
            torch.cuda.synchronize()
            if r >= 2:
                times.append(t0.elapsed_time(t1))
        info = e.guess_search_info()
        print(json.dumps({"case": w.name.split(":")[0], "level": level, "radius": radius, "sectors": e.n_sectors,
                          "search_ms_median": float(np.median(times)), "search_ms_min": float(np.min(times)),
                          "byte_products": int(info["n_samples"].astype(np.int64).sum() * (2 * radius + 1) ** 2),
                          "status_counts": np.bincount(info["status"], minlength=6).tolist(),
                          "c2_one_pair_solve_ms": solve_ms}), flush=True)
        e.close()


if __name__ == "__main__":
    main()
