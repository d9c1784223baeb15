"""The statistical scatter of the photon-transfer fit on the recovery experiment of tests/test_noise_host.py: frames of 150 x
232, a smooth base over about 40 .. 220, Gaussian noise of variance a0 + b0 g, rounded and clipped (tests/noise_ref.py).  For
every case and K, the numpy restatement alone (not the library) estimates a, b and the pooled variance on 20 seeds; the file
records the mean error against the expectation (a0 + 1 / 12, b0, a0 + 1 / 12 + b0 mean g) and 5 x the standard deviation over
the seeds, which is the bound the test holds the library to on a seed of its own.  No GPU.
Usage: python scripts/noise_recovery.py [--seeds N] [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import noise_ref as nr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_recovery.txt"))
    args = ap.parse_args()
    lines = [json.dumps({"frames": list(nr.RECOVERY_SHAPE), "seeds": args.seeds, "fit": nr.RECOVERY_FIT,
                         "estimator": "tests/noise_ref.py (the restatement)", "bound": "5 x std over the seeds"})]
    for K in nr.RECOVERY_FRAMES:
        for a0, b0 in nr.RECOVERY_CASES:
            want = np.array(nr.recovery_expectation(a0, b0))
            est = []
            for seed in range(args.seeds):
                r = nr.from_bins(K, *nr.tables(nr.recovery_frames(K, a0, b0, seed)), **nr.RECOVERY_FIT)
                assert r["status"] == nr.OK
                est.append([r["a"], r["b"], r["var"]])
            est = np.array(est)
            err, sd = est.mean(axis=0) - want, est.std(axis=0, ddof=1)
            line = {"K": K, "a0": a0, "b0": b0, "expect": [float(v) for v in want],
                    "mean_error": [float(v) for v in err], "std": [float(v) for v in sd], "bound": [float(5 * v) for v in sd]}
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
