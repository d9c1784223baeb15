"""Synthetic solve records for the passes that take the caller's records (tests/test_strain_gpu.py and the tests that import it
from there, tests/cell_grid_ref.py): no solve behind them, only the three ways in which a record fails the good rule."""
import numpy as np

import correlation_amd as ca


def synthetic_records(S, rng, chi_max, share):
    """random displacements of a few pixels; `share` of the sectors made bad in EACH of three ways: an error code, a NaN
    parameter, a chi above chi_max"""
    rec = np.zeros(S, ca.RESULT_DTYPE)
    rec["p"] = rng.normal(0, 1, (S, 6)) * np.float32([8, 8, 0.05, 0.05, 0.05, 0.05])
    rec["chi"] = rng.uniform(0.1, 0.9 * chi_max, S)
    rec["n_points"] = 361
    rec["iterations"] = rng.integers(1, 20, S)
    k = max(1, int(round(share * S)))
    bad = rng.permutation(S)[:3 * k]
    rec["error_code"][bad[:k]] = rng.integers(1, 6, k)
    rec["p"][bad[k:2 * k], 0] = np.nan
    rec["chi"][bad[2 * k:]] = chi_max * 1.5
    return rec
