"""Host side of the streaming WAIC (spmf_waic_accumulate, csrc/waic.hip): the six
fp64 sums a batch leaves behind, and what they mean.

    sums[0] cells counted      sums[1] sum_i lppd_i     sums[2] sum_i pwaic_i
    sums[3] sum_i elpd_i^2     sums[4] cells excluded   sums[5] spare

with elpd_i = lppd_i - pwaic_i.  Every slot is a sum over cells: the sums of
several batches, row chunks or row shards are ADDED, then combined once.
"""
from __future__ import annotations

import math

import numpy as np

NSUMS = 6


def combine(sums):
    """[6] sums -> {'waic','se','lppd','pwaic','n','n_excluded'}:
    waic = -2 sum_i elpd_i, se = 2 sqrt(n var_i(elpd_i)) with the unbiased
    var_i = (sum e^2 - (sum e)^2 / n) / (n - 1)."""
    s = np.asarray(sums.detach().cpu() if hasattr(sums, "detach") else sums, dtype=np.float64).reshape(-1)
    if s.shape[0] != NSUMS:
        raise ValueError(f"expected {NSUMS} sums, got {s.shape[0]}")
    n, lppd, pwaic, e2 = float(s[0]), float(s[1]), float(s[2]), float(s[3])
    e = lppd - pwaic
    var = (e2 - e * e / n) / (n - 1.0) if n > 1 else float("nan")
    return {"waic": -2.0 * e, "se": 2.0 * math.sqrt(n * max(var, 0.0)) if var == var else float("nan"),
            "lppd": lppd, "pwaic": pwaic, "n": int(round(n)), "n_excluded": int(round(float(s[4])))}
