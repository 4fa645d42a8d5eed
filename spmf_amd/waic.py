"""Host side of the streaming WAIC (spmf_waic_accumulate, csrc/waic.hip): the six
fp64 sums a batch leaves behind, and what they mean.

    sums[0] cells counted      sums[1] sum_i lppd_i     sums[2] sum_i pwaic_i
    sums[3] sum_i elpd_i^2     sums[4] cells excluded   sums[5] spare

with elpd_i = lppd_i - pwaic_i.  Every slot is a sum over cells: the sums of
several batches, row chunks or row shards are ADDED, then combined once.
spmf_waic_accumulate_cols leaves the first five slots per column as well
([D, 5], ``combine_columns``): they add across batches in the same way.
"""
from __future__ import annotations

import math

import numpy as np

NSUMS = 6
NCOLSUMS = 5


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


def combine_columns(col_sums):
    """[D, 5] fp64 column sums (slots 0..4 of the sums, per column) -> {'col_n', 'col_n_excluded'} int64 and
    {'col_lppd', 'col_pwaic', 'col_waic', 'col_se'} fp64, each [D], on the device of the input:
    col_waic = -2 (lppd - pwaic) and col_se = ``combine``'s formula over the column's own counted cells, NaN
    where the column has at most one."""
    import torch
    s = torch.as_tensor(col_sums).to(torch.float64)
    if s.dim() != 2 or s.shape[1] != NCOLSUMS:
        raise ValueError(f"expected [D, {NCOLSUMS}] column sums, got shape {tuple(s.shape)}")
    n, lppd, pwaic, e2 = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    e = lppd - pwaic
    many = n > 1
    safe_n = torch.where(many, n, torch.full_like(n, 2.0))
    var = (e2 - e * e / safe_n) / (safe_n - 1.0)
    se = torch.where(many, 2.0 * torch.sqrt(safe_n * var.clamp_min(0.0)), torch.full_like(n, float("nan")))
    return {"col_n": n.round().to(torch.int64), "col_n_excluded": s[:, 4].round().to(torch.int64),
            "col_lppd": lppd.contiguous(), "col_pwaic": pwaic.contiguous(), "col_waic": -2.0 * e, "col_se": se}
