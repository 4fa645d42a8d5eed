"""Host side of held-out evaluation (PoissonFactorization.score_cells, spmf_score_cells,
csrc/cells.hip): the summary of the per-cell log pointwise predictive density

    lppd_i = log mean_s p(x_i | theta_s)

of a list of held-out cells.  A cell whose log-pmf is not finite in some draw carries
lppd_i = NaN; it is left out of the sums and counted, as ``waic_streaming`` does.
"""
from __future__ import annotations

import math

import torch


def summarize(lppd):
    """[N] lppd -> {'lppd_sum','lppd_mean','se','n','n_excluded'} over the finite entries, in
    fp64: se = sqrt(n var_i(lppd_i)) with the unbiased variance, the standard error of
    'lppd_sum' (0.0 for n < 2); n = 0 gives lppd_sum = 0.0 and lppd_mean = NaN.

    The finite entries are sorted before they are reduced, so the summary is a function of the
    multiset of values: the same cells listed in another order give the same bits.  The price is
    one device sort of the finite values per call (timed as 'summary' by
    tools/score_cells_probe.py)."""
    l = torch.as_tensor(lppd).reshape(-1)
    if not l.dtype.is_floating_point:
        l = l.double()
    fin = torch.isfinite(l)
    x = torch.sort(l[fin].add_(0.0)).values.double()            # + 0.0: -0.0 and 0.0 are one value
    n = int(x.numel())
    total = float(x.sum()) if n else 0.0
    se = math.sqrt(n * float(x.var(unbiased=True))) if n >= 2 else 0.0
    return {"lppd_sum": total, "lppd_mean": total / n if n else float("nan"), "se": se, "n": n,
            "n_excluded": int(l.numel()) - n}
