"""Host side of held-out evaluation (PoissonFactorization.score_cells, spmf_score_cells,
csrc/cells.hip): the summary of the per-cell log pointwise predictive density

    lppd_i = log mean_s p(x_i | theta_s)

of a list of held-out cells.  A cell whose log-pmf is not finite in some draw carries
lppd_i = NaN; it is left out of the sums and counted, as ``waic_streaming`` does.

And of held-out ranking (PoissonFactorization.rank_cells, spmf_rank_cells, csrc/rank.hip): hit rate,
reciprocal rank and AUC from one integer per cell, its rank among its row's candidates.
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


def rank_summary(rank, candidates, ks=(1, 5, 10, 20, 50)):
    """[N] ranks (0 = best, -1 = no rank: a non-finite score) and [N] candidate counts (the row's
    candidates beside the cell) -> {'n','n_excluded','hit_rate','mrr','auc'}:
    n = the cells with rank >= 0, n_excluded the others; hit_rate[k] = the share of the n cells with
    rank < k (recall@k of one held-out cell each); mrr = the mean of 1 / (rank + 1); auc = the mean of
    1 - rank / candidates over the ranked cells with candidates > 0, the share of a row's other
    candidates the cell is scored above.  n = 0 gives NaN for the three means.

    The summary is a function of the multiset of (rank, candidates) pairs, so the same cells listed in
    another order give the same bits: the cells are counted per rank and their ranks added per candidate
    count, both in integers, and the fp64 sums then run over the sorted distinct values (sum_r n_r / (r + 1)
    and sum_c R_c / c with R_c the rank total of the cells with c candidates).  No vector longer than the
    list or the largest value is made, and none of fp64 as long as the list."""
    r = torch.as_tensor(rank).reshape(-1)
    c = torch.as_tensor(candidates).reshape(-1)
    if r.numel() != c.numel():
        raise ValueError(f"rank_summary: rank and candidates differ in length, {r.numel()} and {c.numel()}")
    ks = (int(ks),) if isinstance(ks, int) else tuple(int(k) for k in ks)
    ok = r >= 0
    total = int(r.numel())
    r, c = r[ok], c[ok]
    del ok
    n = int(r.numel())
    nan = float("nan")
    if n == 0:
        return {"n": 0, "n_excluded": total, "hit_rate": {k: nan for k in ks}, "mrr": nan, "auc": nan}
    per_rank = torch.bincount(r.long())                                      # n_r, r = 0 .. max rank
    below = torch.cumsum(per_rank, 0)
    hits = {k: int(below[min(k, below.numel()) - 1]) / n if k >= 1 else 0.0 for k in ks}
    mrr = float((per_rank.double() / torch.arange(1, per_rank.numel() + 1, dtype=torch.float64,
                                                  device=per_rank.device)).sum()) / n
    has = c > 0
    m = int(has.sum())
    auc = nan
    if m:
        r, c = r[has].long(), c[has].long()
        totals = torch.zeros(int(c.max()) + 1, dtype=torch.int64, device=c.device).index_add_(0, c, r)   # R_c
        auc = 1.0 - float((totals[1:].double() / torch.arange(1, totals.numel(), dtype=torch.float64,
                                                              device=c.device)).sum()) / m
    return {"n": n, "n_excluded": total - n, "hit_rate": hits, "mrr": mrr, "auc": auc}
