"""What follows ``group_means``: contrasts between groups over the draws, and the observed side of an
expected-versus-observed table.  Plain torch on the host layer; nothing here is on the hot path.
"""
import numpy as np
import torch


def _members(what, g, G):
    idx = [int(i) for i in (g if isinstance(g, (tuple, list)) else (g,))]
    if not idx:
        raise ValueError(f"contrast: {what} names no group")
    for i in idx:
        if not 0 <= i < G:
            raise ValueError(f"contrast: group {i} of {what} is outside [0, {G})")
    return idx


def _pooled(sums, count, idx):
    """fp64 [S, C]: the mean over the rows of the groups ``idx`` pooled by their counts (NaN without rows)."""
    n = count[idx].sum().to(torch.float64)
    n = n if float(n) > 0 else torch.full_like(n, float("nan"))
    return sums[:, idx].sum(1) / n


def contrast(result, a, b, pseudocount=1e-3, delta=1.0):
    """The log2 fold change of group ``a`` against group ``b`` with its posterior: per draw
    lfc_s = log2((mean_a + pseudocount) / (mean_b + pseudocount)) from ``result`` = ``group_means(...)``
    ('sum' [S, G, C] and 'count' [G]); ``a`` / ``b``: a group or a tuple of groups, pooled by their counts
    (``b = tuple(the rest)`` is "against the rest").

    Returns {'lfc_draws': fp64 [S, C], 'lfc': their mean, 'sd': their unbiased sd (two draws or more),
    'p_abs_gt': the share of draws with |lfc_s| > delta}.  A side without rows is NaN (share 0)."""
    sums, count = result["sum"], result["count"]
    G = int(sums.shape[1])
    ia, ib = _members("a", a, G), _members("b", b, G)
    pc = float(pseudocount)
    lfc = torch.log2((_pooled(sums, count, ia) + pc) / (_pooled(sums, count, ib) + pc))
    out = {"lfc_draws": lfc, "lfc": lfc.mean(0),
           "p_abs_gt": (lfc.abs() > float(delta)).to(torch.float64).mean(0)}
    if lfc.shape[0] >= 2:
        out["sd"] = lfc.std(0, unbiased=True)
    return out


def observed(data, labels, n_groups, cols=None):
    """The observed side: per group and column the sum of the counts and the number of non-zero counts of the
    group's rows, {'sum': fp64 [G, C], 'nonzero': fp64 [G, C], 'count': int64 [G]}, by fp64 ``index_add_`` over
    the stored entries -- exact for integer counts, hence independent of the order of summation.

    ``data``: a dense array / tensor [B, D], a scipy sparse matrix or a ``SparseCounts``; ``labels`` [B] in
    {-1, 0 .. n_groups - 1} (-1: no group); ``cols``: None or a list of columns (duplicates kept)."""
    G = int(n_groups)
    if G < 1:
        raise ValueError(f"observed: n_groups must be at least 1, got {G}")
    labels = torch.as_tensor(np.asarray(labels.cpu()) if isinstance(labels, torch.Tensor) else np.asarray(labels))
    if labels.dim() != 1 or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError("observed: labels must be 1-D integers")
    labels = labels.to(torch.int64)
    if hasattr(data, "row_ptr") and hasattr(data, "col_idx"):          # SparseCounts
        B, D = int(data.n_rows), int(data.n_cols)
        ptr = data.row_ptr.cpu().to(torch.int64)
        row = torch.repeat_interleave(torch.arange(B), ptr[1:] - ptr[:-1])
        col, val = data.col_idx.cpu().to(torch.int64), data.val.cpu().to(torch.float64)
    elif hasattr(data, "tocoo"):                                       # scipy sparse
        coo = data.tocoo()
        B, D = coo.shape
        row, col = torch.as_tensor(coo.row.astype(np.int64)), torch.as_tensor(coo.col.astype(np.int64))
        val = torch.as_tensor(coo.data.astype(np.float64))
    else:
        x = torch.as_tensor(np.asarray(data.cpu()) if isinstance(data, torch.Tensor) else np.asarray(data))
        x = x.to(torch.float64)
        B, D = x.shape
        row, col = torch.nonzero(x, as_tuple=True)
        val = x[row, col]
    if labels.numel() != B:
        raise ValueError(f"observed: labels must have one entry per row, got {int(labels.numel())} for {B} rows")
    if labels.numel() and (int(labels.min()) < -1 or int(labels.max()) >= G):
        raise ValueError(f"observed: labels must lie in [-1, {G})")
    g = labels[row]
    keep = (g >= 0) & (val != 0)
    flat = g[keep] * D + col[keep]
    total = torch.zeros(G * D, dtype=torch.float64).index_add_(0, flat, val[keep])
    nz = torch.zeros(G * D, dtype=torch.float64).index_add_(0, flat, torch.ones_like(val[keep]))
    total, nz = total.view(G, D), nz.view(G, D)
    if cols is not None:
        sel = torch.as_tensor(np.asarray(cols.cpu()) if isinstance(cols, torch.Tensor) else np.asarray(cols))
        sel = sel.to(torch.int64)
        total, nz = total[:, sel], nz[:, sel]
    return {"sum": total, "nonzero": nz, "count": torch.bincount(labels[labels >= 0], minlength=G)}
