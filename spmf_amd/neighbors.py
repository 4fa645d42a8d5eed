"""Host side of the neighbour calls (PoissonFactorization.knn / neighbors, spmf_knn, csrc/knn.hip):
the CSR layout a graph library expects, the fp64 reference the tests and the probe compare with,
and recall.  Importable without a GPU; numpy and torch only.

The rules of the reference are those of the kernel (include/spmf_hip.h spmf_knn): a candidate is a
finite reference row that is not the excluded self; a non-finite query row has none, nor has a zero
row under the cosine metric; the k nearest are ordered by (distance ascending, index ascending) and a
row with fewer than k candidates is padded with index -1 / distance +inf at the tail.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _args

METRICS = ("euclidean", "cosine")


def to_csr(indices, distances, n_ref=None):
    """[Nq,k] indices (padding -1) and distances -> ``(indptr int64 [Nq+1], indices int32, data
    float32)`` as numpy arrays with the padding dropped: row i's neighbours are
    ``indices[indptr[i]:indptr[i+1]]`` in the order given.  This is the layout of
    ``scipy.sparse.csr_matrix((data, indices, indptr), shape=(Nq, n_ref))``, what scanpy keeps in
    ``obsp["distances"]``.  With ``n_ref`` the indices are checked against it."""
    idx = torch.as_tensor(indices).detach().cpu()
    dist = torch.as_tensor(distances).detach().cpu()
    if idx.dim() != 2 or idx.shape != dist.shape:
        raise ValueError(f"to_csr: indices and distances must be 2-D and of one shape, got {tuple(idx.shape)} "
                         f"and {tuple(dist.shape)}")
    if idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise ValueError(f"to_csr: indices must hold integers, got {idx.dtype}")
    keep = idx >= 0
    if n_ref is not None and idx.numel() and int(idx.max()) >= int(n_ref):
        raise ValueError(f"to_csr: index {int(idx.max())} is outside the {int(n_ref)} reference rows")
    indptr = np.zeros(idx.shape[0] + 1, dtype=np.int64)
    np.cumsum(keep.sum(1).numpy(), out=indptr[1:])
    return indptr, idx[keep].to(torch.int32).numpy(), dist[keep].to(torch.float32).numpy()


def _self_offset(exclude_self):
    if exclude_self is None or exclude_self is False:
        return None
    return 0 if exclude_self is True else int(exclude_self)


def brute_force(q, r, k, metric="euclidean", exclude_self=False, max_elements=1 << 25):
    """The fp64 reference: for every row of ``q`` [Nq,K] the ``k`` nearest rows of ``r`` [Nr,K], formed
    from exact differences on chunks of queries (at most ``max_elements`` differences at a time) on the
    device of ``r``.  ``exclude_self``: True says query i IS reference row i (an int: row
    ``exclude_self + i``) and is no candidate of its own.  Euclidean: sqrt(sum (q - r)^2); cosine:
    1/2 sum (q/|q| - r/|r|)^2 = 1 - cos.  -> (indices int64 [Nq,k], distances float64 [Nq,k])."""
    if metric not in METRICS:
        raise ValueError(f"brute_force: metric must be one of {METRICS}, got {metric!r}")
    r = torch.as_tensor(r).double()
    q = torch.as_tensor(q).to(r.device).double()
    if q.dim() != 2 or r.dim() != 2 or q.shape[1] != r.shape[1]:
        raise ValueError(f"brute_force: q and r must be 2-D of one width, got {tuple(q.shape)} and {tuple(r.shape)}")
    k = int(k)
    if k < 1:
        raise ValueError("brute_force: k must be >= 1")
    off = _self_offset(exclude_self)
    nq, nr = q.shape[0], r.shape[0]
    r_ok = torch.isfinite(r).all(1)
    q_ok = torch.isfinite(q).all(1)
    if metric == "cosine":
        rn, qn = r.norm(dim=1, keepdim=True), q.norm(dim=1, keepdim=True)
        r_ok, q_ok = r_ok & (rn[:, 0] > 0), q_ok & (qn[:, 0] > 0)
        r, q = r / rn, q / qn
    inf = float("inf")
    idx = torch.full((nq, k), -1, dtype=torch.int64, device=r.device)
    dist = torch.full((nq, k), inf, dtype=torch.float64, device=r.device)
    if nr == 0 or nq == 0:
        return idx, dist
    cols = torch.arange(nr, device=r.device)
    step = max(1, int(max_elements) // max(1, nr * r.shape[1]))
    for i0 in range(0, nq, step):
        qi = q[i0:i0 + step]
        d = ((qi[:, None, :] - r[None, :, :]) ** 2).sum(-1)
        d = 0.5 * d if metric == "cosine" else d.sqrt()
        bad = ~r_ok[None, :] | ~q_ok[i0:i0 + step, None] | ~torch.isfinite(d)
        if off is not None:
            bad = bad | (cols[None, :] == (torch.arange(i0, i0 + qi.shape[0], device=r.device) + off)[:, None])
        d = torch.where(bad, torch.full_like(d, inf), d)
        sd, si = torch.sort(d, dim=1, stable=True)            # stable: equal distances by ascending index
        sd, si = sd[:, :k], si[:, :k]
        si = torch.where(torch.gather(bad, 1, si), torch.full_like(si, -1), si)
        idx[i0:i0 + qi.shape[0], :sd.shape[1]] = si
        dist[i0:i0 + qi.shape[0], :sd.shape[1]] = sd
    return idx, dist


def vote(indices, weights, labels, n_classes=None, max_elements=1 << 24):
    """Label transfer over a neighbour result (scanpy's ``ingest``): per query row the class with the largest fp64
    sum of ``weights`` [Q,k] among its neighbours ``indices`` [Q,k] (rows of the reference, padding -1), whose
    classes are ``labels`` [n_ref] integers, and that class's share of the row's summed voting weight.

    A neighbour votes when its index lies in [0, n_ref), its weight is finite and > 0 and its label lies in
    [0, ``n_classes``) (default: the largest label + 1); a label -1 or one outside the range does not vote.  Equal
    sums go to the smaller class; a row without a voting neighbour gets -1 / NaN.

    Plain torch on the device of ``indices``: an equality mask per class and a sum over the k axis on chunks of at
    most ``max_elements`` mask entries -- no scatter-add, so two runs give the same bits.
    -> (labels int64 [Q], share fp64 [Q])."""
    idx = torch.as_tensor(indices)
    dev = idx.device
    w = torch.as_tensor(weights).to(dev)
    lab = torch.as_tensor(labels).to(dev)
    if idx.dim() != 2 or idx.shape != w.shape:
        raise ValueError(f"vote: indices and weights must be 2-D and of one shape, got {tuple(idx.shape)} and "
                         f"{tuple(w.shape)}")
    if idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise ValueError(f"vote: indices must hold integers, got {idx.dtype}")
    if lab.dim() != 1 or lab.dtype.is_floating_point or lab.dtype == torch.bool:
        raise ValueError(f"vote: labels must be a 1-D tensor of integers, got {lab.dtype} {tuple(lab.shape)}")
    if n_classes is not None:
        _args.integer("vote", "n_classes", n_classes, 0)
    idx, lab, w = idx.to(torch.int64), lab.to(torch.int64), w.to(torch.float64)
    n_ref = int(lab.numel())
    G = int(n_classes) if n_classes is not None else (max(int(lab.max()) + 1, 0) if n_ref else 0)
    Q, k = int(idx.shape[0]), int(idx.shape[1])
    out = torch.full((Q,), -1, dtype=torch.int64, device=dev)
    share = torch.full((Q,), float("nan"), dtype=torch.float64, device=dev)
    if Q == 0 or k == 0 or G == 0 or n_ref == 0:
        return out, share
    classes = torch.arange(G, device=dev, dtype=torch.int64)
    step = max(1, int(max_elements) // (k * G))
    for i0 in range(0, Q, step):
        j, wi = idx[i0:i0 + step], w[i0:i0 + step]
        ok = (j >= 0) & (j < n_ref) & torch.isfinite(wi) & (wi > 0)
        cls = torch.where(ok, lab[j.clamp(0, n_ref - 1)], torch.full_like(j, -1))
        ok = ok & (cls >= 0) & (cls < G)
        wi = torch.where(ok, wi, torch.zeros_like(wi))
        sums = (wi[:, :, None] * (cls[:, :, None] == classes[None, None, :])).sum(1)      # [rows, G]
        top = sums.amax(1)
        first = torch.where(sums == top[:, None], classes[None, :], torch.full_like(classes, G)[None, :]).amin(1)
        voted = ok.any(1)
        out[i0:i0 + step] = torch.where(voted, first, torch.full_like(first, -1))
        share[i0:i0 + step] = torch.where(voted, top / wi.sum(1), torch.full_like(top, float("nan")))
    return out, share


def recall(indices, truth):
    """The share of the true neighbours found: over all rows, the entries of ``truth`` (padding -1 left
    out) that appear in the same row of ``indices``.  1.0 when ``truth`` holds no neighbour."""
    a = torch.as_tensor(indices).detach().cpu().long()
    t = torch.as_tensor(truth).detach().cpu().long()
    if a.dim() != 2 or t.dim() != 2 or a.shape[0] != t.shape[0]:
        raise ValueError(f"recall: indices and truth must be 2-D with one row count, got {tuple(a.shape)} and "
                         f"{tuple(t.shape)}")
    valid = t >= 0
    total = int(valid.sum())
    if total == 0:
        return 1.0
    hit = (t[:, :, None] == a[:, None, :]).any(-1) & valid
    return int(hit.sum()) / total
