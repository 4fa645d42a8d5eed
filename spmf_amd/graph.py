"""Host side of the layout calls (PoissonFactorization.fuzzy_graph / graph_layout / umap, spmf_graph_layout,
csrc/graph_layout.hip): the fuzzy neighbour graph of a kNN result (scanpy's ``obsp["connectivities"]``), the curve
parameters (a, b) of a (min_dist, spread), the starting positions, and the fp64 restatement of the library's epochs
that the tests compare with.  Importable without a GPU; numpy and torch only.

The graph and the starts are plain torch on the tensors' device, fp64: a start, not a hot path.  The epochs -- the
hot path -- are the library's; ``layout_reference`` restates include/spmf_hip.h spmf_graph_layout in fp64 numpy,
Philox in integer arithmetic and every skip rule included.

New rows on a fitted layout (graph_transform / umap_transform, spmf_graph_transform, csrc/graph_transform.hip):
``query_weights`` gives their memberships in their neighbours among the reference rows, ``transform_reference``
restates the library's epochs with the reference held fixed, ``transform_negatives`` its draws.
"""
from __future__ import annotations

import numpy as np
import torch

INITS = ("pca", "random")
MAX_NEGATIVES = 64
_PHILOX_TAG = 0x554D4150          # the fourth counter word of a layout draw


# ---- the fuzzy graph -----------------------------------------------------------------------------------------
def _bisect_sigma(excess, valid, n_valid):
    """The 64 bisection steps of smooth_knn_dist for all rows at once: sigma with
    sum_j exp(-excess_ij / sigma) = log2(n_valid_i) over the valid positions (lo = 0, hi = inf, sigma = 1, doubling
    while hi is inf).  ``excess`` fp64 [N,k], 0 where invalid -> fp64 [N], not yet floored."""
    inf = float("inf")
    target = torch.log2(n_valid.clamp_min(1).to(torch.float64))
    lo = torch.zeros_like(target)
    hi = torch.full_like(target, inf)
    sigma = torch.ones_like(target)
    for _ in range(64):
        # an excess of 0 is weight 1 whatever sigma is (0 / 0 never forms)
        w = torch.where(excess > 0, torch.exp(-excess / sigma[:, None]), torch.ones_like(excess))
        psum = (w * valid).sum(1)
        above = psum > target
        hi = torch.where(above, sigma, hi)
        lo = torch.where(above, lo, sigma)
        sigma = torch.where(above | torch.isfinite(hi), 0.5 * (lo + torch.where(torch.isfinite(hi), hi, lo)),
                            2.0 * sigma)
    return sigma


def _smooth_knn(dist, valid):
    """umap-learn's smooth_knn_dist with local_connectivity 1, for all rows at once: ``dist`` fp64 [N,k] with the
    invalid positions anything, ``valid`` bool [N,k] -> (sigma, rho) fp64 [N]."""
    inf = float("inf")
    n_valid = valid.sum(1)
    positive = valid & (dist > 0)
    rho = torch.where(positive, dist, torch.full_like(dist, inf)).amin(1)
    rho = torch.where(torch.isfinite(rho), rho, torch.zeros_like(rho))
    excess = torch.where(valid, (dist - rho[:, None]).clamp_min(0.0), torch.zeros_like(dist))
    sigma = _bisect_sigma(excess, valid, n_valid)
    total = int(n_valid.sum())
    d_valid = torch.where(valid, dist, torch.zeros_like(dist))
    mean_all = float(d_valid.sum() / total) if total else 0.0
    mean_row = d_valid.sum(1) / n_valid.clamp_min(1)
    floor = 1e-3 * torch.where(rho > 0, mean_row, torch.full_like(rho, mean_all))
    return torch.maximum(sigma, floor), rho


def fuzzy_graph(indices, distances, n_rows=None):
    """The fuzzy simplicial set of a kNN result, symmetrised: ``indices`` [N,k] integers and ``distances`` [N,k]
    floats as ``knn`` returns them (padding -1 / +inf; row i lists the neighbours of row i).  The graph is square:
    ``n_rows`` (default N) is checked to be N, and an index >= N is a ValueError.  Self edges, padding and entries
    with a non-finite or negative distance are dropped; a row may not list one neighbour twice.

    Per row with at least one valid neighbour, umap-learn's smooth_knn_dist with local_connectivity 1: rho_i = the
    smallest positive distance of the row (0: none); sigma_i from exactly 64 bisection steps on
    sum_j exp(-max(0, d_ij - rho_i) / sigma) = log2(k_i), k_i the row's valid neighbours (lo = 0, hi = inf,
    sigma = 1, doubling while hi is inf), floored at 1e-3 x the row's mean distance (rho_i > 0) or the mean over
    all valid distances; the directed weight w_ij = exp(-max(0, d_ij - rho_i) / sigma_i).  The symmetric weight
    w_ij + w_ji - w_ij w_ji comes from ONE stable sort of the keys i N + j of both directions -- no scatter-add, so
    the result is reproducible -- and every edge stands in both endpoints' rows with the same bits.

    Returns tensors on the device of ``indices``: 'indptr' int64 [N+1], 'indices' int32 (ascending within a row),
    'weights' float32 (the fp64 value rounded), 'sigma' and 'rho' fp64 [N]."""
    idx = torch.as_tensor(indices)
    dist = torch.as_tensor(distances)
    if idx.dim() != 2 or idx.shape != dist.shape:
        raise ValueError(f"fuzzy_graph: indices and distances must be 2-D and of one shape, got {tuple(idx.shape)} "
                         f"and {tuple(dist.shape)}")
    if idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise ValueError(f"fuzzy_graph: indices must hold integers, got {idx.dtype}")
    if not dist.dtype.is_floating_point:
        raise ValueError(f"fuzzy_graph: distances must be floating point, got {dist.dtype}")
    N, k = int(idx.shape[0]), int(idx.shape[1])
    if n_rows is not None and int(n_rows) != N:
        raise ValueError(f"fuzzy_graph: the graph must be square: {N} rows of neighbours for n_rows={int(n_rows)}")
    dev = idx.device
    idx = idx.to(torch.int64)
    dist = dist.to(device=dev, dtype=torch.float64)
    if idx.numel():
        lo, hi = torch.stack(list(torch.aminmax(idx))).tolist()
        if hi >= N:
            raise ValueError(f"fuzzy_graph: index {hi} is outside the {N} rows (the graph must be square)")
        if lo < -1:
            raise ValueError(f"fuzzy_graph: index {lo} is below the padding -1")
    rows = torch.arange(N, device=dev, dtype=torch.int64)[:, None].expand(N, k)
    valid = (idx >= 0) & (idx != rows) & torch.isfinite(dist) & (dist >= 0)
    sigma, rho = _smooth_knn(dist, valid)
    excess = torch.where(valid, (dist - rho[:, None]).clamp_min(0.0), torch.zeros_like(dist))
    w = torch.where(excess > 0, torch.exp(-excess / sigma[:, None]), torch.ones_like(excess))
    # both directions of every directed edge under the key (row, column), the forward ones first: after a
    # stable sort a key's run is [forward] [backward], each at most once
    r, c, wv = rows[valid], idx[valid], w[valid]
    E = int(r.numel())
    key = torch.cat([r * N + c, c * N + r])
    val = torch.cat([wv, wv])
    back = torch.cat([torch.zeros(E, dtype=torch.bool, device=dev), torch.ones(E, dtype=torch.bool, device=dev)])
    key, order = torch.sort(key, stable=True)
    val, back = val[order], back[order]
    start = torch.ones(2 * E, dtype=torch.bool, device=dev)
    start[1:] = key[1:] != key[:-1]
    if E:
        # a run of two is (forward, backward); anything else lists a neighbour twice
        second = ~start
        prev_ok = torch.zeros_like(start)
        prev_ok[1:] = start[:-1] & ~back[:-1]
        if bool((second & ~(back & prev_ok)).any()):
            raise ValueError("fuzzy_graph: a row lists one neighbour twice")
    has_next = torch.zeros_like(start)
    has_next[:-1] = ~start[1:]
    nxt = torch.zeros_like(val)
    nxt[:-1] = val[1:]
    zero = torch.zeros_like(val)
    w_fwd = torch.where(back, zero, val)
    w_bwd = torch.where(back, val, torch.where(has_next, nxt, zero))
    sym = (w_fwd + w_bwd - w_fwd * w_bwd)[start]
    key = key[start]
    row_of = torch.div(key, max(N, 1), rounding_mode="floor")
    indptr = torch.searchsorted(row_of, torch.arange(N + 1, device=dev, dtype=torch.int64))
    return {"indptr": indptr.to(torch.int64), "indices": (key - row_of * N).to(torch.int32),
            "weights": sym.to(torch.float32), "sigma": sigma, "rho": rho}


def to_csr(g):
    """The graph of ``fuzzy_graph`` as numpy arrays ``(indptr int64 [N+1], indices int32, data float32)``: the
    layout of ``scipy.sparse.csr_matrix((data, indices, indptr), shape=(N, N))``, what scanpy keeps in
    ``obsp["connectivities"]``."""
    return (g["indptr"].detach().cpu().numpy().astype(np.int64), g["indices"].detach().cpu().numpy().astype(np.int32),
            g["weights"].detach().cpu().numpy().astype(np.float32))


def query_weights(indices, distances):
    """The memberships of new rows in their neighbours among the reference rows, as umap-learn's ``transform``
    forms them: ``indices`` [Q,k] integers and ``distances`` [Q,k] floats as ``knn(points, queries=...)`` returns
    them (padding -1 / +inf).  An entry is valid when its index is >= 0 and its distance finite and >= 0.

    Per row with at least one valid entry, smooth_knn_dist with local connectivity 0, so rho_i = 0 throughout:
    sigma_i from the 64 bisection steps of ``fuzzy_graph`` on sum_j exp(-d_ij / sigma) = log2(k_i), k_i the row's
    valid entries, floored at 1e-3 x the mean of all valid distances; w_ij = exp(-d_ij / sigma_i) in fp64, rounded
    to float32; an invalid entry has weight 0.  Nothing is symmetrised: the graph is bipartite and stays in the
    dense [Q,k] form that ``graph_transform`` takes.

    Returns {'weights': float32 [Q,k], 'sigma': fp64 [Q]} on the device of ``indices``."""
    idx = torch.as_tensor(indices)
    dist = torch.as_tensor(distances)
    if idx.dim() != 2 or idx.shape != dist.shape:
        raise ValueError(f"query_weights: indices and distances must be 2-D and of one shape, got "
                         f"{tuple(idx.shape)} and {tuple(dist.shape)}")
    if idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise ValueError(f"query_weights: indices must hold integers, got {idx.dtype}")
    if not dist.dtype.is_floating_point:
        raise ValueError(f"query_weights: distances must be floating point, got {dist.dtype}")
    dist = dist.to(device=idx.device, dtype=torch.float64)
    valid = (idx >= 0) & torch.isfinite(dist) & (dist >= 0)
    n_valid = valid.sum(1)
    d = torch.where(valid, dist, torch.zeros_like(dist))
    sigma = _bisect_sigma(d, valid, n_valid)
    total = int(n_valid.sum())
    mean_all = float(d.sum() / total) if total else 0.0
    sigma = sigma.clamp_min(1e-3 * mean_all)
    w = torch.where(d > 0, torch.exp(-d / sigma[:, None]), torch.ones_like(d))
    return {"weights": torch.where(valid, w, torch.zeros_like(w)).to(torch.float32), "sigma": sigma}


# ---- the curve ---------------------------------------------------------------------------------------------
def find_ab(min_dist=0.1, spread=1.0):
    """(a, b) of the layout's curve 1 / (1 + a x^(2b)) fitted to umap-learn's target -- 1 below ``min_dist``,
    exp(-(x - min_dist) / spread) above -- on 300 points of [0, 3 spread]: least squares by Levenberg-Marquardt
    in fp64 numpy from (1, 1), what umap-learn gets from scipy's curve_fit.  (0.1, 1.0) -> (1.576943, 0.895061)."""
    min_dist, spread = float(min_dist), float(spread)
    if not (np.isfinite(min_dist) and np.isfinite(spread)) or spread <= 0 or min_dist < 0 or min_dist >= 3 * spread:
        raise ValueError(f"find_ab needs spread > 0 and 0 <= min_dist < 3 spread, got {min_dist}, {spread}")
    x = np.linspace(0.0, 3.0 * spread, 300)
    target = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    logx = np.log(np.where(x > 0, x, 1.0))

    def model(p):
        u = np.where(x > 0, np.exp(2.0 * p[1] * logx), 0.0)
        den = 1.0 + p[0] * u
        jac = np.stack([-u / den ** 2, -2.0 * p[0] * u * logx / den ** 2], 1)
        return 1.0 / den - target, jac
    p = np.array([1.0, 1.0])
    res, jac = model(p)
    cost, lam = float(res @ res), 1e-3
    for _ in range(500):
        JtJ, g = jac.T @ jac, jac.T @ res
        step = np.linalg.solve(JtJ + lam * np.diag(np.diag(JtJ)), -g)
        trial = p + step
        if trial[0] > 0 and trial[1] > 0:
            r2, j2 = model(trial)
            c2 = float(r2 @ r2)
        else:
            c2 = np.inf
        if c2 <= cost:
            done = np.abs(step).max() < 1e-13 * (1.0 + np.abs(p).max())
            p, res, jac, cost, lam = trial, r2, j2, c2, max(lam * 0.2, 1e-15)
            if done:
                break
        else:
            lam *= 5.0
            if lam > 1e15:
                break
    return float(p[0]), float(p[1])


# ---- the starts --------------------------------------------------------------------------------------------
def default_epochs(n_rows):
    """umap-learn's rule: 500 epochs up to 10 000 rows, 200 above."""
    return 500 if int(n_rows) <= 10000 else 200


def init_pca(points):
    """The two leading principal axes of ``points`` [N, Kx] as float32 [N, 2] on their device: the eigenvectors
    (``torch.linalg.eigh``) of the fp64 covariance of the finite rows, the scores scaled so that the largest
    |coordinate| is 10.  A non-finite row starts NaN; a width of 1 leaves the second coordinate 0."""
    p = points.to(torch.float64)
    ok = torch.isfinite(p).all(1)
    q = p[ok]
    out = torch.full((p.shape[0], 2), float("nan"), dtype=torch.float64, device=p.device)
    if q.shape[0]:
        q = q - q.mean(0, keepdim=True)
        cov = q.T @ q / max(int(q.shape[0]) - 1, 1)
        _, vec = torch.linalg.eigh(cov)                       # ascending eigenvalues
        axes = vec[:, -2:].flip(1) if p.shape[1] >= 2 else vec[:, -1:]
        score = q @ axes
        if score.shape[1] == 1:
            score = torch.cat([score, torch.zeros_like(score)], 1)
        top = float(score.abs().max())
        out[ok] = score * (10.0 / top) if top > 0 else score
    return out.to(torch.float32).contiguous()


def init_random(n_rows, seed, device):
    """Uniform [-10, 10] positions float32 [n_rows, 2] from a CPU ``torch.Generator`` seeded with ``seed``."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    u = torch.rand(int(n_rows), 2, generator=gen, dtype=torch.float64)
    return (u * 20.0 - 10.0).to(torch.float32).to(device).contiguous()


# ---- the fp64 reference of the epochs --------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 in integer arithmetic: ``counter`` uint32 [..., 4], ``key`` two uint32 words -> uint32
    [..., 4] (Salmon et al., SC'11; csrc/philox.h)."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> sh) ^ c1 ^ np.uint64(k0)) & mask, p1 & mask, ((p0 >> sh) ^ c3 ^ np.uint64(k1)) & mask, \
            p0 & mask
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def negatives(n_rows, epoch, n_negatives, seed):
    """The negative samples r(i, e, m) of epoch ``epoch``: int64 [n_rows, n_negatives]."""
    n, M, seed = int(n_rows), int(n_negatives), int(seed) & (2 ** 64 - 1)
    blocks = (M + 3) // 4
    ctr = np.zeros((n, blocks, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(n, dtype=np.uint64)[:, None]
    ctr[..., 1] = np.arange(blocks, dtype=np.uint64)[None, :]
    ctr[..., 2] = int(epoch) & 0xFFFFFFFF
    ctr[..., 3] = _PHILOX_TAG
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(n, 4 * blocks)[:, :M]
    return ((words.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def _edges(indptr, indices, weights, n, nnz):
    """The entries of every row under the library's rules on the graph's own numbers: indptr clamped to
    [0, nnz], a row whose end lies before its start empty -> (row, column, weight) of the entries, in list order."""
    ptr = np.clip(np.asarray(indptr, dtype=np.int64)[:n + 1], 0, nnz)
    lens = np.maximum(ptr[1:] - ptr[:-1], 0)
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    first = np.cumsum(lens) - lens
    pos = ptr[:-1][row] + (np.arange(int(lens.sum()), dtype=np.int64) - first[row])
    return row, np.asarray(indices, dtype=np.int64)[pos], np.asarray(weights, dtype=np.float64)[pos]


def _row_sums(rows, values, n):
    """fp64 [n, 2]: the sums of ``values`` [E, 2] over the entries of each row, in list order."""
    return np.stack([np.bincount(rows, weights=values[:, k], minlength=n).astype(np.float64) for k in (0, 1)], 1)


def layout_reference(indptr, indices, weights, y, epoch0, n_epochs, total_epochs, lr, a, b, repulsion=1.0,
                     negative_rate=5.0, n_negatives=8, seed=0, details=False):
    """The epochs ``epoch0 .. epoch0 + n_epochs - 1`` of include/spmf_hip.h spmf_graph_layout in fp64 numpy, from
    its definition: the same skip rules, the same negatives, alpha_e rounded to fp32 as the library passes it;
    sums by ``np.bincount`` in list order.  ``y``: [n_rows, 2] (NaN / inf allowed) -> fp64 [n_rows, 2].

    ``details``: -> (y, A, W) with A_i the sum of the absolute values of the row's clipped contributions to F_i
    (the larger of the two components) and W_i, both of the LAST epoch run: the scale of a per-row error bar."""
    y = np.array(y, dtype=np.float64).reshape(-1, 2)
    n = y.shape[0]
    nnz = int(np.asarray(indices).shape[0])
    M, a, b = int(n_negatives), float(a), float(b)
    row, col, w = _edges(indptr, indices, weights, n, nnz)
    keep = (col >= 0) & (col < n) & np.isfinite(w) & (w > 0)
    row, col, w = row[keep], col[keep], w[keep]
    A = W = np.zeros(n)

    def clipped(coef, delta):
        with np.errstate(invalid="ignore", over="ignore"):
            t = coef[:, None] * delta
        return np.clip(np.where(np.isnan(t), 0.0, t), -4.0, 4.0)
    for e in range(int(epoch0), int(epoch0) + int(n_epochs)):
        alpha = float(np.float32(float(lr) * (1.0 - e / float(total_epochs))))
        fin = np.isfinite(y).all(1)
        ok = fin[col]
        r_, c_, w_ = row[ok], col[ok], w[ok]
        W = np.bincount(r_, weights=w_, minlength=n).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            delta = y[r_] - y[c_]
            d2 = (delta ** 2).sum(1)
            live = d2 > 0
            pw = np.where(live, d2, 1.0) ** b
            ca = np.where(live, -2.0 * a * b * np.where(live, d2, 1.0) ** (b - 1.0) / (1.0 + a * pw), 0.0)
        term = w_[:, None] * clipped(ca, np.where(live[:, None], delta, 0.0))
        F = _row_sums(r_, term, n)
        A = _row_sums(r_, np.abs(term), n)
        neg = negatives(n, e, M, seed)
        i_ = np.repeat(np.arange(n, dtype=np.int64), M)
        r2 = neg.reshape(-1)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            delta = y[i_] - y[r2]
            d2 = (delta ** 2).sum(1)
            live = (r2 != i_) & fin[r2] & fin[i_] & (d2 > 0)
            pw = np.where(live, d2, 1.0) ** b
            cr = np.where(live, 2.0 * float(repulsion) * b / ((0.001 + np.where(live, d2, 1.0)) * (1.0 + a * pw)), 0.0)
        scale = float(negative_rate) * W / M
        term = scale[i_][:, None] * clipped(cr, np.where(live[:, None], delta, 0.0))
        F += _row_sums(i_, term, n)
        A += _row_sums(i_, np.abs(term), n)
        moves = fin & (W > 0)
        new = y.copy()
        with np.errstate(invalid="ignore", over="ignore"):
            new[moves] = y[moves] + alpha * F[moves] / np.maximum(1.0, W[moves])[:, None]
        y = new
    if details:
        return y, (A.max(1) if A.ndim == 2 else A), W
    return y


# ---- new rows on a fitted layout: the fp64 reference -------------------------------------------------------------
_TRANSFORM_TAG = 0x554D5854       # the fourth counter word of a transform draw


def default_transform_epochs(n_query):
    """umap-learn's rule for ``transform``: 100 epochs up to 10 000 query rows, 30 above."""
    return 100 if int(n_query) <= 10000 else 30


def transform_negatives(row0, n_query, n_ref, epoch, n_negatives, seed):
    """The negative samples r(g, e, m) of the query rows g = row0 .. row0 + n_query - 1 in epoch ``epoch``, rows of
    the reference: int64 [n_query, n_negatives].  With ``n_ref`` = 0 nothing is drawn: every entry is -1."""
    q, M, n_ref, seed = int(n_query), int(n_negatives), int(n_ref), int(seed) & (2 ** 64 - 1)
    if n_ref == 0:
        return np.full((q, M), -1, dtype=np.int64)
    blocks = (M + 3) // 4
    ctr = np.zeros((q, blocks, 4), dtype=np.uint64)
    ctr[..., 0] = ((np.arange(q, dtype=np.uint64) + np.uint64(int(row0))) & np.uint64(0xFFFFFFFF))[:, None]
    ctr[..., 1] = np.arange(blocks, dtype=np.uint64)[None, :]
    ctr[..., 2] = int(epoch) & 0xFFFFFFFF
    ctr[..., 3] = _TRANSFORM_TAG
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(q, 4 * blocks)[:, :M]
    return ((words.astype(np.uint64) * np.uint64(n_ref)) >> np.uint64(32)).astype(np.int64)


def transform_reference(idx, w, y_ref, y_in, row0, epoch0, n_epochs, total_epochs, lr, a, b, repulsion=1.0,
                        negative_rate=5.0, n_negatives=8, seed=0, details=False):
    """The epochs ``epoch0 .. epoch0 + n_epochs - 1`` of include/spmf_hip.h spmf_graph_transform in fp64 numpy, from
    its definition: ``idx`` / ``w`` [Q,k] (any integers, NaN / inf weights allowed), ``y_ref`` [n_ref,2] (NaN / inf
    allowed), ``y_in`` [Q,2] or None for the weighted-mean start; the same skip rules, the same negatives, alpha_e
    rounded to fp32 as the kernel forms it -> fp64 [Q,2].

    ``details``: -> (y, A, W) with A_i the sum of the absolute values of the row's clipped contributions to F_i
    (the larger of the two components) of the LAST epoch run and W_i: the scale of a per-row error bar."""
    idx = np.asarray(idx, dtype=np.int64)
    Q, k = idx.shape
    w = np.asarray(w, dtype=np.float64).reshape(Q, k)
    y_ref = np.asarray(y_ref, dtype=np.float64).reshape(-1, 2)
    n_ref = y_ref.shape[0]
    M, a, b = int(n_negatives), float(a), float(b)
    ref_ok = np.isfinite(y_ref).all(1)
    valid = (idx >= 0) & (idx < n_ref) & np.isfinite(w) & (w > 0)
    j = np.where(valid, idx, 0)
    if n_ref:
        valid &= ref_ok[j]
    wv = np.where(valid, w, 0.0)
    yj = np.where(valid[..., None], y_ref[j] if n_ref else 0.0, 0.0)          # [Q,k,2]
    W = wv.sum(1)
    has = W > 0
    if y_in is None:
        y = np.full((Q, 2), np.nan)
        y[has] = (wv[..., None] * yj).sum(1)[has] / W[has, None]
    else:
        y = np.array(y_in, dtype=np.float64).reshape(Q, 2)
    A = np.zeros(Q)

    def clipped(coef, delta):
        with np.errstate(invalid="ignore", over="ignore"):
            t = coef[..., None] * delta
        return np.clip(np.where(np.isnan(t), 0.0, t), -4.0, 4.0)
    for e in range(int(epoch0), int(epoch0) + int(n_epochs)):
        alpha = float(np.float32(float(lr) * (1.0 - e / float(total_epochs))))
        moves = has & np.isfinite(y).all(1)
        ys = np.where(moves[:, None], y, 0.0)
        delta = ys[:, None, :] - yj
        d2 = (delta ** 2).sum(-1)
        live = valid & moves[:, None] & (d2 > 0)
        s = np.where(live, d2, 1.0)
        ca = np.where(live, -2.0 * a * b * s ** (b - 1.0) / (1.0 + a * s ** b), 0.0)
        term = wv[..., None] * clipped(ca, np.where(live[..., None], delta, 0.0))
        F = term.sum(1)
        A = np.abs(term).sum(1)
        if n_ref:
            neg = transform_negatives(row0, Q, n_ref, e, M, seed)
            delta = ys[:, None, :] - np.where(ref_ok[neg][..., None], y_ref[neg], 0.0)
            d2 = (delta ** 2).sum(-1)
            live = ref_ok[neg] & moves[:, None] & (d2 > 0)
            s = np.where(live, d2, 1.0)
            cr = np.where(live, 2.0 * float(repulsion) * b / ((0.001 + s) * (1.0 + a * s ** b)), 0.0)
            term = (float(negative_rate) * W / M)[:, None, None] * clipped(cr, np.where(live[..., None], delta, 0.0))
            F = F + term.sum(1)
            A = A + np.abs(term).sum(1)
        new = y.copy()
        new[moves] = y[moves] + alpha * F[moves] / np.maximum(1.0, W[moves])[:, None]
        y = new
    if details:
        return y, (A.max(1) if A.ndim == 2 else A), W
    return y
