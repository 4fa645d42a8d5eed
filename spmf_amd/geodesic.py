"""Host side of the shortest-path calls (PoissonFactorization.geodesic / pseudotime, spmf_graph_relax,
csrc/graph_paths.hip): exact single- and multi-source shortest-path distances along a neighbour graph of edge
lengths -- how far along the graph every row is from a chosen root (pseudotime in the Wishbone / Palantir /
Slingshot sense, the ordering scanpy users put next to ``tl.paga``), Isomap-style landmark distances, and the
distance to the nearest row of a set.  Importable without a GPU; numpy and torch only.

The graph is a CSR dict whose 'weights' are LENGTHS (``length_graph`` of a ``knn`` result, or
``lengths_from_weights`` of a ``fuzzy_graph``), read under spmf_graph_spmm's rules: indptr clamped to [0, nnz], a
falling indptr an empty row, an entry counts only if its column lies in [0, N) and its length is finite and > 0.

One sweep on a float32 [N, 16] block X, a column per source (or set of sources): for row i and column l, with
best = +inf and arg = -1, the counting entries (j, w) of the row in list order: t = X_jl + w, one float32
addition; if t < best then best = t, arg = j; then Y_il = best < X_il ? best : X_il.  Repeated to the fixed point
this is synchronous Bellman-Ford in pull form.  fl(a + w) is monotone in a and a minimum does not depend on the
order, so the fixed point is unique: bit for bit what a float32 Dijkstra making the same left-to-right additions
returns (tests/_geodesic_cases.py fp32_dijkstra), and within (hops + 1) 2^-23 relative of the fp64 distance.  A NaN
never wins a <, so it stays where it is and reaches nobody.

The predecessor of (i, l) is written by a sweep on the converged block: arg where best == Y_il, Y_il is finite and
X_{arg,l} < Y_il, else -1: the first entry in list order that attains the row's distance from a strictly nearer
row.  The chain of predecessors strictly decreases in distance, so it is acyclic and ends at a source (-1, all
lengths being positive).  A reached row that is no source has -1 only where the addition was absorbed: a length
below half an ulp of the distance, fl(X_jl + w) == X_jl; the row then has its neighbour's distance and no strictly
nearer neighbour, and ``path`` raises on it.

The driver (``solve``) is written once over an ops interface with two backends that agree bit for bit in
distances, predecessors and the number of sweeps: ``LibraryOps``, whose ``relax`` is the library's call on the
device, and ``NumpyOps``, whose ``relax`` is the same sweep as a gather, one ``np.float32`` add and
``np.minimum.at``.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _args, _lib
from . import spectral as _spectral

BLOCK = 16                       # include/spmf_hip.h SPMF_BLOCK_COLS: sources (or sets) per block
SWEEPS_PER_CALL = 16             # sweeps between two looks at the "changed" word
UNIT_WEIGHT_LENGTH = 2.0 ** -24  # ``lengths_from_weights``: the length of weight 1, and the floor of every length:
                                 # -log of the largest float32 below 1


# ---- graphs of lengths -------------------------------------------------------------------------------------------
def length_graph(indices, distances):
    """The symmetric union of a ``knn`` result as a graph of lengths: ``indices`` [N, k] integers and ``distances``
    [N, k] floats as ``knn`` returns them (padding -1 / +inf; row i lists the neighbours of row i).  Entry (i, j) is
    present if i lists j or j lists i; its length is the float32 distance, the smaller where both directions exist
    (Euclidean distances are symmetric, so they are equal there).  Padding, self entries and entries with a
    non-finite or negative distance are dropped; an index >= N is a ValueError and a row may not list one neighbour
    twice.  A length of 0 (two rows in one place) stays in the list and does not count, under the library's rule.

    ONE stable sort of the keys i N + j of both directions and no scatter-add, as ``fuzzy_graph``, so the result
    is reproducible, and every edge stands in both endpoints' rows with the same bits.

    Returns tensors on the device of ``indices``: {'indptr': int64 [N + 1], 'indices': int32 (ascending within a
    row), 'weights': float32 (the lengths)}: what ``solve`` / ``PoissonFactorization.geodesic`` take."""
    idx = torch.as_tensor(indices)
    dist = torch.as_tensor(distances)
    if idx.dim() != 2 or idx.shape != dist.shape:
        raise ValueError(f"length_graph: indices and distances must be 2-D and of one shape, got "
                         f"{tuple(idx.shape)} and {tuple(dist.shape)}")
    if idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise ValueError(f"length_graph: indices must hold integers, got {idx.dtype}")
    if not dist.dtype.is_floating_point:
        raise ValueError(f"length_graph: distances must be floating point, got {dist.dtype}")
    N, k = int(idx.shape[0]), int(idx.shape[1])
    dev = idx.device
    idx = idx.to(torch.int64)
    dist = dist.to(device=dev, dtype=torch.float32)
    if idx.numel():
        lo, hi = torch.stack(list(torch.aminmax(idx))).tolist()
        if hi >= N:
            raise ValueError(f"length_graph: index {hi} is outside the {N} rows (the graph must be square)")
        if lo < -1:
            raise ValueError(f"length_graph: index {lo} is below the padding -1")
    rows = torch.arange(N, device=dev, dtype=torch.int64)[:, None].expand(N, k)
    valid = (idx >= 0) & (idx != rows) & torch.isfinite(dist) & (dist >= 0)
    r, c, d = rows[valid], idx[valid], dist[valid]
    E = int(r.numel())
    # both directions of every directed edge under the key (row, column), the forward ones first: after a stable
    # sort a key's run is [forward] [backward], each at most once
    key = torch.cat([r * N + c, c * N + r])
    val = torch.cat([d, d])
    back = torch.cat([torch.zeros(E, dtype=torch.bool, device=dev), torch.ones(E, dtype=torch.bool, device=dev)])
    key, order = torch.sort(key, stable=True)
    val, back = val[order], back[order]
    start = torch.ones(2 * E, dtype=torch.bool, device=dev)
    start[1:] = key[1:] != key[:-1]
    if E:
        second = ~start
        prev_ok = torch.zeros_like(start)
        prev_ok[1:] = start[:-1] & ~back[:-1]
        if bool((second & ~(back & prev_ok)).any()):
            raise ValueError("length_graph: a row lists one neighbour twice")
    has_next = torch.zeros_like(start)
    has_next[:-1] = ~start[1:]
    nxt = torch.zeros_like(val)
    nxt[:-1] = val[1:]
    length = torch.where(has_next, torch.minimum(val, nxt), val)[start]
    key = key[start]
    row_of = torch.div(key, max(N, 1), rounding_mode="floor")
    indptr = torch.searchsorted(row_of, torch.arange(N + 1, device=dev, dtype=torch.int64))
    return {"indptr": indptr.to(torch.int64), "indices": (key - row_of * N).to(torch.int32),
            "weights": length.to(torch.float32)}


def lengths_from_weights(graph):
    """A metric for callers who kept only the connectivities: the graph dict of ``fuzzy_graph`` with every weight w
    replaced by the length max(-log(w), ``UNIT_WEIGHT_LENGTH``) for w in (0, 1], formed in fp64 and rounded to
    float32 -- weight 1, a row's nearest neighbour, has the length ``UNIT_WEIGHT_LENGTH`` = 2^-24, not 0, which
    would not count.  A weight outside (0, 1] (or NaN) becomes +inf and does not count.  -> {'indptr', 'indices',
    'weights'} on the device of the graph, the first two as given."""
    if not isinstance(graph, dict) or any(n not in graph for n in ("indptr", "indices", "weights")):
        raise ValueError("lengths_from_weights: graph must be a dict with 'indptr', 'indices' and 'weights' "
                         "(fuzzy_graph)")
    w = torch.as_tensor(graph["weights"]).to(torch.float64)
    ok = (w > 0) & (w <= 1)
    length = torch.where(ok, (-torch.log(torch.where(ok, w, torch.ones_like(w)))).clamp_min(UNIT_WEIGHT_LENGTH),
                         torch.full_like(w, math.inf))
    return {"indptr": graph["indptr"], "indices": graph["indices"], "weights": length.to(torch.float32)}


# ---- the two backends --------------------------------------------------------------------------------------------
class NumpyOps:
    """The sweep in float32 numpy on a graph dict (tensors or arrays), read as it stands.  The driver's tensors live
    on the CPU."""

    device = torch.device("cpu")

    def __init__(self, graph):
        self.n, self.row, self.col, self.w = _spectral.valid_edges(graph)      # the counting entries in list order
        self._entry = np.arange(len(self.row), dtype=np.int64)[:, None]

    def relax(self, x, n_sweeps, pred=False):
        """``n_sweeps`` >= 0 sweeps from the block ``x`` (float32 [N, 16] tensor) -> (the block after them, the
        predecessors of the last sweep (int32 [N, 16]) with ``pred`` and at least one sweep, else None, whether
        the last sweep changed a value)."""
        f = np.float32
        x = np.ascontiguousarray(x.numpy() if isinstance(x, torch.Tensor) else x, dtype=f)
        E, changed, p = len(self.row), False, None
        for s in range(int(n_sweeps)):
            with np.errstate(invalid="ignore", over="ignore"):
                xj = x[self.col]                                               # the gather [E, 16]
                t = xj + self.w[:, None]                                       # one float32 addition
            assert t.dtype == f
            t = np.where(np.isnan(t), f(np.inf), t)                            # a NaN never wins a <
            best = np.full((self.n, BLOCK), np.inf, dtype=f)
            np.minimum.at(best, self.row, t)
            with np.errstate(invalid="ignore"):
                lower = best < x
            y = np.where(lower, best, x)
            changed = bool(lower.any())
            if pred and s == int(n_sweeps) - 1:
                # the first entry in list order that attains best (+inf never won the strict <)
                hit = (t == best[self.row]) & (t < np.inf)
                first = np.full((self.n, BLOCK), E, dtype=np.int64)
                np.minimum.at(first, self.row, np.where(hit, self._entry, E))
                has = first < E
                e = np.where(has, first, 0)
                lane = np.arange(BLOCK)[None, :]
                arg = np.where(has, self.col[e] if E else 0, -1)
                xa = np.where(has, xj[e, lane] if E else f(np.inf), f(np.inf))
                with np.errstate(invalid="ignore"):
                    keep = has & (best == y) & np.isfinite(y) & (xa < y)
                p = torch.from_numpy(np.where(keep, arg, -1).astype(np.int32))
            x = y
        return torch.from_numpy(x), p, changed


class LibraryOps:
    """The sweeps as the library's call on device tensors of a graph (indptr int64, indices int32, lengths float32).
    One read-back -- the "changed" word -- per call, not per sweep."""

    def __init__(self, lib, handle, indptr, indices, lengths):
        self.lib, self.h = lib, handle
        self.device = indptr.device
        self.n, self.nnz = int(indptr.numel()) - 1, int(indices.numel())
        self.g = (indptr.contiguous(), indices.contiguous(), lengths.contiguous())
        self._changed = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._scratch = _lib.Scratch(self.device)

    def relax(self, x, n_sweeps, pred=False):
        x = x.to(self.device).contiguous()
        y = torch.empty_like(x)
        p = torch.empty(self.n, BLOCK, dtype=torch.int32, device=self.device) if pred and n_sweeps > 0 else None
        _lib.call(self.h, "spmf_graph_relax", self.n, self.nnz, self.g[0].data_ptr(),
                  self.g[1].data_ptr() if self.nnz else None, self.g[2].data_ptr() if self.nnz else None,
                  x.data_ptr(), y.data_ptr(), p.data_ptr() if p is not None else None, self._changed.data_ptr(),
                  int(n_sweeps), device=self.device,
                  scratch=(self._scratch, "spmf_graph_relax_scratch_bytes", self.n))
        return y, p, bool(int(self._changed.item()))


# ---- the driver ----------------------------------------------------------------------------------------------------
def source_sets(name, sources, n_rows):
    """The sources of ``solve`` as a list of int64 numpy arrays, one per column: ``sources`` is a 1-D integer tensor
    (or array) of row numbers, one column each, or a list of such tensors, one column per set.  Refused: a
    non-integer dtype, an empty list or set, a source outside [0, N)."""
    def rows(v):
        t = v.detach().cpu() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
        if t.dtype.is_floating_point or t.dtype == torch.bool or t.dtype.is_complex:
            raise ValueError(f"{name}: sources must hold integers, got {t.dtype}")
        if t.dim() > 1:
            raise ValueError(f"{name}: sources must be 1-D row numbers, got shape {tuple(t.shape)}")
        return t.reshape(-1).to(torch.int64).numpy()
    if isinstance(sources, (list, tuple)):
        sets = [rows(v) for v in sources]
    else:
        sets = [v.reshape(1) for v in rows(sources)]
    if not sets or any(s.size == 0 for s in sets):
        raise ValueError(f"{name}: sources must list at least one row" + (" in every set" if sets else ""))
    for s in sets:
        if int(s.min()) < 0 or int(s.max()) >= n_rows:
            bad = int(s.min()) if int(s.min()) < 0 else int(s.max())
            raise ValueError(f"{name}: sources must lie in [0, {n_rows}), got {bad}")
    return sets


def solve(ops, sources, predecessors=False, max_sweeps=None, sweeps_per_call=SWEEPS_PER_CALL, name="geodesic"):
    """The shortest-path distances along the graph behind ``ops`` (a ``LibraryOps`` or a ``NumpyOps``) from
    ``sources``: a 1-D integer tensor of row numbers, one column each, or a list of such tensors, one column per
    set -- a column then starts at 0 on every row of its set, which gives the distance to the nearest of them.

    The columns are processed in blocks of 16; unused columns start and stay at +inf.  A block is relaxed
    ``sweeps_per_call`` sweeps per call until a call's last sweep changed nothing, or until ``max_sweeps`` sweeps
    (default N, which a graph of N rows cannot need) have run; then, with ``predecessors``, one more call of one
    sweep names them.

    Returns a dict, tensors where the ops live: 'distances' float32 [N, S], +inf for unreached rows;
    'predecessors' int32 [N, S] or None; 'n_sweeps', the largest number of sweeps a block ran up to and including
    the call that found the fixed point -- the converged count rounded up to the call granularity, plus the sweep
    of the changeless look, not the hop count itself; 'converged'.  Reaching ``max_sweeps`` is reported through
    'converged', not raised; the predecessor sweep of a block that did not converge is one more sweep of its
    distances and counts in 'n_sweeps'.  Bit-reproducible, and the same bits on both backends."""
    N = int(ops.n)
    sets = source_sets(name, sources, N)
    max_sweeps = N if max_sweeps is None else _args.integer(name, "max_sweeps", max_sweeps, 1, 2 ** 31 - 1)
    per_call = _args.integer(name, "sweeps_per_call", sweeps_per_call, 1, 2 ** 20)
    S = len(sets)
    dist = torch.empty(N, S, dtype=torch.float32, device=ops.device)
    pred = torch.empty(N, S, dtype=torch.int32, device=ops.device) if predecessors else None
    n_sweeps, converged = 0, True
    for c0 in range(0, S, BLOCK):
        cols = sets[c0:c0 + BLOCK]
        start = np.full((N, BLOCK), np.inf, dtype=np.float32)
        for l, s in enumerate(cols):
            start[s, l] = 0.0
        x = torch.from_numpy(start).to(ops.device)
        ran, done = 0, N == 0
        while not done and ran < max_sweeps:
            step = min(per_call, max_sweeps - ran)
            x, _, changed = ops.relax(x, step, False)
            ran += step
            done = not changed
        p = None
        if predecessors and N:
            x, p, _ = ops.relax(x, 1, True)
            ran += 0 if done else 1
        n_sweeps, converged = max(n_sweeps, ran), converged and done
        dist[:, c0:c0 + len(cols)] = x[:, :len(cols)]
        if p is not None:
            pred[:, c0:c0 + len(cols)] = p[:, :len(cols)]
    return {"distances": dist, "predecessors": pred, "n_sweeps": n_sweeps, "converged": converged}


# ---- what is made from the result ------------------------------------------------------------------------------------
def path(predecessors, column, row, distances=None):
    """The rows from ``row`` back to its source in column ``column``: [row, pred(row), pred(pred(row)), ..], at
    most N steps.  ``predecessors``: the int32 [N, S] tensor of ``solve``, with ``distances`` its float32 [N, S]
    -- or the result dict of ``solve`` itself.  The chain ends where the predecessor is -1; with the distances that
    row must be a source (distance 0), else a ValueError names it: an unreached row, or a row whose last addition
    was absorbed."""
    if isinstance(predecessors, dict):
        predecessors, distances = predecessors["predecessors"], predecessors["distances"]
    if predecessors is None:
        raise ValueError("path: no predecessors: solve / geodesic with predecessors=True returns them")
    p = torch.as_tensor(predecessors)
    if p.dim() != 2 or p.dtype.is_floating_point:
        raise ValueError(f"path: predecessors must be integers [N, S], got {p.dtype} {tuple(p.shape)}")
    N, S = int(p.shape[0]), int(p.shape[1])
    column = _args.integer("path", "column", column, 0, S - 1)
    row = _args.integer("path", "row", row, 0, N - 1)
    chain = p[:, column].detach().cpu().to(torch.int64).numpy()
    out = [row]
    while chain[out[-1]] >= 0:
        if len(out) > N:
            raise ValueError(f"path: the predecessors of column {column} form a cycle through row {out[-1]}")
        nxt = int(chain[out[-1]])
        if nxt >= N:
            raise ValueError(f"path: predecessor {nxt} of row {out[-1]} is outside the {N} rows")
        out.append(nxt)
    if distances is not None:
        d = float(torch.as_tensor(distances)[out[-1], column])
        if d != 0.0:
            raise ValueError(f"path: the chain from row {row} in column {column} ends at row {out[-1]}, which is no "
                             f"source (distance {d}): unreached, or its last addition was absorbed")
    return out


def pseudotime(distances):
    """Per column the distance divided by the column's largest finite one: values in [0, 1], NaN for unreached rows
    (dpt's convention); a column whose largest finite distance is 0 is 0 on its reached rows.  float32, the shape
    and device of ``distances`` ([N] or [N, S])."""
    d = torch.as_tensor(distances)
    if not d.dtype.is_floating_point or d.dim() not in (1, 2):
        raise ValueError(f"pseudotime: distances must be floating point [N] or [N, S], got {d.dtype} "
                         f"{tuple(d.shape)}")
    d = d.to(torch.float32)
    finite = torch.isfinite(d)
    zero = torch.zeros_like(d)
    top = torch.where(finite, d, zero).amax(0, keepdim=True) if d.numel() else d
    scaled = torch.where(top > 0, d / torch.where(top > 0, top, torch.ones_like(top)), zero)
    return torch.where(finite, scaled, torch.full_like(d, math.nan))
