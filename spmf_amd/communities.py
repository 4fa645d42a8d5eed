"""Host side of graph clustering (PoissonFactorization.communities, spmf_graph_move, csrc/graph_move.hip):
deterministic Louvain clustering of the graph ``fuzzy_graph`` returns -- scanpy's ``tl.louvain`` / ``tl.leiden`` on
``obsp["connectivities"]``.  Modularity clustering finds the number of clusters itself; its labels feed
``group_means``, ``silhouette`` and ``neighbors.vote`` unchanged.  Importable without a GPU; numpy and torch only.

Everything is an integer except one formula.  The weights become fixed point, wq = rint(double(w) 2^24) as int64,
so every sum below is an int64 sum: exact, the same in any order, on any backend.  The driver (``solve``) is written
once over an ops interface with two backends: ``LibraryOps``, whose ``move`` is the library's sweep on the device,
and ``NumpyOps``, whose ``move`` is a vectorised numpy restatement of the same definition.  The two agree bit for
bit, labels and modularity.

An entry counts when its column lies in [0, N) and wq >= 1; indptr is read under spmf_graph_spmm's rules (clamped
to [0, nnz], a falling indptr an empty row).  A self entry (i, i) counts in k_i but never as a link to a community;
coarse graphs keep a community's internal weight as one self entry, so M2 is the same at every level.  M2 >= 2^62
is refused.

One level.  Labels start at label[i] = i.  With k_i the sum of row i's counting wq, M2 = sum_i k_i, tot[c] the sum
of k_i over label[i] = c, e_ic the sum of wq over row i's counting entries j != i with label[j] = c and
a = label[i], a sweep is Jacobi -- it reads the labels of the sweep before and writes new ones -- and scores
    score(c) = double(e_ic) - ((gamma double(k_i)) double(tot'[c])) / double(M2),
tot'[a] = tot[a] - k_i, tot'[c] = tot[c] otherwise, each fp64 operation rounded on its own.  Candidates are the
communities of row i's counting non-self neighbours.  Sweep t admits only c > a when t is even ("up") and only
c < a when t is odd ("down"): under synchronous moves two rows that prefer each other's community would otherwise
swap for ever, and with one direction per sweep only one of them may go.  Row i moves to the admitted candidate of
largest score if that score is strictly greater than score(a); equal scores go to the smaller c; a row with
k_i = 0 never moves.  After each sweep tot and Q = in / M2 - gamma sum_c (tot[c] / M2)^2 are recomputed, ``in`` the
int64 sum of the entries whose two ends share a label; the fp64 part of Q is one host function (``_q``) run on the
CPU from the integers.  The level keeps the best labelling seen (Q above the best so far by more than ``tol``) and
stops after an up and a down sweep in a row that moved nothing, after 4 sweeps in a row without a new best, or
after ``max_sweeps``.  Level 0 needs tens of sweeps, labels travel one hop per sweep, and may hit ``max_sweeps``:
the best labelling is kept and the next level finishes the job.

Between levels (torch, integers only): the communities are renumbered 0 .. G' - 1 by ascending old label, the coarse
entries are the int64 sums of wq per (label[row], label[col]), rows and columns ascending; the levels stop when
one merged nothing, or after ``max_levels``.  Final labels: communities by descending size, ties by smallest member
row; rows without a counting entry get -1.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _args, _lib

SHIFT = 24                 # wq = rint(w 2^SHIFT)
GROUP_LEN = 64             # include/spmf_hip.h SPMF_MOVE_GROUP_LEN: longer rows go on the sweep's long_rows list
M2_LIMIT = 2 ** 62
STALE_SWEEPS = 4           # sweeps in a row without a new best after which a level stops


# ---- arguments ---------------------------------------------------------------------------------------------------
def check_args(name, resolution, max_levels, max_sweeps, tol):
    """The arguments of ``solve`` / ``communities`` that need no graph -> (gamma, max_levels, max_sweeps, tol)."""
    gamma = _args.number(name, "resolution", resolution, positive=True)
    max_levels = _args.integer(name, "max_levels", max_levels, 1, 2 ** 31 - 1)
    max_sweeps = _args.integer(name, "max_sweeps", max_sweeps, 1, 2 ** 31 - 1)
    return gamma, max_levels, max_sweeps, _args.number(name, "tol", tol)


# ---- integers ------------------------------------------------------------------------------------------------------
def quantise(weights):
    """wq = rint(double(w) 2^24) as int64, of a tensor (on its device) or an array (numpy).  A non-finite weight
    becomes 0 (it does not count); one beyond 2^62 becomes 2^62, which ``solve`` refuses through M2."""
    if isinstance(weights, torch.Tensor):
        w = weights.to(torch.float64) * float(2 ** SHIFT)
        w = torch.where(torch.isfinite(w), w, torch.zeros_like(w)).clamp(-float(M2_LIMIT), float(M2_LIMIT))
        return torch.round(w).to(torch.int64)                      # half to even, as rint
    w = np.asarray(weights, dtype=np.float64) * float(2 ** SHIFT)
    w = np.clip(np.where(np.isfinite(w), w, 0.0), -float(M2_LIMIT), float(M2_LIMIT))
    return np.rint(w).astype(np.int64)


def _tensor(v, dtype):
    return (v.detach() if isinstance(v, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(v))).to(dtype)


def _wq_of(graph):
    """int64 weights of a graph dict: its 'wq' where it has one (a coarse level), else ``quantise`` of 'weights'."""
    if "wq" in graph:
        return _tensor(graph["wq"], torch.int64)
    return quantise(_tensor(graph["weights"], torch.float64))


def _valid(indptr, indices, wq):
    """``spectral.valid_edges``' rules in torch integers on the tensors' device -> (N, row, col, wq) int64, in
    list order."""
    n, nnz = int(indptr.numel()) - 1, int(indices.numel())
    dev = indptr.device
    ptr = indptr.to(torch.int64).clamp(0, nnz)
    lens = (ptr[1:] - ptr[:-1]).clamp_min(0)
    row = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), lens)
    first = torch.cumsum(lens, 0) - lens
    pos = ptr[:-1][row] + (torch.arange(int(row.numel()), dtype=torch.int64, device=dev) - first[row])
    col, w = indices[pos].to(torch.int64), wq[pos]
    keep = (col >= 0) & (col < n) & (w >= 1)
    return n, row[keep], col[keep], w[keep]


def valid_edges(graph):
    """The entries of a graph dict (tensors or arrays; 'weights' float32, or 'wq' int64) that count ->
    (N, row int64, col int64, wq int64) as numpy, in list order."""
    n, row, col, wq = _valid(_tensor(graph["indptr"], torch.int64).cpu(), _tensor(graph["indices"], torch.int64).cpu(),
                             _wq_of(graph).cpu())
    return n, row.numpy(), col.numpy(), wq.numpy()


def _q(inside, tot, m2, gamma):
    """Q = in / M2 - gamma sum_c (tot[c] / M2)^2 in fp64 on the CPU from the integers: the one place modularity
    is rounded, shared by the backends."""
    t = np.asarray(tot, dtype=np.int64).astype(np.float64) / float(m2)
    return int(inside) / int(m2) - gamma * float(np.sum(t * t))


def _measure(labels, before, row, col, wq, k, m2, gamma):
    """A labelling's integers in one read-back -> (rows whose label differs from ``before``, Q, tot int64 [n] by
    label where the labels live).  ``in`` is the int64 sum of the entries whose two ends share a label."""
    lab = labels.to(torch.int64)
    inside = torch.where(lab[row] == lab[col], wq, torch.zeros_like(wq)).sum()
    tot = torch.zeros_like(k).index_add_(0, lab, k)
    moved = (labels != before).sum()
    host = torch.cat([moved.reshape(1), inside.reshape(1), tot]).cpu().numpy()
    return int(host[0]), _q(int(host[1]), host[2:], m2, gamma), tot


def modularity(labels, graph, resolution=1.0):
    """Q of a labelling (integers [N]; negative = in no community, allowed only on rows without a counting entry)
    on the fixed-point weights of ``graph``, the value ``solve`` reports for its own labels."""
    n, row, col, wq = valid_edges(graph)
    lab = np.asarray(labels.detach().cpu() if isinstance(labels, torch.Tensor) else labels).astype(np.int64)
    if lab.shape != (n,):
        raise ValueError(f"modularity: labels must have one entry per row, got {lab.shape} for {n} rows")
    if len(row) and (lab[row].min() < 0 or lab[col].min() < 0):
        raise ValueError("modularity: a row with a counting entry has a negative label")
    m2 = int(wq.sum())
    if m2 <= 0:
        return float("nan")
    _, dense = np.unique(np.where(lab < 0, -1, lab), return_inverse=True)
    k = np.zeros(n, dtype=np.int64)
    np.add.at(k, row, wq)
    tot = np.zeros(n + 1, dtype=np.int64)
    np.add.at(tot, dense, k)
    inside = int(wq[lab[row] == lab[col]].sum())
    return _q(inside, tot, m2, float(resolution))


def aggregate(labels, row, col, wq):
    """The coarse graph of a labelling, in torch integers: the communities renumbered 0 .. G' - 1 by ascending
    old label, the entries the int64 sums of wq per (label[row], label[col]), rows and columns ascending (a
    community's internal weight is its self entry) -> (G', new label of every node, row, col, wq)."""
    uniq, inv = torch.unique(labels.to(torch.int64), return_inverse=True)
    g = int(uniq.numel())
    key, back = torch.unique(inv[row] * g + inv[col], return_inverse=True)
    w = torch.zeros(int(key.numel()), dtype=torch.int64, device=wq.device).index_add_(0, back, wq)
    r = torch.div(key, max(g, 1), rounding_mode="floor")
    return g, inv, r, key - r * g, w


def canonical_labels(assign, live):
    """The final numbering: communities by descending size, ties by smallest member row; rows that are not
    ``live`` (no counting entry) get -1 and count in no size -> (labels int64 [N], sizes int64 [G]), numpy."""
    assign = np.asarray(assign, dtype=np.int64)
    live = np.asarray(live, dtype=bool)
    n = len(assign)
    out = np.full(n, -1, dtype=np.int64)
    rows = np.flatnonzero(live)
    if not len(rows):
        return out, np.zeros(0, dtype=np.int64)
    uniq, first, inv, size = np.unique(assign[rows], return_index=True, return_inverse=True, return_counts=True)
    order = np.lexsort((rows[first], -size))              # by size descending, then by the smallest member row
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    out[rows] = rank[inv]
    return out, size[order].astype(np.int64)


def _csr(n, row, col, wq):
    """(indptr int64 [n + 1], indices int32, wq int64) of entries sorted by row."""
    indptr = torch.searchsorted(row.contiguous(), torch.arange(n + 1, dtype=torch.int64, device=row.device))
    return indptr.to(torch.int64).contiguous(), col.to(torch.int32).contiguous(), wq.contiguous()


# ---- the two backends ----------------------------------------------------------------------------------------------
class NumpyOps:
    """The sweep as a vectorised numpy restatement of its definition, on a graph dict (tensors or arrays, 'weights'
    or 'wq'), read as it stands.  The driver's tensors live on the CPU."""

    device = torch.device("cpu")

    def __init__(self, graph):
        self._graph = graph
        self.set_level(*self._arrays(graph))

    @staticmethod
    def _arrays(graph):
        return (int(len(graph["indptr"])) - 1, _tensor(graph["indptr"], torch.int64).cpu(),
                _tensor(graph["indices"], torch.int32).cpu(), _wq_of(graph).cpu())

    def edges(self):
        """The counting entries of the graph the ops were made on -> (N, row, col, wq) int64 tensors."""
        _, indptr, indices, wq = self._arrays(self._graph)
        return _valid(indptr, indices, wq)

    def set_level(self, n, indptr, indices, wq):
        self.n, self.row, self.col, self.wq = (v if isinstance(v, int) else v.numpy()
                                               for v in _valid(indptr, indices, wq))
        self.k = np.zeros(self.n, dtype=np.int64)
        np.add.at(self.k, self.row, self.wq)

    def move(self, labels, tot, gamma, m2, direction):
        """One sweep -> new labels (an int32 tensor).  Sort by (row, label), ``np.add.reduceat`` on int64, the fp64
        formula operation by operation."""
        n, k = self.n, self.k
        lab = np.asarray(labels).astype(np.int64)
        tot = np.asarray(tot).astype(np.int64)
        out = lab.copy()
        own_ok = (lab >= 0) & (lab < n)
        link = self.col != self.row
        r, c, w = self.row[link], lab[self.col[link]], self.wq[link]
        order = np.lexsort((c, r))
        r, c, w = r[order], c[order], w[order]
        if not len(r):
            return torch.from_numpy(out.astype(np.int32))
        start = np.ones(len(r), dtype=bool)
        start[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
        at = np.flatnonzero(start)
        e, er, ec = np.add.reduceat(w, at), r[at], c[at]                 # e_ic of every (row, community) that occurs
        own = lab[er]
        e_own = np.zeros(n, dtype=np.int64)
        e_own[er[ec == own]] = e[ec == own]
        m2d, gk = float(m2), float(gamma) * k.astype(np.float64)
        safe = np.where(own_ok, lab, 0)
        stay = e_own.astype(np.float64) - (gk * (tot[safe] - k).astype(np.float64)) / m2d
        cand = (ec >= 0) & (ec < n) & own_ok[er] & ((ec > own) if direction == 0 else (ec < own))
        e, er, ec = e[cand], er[cand], ec[cand]
        score = e.astype(np.float64) - (gk[er] * tot[ec].astype(np.float64)) / m2d
        first = np.lexsort((ec, -score, er))                              # per row: score descending, label ascending
        er, ec, score = er[first], ec[first], score[first]
        head = np.ones(len(er), dtype=bool)
        head[1:] = er[1:] != er[:-1]
        er, ec, score = er[head], ec[head], score[head]
        go = (score > stay[er]) & (k[er] > 0)
        out[er[go]] = ec[go]
        return torch.from_numpy(out.astype(np.int32))


class LibraryOps:
    """The sweep as the library's call on device tensors of a graph (indptr int64, indices int32, weights float32).
    The list of long rows is made once per level from indptr."""

    def __init__(self, lib, handle, indptr, indices, weights):
        self.lib, self.h = lib, handle
        self.device = indptr.device
        self._graph = (indptr.contiguous(), indices.contiguous(), quantise(weights).contiguous())

    def edges(self):
        return _valid(*self._graph)

    def set_level(self, n, indptr, indices, wq):
        self.n, self.g = n, (indptr.contiguous(), indices.contiguous(), wq.contiguous())
        self.long = torch.nonzero(torch.diff(indptr) > GROUP_LEN).reshape(-1).to(torch.int32).contiguous()

    def move(self, labels, tot, gamma, m2, direction):
        out = torch.empty_like(labels)
        n_long = int(self.long.numel())
        _lib.call(self.h, "spmf_graph_move", self.n, int(self.g[1].numel()), self.g[0].data_ptr(),
                  self.g[1].data_ptr(), self.g[2].data_ptr(), labels.data_ptr(), tot.data_ptr(),
                  self.long.data_ptr() if n_long else None, n_long, float(gamma), int(m2), int(direction),
                  out.data_ptr(), device=self.device)
        return out


# ---- the driver ------------------------------------------------------------------------------------------------------
def _one_level(ops, n, row, col, wq, m2, gamma, max_sweeps, tol):
    """The sweeps of one level -> (best labels int32 [n], its Q, sweeps made, whether max_sweeps ended them)."""
    labels = torch.arange(n, dtype=torch.int32, device=wq.device)
    k = torch.zeros(n, dtype=torch.int64, device=wq.device).index_add_(0, row, wq)
    _, best_q, tot = _measure(labels, labels, row, col, wq, k, m2, gamma)
    best = labels
    stale = still = sweeps = 0
    while sweeps < max_sweeps:
        new = ops.move(labels, tot, gamma, m2, sweeps & 1)
        moved, q, tot = _measure(new, labels, row, col, wq, k, m2, gamma)
        labels = new
        sweeps += 1
        if q > best_q + tol:
            best, best_q, stale = labels, q, 0
        else:
            stale += 1
        still = still + 1 if moved == 0 else 0
        if still >= 2 or stale >= STALE_SWEEPS:
            return best, best_q, sweeps, False
    return best, best_q, sweeps, True


def solve(ops, resolution=1.0, max_levels=32, max_sweeps=100, tol=1e-7, name="communities"):
    """Louvain clustering of the graph behind ``ops`` (a ``LibraryOps`` or a ``NumpyOps``) by the algorithm of this
    module's docstring.

    Returns a dict: 'labels' int64 [N] (a tensor where the ops live), communities numbered by descending size,
    ties by smallest member row, -1 for a row without a counting entry; 'n_communities'; 'sizes' int64
    [n_communities]; 'modularity', Q of the labels at ``resolution`` (NaN for a graph without a counting entry);
    'levels', per level a dict of 'n_nodes', 'n_communities', 'modularity', 'n_sweeps' and 'hit_max_sweeps';
    'resolution'.  The graph should be symmetric; an asymmetric one is not refused.  Bit-reproducible, and the same
    bits on both backends."""
    gamma, max_levels, max_sweeps, tol = check_args(name, resolution, max_levels, max_sweeps, tol)
    n0, row, col, wq = ops.edges()
    dev = wq.device
    m2 = int(wq.sum())
    if m2 >= M2_LIMIT:
        raise ValueError(f"{name}: the fixed-point weights sum to {m2}, beyond 2^62: scale the weights down")
    live = torch.zeros(n0, dtype=torch.bool, device=dev)
    live[row] = True
    assign = torch.arange(n0, dtype=torch.int64, device=dev)
    levels, n, q = [], n0, float("nan")
    while m2 > 0 and len(levels) < max_levels:
        ops.set_level(n, *_csr(n, row, col, wq))
        best, q, sweeps, hit = _one_level(ops, n, row, col, wq, m2, gamma, max_sweeps, tol)
        g, inv, row, col, wq = aggregate(best, row, col, wq)
        levels.append({"n_nodes": n, "n_communities": g, "modularity": q, "n_sweeps": sweeps, "hit_max_sweeps": hit})
        assign = inv[assign]
        if g == n:
            break
        n = g
    labels, sizes = canonical_labels(assign.cpu().numpy(), live.cpu().numpy())
    return {"labels": torch.from_numpy(labels).to(dev), "n_communities": int(len(sizes)),
            "sizes": torch.from_numpy(sizes).to(dev), "modularity": q, "levels": levels, "resolution": gamma}
