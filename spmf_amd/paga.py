"""Host side of the coarse graph of the clusters (PoissonFactorization.paga / paga_init, spmf_graph_group_edges,
csrc/graph_groups.hip): PAGA, scanpy's ``tl.paga`` and the ``init_pos='paga'`` start of its ``tl.umap`` -- which
groups of rows touch in the neighbour graph, how much more than chance, and a layout start that keeps the groups'
global arrangement.  Importable without a GPU; numpy and torch only.

Everything is an integer except one function.  The graph comes from ``fuzzy_graph`` (symmetric) or ``knn_graph``
(the directed kNN graph with unit weights, what scanpy's PAGA counts on); the labels from ``communities``,
``cluster``, ``spectral_cluster`` or a file.  The weights become ``communities.quantise``'s fixed point, so the
reduction of the entries by (label of row, label of column) is a sum of integers: exact, the same in any order, on
any backend.  The driver (``solve``) is written once over an ops interface with two backends: ``LibraryOps``, whose
``group_edges`` is the library's call on the device, and ``NumpyOps``, whose ``group_edges`` is ``np.add.at`` on
int64.  The two agree bit for bit, and so does everything made from their integers, because the fp64 part
(``connectivity``) is one host function run on the CPU, shared by the backends like ``communities._q``.

An entry (i, j) counts when a = label[i] and b = label[j] both lie in [0, G), j lies in [0, N) and wq >= 1; indptr
is read under spmf_graph_spmm's rules (clamped to [0, nnz], a falling indptr an empty row); self entries and
repeated columns count as listed.  count[a, b] is the number of counting entries, weight[a, b] the int64 sum of
their wq, size[a] the number of rows labelled a.  A negative label is "no group".
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _args, _lib
from . import communities as _communities

MAX_GROUPS = 1024          # include/spmf_hip.h SPMF_GROUP_EDGES_MAX_GROUPS: a group's row of the tables lives in LDS
START_RADIUS = 10.0        # of ``group_start``'s circle, and the largest |coordinate| of ``layout_init``


# ---- the graph and the labels ------------------------------------------------------------------------------------
def knn_graph(indices):
    """The directed graph of a ``knn`` result with unit weights: ``indices`` [N, k] integers (row i lists the
    neighbours of row i; padding -1) -> {'indptr': int64 [N + 1] = k arange(N + 1), 'indices': int32 [N k],
    'weights': float32 ones} on the device of ``indices``.  Padding entries stay in the list and do not count.
    This is the graph scanpy's PAGA counts on; ``PoissonFactorization.paga`` checks a graph's indices as
    ``graph_layout`` does, so a result with padding goes to ``solve`` directly."""
    idx = torch.as_tensor(indices)
    if idx.dim() != 2 or idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise ValueError(f"knn_graph: indices must be 2-D integers [N, k], got {idx.dtype} {tuple(idx.shape)}")
    n, k = int(idx.shape[0]), int(idx.shape[1])
    return {"indptr": k * torch.arange(n + 1, dtype=torch.int64, device=idx.device),
            "indices": idx.reshape(-1).to(torch.int32).contiguous(),
            "weights": torch.ones(n * k, dtype=torch.float32, device=idx.device)}


def group_count(name, labels, n_groups=None):
    """G of a labelling: ``n_groups``, or max label + 1 (at least 1) for None.  ``labels``: a 1-D integer tensor;
    negative is "no group"; a label >= ``n_groups`` and a G beyond ``MAX_GROUPS`` are refused."""
    if labels.dim() != 1 or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f"{name}: labels must be 1-D integers, got {labels.dtype} {tuple(labels.shape)}")
    top = int(labels.max()) if labels.numel() else -1
    if n_groups is None:
        G = max(top + 1, 1)
    else:
        G = _args.integer(name, "n_groups", n_groups, 1)
        if top >= G:
            raise ValueError(f"{name}: labels must lie below n_groups = {G} (negative: no group), got {top}")
    if G > MAX_GROUPS:
        raise ValueError(f"{name}: {G} groups are beyond the limit of {MAX_GROUPS} (a group's row of the table is "
                         f"kept on chip)")
    return G


# ---- the two backends --------------------------------------------------------------------------------------------
class NumpyOps:
    """The reduction as ``np.add.at`` on int64, on a graph dict (tensors or arrays, 'weights' or 'wq'), read as it
    stands.  The driver's tensors live on the CPU."""

    device = torch.device("cpu")

    def __init__(self, graph):
        _, indptr, indices, wq = _communities.NumpyOps._arrays(graph)
        self.n, self.row, self.col, self.wq = (v if isinstance(v, int) else v.numpy()
                                               for v in _communities._valid(indptr, indices, wq))

    def total(self):
        """The sum of the counting wq, a Python integer."""
        return int(self.wq.sum())

    def group_edges(self, labels, n_groups):
        """-> (count [G, G], weight [G, G], size [G]) int64 tensors of ``labels`` (int32 [N])."""
        G = int(n_groups)
        lab = np.asarray(labels).astype(np.int64)
        a, b = lab[self.row], lab[self.col]
        keep = (a >= 0) & (a < G) & (b >= 0) & (b < G)
        key = a[keep] * G + b[keep]
        count = np.zeros(G * G, dtype=np.int64)
        weight = np.zeros(G * G, dtype=np.int64)
        np.add.at(count, key, 1)
        np.add.at(weight, key, self.wq[keep])
        size = np.zeros(G, dtype=np.int64)
        np.add.at(size, lab[(lab >= 0) & (lab < G)], 1)
        return (torch.from_numpy(count.reshape(G, G)), torch.from_numpy(weight.reshape(G, G)),
                torch.from_numpy(size))


class LibraryOps:
    """The reduction as the library's call on device tensors of a graph (indptr int64, indices int32, weights
    float32), on ``communities.quantise``d weights."""

    def __init__(self, lib, handle, indptr, indices, weights):
        self.lib, self.h = lib, handle
        self.device = indptr.device
        self.n = int(indptr.numel()) - 1
        self.g = (indptr.contiguous(), indices.contiguous(), _communities.quantise(weights).contiguous())

    def total(self):
        return int(_communities._valid(*self.g)[3].sum())

    def group_edges(self, labels, n_groups):
        G = int(n_groups)
        labels = labels.contiguous()
        count, weight = (torch.empty(G, G, dtype=torch.int64, device=self.device) for _ in range(2))
        size = torch.empty(G, dtype=torch.int64, device=self.device)
        _lib.call(self.h, "spmf_graph_group_edges", self.n, int(self.g[1].numel()), self.g[0].data_ptr(),
                  self.g[1].data_ptr(), self.g[2].data_ptr(), labels.data_ptr(), G, count.data_ptr(),
                  weight.data_ptr(), size.data_ptr(), device=self.device,
                  scratch=(_lib.Scratch(self.device), "spmf_graph_group_edges_scratch_bytes", self.n, G))
        return count, weight, size


# ---- the one fp64 function ---------------------------------------------------------------------------------------
def connectivity(count, size):
    """PAGA's connectivities from the integers, in fp64 on the CPU: the one place they are rounded, shared by the
    backends -> (conn, expected) fp64 [G, G] numpy.

    With n = sum size and es[a] = sum_b count[a, b], for a != b: sym = count[a, b] + count[b, a],
    expected[a, b] = float(es[a] size[b] + es[b] size[a]) / float(n - 1), the numerator an exact integer, and
    conn[a, b] = min(1, sym / expected) where sym > 0 (1 where expected is 0), 0 where sym = 0.  Both diagonals are
    zero, and n <= 1 gives all zeros.  This is the model of scanpy's ``tl.paga`` (model='v1.2'): the entries between
    two groups against their number were the rows' entries spread over all other rows alike.  scanpy is not a
    dependency and is not compared with: the parity is by this definition.

    Example: rows 0, 1 in group 0 and rows 2, 3 in group 1, entries 0->1, 1->0, 1->2, 2->3, 3->2, 2->1:
    count = [[2, 1], [1, 2]], es = [3, 3], expected[0, 1] = (3 2 + 3 2) / 3 = 4, conn[0, 1] = 2 / 4 = 0.5."""
    count = np.asarray(count.cpu() if isinstance(count, torch.Tensor) else count).astype(np.int64)
    size = np.asarray(size.cpu() if isinstance(size, torch.Tensor) else size).astype(np.int64)
    G = int(size.shape[0])
    if count.shape != (G, G):
        raise ValueError(f"connectivity: count must be [{G}, {G}] for {G} sizes, got {count.shape}")
    conn, expected = np.zeros((G, G)), np.zeros((G, G))
    n = int(size.sum())
    if n <= 1:
        return conn, expected
    es = count.sum(1)
    if 2 * int(es.max(initial=0)) * int(size.max(initial=0)) < 2 ** 63:
        num = np.outer(es, size)
        num = (num + num.T).astype(np.float64)            # an int64 rounds to fp64 as a Python integer does
    else:
        num = np.outer(es.astype(object), size.astype(object))
        num = (num + num.T).astype(np.float64)
    off = ~np.eye(G, dtype=bool)
    expected = np.where(off, num / float(n - 1), 0.0)
    sym = np.where(off, count + count.T, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(expected > 0, np.minimum(1.0, sym.astype(np.float64) / expected), 1.0)
    return np.where(sym > 0, ratio, 0.0), expected


def tree(conn):
    """The maximum spanning forest of the connectivities: Kruskal over the pairs a < b with conn[a, b] > 0 ordered
    by (conn descending, a ascending, b ascending) -> fp64 [G, G] numpy, symmetric, conn on the kept pairs."""
    conn = np.asarray(conn, dtype=np.float64)
    G = int(conn.shape[0])
    a, b = np.nonzero(np.triu(conn > 0, 1))
    order = np.lexsort((b, a, -conn[a, b]))
    root = list(range(G))

    def find(v):
        while root[v] != v:
            root[v] = root[root[v]]
            v = root[v]
        return v
    out = np.zeros((G, G))
    for i, j in zip(a[order].tolist(), b[order].tolist()):
        ri, rj = find(i), find(j)
        if ri != rj:
            root[max(ri, rj)] = min(ri, rj)
            out[i, j] = out[j, i] = conn[i, j]
    return out


# ---- the driver ------------------------------------------------------------------------------------------------------
def solve(ops, labels, n_groups=None, name="paga"):
    """PAGA of the graph behind ``ops`` (a ``LibraryOps`` or a ``NumpyOps``) under ``labels``: int32 or int64 [N]
    (numpy or torch on any device), negative = in no group; ``n_groups`` = None is max label + 1.

    Returns a dict: 'connectivities', 'connectivities_tree' and 'expected' (fp64 [G, G] tensors where the ops
    live; ``connectivity`` and ``tree``), 'edge_count' and 'edge_weight' (int64 [G, G]: the counting entries from
    group a to group b and the sum of their fixed-point weights, the diagonal the entries inside a group),
    'sizes' (int64 [G]) and 'n_groups'.  More than ``MAX_GROUPS`` groups and fixed-point weights that sum to 2^62
    or more are refused.  Bit-reproducible, and the same bits on both backends."""
    lab = labels.detach() if isinstance(labels, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(labels))
    G = group_count(name, lab, n_groups)
    if int(lab.numel()) != ops.n:
        raise ValueError(f"{name}: labels must have one entry per row, got {int(lab.numel())} for {ops.n} rows")
    total = ops.total()
    if total >= _communities.M2_LIMIT:
        raise ValueError(f"{name}: the fixed-point weights sum to {total}, beyond 2^62: scale the weights down")
    lab32 = lab.to(torch.int64).clamp_min(-1).to(torch.int32).to(ops.device)       # (below G <= 1024 or refused)
    count, weight, size = ops.group_edges(lab32, G)
    conn, expected = connectivity(count, size)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)
    return {"connectivities": dev(conn), "connectivities_tree": dev(tree(conn)), "expected": dev(expected),
            "edge_count": count, "edge_weight": weight, "sizes": size, "n_groups": G}


# ---- the start of a layout ---------------------------------------------------------------------------------------
def group_start(n_groups):
    """The start of the coarse graph's layout: ``n_groups`` points on a circle of radius 10 in label order (one
    group: the origin) -> float32 [G, 2] on the CPU."""
    G = _args.integer("group_start", "n_groups", n_groups, 1)
    if G == 1:
        return torch.zeros(1, 2, dtype=torch.float32)
    t = 2.0 * math.pi * torch.arange(G, dtype=torch.float64) / G
    return (START_RADIUS * torch.stack([torch.cos(t), torch.sin(t)], 1)).to(torch.float32).contiguous()


def layout_init(labels, positions, conn, seed=0):
    """The start of a layout from the groups' positions, scanpy's ``init_pos='paga'`` rule: a group a with a
    neighbour takes nb = argmax_b conn[a, b] (ties to the smaller b) and d = pos[a] - pos[nb], and its rows start
    at pos[a] - d / 2 + u o d, spread over the box of the half way to the nearest group; u is one [N, 2] uniform
    draw from a CPU generator seeded with ``seed``, in row order.  A group without a neighbour starts on pos[a], a
    row without a group (a label outside [0, G)) at the origin.  The whole is scaled so that the largest
    |coordinate| is 10, as ``graph.init_pca`` does -> float32 [N, 2] on the device of ``labels`` (a tensor) or the
    CPU, to pass as ``graph_layout(init=...)``."""
    lab = labels.detach() if isinstance(labels, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(labels))
    dev = lab.device
    pos = torch.as_tensor(positions).detach().cpu().to(torch.float64)
    conn = torch.as_tensor(conn).detach().cpu().to(torch.float64)
    if pos.dim() != 2 or int(pos.shape[1]) != 2 or int(pos.shape[0]) < 1:
        raise ValueError(f"layout_init: positions must be [G, 2], got {tuple(pos.shape)}")
    G = int(pos.shape[0])
    if tuple(conn.shape) != (G, G):
        raise ValueError(f"layout_init: conn must be [{G}, {G}], got {tuple(conn.shape)}")
    if lab.dim() != 1 or lab.dtype.is_floating_point or lab.dtype == torch.bool:
        raise ValueError(f"layout_init: labels must be 1-D integers, got {lab.dtype} {tuple(lab.shape)}")
    seed = _args.integer("layout_init", "seed", seed, 0, 2 ** 63 - 1)
    lab = lab.cpu().to(torch.int64)
    n = int(lab.numel())
    off = conn.clone()
    off.fill_diagonal_(0.0)
    best = off.max(1).values
    # argmax with ties to the smaller b: the first column that holds the row's maximum
    nb = (off == best[:, None]).to(torch.int64).argmax(1)
    d = torch.where((best > 0)[:, None], pos - pos[nb], torch.zeros_like(pos))
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    u = torch.rand(n, 2, generator=gen, dtype=torch.float64)
    member = (lab >= 0) & (lab < G)
    g = torch.where(member, lab, torch.zeros_like(lab))
    out = torch.where(member[:, None], pos[g] - 0.5 * d[g] + u * d[g], torch.zeros(n, 2, dtype=torch.float64))
    top = float(out.abs().max()) if n else 0.0
    if top > 0 and math.isfinite(top):
        out = out * (START_RADIUS / top)
    return out.to(torch.float32).to(dev).contiguous()


def coarse_graph(conn, threshold=0.0):
    """The graph of the groups: the entries conn[a, b] > ``threshold`` of a [G, G] tensor, as a graph dict
    ('indptr' int64 [G + 1], 'indices' int32, 'weights' float32) on the device of ``conn``."""
    conn = torch.as_tensor(conn)
    keep = conn > float(threshold)
    a, b = torch.nonzero(keep, as_tuple=True)                # row-major: rows ascending, columns ascending in a row
    G = int(conn.shape[0])
    indptr = torch.searchsorted(a.contiguous(), torch.arange(G + 1, dtype=torch.int64, device=conn.device))
    return {"indptr": indptr.to(torch.int64).contiguous(), "indices": b.to(torch.int32).contiguous(),
            "weights": conn[a, b].to(torch.float32).contiguous()}
