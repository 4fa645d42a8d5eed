"""What the test files of the shortest-path calls share (test_geodesic_host.py, test_gpu_geodesic.py,
test_gpu_geodesic_cli.py): the argument list of spmf_graph_relax, its raw call and its error contract, asserted without
a device on dummy addresses and with one on real buffers; the hand-made edge graph; the chain of four blobs and the
noisy spiral as graphs of lengths; and ``fp32_dijkstra``, the independent reference: a plain heap Dijkstra with
``np.float32`` additions, which the synchronous sweeps must equal bit for bit."""
import ctypes as C
import functools
import heapq
import math

import numpy as np
import torch

_P, _I64 = C.c_void_p, C.c_int64
ARGS = (("n", _I64), ("nnz", _I64), ("indptr", _P), ("indices", _P), ("lengths", _P), ("x_in", _P), ("x_out", _P),
        ("pred", _P), ("changed", _P), ("n_sweeps", C.c_int), ("ptr", _P), ("nbytes", C.c_size_t), ("stream", _P))
HEADER_ARGS = {"spmf_graph_relax": 14, "spmf_graph_relax_scratch_bytes": 2}
BLOCK = 16                                 # include/spmf_hip.h SPMF_BLOCK_COLS
EDGE_N = 83


def raw_call(good):
    """-> call(**overrides): spmf_graph_relax through a binding of its own with the arguments of ``good``."""
    from spmf_amd import _lib
    fn = C.CDLL(_lib.LIB_PATH).spmf_graph_relax
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [t for _, t in ARGS]

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], *[a[n] for n, _ in ARGS])
    return call


def scratch_bytes(lib, h, n):
    return int(lib.spmf_graph_relax_scratch_bytes(h, n))


def host_good(lib, h):
    """A valid-looking call that needs no device: dummy aligned addresses -- only refused calls may be made with
    it."""
    need = scratch_bytes(lib, h, EDGE_N)
    return dict(h=h, n=EDGE_N, nnz=300, indptr=0x1000000, indices=0x2000000, lengths=0x3000000, x_in=0x4000000,
                x_out=0x5000000, pred=0x6000000, changed=0x7000000, n_sweeps=3, ptr=0x8000000, nbytes=need,
                stream=None)


def assert_scratch_sizes(lib, h):
    """The size function: two blocks, a multiple of 256, non-decreasing in the rows, 0 for rows the call refuses."""
    last = 0
    for n in (0, 1, 15, 16, 17, 83, 4097, 122880, 2 ** 31 - 64):
        need = scratch_bytes(lib, h, n)
        assert need >= 2 * max(n, 1) * BLOCK * 4 and need % 256 == 0 and need >= last, (n, need, last)
        last = need
    for n in (-1, 2 ** 31 - 63, 2 ** 40):
        assert scratch_bytes(lib, h, n) == 0, n
    assert scratch_bytes(lib, None, 83) == 0


def assert_errors(lib, good, after=lambda: None):
    """The error contract of spmf_graph_relax; every call here returns before a launch or a write, and ``after`` is
    run behind each (the GPU file checks its sentinels there)."""
    call, h = raw_call(good), good["h"]

    def refused(code=-1, **kw):
        assert call(**kw) == code, kw
        msg = lib.spmf_last_error(h).decode()
        assert msg.startswith("graph_relax: "), msg
        after()
        return msg
    for rows in (-1, 2 ** 31 - 63, 2 ** 40):
        assert "n_rows" in refused(n=rows)
    assert "nnz" in refused(nnz=-1)
    for s in (-1, -(2 ** 31)):
        assert "n_sweeps" in refused(n_sweeps=s)
    for name in ("indptr", "indices", "lengths", "x_in", "x_out", "ptr"):
        assert "null" in refused(**{name: None})
    assert "null" in refused(n=0, ptr=None)                # the scratch is needed without rows too
    for out in ("x_out", "pred", "changed"):
        for src in ("indptr", "indices", "lengths"):
            assert "aliases" in refused(**{out: good[src]})
    assert "aliases" in refused(pred=good["x_out"])
    assert "aliases" in refused(changed=good["x_out"])
    assert "aliases" in refused(changed=good["pred"])
    assert "aliases" in refused(pred=good["x_in"])
    assert "aliases" in refused(changed=good["x_in"])
    assert "aligned" in refused(ptr=good["ptr"] + 4)
    assert str(good["nbytes"]) in refused(-3, nbytes=good["nbytes"] - 256)
    refused(n=0, n_sweeps=-1)                # errors come before the empty return
    refused(-3, n=0, nbytes=0)
    assert call(h=None) == -1


# ---- the hand-made edge graph ----------------------------------------------------------------------------------------
EDGE_LENGTHS = {2: 0, 3: 1, 4: 7, 5: 8, 6: 9, 7: 15, 8: 16, 9: 17, 10: 64, 11: 600}
EDGE_SPLIT = 60                            # rows 0 .. 59 and rows 60 .. 82 are two components
EDGE_JUNK, EDGE_NEAR, EDGE_ABSORBED, EDGE_TIE = 14, 30, 31, 33


@functools.lru_cache(maxsize=None)
def edge_graph():
    """The hand-made graph, N = 83 (no multiple of 16), float32 lengths -> dict(indptr, indices, weights: numpy);
    read-only.  Entry (i, j) of row i is the edge j -> i: row i pulls from the rows it lists.
      rows 2 .. 11: 0, 1, 7, 8, 9, 15, 16, 17, 64 and 600 entries (the edges of the eight-entry step); with 60 columns
        the long rows list columns many times over, at different lengths;
      row 14: column 5 twice, at 0.7 and then at 0.4, a self entry, columns -1 and N, and lengths 0, negative, +inf
        and NaN on good columns: none of the latter count;
      row 20 has a falling indptr and is empty, which makes row 21 re-read the tail of row 19 and all of row 20;
      rows 60 .. 82 list one another only, and no row below 60 lists them: from a source below 60 they stay +inf;
      row 30 = [(0, 1.0)] and row 31 = [(30, 1e-9)]: from source 0 row 30 is at 1, and fl(1 + 1e-9) = 1: the absorbed
        addition -- row 31 has the same distance and predecessor -1;
      row 33 = [(34, 0.5), (35, 0.25)], row 34 = [(0, 0.25)], row 35 = [(0, 0.5)]: from source 0 both entries of row 33
        give exactly 0.75, and the first in list order, 34, is the predecessor.
    Every other row has 3 .. 12 random entries inside its component with lengths in [0.05, 2)."""
    rng = np.random.default_rng(83)
    N, inf, nan = EDGE_N, float("inf"), float("nan")
    rows = []
    for i in range(N):
        d = EDGE_LENGTHS.get(i, int(rng.integers(3, 13)))
        lo, hi = (0, EDGE_SPLIT) if i < EDGE_SPLIT else (EDGE_SPLIT, N)
        col = rng.integers(lo, hi, size=d)
        w = rng.uniform(0.05, 2.0, size=d)
        rows.append([(int(c), float(v)) for c, v in zip(col, w)])
    rows[EDGE_JUNK] = [(5, 0.7), (14, 1.0), (5, 0.4), (-1, 0.5), (N, 0.5), (40, 0.0), (41, -3.0), (42, inf), (43, nan),
                       (50, 1.25), (51, 0.5)]
    rows[EDGE_NEAR], rows[EDGE_ABSORBED] = [(0, 1.0)], [(EDGE_NEAR, 1e-9)]
    rows[EDGE_TIE], rows[34], rows[35] = [(34, 0.5), (35, 0.25)], [(0, 0.25)], [(0, 0.5)]
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indptr[21] = indptr[20] - 3                # row 20: falling, empty; row 21 starts inside row 19
    flat = [e for r in rows for e in r]
    g = dict(indptr=indptr, indices=np.array([c for c, _ in flat], dtype=np.int32),
             weights=np.array([v for _, v in flat], dtype=np.float32))
    for v in g.values():
        v.setflags(write=False)
    return g


def edge_sources():
    """16 different sources for the 16 columns of one block on the edge graph: column 0 is row 0 (the absorbed
    addition and the tie are stated from it), column 15 is used, two lie in the second component and one is the row
    without entries."""
    return np.array([0, 1, 5, 9, 11, 14, 20, 21, 2, 31, 33, 45, 59, 60, 82, 7], dtype=np.int64)


# ---- the independent reference -----------------------------------------------------------------------------------
def _pull_lists(g):
    """Per row j the (i, length) of the counting entries (i, j), by a plain Python loop from the definition."""
    indptr, indices, w = (np.asarray(g[k].cpu() if isinstance(g[k], torch.Tensor) else g[k])
                          for k in ("indptr", "indices", "weights"))
    n, nnz = len(indptr) - 1, len(indices)
    out = [[] for _ in range(n)]
    for i in range(n):
        p0, p1 = (min(max(int(indptr[i + d]), 0), nnz) for d in (0, 1))
        for p in range(p0, p1):
            j, v = int(indices[p]), np.float32(w[p])
            if 0 <= j < n and np.isfinite(v) and v > 0:
                out[j].append((i, v))
    return out


def fp32_dijkstra(g, sources, lists=None):
    """A plain heap Dijkstra from the set ``sources`` on the graph dict ``g`` with ``np.float32`` additions, a path's
    lengths added from the source outwards -> float32 [N], +inf for unreached rows."""
    lists = _pull_lists(g) if lists is None else lists
    n = len(lists)
    dist = np.full(n, np.inf, dtype=np.float32)
    heap = []
    for s in np.atleast_1d(np.asarray(sources)).tolist():
        dist[s] = 0.0
        heap.append((0.0, int(s)))
    heapq.heapify(heap)
    done = np.zeros(n, dtype=bool)
    while heap:
        d, j = heapq.heappop(heap)
        if done[j]:
            continue
        done[j] = True
        for i, w in lists[j]:
            t = np.float32(d) + w                  # one float32 addition
            if t < dist[i]:
                dist[i] = t
                heapq.heappush(heap, (float(t), i))
    return dist


def scipy_dijkstra(g, sources):
    """scipy's fp64 ``dijkstra`` from the set ``sources`` on the counting entries (the smallest length of a repeated
    entry) -> fp64 [N]."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    from spmf_amd import spectral
    n, row, col, w = spectral.valid_edges(g)
    # entry (i, j) is the edge j -> i; duplicates would be summed by scipy, so keep the smallest
    order = np.lexsort((w, row, col))
    row, col, w = row[order], col[order], w[order].astype(np.float64)
    first = np.ones(len(row), dtype=bool)
    first[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
    m = sp.csr_matrix((w[first], (col[first], row[first])), shape=(n, n))
    return dijkstra(m, directed=True, indices=np.atleast_1d(np.asarray(sources)), min_only=True)


# ---- the graphs of points ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_lengths():
    """``_paga_cases.chain``'s four blobs as a graph of lengths: ``length_graph`` of their exact 10 nearest
    neighbours on the CPU -> (graph dict of CPU tensors, the points float32 [320, 8], the truth int64 [320])."""
    from _paga_cases import chain
    from spmf_amd import geodesic, neighbors
    _, x, truth = chain()
    idx, dist = neighbors.brute_force(x, x, 10, exclude_self=True)
    return geodesic.length_graph(idx, dist), x, truth


@functools.lru_cache(maxsize=None)
def spiral():
    """3 000 points on a noisy spiral, a worst case for the hop count: the symmetrised graph of their exact 10
    nearest neighbours, as lengths -> (graph dict of CPU tensors, the points float32 [3000, 2]).  The arms are 2 pi
    apart and the noise 0.5 wide, so the graph follows the curve."""
    from spmf_amd import geodesic, neighbors
    gen = torch.Generator(device="cpu")
    gen.manual_seed(11)
    t = 3.0 * math.pi * (0.25 + 1.25 * torch.rand(3000, generator=gen, dtype=torch.float64))
    xy = torch.stack([t * torch.cos(t), t * torch.sin(t)], 1) + 0.5 * torch.randn(3000, 2, generator=gen,
                                                                                    dtype=torch.float64)
    x = xy.to(torch.float32)
    idx, dist = neighbors.brute_force(x, x, 10, exclude_self=True)
    return geodesic.length_graph(idx, dist), x


def graph_numpy(g):
    """A graph dict of tensors as numpy arrays."""
    return {k: (g[k].cpu().numpy() if isinstance(g[k], torch.Tensor) else np.asarray(g[k]))
            for k in ("indptr", "indices", "weights")}
