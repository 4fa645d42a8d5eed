"""What the test files of graph clustering share (test_communities_host.py, test_gpu_communities.py,
test_gpu_communities_cli.py): the argument list of spmf_graph_move, its raw call and its error contract, asserted
without a device on dummy addresses and with one on real buffers; the small graphs of the end-to-end tests (blobs,
two rings, a ring of cliques) with networkx's view of them; and the hand-made "edge" graph of the one-sweep test."""
import ctypes as C
import functools

import numpy as np
import torch

from _spectral_cases import rings

_P, _I64 = C.c_void_p, C.c_int64
ARGS = (("n", _I64), ("nnz", _I64), ("indptr", _P), ("indices", _P), ("wq", _P), ("labels_in", _P), ("tot", _P),
        ("long_rows", _P), ("n_long", _I64), ("gamma", C.c_double), ("m2", _I64), ("direction", C.c_int),
        ("labels_out", _P), ("stream", _P))
HEADER_ARGS = {"spmf_graph_move": 15}      # the argument count of include/spmf_hip.h
GROUP_LEN = 64                             # include/spmf_hip.h SPMF_MOVE_GROUP_LEN


def raw_call(good):
    """-> call(**overrides): spmf_graph_move through a binding of its own with the arguments of ``good``."""
    from spmf_amd import _lib
    fn = C.CDLL(_lib.LIB_PATH).spmf_graph_move
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [t for _, t in ARGS]

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], *[a[n] for n, _ in ARGS])
    return call


def host_good(h):
    """A valid-looking call that needs no device: dummy aligned addresses -- only refused and empty calls may be
    made with it."""
    return dict(h=h, n=83, nnz=300, indptr=0x1000000, indices=0x2000000, wq=0x3000000, labels_in=0x4000000,
                tot=0x5000000, long_rows=0x6000000, n_long=3, gamma=1.0, m2=1 << 40, direction=0,
                labels_out=0x7000000, stream=None)


def assert_errors(lib, good, after=lambda: None):
    """The error contract of spmf_graph_move; every call here returns before a launch, and ``after`` is run behind
    each (the GPU file checks its sentinels there)."""
    call, h = raw_call(good), good["h"]
    nan, inf = float("nan"), float("inf")

    def refused(**kw):
        assert call(**kw) == -1, kw
        msg = lib.spmf_last_error(h).decode()
        assert msg.startswith("graph_move: "), msg
        after()
        return msg
    for rows in (-1, 2 ** 31 - 63, 2 ** 40):
        assert "n_rows" in refused(n=rows)
    assert "nnz" in refused(nnz=-1)
    for count in (-1, 2 ** 31 - 63):
        assert "n_long" in refused(n_long=count)
    for name in ("indptr", "indices", "wq", "labels_in", "tot", "labels_out", "long_rows"):
        assert "null" in refused(**{name: None})
    for v in (0.0, -1.0, nan, inf, -inf):
        assert "gamma" in refused(gamma=v)
    for v in (0, -1, -2 ** 62):
        assert "m2" in refused(m2=v)
    for v in (-1, 2):
        assert "direction" in refused(direction=v)
    assert "aliases" in refused(labels_out=good["labels_in"])
    refused(n=0, gamma=nan)                  # errors come before the empty return
    assert call(n=0) == 0
    assert call(n=0, indptr=None, labels_in=None, tot=None, labels_out=None) == 0
    after()
    assert call(h=None) == -1


# ---- the graphs of the end-to-end tests ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blobs(n_blobs=6, per=100, dim=8, k=10, seed=11):
    """6 far-apart Gaussian blobs of 100 points in 8 dimensions (centres 6 N(0, I), unit noise) -> (the fuzzy graph of
    their exact kNN on the CPU, the points float32 [600, 8], the truth int64 [600]); read-only."""
    from spmf_amd import graph, neighbors
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    centres = 6.0 * torch.randn(n_blobs, dim, generator=gen, dtype=torch.float64)
    truth = torch.arange(n_blobs).repeat_interleave(per)
    x = (centres[truth] + torch.randn(n_blobs * per, dim, generator=gen, dtype=torch.float64)).to(torch.float32)
    idx, dist = neighbors.brute_force(x, x, k, exclude_self=True)
    return graph.fuzzy_graph(idx, dist), x, truth


def two_rings():
    """Two concentric rings, N = 400: the fuzzy graph of ``_spectral_cases.rings``."""
    return rings()[0]


@functools.lru_cache(maxsize=None)
def cliques(n_cliques=30, size=5):
    """A ring of 30 cliques of 5 rows, unit weights, neighbouring cliques joined by one edge -> (graph, the clique of
    every row).  Known optimum at resolution 1: the cliques merge in pairs (the resolution limit)."""
    n = n_cliques * size
    pairs = set()
    for c in range(n_cliques):
        rows = range(c * size, (c + 1) * size)
        pairs |= {(i, j) for i in rows for j in rows if i != j}
        a, b = c * size + size - 1, ((c + 1) % n_cliques) * size
        pairs |= {(a, b), (b, a)}
    e = np.array(sorted(pairs), dtype=np.int64)
    indptr = np.searchsorted(e[:, 0], np.arange(n + 1)).astype(np.int64)
    g = {"indptr": torch.from_numpy(indptr), "indices": torch.from_numpy(e[:, 1].astype(np.int32)),
         "weights": torch.ones(len(e), dtype=torch.float32)}
    return g, np.arange(n) // size


def end_to_end_graphs():
    return (("blobs", blobs()[0]), ("rings", two_rings()), ("cliques", cliques()[0]))


def nx_graphs(graph):
    """networkx's view of a graph on its dequantised weights wq / 2^24 -> (the DiGraph of all counting entries, on
    which networkx's modularity is in / M2 - gamma sum (tot / M2)^2 whatever the self entries; the undirected Graph
    of the entries with row < col, what ``louvain_communities`` takes)."""
    import networkx as nx
    from spmf_amd import communities
    n, row, col, wq = communities.valid_edges(graph)
    w = wq.astype(np.float64) / 2.0 ** 24
    di, un = nx.DiGraph(), nx.Graph()
    di.add_nodes_from(range(n))
    un.add_nodes_from(range(n))
    di.add_weighted_edges_from((int(r), int(c), float(v)) for r, c, v in zip(row, col, w))
    un.add_weighted_edges_from((int(r), int(c), float(v)) for r, c, v in zip(row, col, w) if r < c)
    return di, un


def partition(labels):
    """The communities of a labelling as a list of sets; a row labelled -1 is a community of its own."""
    labels = np.asarray(labels)
    groups = {}
    for i, c in enumerate(labels.tolist()):
        groups.setdefault(c if c >= 0 else ("alone", i), set()).add(i)
    return list(groups.values())


@functools.lru_cache(maxsize=None)
def nx_louvain_range(name):
    """(min, max) of networkx's modularity of ``louvain_communities(seed=s)``, s = 0..9, on an end-to-end graph:
    the reference's own quality and spread, computed once."""
    import networkx as nx
    g = dict(end_to_end_graphs())[name]
    _, un = nx_graphs(g)
    qs = [nx.community.modularity(un, nx.community.louvain_communities(un, weight="weight", seed=s), weight="weight")
          for s in range(10)]
    return min(qs), max(qs)


# ---- the one-sweep case ----------------------------------------------------------------------------------------------
EDGE_N = 83
EDGE_LENGTHS = {2: 0, 3: 1, 4: 15, 5: 16, 6: 17, 7: 63, 8: 64, 9: 65, 10: 255, 11: 256, 12: 257, 13: 600, 20: 40,
                21: 30}
EDGE_LONG = (9, 10, 11, 12, 13, 21)      # the rows of more than 64 entries (21: behind the falling indptr)
EDGE_TIE_UP, EDGE_TIE_DOWN, EDGE_WRONG_SIDE = 30, 33, 36


@functools.lru_cache(maxsize=None)
def edge_graph():
    """The hand-made graph of the one-sweep test, N = 83 (no multiple of 16) -> dict(indptr, indices, wq, labels, tot,
    m2: numpy / int); read-only.
      rows 2..13: 0, 1, 15, 16, 17, 63, 64 entries (group path) and 65, 255, 256, 257, 600 (wide path, tile edges);
        with 83 columns the long rows list columns many times over;
      rows 7, 8 and 10..13 carry wq near 2^50 with random low bits, so a community's tot is near 2^58, (double)
        rounds and the score's product exceeds 2^53 -- a coarse level's numbers;
      row 14: a column listed twice, two self entries, columns -1 and N, a wq of 0 and a negative one;
      row 20 (40 entries) has a falling indptr and is empty, which makes row 21 (30 entries) re-read the tail of row 19
        and all of row 20: a long row of 73;
      row 30 (label 1) ties exactly between the labels 70 and 75 (rows 31, 32: equal wq, equal tot), row 33 (label 80)
        between 62 and 66 (rows 34, 35): the smaller label wins, 70 on an up sweep, 62 on a down sweep;
      row 36 (label 40) has one neighbour, of label 68: it moves on an up sweep only.
    Labels: random in [5, 60) but for the reserved ones; tot is computed from them."""
    rng = np.random.default_rng(83)
    N = EDGE_N
    big = {7, 8, 10, 11, 12, 13}
    rows = []
    for i in range(N):
        d = EDGE_LENGTHS.get(i, int(rng.integers(3, 13)))
        col = rng.integers(0, N, size=d)
        if i in big:
            w = (1 << 50) + rng.integers(-(1 << 30), 1 << 30, size=d)
        else:
            w = rng.integers(1, 1 << 26, size=d)
        rows.append([(int(c), int(v)) for c, v in zip(col, w)])
    rows[14] = [(5, 900), (14, 77), (5, 1200), (-1, 500), (N, 500), (40, 0), (41, -3), (14, 5), (50, 1 << 20),
                (51, 1 << 20)]
    big_w = 1 << 40
    rows[30], rows[31], rows[32] = [(31, big_w), (32, big_w)], [(30, big_w)], [(30, big_w)]
    rows[33], rows[34], rows[35] = [(35, big_w), (34, big_w)], [(33, big_w)], [(33, big_w)]
    rows[36], rows[37] = [(37, big_w)], [(36, big_w)]
    # other rows may list a helper's column (that changes the listing row's sums only); the helpers' labels are theirs
    # alone, so their tot is their own k
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indptr[21] = indptr[20] - 3                # row 20: falling, empty; row 21 starts inside row 19
    flat = [e for r in rows for e in r]
    indices = np.array([c for c, _ in flat], dtype=np.int32)
    wq = np.array([v for _, v in flat], dtype=np.int64)
    labels = rng.integers(5, 60, size=N).astype(np.int32)
    for i, c in {30: 1, 31: 70, 32: 75, 33: 80, 34: 62, 35: 66, 36: 40, 37: 68}.items():
        labels[i] = c
    g = dict(indptr=indptr, indices=indices, wq=wq)
    from spmf_amd import communities
    n, row, col, w = communities.valid_edges(g)
    k = np.zeros(N, dtype=np.int64)
    np.add.at(k, row, w)
    tot = np.zeros(N, dtype=np.int64)
    np.add.at(tot, labels, k)
    assert (indptr[EDGE_LONG[-1] + 1] - indptr[EDGE_LONG[-1]]) > GROUP_LEN
    return dict(g, labels=labels, tot=tot, m2=int(k.sum()), k=k)
