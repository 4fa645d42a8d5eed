"""What the test files of PAGA share (test_paga_host.py, test_gpu_paga.py, test_gpu_paga_cli.py): the argument list of
spmf_graph_group_edges, its raw call and its error contract, asserted without a device on dummy addresses and with one
on real buffers; the labellings of the hand-made edge graph (tests/_communities_cases.py edge_graph); and the chain of
four blobs whose coarse graph is a path."""
import ctypes as C
import functools

import numpy as np
import torch

_P, _I64, _I32 = C.c_void_p, C.c_int64, C.c_int32
ARGS = (("n", _I64), ("nnz", _I64), ("indptr", _P), ("indices", _P), ("wq", _P), ("labels", _P), ("G", _I32),
        ("count", _P), ("weight", _P), ("size", _P), ("ptr", _P), ("nbytes", C.c_size_t), ("stream", _P))
HEADER_ARGS = {"spmf_graph_group_edges": 14, "spmf_graph_group_edges_scratch_bytes": 3}
MAX_GROUPS = 1024                          # include/spmf_hip.h SPMF_GROUP_EDGES_MAX_GROUPS


def raw_call(good):
    """-> call(**overrides): spmf_graph_group_edges through a binding of its own with the arguments of ``good``."""
    from spmf_amd import _lib
    fn = C.CDLL(_lib.LIB_PATH).spmf_graph_group_edges
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [t for _, t in ARGS]

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], *[a[n] for n, _ in ARGS])
    return call


def scratch_bytes(lib, h, n, G):
    return int(lib.spmf_graph_group_edges_scratch_bytes(h, n, G))


def host_good(lib, h):
    """A valid-looking call that needs no device: dummy aligned addresses -- only refused calls may be made with
    it (the empty call fills its outputs, so it needs real ones)."""
    need = scratch_bytes(lib, h, 83, 5)
    return dict(h=h, n=83, nnz=300, indptr=0x1000000, indices=0x2000000, wq=0x3000000, labels=0x4000000, G=5,
                count=0x5000000, weight=0x6000000, size=0x7000000, ptr=0x8000000, nbytes=need, stream=None)


def assert_scratch_sizes(lib, h):
    """The size function: a multiple of 256, non-decreasing in the rows, 0 for arguments the call refuses."""
    for G in (1, 5, 83, MAX_GROUPS):
        last = 0
        for n in (0, 1, 63, 64, 65, 1023, 1024, 1025, 5000, 122880, 2 ** 31 - 64):
            need = scratch_bytes(lib, h, n, G)
            assert need > 0 and need % 256 == 0 and need >= last, (n, G, need, last)
            last = need
    for n, G in ((-1, 5), (2 ** 31 - 63, 5), (83, 0), (83, -1), (83, MAX_GROUPS + 1)):
        assert scratch_bytes(lib, h, n, G) == 0, (n, G)
    assert scratch_bytes(lib, None, 83, 5) == 0


def assert_errors(lib, good, after=lambda: None):
    """The error contract of spmf_graph_group_edges; every call here returns before a launch or a fill, and ``after``
    is run behind each (the GPU file checks its sentinels there)."""
    call, h = raw_call(good), good["h"]

    def refused(code=-1, **kw):
        assert call(**kw) == code, kw
        msg = lib.spmf_last_error(h).decode()
        assert msg.startswith("graph_group_edges: "), msg
        after()
        return msg
    for rows in (-1, 2 ** 31 - 63, 2 ** 40):
        assert "n_rows" in refused(n=rows)
    assert "nnz" in refused(nnz=-1)
    for G in (0, -1, MAX_GROUPS + 1, 2 ** 31 - 1):
        assert "n_groups" in refused(G=G) and "1024" in refused(G=G)
    for name in ("indptr", "indices", "wq", "labels", "count", "weight", "size", "ptr"):
        assert "null" in refused(**{name: None})
    for name in ("count", "weight", "size", "ptr"):        # the outputs and the scratch are needed without rows too
        assert "null" in refused(n=0, **{name: None})
    for out in ("count", "weight", "size"):
        for src in ("indptr", "indices", "wq", "labels"):
            assert "aliases" in refused(**{out: good[src]})
    assert "aliases" in refused(weight=good["count"])
    assert "aliases" in refused(size=good["weight"])
    assert "aligned" in refused(ptr=good["ptr"] + 4)
    assert str(good["nbytes"]) in refused(-3, nbytes=good["nbytes"] - 256)
    refused(n=0, G=0)                        # errors come before the empty return
    refused(-3, n=0, nbytes=0)
    assert call(h=None) == -1


# ---- the labellings of the edge graph ------------------------------------------------------------------------------
def edge_labellings():
    """(name, labels int32 [83], G) on ``_communities_cases.edge_graph``: every row a group of its own; the rows folded
    to 5 groups with group 3 empty, some rows -1 and some at or beyond G (skipped as source and as target); one
    group."""
    n = 83
    own = np.arange(n, dtype=np.int32)
    rng = np.random.default_rng(5)
    folded = rng.choice(np.array([0, 1, 2, 4], dtype=np.int32), size=n)
    folded[[3, 14, 40, 61]] = -1
    folded[[9, 13, 50]] = (5, 6, 2 ** 31 - 1)             # two long rows among them
    folded[[7, 77]] = -(2 ** 31)
    return (("own", own, n), ("folded", folded, 5), ("one", np.zeros(n, dtype=np.int32), 1))


def loop_group_edges(e, labels, G):
    """count, weight and size of ``edge_graph``'s arrays by a plain Python double loop over the rows and their
    entries, from the definition in include/spmf_hip.h."""
    indptr, indices, wq = e["indptr"], e["indices"], e["wq"]
    n, nnz = len(indptr) - 1, len(indices)
    count = [[0] * G for _ in range(G)]
    weight = [[0] * G for _ in range(G)]
    size = [0] * G
    for i in range(n):
        a = int(labels[i])
        if not 0 <= a < G:
            continue
        size[a] += 1
        p0, p1 = (min(max(int(indptr[i + d]), 0), nnz) for d in (0, 1))
        for p in range(p0, p1):
            j, w = int(indices[p]), int(wq[p])
            if not 0 <= j < n or w < 1:
                continue
            b = int(labels[j])
            if 0 <= b < G:
                count[a][b] += 1
                weight[a][b] += w
    return np.array(count, dtype=np.int64), np.array(weight, dtype=np.int64), np.array(size, dtype=np.int64)


# ---- the chain of blobs ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain(step=4.5):
    """4 blobs of 80 points in 8 dimensions, centres ``step`` apart on the first axis, unit noise (torch CPU generator,
    seed 5) -> (the fuzzy graph of their exact 10 nearest neighbours on the CPU, the points float32 [320, 8], the
    truth int64 [320]); read-only."""
    from spmf_amd import graph, neighbors
    gen = torch.Generator(device="cpu")
    gen.manual_seed(5)
    centres = torch.zeros(4, 8, dtype=torch.float64)
    centres[:, 0] = step * torch.arange(4, dtype=torch.float64)
    truth = torch.arange(4).repeat_interleave(80)
    x = (centres[truth] + torch.randn(320, 8, generator=gen, dtype=torch.float64)).to(torch.float32)
    idx, dist = neighbors.brute_force(x, x, 10, exclude_self=True)
    return graph.fuzzy_graph(idx, dist), x, truth


def path_order(conn):
    """The groups of a [G, G] connectivity matrix in the order of the path its non-zero pairs form, starting at the
    end with the smaller label; asserts that they do form one path through all groups."""
    conn = np.asarray(conn)
    G = conn.shape[0]
    adj = [sorted(np.flatnonzero(conn[a] > 0).tolist()) for a in range(G)]
    assert np.array_equal(conn > 0, (conn > 0).T)
    deg = [len(v) for v in adj]
    assert sorted(deg) == [1, 1] + [2] * (G - 2), deg
    order = [min(a for a in range(G) if deg[a] == 1)]
    while len(order) < G:
        nxt = [b for b in adj[order[-1]] if b not in order]
        assert len(nxt) == 1, (order, adj)
        order.append(nxt[0])
    return order
