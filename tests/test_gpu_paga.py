"""GPU: spmf_graph_group_edges (csrc/graph_groups.hip) and ``paga`` / ``paga_init`` on top of it.

Raw library calls with 8 sentinel words on both sides of each of the three outputs: on the hand-made edge graph
(tests/_communities_cases.py edge_graph) under three labellings, at the block edges of the ordering, under contention
on one diagonal word with weights that need 64 bits, the error contract and the empty call.  All three outputs equal
``NumpyOps.group_edges`` exactly -- there is no tolerance anywhere: every compared value is an integer, or an fp64 made
from integers by the one shared function.  Then end to end: ``model.paga`` returns the arrays of ``solve(NumpyOps)``,
twice; a chain of four blobs gives a path; and ``paga_init`` feeds ``graph_layout`` a start that keeps the path."""
import numpy as np
import pytest
import torch

from _communities_cases import blobs, edge_graph
from _paga_cases import MAX_GROUPS, assert_errors, chain, edge_labellings, path_order, raw_call, scratch_bytes
from spmf_amd import communities, paga

pytestmark = pytest.mark.gpu

SENTINEL = -77
PAD = 8


def _model():
    from spmf_amd import PoissonFactorization
    return PoissonFactorization(latent_dim=3, feature_dim=8, initialize_distributions=False, device="cuda")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


class _Call:
    """Raw calls on a graph of numpy arrays (indptr, indices, wq): device copies, the three outputs inside buffers of
    sentinels (8 words in front, 8 behind), an exactly sized scratch."""

    def __init__(self, m, g):
        from spmf_amd import _lib
        self.m = m                         # the model owns the context: it lives as long as the handle is used
        self.lib, self.h = _lib.load(), m._handle()
        self.n = len(g["indptr"]) - 1
        self.t = {k: _dev(g[k]) for k in ("indptr", "indices", "wq")}
        self.keep = None

    def args(self, labels, G):
        need = scratch_bytes(self.lib, self.h, self.n, G)
        assert need > 0 and need % 256 == 0
        scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
        self.G = G
        self.out = {k: torch.full((s + 2 * PAD,), SENTINEL, dtype=torch.int64, device="cuda")
                    for k, s in (("count", G * G), ("weight", G * G), ("size", G))}
        self.keep = (_dev(np.asarray(labels, dtype=np.int32)), scratch)
        return dict(h=self.h, n=self.n, nnz=int(self.t["indices"].numel()), indptr=self.t["indptr"].data_ptr(),
                    indices=self.t["indices"].data_ptr() if self.t["indices"].numel() else None,
                    wq=self.t["wq"].data_ptr() if self.t["wq"].numel() else None,
                    labels=self.keep[0].data_ptr(), G=G, count=self.out["count"][PAD:].data_ptr(),
                    weight=self.out["weight"][PAD:].data_ptr(), size=self.out["size"][PAD:].data_ptr(),
                    ptr=scratch.data_ptr() + (-scratch.data_ptr()) % 256, nbytes=need,
                    stream=torch.cuda.current_stream().cuda_stream)

    def untouched(self, whole=False):
        for t in self.out.values():
            inner = t[PAD:-PAD]
            if not bool((t[:PAD] == SENTINEL).all()) or not bool((t[-PAD:] == SENTINEL).all()):
                return False
            if whole and not bool((inner == SENTINEL).all()):
                return False
        return True

    def run(self, labels, G, **kw):
        rc = raw_call(self.args(labels, G))(**kw)
        assert rc == 0, self.lib.spmf_last_error(self.h).decode()
        torch.cuda.synchronize()
        assert self.untouched(), "a write outside an output"
        count, weight, size = (self.out[k][PAD:-PAD].cpu() for k in ("count", "weight", "size"))
        return count.reshape(G, G), weight.reshape(G, G), size


def _assert_is_numpy(call, g, labels, G):
    got = call.run(labels, G)
    want = paga.NumpyOps(g).group_edges(torch.from_numpy(np.asarray(labels, dtype=np.int32)), G)
    for a, b, what in zip(got, want, ("count", "weight", "size")):
        assert torch.equal(a, b), (what, torch.nonzero(a != b)[:5].tolist())
    return got


def _random_graph(n, per_row, seed, wmax=1 << 26):
    """Rows of 0 .. 2 ``per_row`` entries with random columns and weights -> dict(indptr, indices, wq) numpy."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 2 * per_row + 1, size=n)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(indptr[-1])
    return dict(indptr=indptr, indices=rng.integers(0, n, size=nnz).astype(np.int32),
                wq=rng.integers(1, wmax, size=nnz).astype(np.int64))


@pytest.mark.parametrize("name", ["own", "folded", "one"])
def test_the_edge_graph_is_the_numpy_reduction(name):
    e = edge_graph()
    labels, G = {n: (lab, g) for n, lab, g in edge_labellings()}[name]
    call = _Call(_model(), e)
    count, weight, size = _assert_is_numpy(call, e, labels, G)
    assert int(count.sum()) > 500 and int(weight.max()) > 2 ** 50
    if name == "folded":
        assert int(size[3]) == 0 and int(size.sum()) == 83 - 9 and not count[3].any() and not count[:, 3].any()
    if name == "one":
        assert size.tolist() == [83]
    again = call.run(labels, G)
    assert all(torch.equal(a, b) for a, b in zip((count, weight, size), again)), "the same bits twice"


def test_block_edges_of_the_ordering():
    m = _model()
    # groups of exactly 64, 65 and 1 rows, an empty one (3) and the rest in group 4; rows in no order
    n = 200
    labels = np.full(n, 4, dtype=np.int32)
    perm = np.random.default_rng(1).permutation(n)
    labels[perm[:64]] = 0
    labels[perm[64:129]] = 1
    labels[perm[129:130]] = 2
    g = _random_graph(n, 12, 2)
    _, _, size = _assert_is_numpy(_Call(m, g), g, labels, 5)
    assert size.tolist() == [64, 65, 1, 0, 70]
    # one row, with entries that point at itself
    one = dict(indptr=np.array([0, 3], dtype=np.int64), indices=np.zeros(3, dtype=np.int32),
               wq=np.array([5, 1, 1 << 40], dtype=np.int64))
    count, weight, size = _assert_is_numpy(_Call(m, one), one, [0], 1)
    assert count.tolist() == [[3]] and weight.tolist() == [[6 + (1 << 40)]] and size.tolist() == [1]
    count, _, size = _assert_is_numpy(_Call(m, one), one, [-1], 2)
    assert not count.any() and not size.any()
    # the full LDS table: G = 1024, most groups a single row
    n = 1100
    g = _random_graph(n, 10, 3)
    labels = (np.arange(n) % MAX_GROUPS).astype(np.int32)
    count, _, size = _assert_is_numpy(_Call(m, g), g, labels, MAX_GROUPS)
    assert int(size.max()) == 2 and int(size.min()) == 1 and int((count > 0).sum()) > 5000
    # a graph without entries
    empty = dict(indptr=np.zeros(71, dtype=np.int64), indices=np.zeros(0, dtype=np.int32), wq=np.zeros(0, dtype=np.int64))
    count, weight, size = _assert_is_numpy(_Call(m, empty), empty, np.arange(70) % 3, 3)
    assert not count.any() and not weight.any() and size.tolist() == [24, 23, 23]


def test_contention_on_one_word_and_64_bit_sums():
    """One group of 5 000 rows, 15 entries per row, all inside the group, wq = 2^24 each: 75 000 adds meet on one word,
    and their sum needs 41 bits -- a 32-bit accumulator or a lost atomic shows."""
    n, k = 5000, 15
    rng = np.random.default_rng(7)
    g = dict(indptr=(k * np.arange(n + 1)).astype(np.int64), indices=rng.integers(0, n, size=n * k).astype(np.int32),
             wq=np.full(n * k, 1 << 24, dtype=np.int64))
    call = _Call(_model(), g)
    count, weight, size = call.run(np.zeros(n, dtype=np.int32), 1)
    assert count.tolist() == [[75000]] and weight.tolist() == [[75000 << 24]] and size.tolist() == [n]
    # the same rows split at random into 3 groups
    labels = rng.integers(0, 3, size=n).astype(np.int32)
    count, weight, size = _assert_is_numpy(call, g, labels, 3)
    assert int(count.sum()) == 75000 and int(weight.sum()) == 75000 << 24 and int(count.min()) > 7000


def test_errors_return_before_a_launch_and_the_empty_call_fills_zeros():
    e = edge_graph()
    call = _Call(_model(), e)
    labels, G = edge_labellings()[1][1:]
    good = call.args(labels, G)

    def after():
        torch.cuda.synchronize()
        assert call.untouched(whole=True), "an output was written by a refused call"
    assert_errors(call.lib, good, after=after)
    # n_rows = 0: the outputs are zero-filled in full, nothing around them is touched
    rc = raw_call(good)(n=0, indptr=None, labels=None)
    assert rc == 0, call.lib.spmf_last_error(call.h).decode()
    torch.cuda.synchronize()
    assert call.untouched() and all(not bool(t[PAD:-PAD].any()) for t in call.out.values())


def test_paga_is_the_numpy_backends_arrays():
    g, _, truth = blobs()
    m = _model()
    dev = {n: g[n].cuda() for n in ("indptr", "indices", "weights")}
    labels = m.communities(dev)["labels"]
    assert labels.cpu().tolist() == truth.tolist()
    want = paga.solve(paga.NumpyOps(g), labels.cpu())
    tensors = ("connectivities", "connectivities_tree", "expected", "edge_count", "edge_weight", "sizes")
    for _ in range(2):
        res = m.paga(dev, labels)
        assert set(res) == set(tensors) | {"n_groups"} and res["n_groups"] == 6
        for k in tensors:
            assert res[k].is_cuda and res[k].dtype == want[k].dtype and torch.equal(res[k].cpu(), want[k]), k
    # six far-apart blobs: no entry between two of them, so no connectivity and an empty tree
    assert not res["connectivities"].any() and not res["connectivities_tree"].any()
    assert res["sizes"].tolist() == [100] * 6 and int(res["edge_count"].sum()) == int(g["indices"].numel())
    assert torch.equal(res["edge_count"], torch.diag(torch.diagonal(res["edge_count"])))
    # numpy labels with rows in no group, an explicit G with empty groups
    lab = truth.numpy().copy()
    lab[::7] = -1
    a = m.paga(dev, lab, n_groups=9)
    b = paga.solve(paga.NumpyOps(g), lab, n_groups=9)
    assert all(torch.equal(a[k].cpu(), b[k]) for k in tensors) and a["sizes"].tolist()[6:] == [0, 0, 0]


def _chain_on_device():
    """The chain's graph (made on the CPU, so that both backends read the same weights) on the device."""
    return {n: chain()[0][n].cuda() for n in ("indptr", "indices", "weights")}


def test_a_chain_of_blobs_gives_a_path():
    """4 blobs of 80 points, centres 4.5 apart on one axis: ``communities`` finds 4 communities of 78 .. 82 rows, and
    their connectivities are non-zero on exactly three pairs, which form a path (the values were 0.09 .. 0.14 on the
    numpy backends; the pattern is asserted, not the values).  The numpy backends alone satisfy the pattern first."""
    g, _, _ = chain()
    host_labels = communities.solve(communities.NumpyOps(g))
    host = paga.solve(paga.NumpyOps(g), host_labels["labels"])

    def pattern(res):
        conn = res["connectivities"].cpu().numpy()
        print("chain: sizes", res["sizes"].tolist(), "connectivities", sorted(conn[np.triu(conn > 0, 1)].tolist()))
        assert res["n_groups"] == 4 and all(78 <= s <= 82 for s in res["sizes"].tolist())
        assert int(np.triu(conn > 0, 1).sum()) == 3
        order = path_order(conn)
        assert np.array_equal(res["connectivities_tree"].cpu().numpy() > 0, conn > 0)
        return order
    assert host_labels["n_communities"] == 4
    host_order = pattern(host)
    m = _model()
    dev = _chain_on_device()
    labels = m.communities(dev)["labels"]
    res = m.paga(dev, labels)
    assert pattern(res) == host_order
    assert torch.equal(labels.cpu(), host_labels["labels"])
    assert all(torch.equal(res[k].cpu(), host[k]) for k in host if isinstance(host[k], torch.Tensor))


def test_paga_init_feeds_graph_layout_a_start_that_keeps_the_path():
    m = _model()
    dev = _chain_on_device()
    labels = m.communities(dev)["labels"]
    start = m.paga_init(dev, labels, seed=3)
    assert set(start) == {"init", "positions", "paga"}
    init, pos = start["init"], start["positions"]
    assert init.is_cuda and init.dtype == torch.float32 and tuple(init.shape) == (320, 2)
    assert pos.is_cuda and pos.dtype == torch.float32 and tuple(pos.shape) == (4, 2)
    assert bool(torch.isfinite(init).all()) and float(init.abs().max()) == 10.0
    res = m.graph_layout(dev, init=init, n_epochs=60)
    assert bool(torch.isfinite(res["embedding"]).all()) and tuple(res["embedding"].shape) == (320, 2)
    again = m.paga_init(dev, labels, seed=3)
    assert torch.equal(again["init"], init) and torch.equal(again["positions"], pos), "the same bits twice"
    assert torch.equal(m.graph_layout(dev, init=again["init"], n_epochs=60)["embedding"], res["embedding"])
    # the start's group centroids keep the order of the path along their principal axis
    order = path_order(start["paga"]["connectivities"].cpu().numpy())
    lab = labels.cpu()
    cent = torch.stack([init.cpu().double()[lab == a].mean(0) for a in range(4)])
    c = cent - cent.mean(0)
    axis = torch.linalg.eigh(c.T @ c)[1][:, -1]
    along = (c @ axis)[order]
    assert bool((along[1:] > along[:-1]).all()) or bool((along[1:] < along[:-1]).all()), along.tolist()
