"""GPU: spmf_graph_move (csrc/graph_move.hip) and ``communities`` on top of it.

One sweep on the hand-made edge graph (tests/_communities_cases.py edge_graph) through raw library calls with
sentinels around the output, both directions: labels_out equals ``NumpyOps.move`` exactly -- there is no tolerance,
everything is an integer or a single rounded fp64 operation -- whatever the order of long_rows, with a short row
added to it, and with a long row left off it (that row keeps its label).  Then the error contract with sentinels,
and end to end: ``model.communities`` returns the labels and the modularity bits of ``solve(NumpyOps)``, twice, and
the chain knn -> fuzzy_graph -> communities -> silhouette runs."""
import numpy as np
import pytest
import torch

from _communities_cases import (EDGE_LONG, EDGE_TIE_DOWN, EDGE_TIE_UP, EDGE_WRONG_SIDE, GROUP_LEN, assert_errors,
                                blobs, edge_graph, raw_call, two_rings)
from spmf_amd import communities

pytestmark = pytest.mark.gpu

SENTINEL = -77
PAD = 8


def _model():
    from spmf_amd import PoissonFactorization
    return PoissonFactorization(latent_dim=3, feature_dim=8, initialize_distributions=False, device="cuda")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


class _Call:
    """Raw calls on the edge graph: device copies of the arrays, labels_out inside a buffer of sentinels (8 entries in
    front, 8 behind)."""

    def __init__(self, m, e):
        from spmf_amd import _lib
        self.lib, self.h = _lib.load(), m._handle()
        self.n = len(e["indptr"]) - 1
        self.t = {k: _dev(e[k]) for k in ("indptr", "indices", "wq", "labels", "tot")}
        self.m2 = e["m2"]
        self.out = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.keep = None

    def args(self, long_rows=(), gamma=1.0, direction=0):
        self.keep = _dev(np.asarray(long_rows, dtype=np.int32)) if len(long_rows) else None
        return dict(h=self.h, n=self.n, nnz=int(self.t["indices"].numel()), indptr=self.t["indptr"].data_ptr(),
                    indices=self.t["indices"].data_ptr(), wq=self.t["wq"].data_ptr(),
                    labels_in=self.t["labels"].data_ptr(), tot=self.t["tot"].data_ptr(),
                    long_rows=self.keep.data_ptr() if self.keep is not None else None, n_long=len(long_rows),
                    gamma=gamma, m2=self.m2, direction=direction, labels_out=self.out[PAD:].data_ptr(),
                    stream=torch.cuda.current_stream().cuda_stream)

    def untouched(self):
        return bool((self.out[:PAD] == SENTINEL).all()) and bool((self.out[PAD + self.n:] == SENTINEL).all())

    def move(self, **kw):
        self.out.fill_(SENTINEL)
        rc = raw_call(self.args(**kw))()
        assert rc == 0, self.lib.spmf_last_error(self.h).decode()
        torch.cuda.synchronize()
        assert self.untouched(), "a write outside labels_out"
        return self.out[PAD:PAD + self.n].cpu().numpy()


@pytest.mark.parametrize("direction", [0, 1])
def test_one_sweep_on_the_edge_graph_is_the_numpy_sweep(direction):
    e = edge_graph()
    call = _Call(_model(), e)
    ops = communities.NumpyOps(e)
    lab = e["labels"]
    lens = np.diff(e["indptr"])
    assert sorted(np.flatnonzero(lens > GROUP_LEN).tolist()) == sorted(EDGE_LONG)
    for gamma in (1.0, 0.37):
        want = ops.move(torch.from_numpy(lab), torch.from_numpy(e["tot"]), gamma, e["m2"], direction).numpy()
        assert int((want != lab).sum()) > 20 and (want[list(EDGE_LONG)] != lab[list(EDGE_LONG)]).any()
        got = call.move(long_rows=EDGE_LONG, gamma=gamma, direction=direction)
        assert np.array_equal(got, want), np.flatnonzero(got != want)
        # the list reversed, and with short rows on it (an empty one, one of 16, one of 64, the tie row): the wide
        # path writes what the group path writes
        assert np.array_equal(call.move(long_rows=EDGE_LONG[::-1], gamma=gamma, direction=direction), want)
        mixed = (8, 13, 2, 9, 5, EDGE_TIE_UP, 21, 12, 11, 10, EDGE_TIE_DOWN, 14, 9)
        assert np.array_equal(call.move(long_rows=mixed, gamma=gamma, direction=direction), want)
        # every row on the list: the wide path alone agrees with the definition on all of them
        assert np.array_equal(call.move(long_rows=tuple(range(call.n)), gamma=gamma, direction=direction), want)
        # a long row left off the list keeps its label; nothing else changes
        for off in (13, 9):
            rest = tuple(r for r in EDGE_LONG if r != off)
            got = call.move(long_rows=rest, gamma=gamma, direction=direction)
            kept = want.copy()
            kept[off] = lab[off]
            assert np.array_equal(got, kept)
        none = call.move(long_rows=(), gamma=gamma, direction=direction)
        kept = want.copy()
        kept[list(EDGE_LONG)] = lab[list(EDGE_LONG)]
        assert np.array_equal(none, kept)
        # entries of the list outside the rows are skipped
        assert np.array_equal(call.move(long_rows=EDGE_LONG + (-1, call.n, 2 ** 31 - 1), gamma=gamma,
                                        direction=direction), want)
    got = call.move(long_rows=EDGE_LONG, direction=direction)
    assert got[EDGE_TIE_UP] == (70 if direction == 0 else 1)
    assert got[EDGE_TIE_DOWN] == (80 if direction == 0 else 62)
    assert got[EDGE_WRONG_SIDE] == (68 if direction == 0 else 40)


def test_labels_outside_the_rows_are_never_candidates():
    """A label outside [0, N) is not a candidate and tot is not read at it; a row that carries one does not move."""
    e = dict(edge_graph())
    lab = e["labels"].copy()
    lab[[16, 40, 60]] = (-5, 83, 2 ** 31 - 1)
    e["labels"] = lab
    call = _Call(_model(), e)
    ops = communities.NumpyOps(e)
    for direction in (0, 1):
        want = ops.move(torch.from_numpy(lab), torch.from_numpy(e["tot"]), 1.0, e["m2"], direction).numpy()
        got = call.move(long_rows=EDGE_LONG, direction=direction)
        assert np.array_equal(got, want)
        assert (got[[16, 40, 60]] == lab[[16, 40, 60]]).all()
        assert not np.isin(got[np.arange(83) != 16], [-5]).any() and not (got[np.arange(83) != 40] == 83).any()


def test_errors_return_before_a_launch_and_aliasing_is_refused():
    e = edge_graph()
    call = _Call(_model(), e)
    call.out.fill_(SENTINEL)
    good = call.args(long_rows=EDGE_LONG)

    def after():
        torch.cuda.synchronize()
        assert bool((call.out == SENTINEL).all()), "an output was written by a refused call"
    assert_errors(call.lib, good, after=after)
    rc = raw_call(good)(labels_out=good["labels_in"])
    assert rc == -1 and "aliases" in call.lib.spmf_last_error(call.h).decode()
    torch.cuda.synchronize()
    assert torch.equal(call.t["labels"].cpu(), torch.from_numpy(e["labels"]))


@pytest.mark.parametrize("name", ["blobs", "rings"])
def test_communities_is_the_numpy_backends_bits(name):
    g = blobs()[0] if name == "blobs" else two_rings()
    want = communities.solve(communities.NumpyOps(g))
    m = _model()
    dev = {n: g[n].cuda() for n in ("indptr", "indices", "weights")}
    res = m.communities(dev)
    assert res["labels"].is_cuda and res["labels"].dtype == torch.int64 and res["sizes"].is_cuda
    assert torch.equal(res["labels"].cpu(), want["labels"])
    assert np.float64(res["modularity"]).tobytes() == np.float64(want["modularity"]).tobytes()
    assert res["levels"] == want["levels"] and res["n_communities"] == want["n_communities"]
    assert torch.equal(res["sizes"].cpu(), want["sizes"])
    again = m.communities(dev)
    assert torch.equal(res["labels"], again["labels"]), "the same bits twice"
    assert np.float64(res["modularity"]).tobytes() == np.float64(again["modularity"]).tobytes()
    assert res["levels"] == again["levels"]
    if name == "blobs":
        assert res["n_communities"] == 6 and res["labels"].cpu().tolist() == blobs()[2].tolist()
    for gamma in (0.5, 2.0):
        a = m.communities(dev, resolution=gamma)
        b = communities.solve(communities.NumpyOps(g), resolution=gamma)
        assert torch.equal(a["labels"].cpu(), b["labels"]) and a["modularity"] == b["modularity"]


def test_a_coarse_level_with_long_rows_is_the_numpy_backends_bits():
    """A hub graph: row 0 is joined to every row, so level 0 takes the wide path and the coarse levels keep a long row
    for as long as there are more than 64 communities."""
    n = 700
    rng = np.random.default_rng(5)
    pairs = {(0, j) for j in range(1, n)} | {(i, i + 1) for i in range(1, n - 1)}
    while len(pairs) < 4 * n:
        i, j = (int(v) for v in rng.integers(1, n, size=2))
        if i != j and abs(i - j) < 12:
            pairs.add((min(i, j), max(i, j)))
    und = np.array(sorted(pairs), dtype=np.int64)
    w = rng.uniform(0.05, 1.0, size=len(und)).astype(np.float32)
    w[und[:, 0] == 0] *= np.float32(0.02)
    rows = np.concatenate([und[:, 0], und[:, 1]])
    cols = np.concatenate([und[:, 1], und[:, 0]])
    order = np.argsort(rows * n + cols, kind="stable")
    g = {"indptr": torch.from_numpy(np.searchsorted(rows[order], np.arange(n + 1)).astype(np.int64)),
         "indices": torch.from_numpy(cols[order].astype(np.int32)),
         "weights": torch.from_numpy(np.concatenate([w, w])[order])}
    want = communities.solve(communities.NumpyOps(g))
    res = _model().communities({k: v.cuda() for k, v in g.items()})
    assert torch.equal(res["labels"].cpu(), want["labels"]) and res["modularity"] == want["modularity"]
    assert res["levels"] == want["levels"] and 1 < res["n_communities"] < n


def test_chain_knn_graph_communities_silhouette():
    _, x, truth = blobs()
    m = _model()
    pts = x.cuda()
    nn = m.knn(pts, k=10)
    g = m.fuzzy_graph(nn["indices"], nn["distances"])
    res = m.communities(g)
    assert res["n_communities"] == 6 and res["labels"].cpu().tolist() == truth.tolist()
    sil = m.silhouette(pts, res["labels"])
    assert sil["n_scored"] == 600 and sil["score"] > 0.5
    assert sil["counts"].cpu().tolist() == res["sizes"].cpu().tolist()
