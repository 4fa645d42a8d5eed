"""CPU-side tests of the transform calls (PoissonFactorization.graph_transform / umap_transform,
spmf_amd.graph.query_weights / transform_negatives / transform_reference, spmf_amd.neighbors.vote,
spmf_graph_transform, csrc/graph_transform.hip): the memberships against a plain double loop, the unchanged bits of
fuzzy_graph, the draws against Philox by hand, the fp64 restatement against an independent loop form, the vote, the
entry point in the header, the export list and the binding, the raw entry's refusals through a ctypes call with dummy
addresses, every argument check of the two methods before a library call, and the quality of the fp64 restatement on
the split of the blobs that the GPU test maps.  (The valid calls: tests/test_gpu_graph_transform.py.)

fuzzy_graph: the hashes below were recorded on the commit before query_weights shared the bisection with it; the fp64
sigma and rho are hashed after rounding to float32, so that the last bit of a machine's exp does not decide the test.

Quality, measured with the fp64 restatement (80 query rows, 400 reference rows, k = 10, M = 8): purity 1.0000 at the
weighted-mean start and after 30 or 100 epochs at lr 0.25 and at lr 1.0; spacing ratio 0.966 at the start, 0.915 /
0.980 after 30 / 100 epochs at lr 0.25, 1.031 / 0.863 at lr 1.0; mean displacement from the start 0.30 - 0.50."""
import hashlib
import inspect
import math

import numpy as np
import pytest
import torch

from _graph_layout_cases import blob_graph
from _graph_transform_cases import (N_HEADER_ARGS, assert_graph_transform_errors, blob_split,
                                    graph_transform_raw_call, transform_quality)
from _stream_cases import K, assert_declared_exported_bound, cpu_model, host_ctx, library, no_library
from spmf_amd import graph, neighbors

INF, NAN = float("inf"), float("nan")


# ---- query_weights -----------------------------------------------------------------------------------------------
def _weights_by_loops(idx, dist):
    """smooth_knn_dist with local connectivity 0 for one row at a time, in Python floats."""
    Q, k = len(idx), len(idx[0])
    ok = [[idx[i][t] >= 0 and math.isfinite(dist[i][t]) and dist[i][t] >= 0 for t in range(k)] for i in range(Q)]
    every = [dist[i][t] for i in range(Q) for t in range(k) if ok[i][t]]
    mean_all = sum(every) / len(every) if every else 0.0
    sigmas, weights = [], []
    for i in range(Q):
        d = [dist[i][t] for t in range(k) if ok[i][t]]
        target = math.log2(max(len(d), 1))
        lo, hi, sigma = 0.0, INF, 1.0
        for _ in range(64):
            if sum(math.exp(-v / sigma) for v in d) > target:
                hi = sigma
                sigma = 0.5 * (lo + hi)
            else:
                lo = sigma
                sigma = 2.0 * sigma if hi == INF else 0.5 * (lo + hi)
        sigma = max(sigma, 1e-3 * mean_all)
        sigmas.append(sigma)
        weights.append([math.exp(-dist[i][t] / sigma) if ok[i][t] else 0.0 for t in range(k)])
    return np.array(weights), np.array(sigmas)


@pytest.mark.parametrize("k", [1, 2, 5])
def test_query_weights_against_a_double_loop(k):
    rng = np.random.default_rng(30 + k)
    Q = 8
    dist = np.sort(rng.uniform(0.1, 3.0, size=(Q, k)), 1)
    idx = rng.integers(0, 50, size=(Q, k))
    dist[1, 0] = 0.0                                           # a query on a reference row
    idx[2, -1], dist[2, -1] = -1, INF                          # padding
    idx[3, :], dist[3, :] = -1, INF                            # no valid entry
    dist[4, -1] = NAN
    dist[5, 0] = -0.5                                          # negative: invalid
    dist[6, :] = 0.7                                           # all equal
    got = graph.query_weights(torch.as_tensor(idx), torch.as_tensor(dist))
    assert set(got) == {"weights", "sigma"}
    assert got["weights"].dtype == torch.float32 and tuple(got["weights"].shape) == (Q, k)
    assert got["sigma"].dtype == torch.float64 and tuple(got["sigma"].shape) == (Q,)
    w, sigma = _weights_by_loops(idx.tolist(), dist.tolist())
    np.testing.assert_allclose(got["sigma"].numpy(), sigma, rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["weights"].numpy(), w.astype(np.float32), rtol=1e-6, atol=1e-30)
    gw = got["weights"].numpy()
    assert gw[1, 0] == 1.0, "a zero distance is weight 1"
    assert (gw[3] == 0).all() and gw[2, -1] == 0 and gw[4, -1] == 0 and gw[5, 0] == 0, "invalid entries weigh 0"
    assert np.isfinite(gw).all() and (gw >= 0).all() and (gw <= 1).all() and np.isfinite(got["sigma"].numpy()).all()
    if k == 5:          # where no floor applies the weights sum to log2(k_i): rows 0 and 7 have five distinct distances
        for i in (0, 7):
            assert abs(float(got["weights"][i].double().sum()) - math.log2(5)) <= 1e-6
    # float32 input as knn returns it, numpy input, and the same bits twice
    again = graph.query_weights(idx.astype(np.int32), dist)
    assert torch.equal(again["weights"].view(torch.int32), got["weights"].view(torch.int32))
    assert torch.equal(again["sigma"], got["sigma"])


def test_query_weights_argument_errors_and_edges():
    with pytest.raises(ValueError, match="one shape"):
        graph.query_weights(torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3, 3))
    with pytest.raises(ValueError, match="integers"):
        graph.query_weights(torch.zeros(3, 2), torch.zeros(3, 2))
    with pytest.raises(ValueError, match="floating"):
        graph.query_weights(torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3, 2, dtype=torch.int64))
    empty = graph.query_weights(torch.zeros(0, 4, dtype=torch.int64), torch.zeros(0, 4))
    assert tuple(empty["weights"].shape) == (0, 4) and tuple(empty["sigma"].shape) == (0,)
    none = graph.query_weights(torch.full((2, 3), -1), torch.full((2, 3), INF))
    assert (none["weights"] == 0).all() and torch.isfinite(none["sigma"]).all()


def test_fuzzy_graph_keeps_its_bits():
    g = blob_graph()

    def sha(t):
        return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    assert tuple(g["indices"].shape) == (6870,)
    assert sha(g["indptr"]) == "88605a656939a62c2f5152edb7f65a6d05bd44ad0eb370e21a9336b7410c4960"
    assert sha(g["indices"]) == "8ae98ec90979224baf12f69a33cdae013b4ba180aa9a81db9916c536f062791a"
    assert sha(g["weights"]) == "f25d894caf531b1eb46b47602f1e1d5cecede2aa75948ddf95da228ef598e2aa"
    assert sha(g["sigma"].to(torch.float32)) == "1765c27e21b35b91d3a8d31887159cad15afcb5f9ec4602e70d513b4a2152cb6"
    assert sha(g["rho"].to(torch.float32)) == "a51d1e254d6737f765a44eefbf888f8b4e4efb70df24538b4370498d61ea988c"
    # _smooth_knn as fuzzy_graph calls it
    dist = torch.tensor([[0.5, 0.9, 1.4], [0.0, 0.5, INF]], dtype=torch.float64)
    sigma, rho = graph._smooth_knn(dist, torch.tensor([[True, True, True], [True, True, False]]))
    assert rho.tolist() == [0.5, 0.5] and torch.isfinite(sigma).all() and (sigma > 0).all()


# ---- the draws ---------------------------------------------------------------------------------------------------
def test_transform_negatives_against_philox_by_hand():
    row0, Q, n_ref, e, M, seed = 1000, 9, 777, 3, 6, 5 + (7 << 32)
    neg = graph.transform_negatives(row0, Q, n_ref, e, M, seed)
    assert neg.shape == (Q, M) and neg.dtype == np.int64 and neg.min() >= 0 and neg.max() < n_ref
    i, m = 4, 5
    blk = graph.philox4x32_10(np.array([row0 + i, m >> 2, e, 0x554D5854], dtype=np.uint32), (5, 7))
    assert int(neg[i, m]) == (int(blk[m & 3]) * n_ref) >> 32
    whole = graph.philox4x32_10(np.array([[row0 + i, 0, e, 0x554D5854], [row0 + i, 1, e, 0x554D5854]],
                                         dtype=np.uint32), (5, 7))
    assert neg[i].tolist() == [(int(v) * n_ref) >> 32 for v in list(whole[0]) + list(whole[1][:2])]
    # another stream than the layout's: the tag differs
    assert not np.array_equal(neg, graph.negatives(n_ref, e, M, seed)[row0:row0 + Q])
    # row0 shifts the draws: rows [5, 9) of a 9-row call are a 4-row call at row0 = 5
    nine = graph.transform_negatives(0, 9, n_ref, e, M, seed)
    assert np.array_equal(nine[5:], graph.transform_negatives(5, 4, n_ref, e, M, seed))
    assert not np.array_equal(nine[:4], nine[5:])
    # the row number is taken modulo 2^32, the last one allowed is 2^32 - 1
    top = graph.transform_negatives(2 ** 32 - 1, 1, n_ref, e, M, seed)
    blk = graph.philox4x32_10(np.array([0xFFFFFFFF, 0, e, 0x554D5854], dtype=np.uint32), (5, 7))
    assert int(top[0, 1]) == (int(blk[1]) * n_ref) >> 32
    assert (graph.transform_negatives(0, 3, 0, e, M, seed) == -1).all(), "no reference row: nothing is drawn"
    assert (graph.transform_negatives(0, 50, 1, e, M, seed) == 0).all()


# ---- the fp64 restatement ------------------------------------------------------------------------------------------
def _reference_by_loops(idx, w, y_ref, y_in, row0, epoch0, n_epochs, total, lr, a, b, gamma, rate, M, seed):
    """include/spmf_hip.h spmf_graph_transform entry by entry in Python floats."""
    Q, k = len(idx), len(idx[0])
    n_ref = len(y_ref)

    def fin(p):
        return math.isfinite(p[0]) and math.isfinite(p[1])
    out = []
    for i in range(Q):
        ent = [(y_ref[idx[i][t]], w[i][t]) for t in range(k)
               if 0 <= idx[i][t] < n_ref and math.isfinite(w[i][t]) and w[i][t] > 0 and fin(y_ref[idx[i][t]])]
        W = sum(v for _, v in ent)
        if y_in is None:
            y = [sum(v * p[c] for p, v in ent) / W for c in (0, 1)] if W > 0 else [NAN, NAN]
        else:
            y = list(y_in[i])
        for e in range(epoch0, epoch0 + n_epochs):
            if not (W > 0 and fin(y)):
                break
            alpha = float(np.float32(lr * (1.0 - e / total)))
            F = [0.0, 0.0]
            for p, v in ent:
                D = [y[0] - p[0], y[1] - p[1]]
                d2 = D[0] ** 2 + D[1] ** 2
                if d2 > 0:
                    ca = -2.0 * a * b * d2 ** (b - 1.0) / (1.0 + a * d2 ** b)
                    for c in (0, 1):
                        F[c] += v * min(max(ca * D[c], -4.0), 4.0)
            if n_ref:
                neg = graph.transform_negatives(row0 + i, 1, n_ref, e, M, seed)[0]
                for r in neg:
                    p = y_ref[int(r)]
                    if not fin(p):
                        continue
                    D = [y[0] - p[0], y[1] - p[1]]
                    d2 = D[0] ** 2 + D[1] ** 2
                    if d2 > 0:
                        cr = 2.0 * gamma * b / ((0.001 + d2) * (1.0 + a * d2 ** b))
                        for c in (0, 1):
                            F[c] += rate * W / M * min(max(cr * D[c], -4.0), 4.0)
            y = [y[c] + alpha * F[c] / max(1.0, W) for c in (0, 1)]
        out.append(y)
    return np.array(out)


def _small_case():
    rng = np.random.default_rng(11)
    Q, k, n_ref = 3, 4, 6
    idx = rng.integers(0, n_ref, size=(Q, k))
    w = rng.uniform(0.1, 1.0, size=(Q, k)).astype(np.float32)
    y_ref = rng.uniform(-3, 3, size=(n_ref, 2)).astype(np.float32)
    y_in = rng.uniform(-3, 3, size=(Q, 2)).astype(np.float32)
    y_in[1] = y_ref[idx[1, 0]]                                 # d2 = 0 with its first neighbour
    return idx, w, y_ref, y_in


def test_transform_reference_against_a_loop_form():
    idx, w, y_ref, y_in = _small_case()
    args = dict(total_epochs=5, lr=0.25, a=1.58, b=0.9, repulsion=1.2, negative_rate=4.0, n_negatives=5, seed=9)
    loop = dict(total=5, lr=0.25, a=1.58, b=0.9, gamma=1.2, rate=4.0, M=5, seed=9)
    for start in (y_in, None):
        for row0 in (0, 40):
            whole = graph.transform_reference(idx, w, y_ref, start, row0, 0, 5, **args)
            want = _reference_by_loops(idx.tolist(), w.tolist(), y_ref.tolist(),
                                       None if start is None else start.tolist(), row0, 0, 5, **loop)
            np.testing.assert_allclose(whole, want, rtol=1e-12, atol=1e-13)
            assert np.isfinite(whole).all()
    whole = graph.transform_reference(idx, w, y_ref, y_in, 0, 0, 5, **args)
    assert not np.array_equal(whole, graph.transform_reference(idx, w, y_ref, y_in, 40, 0, 5, **args)), "row0 counts"
    # epochs 2 + 3 are the 5 of one call
    part = graph.transform_reference(idx, w, y_ref, y_in, 0, 0, 2, **args)
    assert np.array_equal(whole, graph.transform_reference(idx, w, y_ref, part, 0, 2, 3, **args))
    # no epoch: the start
    assert np.array_equal(graph.transform_reference(idx, w, y_ref, y_in, 0, 3, 0, **args), y_in.astype(np.float64))
    y0 = graph.transform_reference(idx, w, y_ref, None, 0, 0, 0, **args)
    for i in range(3):
        np.testing.assert_allclose(y0[i], (w[i].astype(np.float64)[:, None] * y_ref[idx[i]]).sum(0) / w[i].sum(dtype=np.float64),
                                   rtol=1e-14)
    y, A, W = graph.transform_reference(idx, w, y_ref, y_in, 0, 0, 1, details=True, **args)
    assert A.shape == (3,) and (A > 0).all() and np.allclose(W, w.astype(np.float64).sum(1))


def test_transform_reference_skip_rules():
    idx, w, y_ref, y_in = _small_case()
    args = dict(total_epochs=4, lr=0.5, a=1.58, b=0.9, n_negatives=8, seed=2)
    loop = dict(total=4, lr=0.5, a=1.58, b=0.9, gamma=1.0, rate=5.0, M=8, seed=2)
    whole = graph.transform_reference(idx, w, y_ref, y_in, 0, 0, 4, **args)
    # entries the rules skip, appended to every row: the result is that of the clean rows
    bad_i = np.concatenate([idx, np.tile(np.array([-1, 6, -2 ** 31, 0, 1, 2, 3]), (3, 1))], 1)
    bad_w = np.concatenate([w, np.tile(np.array([1, 1, 1, 0, -1, NAN, INF], dtype=np.float32), (3, 1))], 1)
    assert np.array_equal(graph.transform_reference(bad_i, bad_w, y_ref, y_in, 0, 0, 4, **args), whole)
    # a non-finite reference row is no neighbour and no negative
    yr = y_ref.copy()
    yr[2] = (NAN, 1.0)
    yr[4] = (INF, -INF)
    got = graph.transform_reference(idx, w, yr, y_in, 0, 0, 4, **args)
    want = _reference_by_loops(idx.tolist(), w.tolist(), yr.tolist(), y_in.tolist(), 0, 0, 4, **loop)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13)
    assert np.isfinite(got).all() and not np.array_equal(got, whole)
    # a row of only invalid entries keeps its position; from no start it is NaN; a NaN row keeps its bits
    dead_w = w.copy()
    dead_w[1] = 0.0
    yn = y_in.copy()
    yn[2] = (NAN, 3.0)
    got = graph.transform_reference(idx, dead_w, y_ref, yn, 0, 0, 4, **args)
    assert np.array_equal(got[1], y_in[1].astype(np.float64)) and np.isnan(got[2, 0]) and got[2, 1] == 3.0
    assert np.isfinite(got[0]).all() and not np.array_equal(got[0], y_in[0].astype(np.float64))
    y0 = graph.transform_reference(idx, dead_w, y_ref, None, 0, 0, 2, **args)
    assert np.isnan(y0[1]).all() and np.isfinite(y0[[0, 2]]).all()
    # no reference row: nothing valid, nothing drawn
    none = graph.transform_reference(idx, w, np.zeros((0, 2)), y_in, 0, 0, 4, **args)
    assert np.array_equal(none, y_in.astype(np.float64))
    assert np.isnan(graph.transform_reference(idx, w, np.zeros((0, 2)), None, 0, 0, 4, **args)).all()


# ---- the vote ------------------------------------------------------------------------------------------------------
def test_vote_rules():
    labels = torch.tensor([0, 1, 1, 2, -1, 7, 2])             # rows 4 and 5: no label, a label out of range (G = 3)
    idx = torch.tensor([[0, 1, 2, 3],                          # 1 wins 2 : 1 : 1
                        [0, 1, 3, -1],                         # a three-way tie: the smallest class
                        [3, 6, 1, 2],                          # 1 against 2, equal sums: 1
                        [4, 5, -1, 7],                         # nobody votes (7 is no row)
                        [4, 0, 5, 3],                          # the unlabelled do not count in the share
                        [-1, -1, -1, -1]])
    ones = torch.ones(6, 4)
    got, share = neighbors.vote(idx, ones, labels, n_classes=3)
    assert got.dtype == torch.int64 and share.dtype == torch.float64
    assert got.tolist() == [1, 0, 1, -1, 0, -1]
    assert share[:3].tolist() == [0.5, 1.0 / 3.0, 0.5] and share[4].item() == 0.5
    assert torch.isnan(share[3]) and torch.isnan(share[5])
    # n_classes from the labels: 7 is a class now
    got8, share8 = neighbors.vote(idx, ones, labels)
    assert got8.tolist() == [1, 0, 1, 7, 0, -1] and share8[3].item() == 1.0 and share8[4].item() == 1.0 / 3.0
    # weights decide, and bad weights do not vote
    w = torch.tensor([[0.9, 0.3, 0.3, 0.1], [0.2, 0.2, 0.3, 1.0], [NAN, INF, 0.5, 0.0], [1.0, 1.0, 1.0, 1.0],
                      [1.0, -1.0, 1.0, 0.25], [1.0, 1.0, 1.0, 1.0]])
    got, share = neighbors.vote(idx, w, labels, n_classes=3)
    assert got.tolist() == [0, 2, 1, -1, 2, -1]
    assert abs(share[0].item() - 0.9 / 1.6) <= 1e-7 and share[2].item() == 1.0 and share[4].item() == 1.0
    # unit weights give exact integer sums: 40 neighbours, 13 / 13 / 14 votes, and a tie of 20 : 20
    many = torch.arange(40)[None, :]
    lab40 = torch.cat([torch.zeros(13), torch.ones(13), torch.full((14,), 2)]).long()
    got, share = neighbors.vote(many, torch.ones(1, 40), lab40)
    assert got.tolist() == [2] and share.item() == 14.0 / 40.0
    got, share = neighbors.vote(many, torch.ones(1, 40), (torch.arange(40) % 2 == 0).long() * 3)
    assert got.tolist() == [0] and share.item() == 0.5
    # chunks of any size and a second run give the same bits; numpy and int32 inputs are taken
    rng = np.random.default_rng(3)
    idx = torch.as_tensor(rng.integers(-1, 60, size=(300, 15)))
    w = torch.as_tensor(rng.uniform(0, 1, size=(300, 15)).astype(np.float32))
    lab = torch.as_tensor(rng.integers(-1, 9, size=60))
    a = neighbors.vote(idx, w, lab)
    for other in (neighbors.vote(idx, w, lab), neighbors.vote(idx, w, lab, max_elements=1),
                  neighbors.vote(idx.numpy().astype(np.int32), w.numpy(), lab.numpy(), n_classes=9)):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1].view(torch.int64), other[1].view(torch.int64))
    by_hand = [max(range(9), key=lambda g: (sum(float(w[i, t]) for t in range(15)
                                                if idx[i, t] >= 0 and lab[idx[i, t]] == g), -g)) for i in range(300)]
    assert a[0].tolist() == by_hand
    for bad in (dict(indices=idx.double()), dict(weights=w[:, :3]), dict(labels=lab.double()), dict(n_classes=-1),
                dict(n_classes=2.0), dict(labels=lab[:, None])):
        with pytest.raises(ValueError, match="vote"):
            neighbors.vote(**dict(dict(indices=idx, weights=w, labels=lab), **bad))
    e = neighbors.vote(idx[:0], w[:0], lab)
    assert tuple(e[0].shape) == (0,) and tuple(e[1].shape) == (0,)
    assert neighbors.vote(idx, w, lab[:0])[0].tolist() == [-1] * 300


# ---- the entry point -----------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    lib = library()
    assert N_HEADER_ARGS == 21
    assert_declared_exported_bound("spmf_graph_transform", N_HEADER_ARGS)
    assert callable(lib.spmf_graph_transform) and lib.spmf_version() == 6


def test_raw_errors_return_before_any_device_call():
    """A context of spmf_ctx_create and dummy addresses: no call here is valid, so nothing may be launched or
    dereferenced; the empty call returns SPMF_OK without touching anything either."""
    lib = library()
    h = host_ctx(lib, K)
    try:
        good = dict(h=h, n=70, k=15, idx=0x1000000, w=0x2000000, y_ref=0x3000000, n_ref=300, y_in=0x4000000,
                    y_out=0x5000000, row0=0, epoch0=0, n_epochs=3, total=3, lr=0.25, a=1.58, b=0.9, gamma=1.0,
                    rate=5.0, M=8, seed=0, stream=None)
        assert_graph_transform_errors(lib, good)
        call = graph_transform_raw_call(good)
        assert call(n=0) == 0                                  # no row: nothing to do
        assert call(n=0, idx=None, w=None, y_in=None, y_out=None, row0=2 ** 32) == 0
        assert call(n=0, n_ref=0, y_ref=None) == 0
        assert call(n_epochs=0, y_out=good["y_in"]) == 0       # no epoch in place: nothing to copy
    finally:
        lib.spmf_ctx_destroy(h)


def test_methods_and_signatures_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    E = inspect.Parameter.empty
    want = {"graph_transform": [("indices", E), ("distances", E), ("reference_layout", E), ("weights", None),
                                ("init", None), ("n_epochs", None), ("min_dist", 0.1), ("spread", 1.0), ("a", None),
                                ("b", None), ("n_negatives", 8), ("negative_rate", 5.0), ("repulsion", 1.0),
                                ("learning_rate", 0.25), ("seed", 0), ("row_offset", 0)],
            "umap_transform": [("data", E), ("reference", E), ("k", 15), ("metric", "euclidean"), ("nsamples", 32),
                               ("draws", None), ("max_rows", None), ("labels", None), ("n_classes", None),
                               ("n_epochs", None), ("learning_rate", 0.25), ("n_negatives", 8),
                               ("negative_rate", 5.0), ("repulsion", 1.0), ("seed", 0)]}
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        for name, params in want.items():
            fn = getattr(cls, name, None)
            assert callable(fn), (cls.__name__, name)
            got = [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]
            assert got == params, (cls.__name__, name, got)
    got = [(p.name, p.default) for p in inspect.signature(neighbors.vote).parameters.values()][:4]
    assert got == [("indices", E), ("weights", E), ("labels", E), ("n_classes", None)]
    got = [p.name for p in inspect.signature(graph.transform_reference).parameters.values()]
    assert got[:11] == ["idx", "w", "y_ref", "y_in", "row0", "epoch0", "n_epochs", "total_epochs", "lr", "a", "b"]
    assert got[-1] == "details"
    assert [p.name for p in inspect.signature(graph.transform_negatives).parameters.values()] == \
        ["row0", "n_query", "n_ref", "epoch", "n_negatives", "seed"]
    assert graph.default_transform_epochs(10000) == 100 and graph.default_transform_epochs(10001) == 30


def test_every_argument_check_raises_before_a_library_call(monkeypatch):
    m = cpu_model()[0]
    no_library(monkeypatch)
    idx = torch.zeros(7, 4, dtype=torch.int32)
    dist = torch.ones(7, 4)
    ref = torch.zeros(9, 2)
    counts = {"counts": np.zeros((7, 6))}
    reference = {"latent": torch.zeros(9, 2), "embedding": ref, "a": 1.58, "b": 0.9}
    for kw, what in ((dict(n_epochs=-1), "n_epochs"), (dict(n_epochs=2.0), "n_epochs"), (dict(n_epochs=True), "n_epochs"),
                     (dict(n_negatives=0), "n_negatives"), (dict(n_negatives=65), "n_negatives"),
                     (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"), (dict(negative_rate=-1.0), "negative_rate"),
                     (dict(negative_rate=NAN), "negative_rate"), (dict(repulsion=INF), "repulsion"),
                     (dict(learning_rate=-0.5), "learning_rate"), (dict(learning_rate=None), "learning_rate")):
        with pytest.raises(ValueError, match=what):
            m.graph_transform(idx, dist, ref, **kw)
        with pytest.raises(ValueError, match=what):
            m.umap_transform(counts, reference, **kw)
    for kw, what in ((dict(a=1.0), "a and b"), (dict(b=1.0), "a and b"), (dict(a=0.0, b=1.0), "a must"),
                     (dict(a=1.0, b=NAN), "b must"), (dict(min_dist=-1.0), "min_dist"), (dict(spread=0.0), "spread"),
                     (dict(init="pca"), "init"), (dict(init=3), "init"), (dict(init=torch.zeros(6, 2)), "init tensor"),
                     (dict(init=torch.zeros(7, 2, dtype=torch.float64)), "init tensor"),
                     (dict(row_offset=-1), "row_offset"), (dict(row_offset=1.0), "row_offset"),
                     (dict(row_offset=2 ** 32 - 6), "row_offset"),
                     (dict(weights=torch.ones(7, 3)), "weights"), (dict(weights=torch.ones(7, 4).double()), "weights"),
                     (dict(weights=np.ones((7, 4), dtype=np.float32)), "weights")):
        with pytest.raises(ValueError, match=what):
            m.graph_transform(idx, dist, ref, **kw)
    for bad, what in (((idx.numpy(), dist, ref), "indices"), ((idx[0], dist[0], ref), "indices"),
                      ((idx.float(), dist, ref), "integers"), ((idx, dist.long(), ref), "distances"),
                      ((idx, dist[:, :3], ref), "distances"), ((idx, dist, ref.double()), "reference_layout"),
                      ((idx, dist, torch.zeros(9, 3)), "reference_layout"), ((idx, dist, torch.zeros(18)), "reference_layout"),
                      ((torch.zeros(7, 65, dtype=torch.int32), torch.ones(7, 65), ref), "k <= 64"),
                      ((torch.zeros(7, 0, dtype=torch.int32), torch.ones(7, 0), ref), "k <= 64")):
        with pytest.raises(ValueError, match=what):
            m.graph_transform(*bad)
    # host memory is never handed to the library
    with pytest.raises(ValueError, match="device"):
        m.graph_transform(idx, dist, ref)
    with pytest.raises(ValueError, match="device"):
        m.graph_transform(idx, dist, ref, weights=torch.ones(7, 4), init=torch.zeros(7, 2), n_epochs=0)
    # umap_transform: its own arguments
    for k in (0, 65, 2.0):
        with pytest.raises(ValueError, match="k"):
            m.umap_transform(counts, reference, k=k)
    with pytest.raises(ValueError, match="metric"):
        m.umap_transform(counts, reference, metric="l2")
    for bad in (None, {}, {"latent": reference["latent"], "embedding": ref}):
        with pytest.raises(ValueError, match="what umap returned"):
            m.umap_transform(counts, bad)
    for name, v, what in (("a", 0.0, "a must"), ("b", None, "a and b"), ("latent", torch.zeros(9, 3), "latent"),
                          ("latent", np.zeros((9, 2)), "latent"), ("embedding", torch.zeros(8, 2), "embedding"),
                          ("embedding", torch.zeros(9, 2).double(), "embedding")):
        with pytest.raises(ValueError, match=what):
            m.umap_transform(counts, dict(reference, **{name: v}))
    for kw, what in ((dict(labels=np.zeros(8, dtype=np.int64)), "one entry per reference row"),
                     (dict(labels=np.zeros(9)), "integers"), (dict(labels=np.zeros((9, 1), dtype=np.int64)), "1-D"),
                     (dict(labels=np.zeros(9, dtype=np.int64), n_classes=-2), "n_classes"),
                     (dict(labels=np.zeros(9, dtype=np.int64), n_classes=2.0), "n_classes")):
        with pytest.raises(ValueError, match=what):
            m.umap_transform(counts, reference, **kw)


# ---- the quality of the restatement ----------------------------------------------------------------------------------
def test_reference_quality_on_the_split_blobs():
    """The input of the GPU quality test is one on which the fp64 restatement alone passes, with the figures of the
    docstring above: purity 1.0 at the start and after 30 or 100 epochs at either learning rate, the spacing ratio
    within 0.86 .. 1.04."""
    s = blob_split()
    assert s["idx"].shape == (80, 10) and s["y_ref"].shape == (400, 2) and s["y_ref"].dtype == np.float32
    assert np.isfinite(s["y_ref"]).all() and (s["w"] > 0).all()
    y0 = graph.transform_reference(s["idx"], s["w"], s["y_ref"], None, 0, 0, 0, 100, 0.25, s["a"], s["b"])
    pure, ratio = transform_quality(y0, s)
    assert pure == 1.0 and 0.86 <= ratio <= 1.04, (pure, ratio)
    for E, lr in ((30, 0.25), (100, 0.25), (30, 1.0), (100, 1.0)):
        y = graph.transform_reference(s["idx"], s["w"], s["y_ref"], None, 0, 0, E, E, lr, s["a"], s["b"], 1.0, 5.0, 8, 0)
        pure, ratio = transform_quality(y, s)
        moved = float(np.abs(y - y0).max(1).mean())
        print(f"transform_reference blobs: {E} epochs at lr {lr}: purity {pure:.4f}, spacing ratio {ratio:.3f}, "
              f"mean displacement {moved:.3f}")
        assert np.isfinite(y).all() and pure == 1.0 and 0.86 <= ratio <= 1.04 and moved > 0.1, (E, lr, pure, ratio)
