"""CPU-side tests of the layout calls (PoissonFactorization.fuzzy_graph / graph_layout / umap, spmf_amd/graph.py,
spmf_graph_layout, csrc/graph_layout.hip): the curve fit, the fuzzy graph on hand cases, Philox of the reference,
the two entry points in the header, the export list and the binding, the scratch size, the raw entry's refusals
through a ctypes call with dummy aligned addresses, every argument check of the methods before a library call, and
the quality of the fp64 reference on the blobs the GPU test lays out.  (The valid calls: tests/test_gpu_graph_layout.py.)

Philox: the first three vectors are the published Philox4x32-10 known answers of Random123 (kat_vectors: zero,
all ones, the digits of pi); the fourth is this implementation's own output on a layout counter, pinned once the
three agreed -- the device kernel shares csrc/philox.h with the surrogate and is held against the same negatives in
test_gpu_graph_layout.py."""
import inspect

import numpy as np
import pytest
import torch

from _graph_layout_cases import assert_graph_layout_errors, blob_graph, blobs, purity
from _stream_cases import K, assert_declared_exported_bound, cpu_model, host_ctx, library, no_library
from spmf_amd import graph

HEADER_ARGS = {"spmf_graph_layout_scratch_bytes": 2, "spmf_graph_layout": 21}


def test_find_ab_against_curve_fit():
    for (min_dist, spread), (a, b) in {(0.1, 1.0): (1.576943, 0.895061), (0.5, 1.0): (0.583030, 1.334167),
                                       (0.001, 1.0): (1.929074, 0.791504), (0.3, 2.0): (0.379495, 0.948815)}.items():
        got = graph.find_ab(min_dist, spread)
        assert abs(got[0] - a) <= 1e-4 and abs(got[1] - b) <= 1e-4, (min_dist, spread, got)
    for bad in ((0.1, 0.0), (-0.1, 1.0), (3.0, 1.0), (float("nan"), 1.0)):
        with pytest.raises(ValueError):
            graph.find_ab(*bad)


def _hand_case():
    """Seven rows, k = 4: row 0 ordinary; row 1 with padding and a self edge; row 2 of all-equal distances; row 3
    with zero distances (duplicates); row 4 empty; rows 5 and 6 ordinary, 6 listing 4 (which lists nobody)."""
    inf = float("inf")
    idx = torch.tensor([[1, 2, 3, 5], [1, 0, 2, -1], [0, 1, 3, 5], [2, 0, 5, 6], [-1, -1, -1, -1], [0, 2, 3, 6],
                        [5, 3, 4, 0]])
    dist = torch.tensor([[0.5, 0.9, 1.4, 2.0], [0.0, 0.5, 0.7, inf], [1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.8, 1.1],
                         [inf, inf, inf, inf], [0.3, 0.6, 0.8, 1.7], [0.2, 1.1, 1.3, 2.2]], dtype=torch.float64)
    return idx, dist


def test_fuzzy_graph_on_a_hand_case():
    idx, dist = _hand_case()
    g = graph.fuzzy_graph(idx, dist)
    indptr, indices, data = graph.to_csr(g)
    N = 7
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
    assert indptr.shape == (N + 1,) and indptr[0] == 0 and indptr[-1] == indices.size == data.size
    assert g["sigma"].dtype == torch.float64 and g["rho"].dtype == torch.float64
    dense = np.zeros((N, N), dtype=np.float32)
    for i in range(N):
        cols = indices[indptr[i]:indptr[i + 1]]
        assert (np.diff(cols) > 0).all(), "ascending, no duplicate"
        assert i not in cols, "self edges are dropped"
        assert cols.min(initial=0) >= 0, "padding is dropped"
        dense[i, cols] = data[indptr[i]:indptr[i + 1]]
    assert np.array_equal(dense.view(np.int32), dense.T.copy().view(np.int32)), "every edge twice, with the same bits"
    assert np.isfinite(data).all() and (data > 0).all() and (data <= 1).all()
    assert torch.isfinite(g["sigma"]).all() and torch.isfinite(g["rho"]).all() and (g["sigma"] > 0).all()
    # the edge pattern is the union of both directions: 4 lists nobody but is listed by 6
    assert set(indices[indptr[4]:indptr[5]]) == {6} and 4 in indices[indptr[6]:indptr[7]]
    # rho: the smallest positive distance; row 1's self edge at 0 does not count, row 3's zeros are skipped
    assert g["rho"].tolist() == [0.5, 0.5, 1.0, 0.8, 0.0, 0.3, 0.2]
    # the directed weights sum to log2(k_i) where no floor applies (rows 0, 5, 6: four distinct distances)
    rows = torch.arange(N)[:, None].expand(N, 4)
    valid = (idx >= 0) & (idx != rows) & torch.isfinite(dist)
    w = torch.exp(-(dist - g["rho"][:, None]).clamp_min(0) / g["sigma"][:, None]) * valid
    for i in (0, 5, 6):
        assert abs(float(w[i].sum()) - 2.0) <= 1e-5, (i, float(w[i].sum()))
    # symmetric weight of the pair (0, 5): both list each other
    w05, w50 = float(w[0, 3]), float(w[5, 0])
    assert dense[0, 5] == np.float32(w05 + w50 - w05 * w50)
    # one direction only: (6, 4)
    assert dense[6, 4] == np.float32(float(w[6, 2]))
    # all-equal distances (row 2) and duplicates (row 3): every directed weight of an excess 0 is 1
    assert dense[2, 1] >= np.float32(1.0) - 1e-6 and dense[3, 2] == 1.0 and dense[3, 0] == 1.0


def test_fuzzy_graph_argument_errors_and_edges():
    idx, dist = _hand_case()
    with pytest.raises(ValueError, match="square"):
        graph.fuzzy_graph(torch.tensor([[1, 7]]), torch.tensor([[0.1, 0.2]]))
    with pytest.raises(ValueError, match="square"):
        graph.fuzzy_graph(idx, dist, n_rows=8)
    with pytest.raises(ValueError, match="twice"):
        graph.fuzzy_graph(torch.tensor([[1, 1], [0, -1]]), torch.tensor([[0.1, 0.2], [0.1, float("inf")]]))
    with pytest.raises(ValueError, match="integers"):
        graph.fuzzy_graph(idx.double(), dist)
    with pytest.raises(ValueError, match="one shape"):
        graph.fuzzy_graph(idx[:, :3], dist)
    with pytest.raises(ValueError, match="below"):
        graph.fuzzy_graph(torch.tensor([[-2, 1], [0, -1]]), torch.ones(2, 2))
    empty = graph.fuzzy_graph(torch.zeros(0, 3, dtype=torch.int64), torch.zeros(0, 3))
    assert empty["indptr"].tolist() == [0] and empty["indices"].numel() == 0
    none = graph.fuzzy_graph(torch.full((3, 2), -1), torch.full((3, 2), float("inf")))
    assert none["indptr"].tolist() == [0, 0, 0, 0] and torch.isfinite(none["sigma"]).all()
    # all points coincide: every distance 0, every weight 1
    same = graph.fuzzy_graph(torch.tensor([[1, 2], [0, 2], [0, 1]]), torch.zeros(3, 2))
    assert same["weights"].tolist() == [1.0] * 6 and torch.isfinite(same["sigma"]).all()
    a, b = graph.fuzzy_graph(idx, dist), graph.fuzzy_graph(idx.numpy(), dist.numpy().astype(np.float32))
    assert torch.equal(a["indices"], b["indices"]) and torch.allclose(a["weights"], b["weights"], rtol=1e-5)


def test_philox_of_the_reference_against_known_answers():
    vectors = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
               ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
               ((1, 2, 3, 0x554D4150), (5, 7), (0xf0975b03, 0x33647169, 0xb260aa60, 0xed58c1f9))]
    for ctr, key, want in vectors:
        got = graph.philox4x32_10(np.array(ctr, dtype=np.uint32), key)
        assert tuple(int(v) for v in got) == want, (ctr, key, [hex(int(v)) for v in got])
    batch = graph.philox4x32_10(np.array([v[0] for v in vectors[:1] * 3], dtype=np.uint32), (0, 0))
    assert batch.shape == (3, 4) and (batch == batch[0]).all()
    # the negatives: word m & 3 of block m >> 2 under the counter (i, m >> 2, e, tag), scaled by n_rows
    neg = graph.negatives(1000, 3, 6, 5 + (7 << 32))
    assert neg.shape == (1000, 6) and neg.min() >= 0 and neg.max() < 1000
    blk = graph.philox4x32_10(np.array([[1, 0, 3, 0x554D4150], [1, 1, 3, 0x554D4150]], dtype=np.uint32), (5, 7))
    assert neg[1].tolist() == [(int(v) * 1000) >> 32 for v in list(blk[0]) + list(blk[1][:2])]
    assert int(blk[0][0]) != 0xf0975b03                      # (another block index than the pinned vector's)


def test_entry_points_are_declared_exported_and_bound():
    lib = library()
    for name, nargs in HEADER_ARGS.items():
        assert_declared_exported_bound(name, nargs)
        assert callable(getattr(lib, name)), name
    assert lib.spmf_version() == 6


def test_methods_and_signatures_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    E = inspect.Parameter.empty
    layout = [("n_epochs", None), ("min_dist", 0.1), ("spread", 1.0), ("a", None), ("b", None), ("n_negatives", 8),
              ("negative_rate", 5.0), ("repulsion", 1.0), ("learning_rate", 1.0), ("seed", 0)]
    want = {"fuzzy_graph": [("indices", E), ("distances", E)],
            "graph_layout": [("graph", E), ("init", "pca"), ("points", None)] + layout,
            "umap": [("data", E), ("k", 15), ("metric", "euclidean"), ("nsamples", 32), ("draws", None),
                     ("max_rows", None), ("init", "pca")] + layout}
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        for name, params in want.items():
            fn = getattr(cls, name, None)
            assert callable(fn), (cls.__name__, name)
            got = [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]
            assert got == params, (cls.__name__, name, got)


def test_scratch_size():
    """0 for arguments the call refuses, else a positive multiple of 256 that holds two position buffers and does
    not shrink as the rows grow."""
    lib = library()
    h = host_ctx(lib, K)
    try:
        for bad in (-1, 2 ** 31 - 63, 2 ** 40):
            assert int(lib.spmf_graph_layout_scratch_bytes(h, bad)) == 0, bad
        assert int(lib.spmf_graph_layout_scratch_bytes(None, 5)) == 0
        last = 0
        for n in (0, 1, 31, 32, 33, 63, 64, 65, 1000, 4096, 10 ** 6, 10 ** 6 + 1, 2 ** 31 - 64):
            need = int(lib.spmf_graph_layout_scratch_bytes(h, n))
            assert need > 0 and need % 256 == 0 and need >= 2 * 8 * n and need >= last, (n, need, last)
            last = need
    finally:
        lib.spmf_ctx_destroy(h)


def test_raw_errors_return_before_any_device_call():
    """A context of spmf_ctx_create and dummy aligned addresses: no call here is valid, so nothing may be
    launched or dereferenced; the empty calls return SPMF_OK without touching anything either."""
    from _graph_layout_cases import graph_layout_raw_call
    lib = library()
    h = host_ctx(lib, K)
    try:
        n = 70
        need = int(lib.spmf_graph_layout_scratch_bytes(h, n))
        good = dict(h=h, n=n, nnz=300, indptr=0x1000000, indices=0x2000000, weights=0x3000000, y_in=0x4000000,
                    y_out=0x5000000, epoch0=0, n_epochs=3, total=3, lr=1.0, a=1.58, b=0.9, gamma=1.0, rate=5.0, M=8,
                    seed=0, ptr=0x8000000, nbytes=need, stream=None)
        assert_graph_layout_errors(lib, good, need)
        call = graph_layout_raw_call(good)
        assert call(n=0) == 0                                  # no row: nothing to do
        assert call(n=0, indptr=None, indices=None, weights=None, y_in=None, y_out=None) == 0
        assert call(n_epochs=0, y_out=good["y_in"]) == 0       # no epoch in place: nothing to copy
    finally:
        lib.spmf_ctx_destroy(h)


def _cpu_graph():
    idx, dist = _hand_case()
    g = graph.fuzzy_graph(idx, dist)
    return g, torch.zeros(7, 2)


def test_every_argument_check_raises_before_a_library_call(monkeypatch):
    m = cpu_model()[0]
    no_library(monkeypatch)
    g, y0 = _cpu_graph()
    nan = float("nan")
    for kw, what in ((dict(n_epochs=-1), "n_epochs"), (dict(n_epochs=2.0), "n_epochs"), (dict(n_epochs=True), "n_epochs"),
                     (dict(n_negatives=0), "n_negatives"), (dict(n_negatives=65), "n_negatives"),
                     (dict(n_negatives=8.0), "n_negatives"), (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"),
                     (dict(negative_rate=-1.0), "negative_rate"), (dict(negative_rate=nan), "negative_rate"),
                     (dict(repulsion=float("inf")), "repulsion"), (dict(repulsion="1"), "repulsion"),
                     (dict(learning_rate=-0.5), "learning_rate"), (dict(learning_rate=None), "learning_rate"),
                     (dict(a=1.0), "a and b"), (dict(b=1.0), "a and b"), (dict(a=0.0, b=1.0), "a must"),
                     (dict(a=1.0, b=nan), "b must"), (dict(min_dist=-1.0), "min_dist"), (dict(spread=0.0), "spread"),
                     (dict(min_dist=5.0), "min_dist")):
        with pytest.raises(ValueError, match=what):
            m.graph_layout(g, y0, **kw)
        with pytest.raises(ValueError, match=what):
            m.umap({"counts": np.zeros((7, 6))}, **kw)
    for init in ("spectral", None, 3):
        with pytest.raises(ValueError, match="init"):
            m.graph_layout(g, init)
        with pytest.raises(ValueError, match="init"):
            m.umap({"counts": np.zeros((7, 6))}, init=init)
    for k in (0, 65, 2.0):
        with pytest.raises(ValueError, match="k"):
            m.umap({"counts": np.zeros((7, 6))}, k=k)
    with pytest.raises(ValueError, match="metric"):
        m.umap({"counts": np.zeros((7, 6))}, metric="l2")
    # the graph
    for bad in (None, {}, {"indptr": g["indptr"], "indices": g["indices"]}):
        with pytest.raises(ValueError, match="dict"):
            m.graph_layout(bad, y0)
    for name, t in (("indptr", g["indptr"].to(torch.int32)), ("indices", g["indices"].to(torch.int64)),
                    ("weights", g["weights"].double()), ("indptr", g["indptr"][:, None]),
                    ("weights", g["weights"].numpy())):
        with pytest.raises(ValueError, match=name):
            m.graph_layout(dict(g, **{name: t}), y0)
    with pytest.raises(ValueError, match="N \\+ 1"):
        m.graph_layout(dict(g, indptr=g["indptr"][:0]), y0)
    with pytest.raises(ValueError, match="entries"):
        m.graph_layout(dict(g, weights=g["weights"][:-1]), y0)
    ptr = g["indptr"].clone()
    ptr[0] = 1
    with pytest.raises(ValueError, match="rise from 0"):
        m.graph_layout(dict(g, indptr=ptr), y0)
    ptr = g["indptr"].clone()
    ptr[-1] += 1
    with pytest.raises(ValueError, match="rise from 0"):
        m.graph_layout(dict(g, indptr=ptr), y0)
    ptr = g["indptr"].clone()
    ptr[2], ptr[3] = g["indptr"][3], g["indptr"][2]
    with pytest.raises(ValueError, match="falling"):
        m.graph_layout(dict(g, indptr=ptr), y0)
    for v in (-1, 7):
        ind = g["indices"].clone()
        ind[3] = v
        with pytest.raises(ValueError, match="must lie in"):
            m.graph_layout(dict(g, indices=ind), y0)
    # the start
    for bad in (torch.zeros(6, 2), torch.zeros(7, 3), torch.zeros(7, 2, dtype=torch.float64), torch.zeros(14)):
        with pytest.raises(ValueError, match="init tensor"):
            m.graph_layout(g, bad)
    for pts in (None, torch.zeros(6, 3), torch.zeros(7), torch.zeros(7, 3, dtype=torch.int64), np.zeros((7, 3))):
        with pytest.raises(ValueError, match="points"):
            m.graph_layout(g, "pca", points=pts)
    # host memory is never handed to the library
    with pytest.raises(ValueError, match="device"):
        m.graph_layout(g, y0)
    with pytest.raises(ValueError, match="device"):
        m.graph_layout(g, "pca", points=torch.zeros(7, 3), n_epochs=0)
    with pytest.raises(ValueError, match="device"):
        m.graph_layout(g, "random", a=1.0, b=1.0)
    # fuzzy_graph is the module's function
    got = m.fuzzy_graph(*_hand_case())
    assert torch.equal(got["weights"], g["weights"]) and torch.equal(got["indptr"], g["indptr"])


def test_starts():
    x, _ = blobs()
    y = graph.init_pca(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == (480, 2) and float(y.abs().max()) == 10.0
    q = x.double() - x.double().mean(0)
    var = (q @ torch.linalg.svd(q, full_matrices=False)[2][:2].T).var(0)
    got = y.double().var(0)
    assert got[0] >= got[1] and abs(float(got[0] / got[1]) - float(var[0] / var[1])) <= 1e-5 * float(var[0] / var[1])
    bad = x.clone()
    bad[5, 3] = float("nan")
    bad[9, 0] = float("inf")
    yb = graph.init_pca(bad)
    assert torch.isnan(yb[5]).all() and torch.isnan(yb[9]).all() and int(torch.isfinite(yb).all(1).sum()) == 478
    assert torch.equal(graph.init_pca(torch.zeros(4, 3)), torch.zeros(4, 2))
    assert tuple(graph.init_pca(torch.arange(5.0)[:, None]).shape) == (5, 2)
    r = graph.init_random(100, 3, "cpu")
    assert torch.equal(r, graph.init_random(100, 3, "cpu")) and not torch.equal(r, graph.init_random(100, 4, "cpu"))
    assert r.dtype == torch.float32 and float(r.abs().max()) <= 10.0 and float(r.abs().max()) > 8.0
    assert graph.default_epochs(10000) == 500 and graph.default_epochs(10001) == 200


def test_reference_rules_on_a_small_graph():
    """The restatement's own skip rules: a NaN row and a row without a valid edge keep their position, an epoch
    split through epoch0 is the whole, a bad entry changes nothing."""
    g, _ = _cpu_graph()
    indptr, indices, w = graph.to_csr(g)
    rng = np.random.default_rng(2)
    y = rng.uniform(-3, 3, size=(7, 2)).astype(np.float32)
    args = dict(total_epochs=7, lr=1.0, a=1.58, b=0.9, n_negatives=5, seed=9)
    whole = graph.layout_reference(indptr, indices, w, y, 0, 7, **args)
    part = graph.layout_reference(indptr, indices, w, y, 0, 3, **args)
    assert np.array_equal(whole, graph.layout_reference(indptr, indices, w, part, 3, 4, **args))
    assert np.isfinite(whole).all() and not np.array_equal(whole, y.astype(np.float64))
    yn = y.copy()
    yn[2] = np.nan
    out = graph.layout_reference(indptr, indices, w, yn, 0, 2, **args)
    assert np.isnan(out[2]).all() and np.isfinite(np.delete(out, 2, 0)).all()
    lone = graph.layout_reference(np.zeros(8, dtype=np.int64), indices[:0], w[:0], y, 0, 2, **args)
    assert np.array_equal(lone, y.astype(np.float64))
    # entries the rules skip, appended to row 6's list: the result is that of the clean graph
    bad_i = np.concatenate([indices, np.array([-1, 7, 0, 1, 2, 3], dtype=np.int32)])
    bad_w = np.concatenate([w, np.array([1, 1, 0, -1, np.nan, np.inf], dtype=np.float32)])
    ptr = indptr.copy()
    ptr[-1] += 6
    assert np.array_equal(graph.layout_reference(ptr, bad_i, bad_w, y, 0, 7, **args), whole)


def test_reference_quality_on_the_blobs():
    """The input of the GPU quality test is one on which the reference alone passes: the PCA start is at most 0.90
    pure, the fp64 reference's layout at least 0.97 (8 blobs of 60 points in 16 dimensions, torch generator seed 1;
    measured: start 0.881, layout 0.998 with the negatives' seed 0 and 0.998 with 1)."""
    x, labels = blobs()
    indptr, indices, w = graph.to_csr(blob_graph())
    y0 = graph.init_pca(x)
    assert purity(y0, labels) <= 0.90
    a, b = graph.find_ab(0.1, 1.0)
    y = graph.layout_reference(indptr, indices, w, y0.numpy(), 0, 200, 200, 1.0, a, b, 1.0, 5.0, 8, 0)
    assert np.isfinite(y).all()
    assert purity(y, labels) >= 0.97
