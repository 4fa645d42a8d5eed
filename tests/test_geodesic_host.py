"""CPU-side tests of the shortest-path calls (PoissonFactorization.geodesic / pseudotime, spmf_amd/geodesic.py,
spmf_graph_relax, csrc/graph_paths.hip): the entry point's declaration, size function and error contract on dummy
addresses; the numpy backend through ``solve`` against ``fp32_dijkstra`` -- bit for bit -- on the hand-made edge graph,
the chain of blobs and the spiral, for single sources and for a source set; against scipy's fp64 ``dijkstra`` within
the one derived bound; the predecessor chains; the absorbed addition, the tie and the unreached component;
``length_graph`` against a dense construction; ``pseudotime``, ``path`` and every refusal.  (The valid calls of the
library: tests/test_gpu_geodesic.py.)

The only tolerance is |d - d64| <= (n_sweeps + 1) 2^-23 d: a path of h hops is h float32 additions, each within 2^-24
relative of the exact sum of its operands, so the float32 length of ANY path is within about h 2^-24 of its fp64
length; the float32 optimum is at most the float32 length of the fp64-optimal path and the fp64 optimum at most the
fp64 length of the float32-optimal one -- the rounding counts once each way, and h <= n_sweeps."""
import functools
import inspect

import numpy as np
import pytest
import torch

from _geodesic_cases import (EDGE_ABSORBED, EDGE_N, EDGE_NEAR, EDGE_SPLIT, EDGE_TIE, HEADER_ARGS, assert_errors,
                             assert_scratch_sizes, chain_lengths, edge_graph, edge_sources, fp32_dijkstra, graph_numpy,
                             host_good, scipy_dijkstra, spiral)
from _stream_cases import assert_declared_exported_bound, cpu_model, host_ctx, library, no_library
from spmf_amd import geodesic


def test_entry_point_is_declared_exported_and_bound():
    lib = library()
    for name, nargs in HEADER_ARGS.items():
        assert_declared_exported_bound(name, nargs)
        assert callable(getattr(lib, name)), name
    assert geodesic.BLOCK == 16


def test_methods_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    empty = inspect.Parameter.empty
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        got = [(p.name, p.default) for p in list(inspect.signature(cls.geodesic).parameters.values())[1:]]
        assert got == [("graph", empty), ("sources", empty), ("predecessors", False), ("max_sweeps", None)], got
        got = [(p.name, p.default) for p in list(inspect.signature(cls.pseudotime).parameters.values())[1:5]]
        assert got == [("data", empty), ("root", empty), ("k", 15), ("metric", "euclidean")], got


def test_raw_errors_and_sizes_before_any_device_call():
    """A context of spmf_ctx_create and dummy addresses: no call here is valid, so nothing may be launched, written or
    dereferenced."""
    lib = library()
    h = host_ctx(lib, 3)
    try:
        assert_scratch_sizes(lib, h)
        assert_errors(lib, host_good(lib, h))
    finally:
        lib.spmf_ctx_destroy(h)


# ---- the solved cases, once ------------------------------------------------------------------------------------------
def _spiral_sources():
    x = spiral()[1].double()
    r2 = (x ** 2).sum(1)
    return [int(torch.argmin(r2)), int(torch.argmax(r2)), 1500]


@functools.lru_cache(maxsize=None)
def _solved(case):
    """-> (graph as numpy, the sources of the columns (a list of sets), the result of ``solve`` with predecessors)."""
    if case == "edge":
        g, sets = edge_graph(), [np.array([s]) for s in edge_sources()]
    elif case == "edge_set":
        g, sets = edge_graph(), [np.array([0, 45, 70]), np.array([59, 1])]
    elif case == "chain":
        g, sets = graph_numpy(chain_lengths()[0]), [np.array([0]), np.array([319]), np.array([5, 170, 300])]
    else:
        g, sets = graph_numpy(spiral()[0]), [np.array([s]) for s in _spiral_sources()] + [np.array(_spiral_sources())]
    res = geodesic.solve(geodesic.NumpyOps(g), [torch.from_numpy(s) for s in sets], predecessors=True)
    return g, sets, res


CASES = ["edge", "edge_set", "chain", "spiral"]


@pytest.mark.parametrize("case", CASES)
def test_numpy_backend_is_the_float32_dijkstra_bit_for_bit(case):
    g, sets, res = _solved(case)
    d = res["distances"]
    assert d.dtype == torch.float32 and tuple(d.shape) == (len(g["indptr"]) - 1, len(sets)) and res["converged"]
    print(case, "n_sweeps", res["n_sweeps"])
    for l, s in enumerate(sets):
        want = fp32_dijkstra(g, s)
        assert np.array_equal(d[:, l].numpy(), want), (case, l, np.flatnonzero(d[:, l].numpy() != want)[:5])
        assert not d[s, l].any()
    if case == "spiral":
        assert res["n_sweeps"] < 300 and bool(torch.isfinite(d).all())
    # a single tensor of row numbers is one column each
    if case == "edge":
        one = geodesic.solve(geodesic.NumpyOps(g), torch.from_numpy(edge_sources()))
        assert torch.equal(one["distances"], d) and one["predecessors"] is None and one["n_sweeps"] == res["n_sweeps"]


@pytest.mark.parametrize("case", CASES)
def test_within_the_derived_bound_of_scipys_fp64_dijkstra(case):
    g, sets, res = _solved(case)
    bound = (res["n_sweeps"] + 1) * 2.0 ** -23
    worst = 0.0
    for l, s in enumerate(sets):
        d64 = scipy_dijkstra(g, s)
        d = res["distances"][:, l].double().numpy()
        assert np.array_equal(np.isinf(d), np.isinf(d64))
        ok = np.isfinite(d64)
        rel = np.abs(d[ok] - d64[ok]) / np.where(d64[ok] > 0, d64[ok], 1.0)
        worst = max(worst, float(rel.max()))
        assert (np.abs(d[ok] - d64[ok]) <= bound * d64[ok]).all(), (case, l, float(rel.max()), bound)
    print(case, "worst relative error", worst, "bound", bound)


def _smallest_length(g):
    """{(i, j): the smallest counting length of the entries (i, j)}."""
    from spmf_amd import spectral
    _, row, col, w = spectral.valid_edges(g)
    out = {}
    for i, j, v in zip(row.tolist(), col.tolist(), w.tolist()):
        out[(i, j)] = min(out.get((i, j), np.inf), v)
    return out


@pytest.mark.parametrize("case", CASES)
def test_predecessor_chains_reach_a_source_and_re_add_to_the_distance(case):
    """Every row of the edge graph and of the chain; on the spiral every 7th row (3 000 rows, chains of up to 225)."""
    g, sets, res = _solved(case)
    d, p = res["distances"].numpy(), res["predecessors"]
    assert p.dtype == torch.int32 and p.shape == res["distances"].shape
    length = _smallest_length(g)
    n, absorbed = d.shape[0], 0
    rows = range(n) if n < 400 else range(0, n, 7)
    for l, s in enumerate(sets):
        src = set(s.tolist())
        assert all(int(p[i, l]) == -1 for i in src), "a source has no predecessor"
        assert not ((p[:, l].numpy() >= 0) & ~np.isfinite(d[:, l])).any(), "an unreached row has none either"
        for i in rows:
            if not np.isfinite(d[i, l]):
                with pytest.raises(ValueError, match=f"ends at row {i}"):
                    geodesic.path(res, l, i)
                continue
            chain = geodesic.path(p, l, i)
            end = chain[-1]
            assert chain[0] == i and len(chain) <= res["n_sweeps"] + 1
            if end not in src:                                   # only an absorbed addition may end a chain early
                absorbed += end == i
                j = [c for (r, c), v in length.items() if r == end and d[c, l] == d[end, l]
                     and np.float32(d[c, l]) + np.float32(v) == d[end, l]]
                assert j, (case, l, i, end)
                with pytest.raises(ValueError, match=f"ends at row {end}, which is no source"):
                    geodesic.path(p, l, i, distances=res["distances"])
            else:
                assert geodesic.path(res, l, i) == chain
            along = d[chain, l]
            assert (along[:-1] > along[1:]).all(), "strictly decreasing towards the source"
            back = np.float32(d[end, l])                          # 0 at a source
            for a, b in zip(chain[::-1][:-1], chain[::-1][1:]):   # from the source outwards: the edge a -> b
                back = np.float32(back + np.float32(length[(b, a)]))
            assert back == d[i, l], (case, l, i, float(back), float(d[i, l]))
    assert absorbed >= 1 if case == "edge" else absorbed == 0 or case == "edge_set"


def test_the_absorbed_addition_the_tie_and_the_unreached_component():
    g, _, res = _solved("edge")
    d, p = res["distances"][:, 0], res["predecessors"][:, 0]         # column 0: source row 0
    assert float(d[EDGE_NEAR]) == 1.0 and int(p[EDGE_NEAR]) == 0
    assert float(d[EDGE_ABSORBED]) == 1.0 and int(p[EDGE_ABSORBED]) == -1
    with pytest.raises(ValueError, match=f"ends at row {EDGE_ABSORBED}, which is no source"):
        geodesic.path(res, 0, EDGE_ABSORBED)
    assert float(d[34]) == 0.25 and float(d[35]) == 0.5 and float(d[EDGE_TIE]) == 0.75
    assert int(p[EDGE_TIE]) == 34, "the first in list order wins a tie"
    assert geodesic.path(res, 0, EDGE_TIE) == [EDGE_TIE, 34, 0]
    assert bool(torch.isinf(d[EDGE_SPLIT:]).all()) and bool((p[EDGE_SPLIT:] == -1).all())
    assert float(d[2]) == float("inf"), "the row without entries is reached by nobody"
    # from a source in the second component, the first stays unreached; the row without entries reaches all it can
    sources = edge_sources().tolist()
    assert bool(torch.isinf(res["distances"][:EDGE_SPLIT, sources.index(60)]).all())
    assert int(torch.isfinite(res["distances"][:, sources.index(2)]).sum()) > 30
    # the junk row: only (5, 0.7), (5, 0.4), (14, 1.0), (50, 1.25), (51, 0.5) count, and the smaller repeat is used
    d0 = res["distances"][:, 0]
    want = min(np.float32(d0[5]) + np.float32(0.4), np.float32(d0[50]) + np.float32(1.25),
               np.float32(d0[51]) + np.float32(0.5))
    assert float(d0[14]) == float(want)
    # a NaN stays where it is and reaches nobody
    ops = geodesic.NumpyOps(g)
    x = torch.full((EDGE_N, 16), float("inf"))
    x[0, 0], x[5, 0], x[5, 1] = 0.0, float("nan"), float("nan")
    y, _, _ = ops.relax(x, 20, False)
    assert bool(torch.isnan(y[5, 0])) and int(torch.isnan(y).sum()) == 2
    assert bool(torch.isinf(y[:, 1][torch.arange(EDGE_N) != 5]).all())


def test_relax_counts_sweeps_and_reports_the_change():
    ops = geodesic.NumpyOps(edge_graph())
    x = torch.full((EDGE_N, 16), float("inf"))
    x[0, 0] = 0.0
    y0, p0, c0 = ops.relax(x, 0, True)
    assert torch.equal(y0, x) and p0 is None and c0 is False
    y1, _, c1 = ops.relax(x, 1, False)
    y2, _, c2 = ops.relax(y1, 1, False)
    y12, p12, c12 = ops.relax(x, 2, True)
    assert c1 and c2 and c12 and torch.equal(y2, y12) and not torch.equal(y1, y2) and p12.dtype == torch.int32
    fixed, _, changed = ops.relax(x, EDGE_N, False)
    assert not changed and torch.equal(ops.relax(fixed, 1, False)[0], fixed)
    # the driver: max_sweeps is reported, not raised; the count is in units of a call
    short = geodesic.solve(ops, torch.tensor([0]), max_sweeps=2)
    assert not short["converged"] and short["n_sweeps"] == 2 and torch.equal(short["distances"][:, 0], y2[:, 0])
    full = geodesic.solve(ops, torch.tensor([0]), sweeps_per_call=1)
    coarse = geodesic.solve(ops, torch.tensor([0]), sweeps_per_call=16)
    assert full["converged"] and coarse["converged"] and torch.equal(full["distances"], coarse["distances"])
    assert coarse["n_sweeps"] == 16 * -(-full["n_sweeps"] // 16) and full["n_sweeps"] <= 16


def test_column_16_of_17_sources_is_a_single_source_run():
    g = graph_numpy(chain_lengths()[0])
    ops = geodesic.NumpyOps(g)
    sources = torch.arange(0, 17 * 18, 18)
    res = geodesic.solve(ops, sources, predecessors=True)
    assert tuple(res["distances"].shape) == (320, 17)
    one = geodesic.solve(ops, sources[16:], predecessors=True)
    assert torch.equal(res["distances"][:, 16], one["distances"][:, 0])
    assert torch.equal(res["predecessors"][:, 16], one["predecessors"][:, 0])
    first = geodesic.solve(ops, sources[3:4])
    assert torch.equal(res["distances"][:, 3], first["distances"][:, 0])


def test_length_graph_is_the_dense_construction():
    N, k = 9, 3
    idx = torch.tensor([[1, 2, 3], [0, 2, -1], [1, 0, 4], [0, 4, 5], [3, 5, 2], [4, 3, -1], [7, -1, -1], [6, 8, 1],
                        [7, -1, -1]])
    rng = np.random.default_rng(2)
    pts = rng.normal(size=(N, 2))
    dist = torch.tensor([[np.linalg.norm(pts[i] - pts[j]) if j >= 0 else np.inf for j in row]
                         for i, row in enumerate(idx.tolist())], dtype=torch.float32)
    dist[7, 2] = 9.0                                        # an asymmetric pair: 1 does not list 7
    g = geodesic.length_graph(idx, dist)
    dense = np.full((N, N), np.inf, dtype=np.float32)
    for i in range(N):
        for c in range(k):
            j = int(idx[i, c])
            if j >= 0:
                dense[i, j] = min(dense[i, j], float(dist[i, c]))
                dense[j, i] = min(dense[j, i], float(dist[i, c]))
    indptr, indices, w = g["indptr"].numpy(), g["indices"].numpy(), g["weights"].numpy()
    assert g["indptr"].dtype == torch.int64 and g["indices"].dtype == torch.int32 and g["weights"].dtype == torch.float32
    got = np.full((N, N), np.inf, dtype=np.float32)
    for i in range(N):
        cols = indices[indptr[i]:indptr[i + 1]]
        assert (np.diff(cols) > 0).all(), "ascending, no repeats"
        got[i, cols] = w[indptr[i]:indptr[i + 1]]
    assert np.array_equal(got, dense) and np.array_equal(got, got.T) and int(indptr[-1]) == len(indices)
    assert np.isfinite(got[1, 7]) and got[1, 7] == np.float32(9.0)
    # the smaller of two directions, self entries and bad distances dropped
    g2 = geodesic.length_graph(torch.tensor([[1, 0], [0, -1]]), torch.tensor([[2.0, 0.5], [1.5, float("inf")]]))
    assert g2["indptr"].tolist() == [0, 1, 2] and g2["indices"].tolist() == [1, 0] and g2["weights"].tolist() == [1.5, 1.5]
    for bad, what in (((torch.tensor([[2]]), torch.tensor([[1.0]])), "outside"),
                      ((torch.tensor([[1, 1], [0, 0]]), torch.ones(2, 2)), "twice"),
                      ((torch.tensor([[1.0]]), torch.tensor([[1.0]])), "integers"),
                      ((torch.tensor([[0]]), torch.tensor([[1]])), "floating point"),
                      ((torch.tensor([0]), torch.tensor([1.0])), "2-D")):
        with pytest.raises(ValueError, match="length_graph: .*" + what):
            geodesic.length_graph(*bad)


def test_lengths_from_weights():
    g = {"indptr": torch.tensor([0, 3, 6]), "indices": torch.tensor([1, 1, 1, 0, 0, 0], dtype=torch.int32),
         "weights": torch.tensor([1.0, 0.5, 0.0, 1.5, float("nan"), 1e-30], dtype=torch.float32)}
    out = geodesic.lengths_from_weights(g)
    w = out["weights"]
    assert w.dtype == torch.float32 and out["indptr"] is g["indptr"] and out["indices"] is g["indices"]
    assert float(w[0]) == geodesic.UNIT_WEIGHT_LENGTH == 2.0 ** -24
    assert float(w[1]) == float(np.float32(-np.log(0.5))) and bool(torch.isinf(w[2:5]).all())
    assert float(w[5]) == float(np.float32(-np.log(np.float64(np.float32(1e-30)))))
    near = geodesic.lengths_from_weights(dict(g, weights=torch.tensor([1.0 - 2.0 ** -24] * 6)))["weights"]
    assert float(near[0]) >= geodesic.UNIT_WEIGHT_LENGTH
    with pytest.raises(ValueError, match="lengths_from_weights: graph must be a dict"):
        geodesic.lengths_from_weights({"indptr": g["indptr"]})


def test_pseudotime_and_path():
    inf, nan = float("inf"), float("nan")
    d = torch.tensor([[0.0, inf, 0.0], [2.0, 0.0, inf], [4.0, 1.0, inf], [inf, 0.5, inf]])
    t = geodesic.pseudotime(d)
    assert t.dtype == torch.float32 and t.shape == d.shape
    assert t[:, 0].tolist()[:3] == [0.0, 0.5, 1.0] and bool(torch.isnan(t[3, 0]))
    assert t[1:, 1].tolist() == [0.0, 1.0, 0.5] and bool(torch.isnan(t[0, 1]))
    assert float(t[0, 2]) == 0.0 and bool(torch.isnan(t[1:, 2]).all())
    assert geodesic.pseudotime(d[:, 0]).tolist()[:3] == [0.0, 0.5, 1.0]
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, 2, 2)):
        with pytest.raises(ValueError, match="pseudotime: distances"):
            geodesic.pseudotime(bad)
    pred = torch.tensor([[-1, 1], [0, -1], [1, 0], [-1, 3]], dtype=torch.int32)
    dist = torch.tensor([[0.0, 1.0], [1.0, 0.0], [2.0, 2.0], [inf, inf]])
    assert geodesic.path(pred, 0, 2) == [2, 1, 0] and geodesic.path(pred, 0, 2, distances=dist) == [2, 1, 0]
    assert geodesic.path(pred, 1, 2, distances=dist) == [2, 0, 1]
    assert geodesic.path({"predecessors": pred, "distances": dist}, 0, 0) == [0]
    with pytest.raises(ValueError, match="ends at row 3, which is no source"):
        geodesic.path(pred, 0, 3, distances=dist)
    with pytest.raises(ValueError, match="cycle"):
        geodesic.path(pred, 1, 3)
    for kw, what in ((dict(column=2, row=0), "column"), (dict(column=0, row=4), "row"),
                     (dict(column=-1, row=0), "column"), (dict(column=0, row=1.0), "row")):
        with pytest.raises(ValueError, match="path: " + what):
            geodesic.path(pred, **kw)
    with pytest.raises(ValueError, match="path: no predecessors"):
        geodesic.path({"predecessors": None, "distances": dist}, 0, 0)
    with pytest.raises(ValueError, match="path: predecessors must be integers"):
        geodesic.path(dist, 0, 0)


def test_solve_refuses_bad_sources():
    ops = geodesic.NumpyOps(edge_graph())
    for bad, what in ((torch.tensor([EDGE_N]), r"must lie in \[0, 83\), got 83"), (torch.tensor([-1]), "got -1"),
                      (torch.tensor([], dtype=torch.int64), "at least one row"), ([], "at least one row"),
                      ([torch.tensor([0]), torch.tensor([], dtype=torch.int64)], "in every set"),
                      (torch.tensor([0.0]), "integers"), (torch.tensor([True]), "integers"),
                      (torch.zeros(2, 2, dtype=torch.int64), "1-D"), ([torch.tensor([0, 90])], "got 90")):
        with pytest.raises(ValueError, match="geodesic: sources .*" + what):
            geodesic.solve(ops, bad)
    for kw, what in ((dict(max_sweeps=0), "max_sweeps"), (dict(max_sweeps=1.5), "max_sweeps"),
                     (dict(sweeps_per_call=0), "sweeps_per_call")):
        with pytest.raises(ValueError, match="geodesic: " + what):
            geodesic.solve(ops, torch.tensor([0]), **kw)
    assert geodesic.solve(ops, np.array([0, 1]))["distances"].shape == (EDGE_N, 2)        # numpy rows are taken


def test_every_argument_check_raises_before_a_library_call(monkeypatch):
    g = {n: t for n, t in chain_lengths()[0].items()}
    m = cpu_model()[0]
    no_library(monkeypatch)
    src = torch.tensor([0])
    for bad in (None, {}, {"indptr": g["indptr"], "indices": g["indices"]}):
        with pytest.raises(ValueError, match="geodesic: graph must be a dict"):
            m.geodesic(bad, src)
    for key, t in (("indptr", g["indptr"].to(torch.int32)), ("indices", g["indices"].to(torch.int64)),
                   ("weights", g["weights"].double())):
        with pytest.raises(ValueError, match="geodesic: .*" + key):
            m.geodesic(dict(g, **{key: t}), src)
    ind = g["indices"].clone()
    ind[3] = -1
    with pytest.raises(ValueError, match="must lie in"):
        m.geodesic(dict(g, indices=ind), src)
    for bad, what in ((torch.tensor([320]), "must lie in"), (torch.tensor([0.5]), "integers"), ([], "at least one")):
        with pytest.raises(ValueError, match="geodesic: sources .*" + what):
            m.geodesic(g, bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="geodesic: max_sweeps"):
            m.geodesic(g, src, max_sweeps=bad)
    # a model on the CPU runs the numpy backend: the arrays of solve(NumpyOps), without the library
    res = m.geodesic(g, torch.tensor([0, 319]), predecessors=True)
    want = geodesic.solve(geodesic.NumpyOps(g), torch.tensor([0, 319]), predecessors=True)
    assert torch.equal(res["distances"], want["distances"]) and torch.equal(res["predecessors"], want["predecessors"])
    assert res["n_sweeps"] == want["n_sweeps"] and res["converged"]
    for kw, what in ((dict(k=0), "k"), (dict(k=65), "k"), (dict(metric="manhattan"), "metric")):
        with pytest.raises(ValueError, match="pseudotime.*" + what):
            m.pseudotime(np.ones((4, 6)), 0, **kw)
    for root, what in ((0.5, "root"), (None, "root"), (True, "root"), (torch.tensor([0.5]), "integers"),
                       (-1, "must lie in"), (torch.tensor([], dtype=torch.int64), "at least one")):
        with pytest.raises(ValueError, match="pseudotime: .*" + what):
            m.pseudotime(np.ones((4, 6)), root)


def test_the_blob_chain_is_ordered_by_pseudotime():
    g, _, truth = chain_lengths()
    res = geodesic.solve(geodesic.NumpyOps(g), torch.tensor([0]))
    t = geodesic.pseudotime(res["distances"][:, 0])
    assert bool(torch.isfinite(t).all()) and float(t.max()) == 1.0 and float(t[0]) == 0.0
    means = [float(t[truth == b].mean()) for b in range(4)]
    assert means == sorted(means) and means[0] < 0.25 and means[3] > 0.6, means
