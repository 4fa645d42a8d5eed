"""CPU-side tests of graph clustering (PoissonFactorization.communities, spmf_amd/communities.py, spmf_graph_move,
csrc/graph_move.hip): the entry point's declaration and its error contract on dummy addresses, the driver on its numpy
backend -- modularity against networkx, the planted partitions, the quality bar against networkx's own Louvain,
determinism and the invariants of the integer steps -- and every argument check with the library unloadable.  (The
valid calls of the library: tests/test_gpu_communities.py.)

Measured here with the numpy backend (communities / Q / sweeps per level), beside networkx's louvain_communities over
the seeds 0..9 (min .. max of Q):
  blobs, N = 600:   6 / 0.8333285 / 26, 12, 8, 2     networkx 0.8333285 .. 0.8333285
  two rings, N = 400: 17 / 0.9024646 / 18, 10, 7, 3, 2  networkx 0.9041597 .. 0.9059729 (bar 0.9023465)
  30 cliques of 5:  15 / 0.8878788 / 6, 17, 2        networkx 0.8854545 .. 0.8878788"""
import inspect
import os

import numpy as np
import pytest
import torch

from _communities_cases import (GROUP_LEN, HEADER_ARGS, assert_errors, blobs, cliques, edge_graph, end_to_end_graphs,
                                host_good, nx_graphs, nx_louvain_range, partition, two_rings)
from _stream_cases import ROOT, assert_declared_exported_bound, cpu_model, host_ctx, library, no_library
from spmf_amd import communities


def _solve(g, **kw):
    return communities.solve(communities.NumpyOps(g), **kw)


def test_entry_point_is_declared_exported_and_bound():
    lib = library()
    for name, nargs in HEADER_ARGS.items():
        assert_declared_exported_bound(name, nargs)
        assert callable(getattr(lib, name)), name
    hdr = open(os.path.join(ROOT, "include", "spmf_hip.h")).read()
    assert f"#define SPMF_MOVE_GROUP_LEN {GROUP_LEN}" in hdr and communities.GROUP_LEN == GROUP_LEN


def test_method_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    want = [("graph", inspect.Parameter.empty), ("resolution", 1.0), ("max_levels", 32), ("max_sweeps", 100),
            ("tol", 1e-7)]
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        got = [(p.name, p.default) for p in list(inspect.signature(cls.communities).parameters.values())[1:]]
        assert got == want, (cls.__name__, got)


def test_raw_errors_return_before_any_device_call():
    """A context of spmf_ctx_create and dummy addresses: no call here is valid but the empty ones, so nothing may be
    launched or dereferenced."""
    lib = library()
    h = host_ctx(lib, 3)
    try:
        assert_errors(lib, host_good(h))
    finally:
        lib.spmf_ctx_destroy(h)


@pytest.mark.parametrize("name", ["blobs", "rings", "cliques"])
def test_modularity_is_networkx_modularity(name):
    import networkx as nx
    g = dict(end_to_end_graphs())[name]
    di, _ = nx_graphs(g)
    res = _solve(g)
    want = nx.community.modularity(di, partition(res["labels"].numpy()), weight="weight")
    assert abs(communities.modularity(res["labels"], g) - want) <= 1e-9
    assert abs(res["modularity"] - want) <= 1e-9
    assert res["modularity"] == res["levels"][-1]["modularity"]
    # another labelling and another resolution, self entries included (the coarse graph of the result)
    rng = np.random.default_rng(1)
    lab = rng.integers(0, 7, size=len(res["labels"]))
    for gamma in (1.0, 0.6, 2.5):
        want = nx.community.modularity(di, partition(lab), weight="weight", resolution=gamma)
        assert abs(communities.modularity(lab, g, gamma) - want) <= 1e-9


def test_modularity_with_self_entries_is_the_coarse_graphs():
    import networkx as nx
    g = two_rings()
    n, row, col, wq = (torch.as_tensor(v) for v in communities.valid_edges(g))
    lab = torch.arange(400) // 7
    G, inv, r, c, w = communities.aggregate(lab, row, col, wq)
    assert G == 58 and int((r == c).sum()) > 0                      # groups with internal weight: self entries
    coarse = {"indptr": torch.searchsorted(r, torch.arange(G + 1)), "indices": c.to(torch.int32), "wq": w}
    di, _ = nx_graphs(coarse)
    pairs = np.arange(G) // 2
    want = nx.community.modularity(di, partition(pairs), weight="weight")
    assert abs(communities.modularity(pairs, coarse) - want) <= 1e-9
    assert abs(communities.modularity(pairs[inv.numpy()], g) - want) <= 1e-9       # the same partition of the rows


def test_blobs_give_exactly_the_planted_partition():
    g, _, truth = blobs()
    res = _solve(g)
    assert res["n_communities"] == 6 and res["sizes"].tolist() == [100] * 6
    lab = res["labels"].numpy()
    for b in range(6):
        assert len(set(lab[truth.numpy() == b].tolist())) == 1, b
    assert len(set(lab.tolist())) == 6
    assert lab.tolist() == truth.tolist()          # equal sizes: numbered by the smallest member row


def test_no_clique_is_split():
    g, clique = cliques()
    res = _solve(g)
    lab = res["labels"].numpy()
    for c in range(30):
        assert len(set(lab[clique == c].tolist())) == 1, c
    assert res["n_communities"] == 15 and res["sizes"].tolist() == [10] * 15       # the known optimum: pairs


@pytest.mark.parametrize("name", ["blobs", "rings", "cliques"])
def test_quality_against_networkx_louvain(name):
    """Ours >= the minimum of networkx's Louvain over the seeds 0..9 minus the seeds' own spread (max - min, with
    a floor of 1e-3): the bar comes from the reference's own variation."""
    g = dict(end_to_end_graphs())[name]
    lo, hi = nx_louvain_range(name)
    res = _solve(g)
    bar = lo - max(hi - lo, 1e-3)
    print(f"communities {name}: ours {res['modularity']:.7f} in {res['n_communities']} communities, sweeps "
          f"{[lv['n_sweeps'] for lv in res['levels']]}; networkx {lo:.7f} .. {hi:.7f}, bar {bar:.7f}")
    assert res["modularity"] >= bar


def test_quantise_and_aggregate_keep_m2():
    g = two_rings()
    wq = communities.quantise(g["weights"])
    assert wq.dtype == torch.int64
    want = np.rint(g["weights"].numpy().astype(np.float64) * 2.0 ** 24).astype(np.int64)
    assert np.array_equal(wq.numpy(), want) and np.array_equal(communities.quantise(g["weights"].numpy()), want)
    assert communities.quantise(torch.tensor([float("nan"), float("inf"), -1.0, 2.0 ** -26, 0.75])).tolist() == \
        [0, 0, -2 ** 24, 0, 3 * 2 ** 22]
    n, row, col, w = (torch.as_tensor(v) for v in communities.valid_edges(g))
    m2 = int(w.sum())
    assert m2 == int(wq[wq >= 1].sum())
    lab = torch.as_tensor(np.random.default_rng(0).integers(0, 400, size=400))
    G, inv, r, c, cw = communities.aggregate(lab, row, col, w)
    assert int(cw.sum()) == m2 and G == len(set(lab.tolist()))
    assert torch.equal(torch.unique(lab)[inv], lab)                   # renumbered by ascending old label
    key = r * G + c
    assert bool((key[1:] > key[:-1]).all())                          # rows and columns ascending, each pair once
    dense = torch.zeros(G, G, dtype=torch.int64)
    dense.index_put_((inv[row], inv[col]), w, accumulate=True)
    assert torch.equal(dense[r, c], cw) and int((dense != 0).sum()) == len(cw)
    # every level of a run has the same M2: the levels' modularity is comparable
    res = _solve(g)
    assert [lv["n_nodes"] for lv in res["levels"][1:]] == [lv["n_communities"] for lv in res["levels"][:-1]]
    assert res["levels"][-1]["n_communities"] == res["levels"][-1]["n_nodes"]
    q = [lv["modularity"] for lv in res["levels"]]
    assert all(b >= a - 1e-12 for a, b in zip(q, q[1:])), q


def test_two_runs_give_equal_labels_and_bits():
    for _, g in end_to_end_graphs():
        a, b = _solve(g), _solve(g)
        assert torch.equal(a["labels"], b["labels"]) and a["labels"].dtype == torch.int64
        assert np.float64(a["modularity"]).tobytes() == np.float64(b["modularity"]).tobytes()
        assert a["levels"] == b["levels"]


def test_labels_are_ordered_by_size_and_isolated_rows_get_minus_one():
    g = {n: t.clone() for n, t in two_rings().items() if n in ("indptr", "indices", "weights")}
    dead = (5, 300)
    row = torch.repeat_interleave(torch.arange(400), torch.diff(g["indptr"]))
    for d in dead:
        g["weights"][(row == d) | (g["indices"] == d)] = 0.0
    res = _solve(g)
    lab = res["labels"].numpy()
    assert (lab[list(dead)] == -1).all() and int((lab == -1).sum()) == 2
    sizes = res["sizes"].numpy()
    assert (np.diff(sizes) <= 0).all() and sizes.sum() == 398 and len(sizes) == res["n_communities"]
    assert np.array_equal(np.bincount(lab[lab >= 0]), sizes)
    first = np.array([np.flatnonzero(lab == c)[0] for c in range(len(sizes))])
    for c in range(len(sizes) - 1):
        assert sizes[c] > sizes[c + 1] or first[c] < first[c + 1]       # ties by the smallest member row
    lab2, sz2 = communities.canonical_labels([7, 7, 3, 3, 9, 3, 1], [True, True, True, True, True, True, False])
    assert lab2.tolist() == [1, 1, 0, 0, 2, 0, -1] and sz2.tolist() == [3, 2, 1]
    lab3, sz3 = communities.canonical_labels([4, 2, 4, 2], [True] * 4)
    assert lab3.tolist() == [0, 1, 0, 1] and sz3.tolist() == [2, 2]
    # a graph without a counting entry: every row -1, no level
    empty = {"indptr": torch.zeros(6, dtype=torch.int64), "indices": torch.zeros(0, dtype=torch.int32),
             "weights": torch.zeros(0)}
    res = _solve(empty)
    assert res["labels"].tolist() == [-1] * 5 and res["n_communities"] == 0 and res["levels"] == []
    assert np.isnan(res["modularity"])


def test_higher_resolution_gives_at_least_as_many_communities_on_the_rings():
    g = two_rings()
    counts = [_solve(g, resolution=r)["n_communities"] for r in (0.25, 0.5, 1.0, 2.0, 4.0)]
    assert all(b >= a for a, b in zip(counts, counts[1:])) and counts[-1] > counts[0], counts


def test_max_sweeps_and_max_levels_cut_the_run_short_and_keep_the_best():
    g = two_rings()
    res = _solve(g, max_sweeps=3)
    assert res["levels"][0]["n_sweeps"] == 3 and res["levels"][0]["hit_max_sweeps"]
    assert abs(communities.modularity(res["labels"], g) - res["modularity"]) <= 1e-12
    one = _solve(g, max_levels=1)
    assert len(one["levels"]) == 1 and one["n_communities"] == one["levels"][0]["n_communities"]
    assert abs(communities.modularity(one["labels"], g) - one["modularity"]) <= 1e-12


def test_the_sweep_on_the_edge_graph_follows_its_definition():
    """NumpyOps.move against a plain-Python restatement of the definition, row by row, on the hand-made graph: the
    vectorised sweep is what the kernel is held to, so it is held to the text first."""
    from _communities_cases import EDGE_TIE_DOWN, EDGE_TIE_UP, EDGE_WRONG_SIDE
    e = edge_graph()
    n, row, col, wq = communities.valid_edges(e)
    lab, tot, k, m2 = e["labels"].astype(np.int64), e["tot"], e["k"], e["m2"]
    ops = communities.NumpyOps(e)
    for direction in (0, 1):
        for gamma in (1.0, 0.37):
            got = ops.move(torch.from_numpy(e["labels"]), torch.from_numpy(tot), gamma, m2, direction).numpy()
            want = lab.copy()
            for i in range(n):
                mine = (row == i) & (col != i)
                links = {}
                for c, w in zip(lab[col[mine]].tolist(), wq[mine].tolist()):
                    links[c] = links.get(c, 0) + w
                a, ki = int(lab[i]), int(k[i])
                if ki == 0:
                    continue
                gk = gamma * float(ki)

                def score(c):
                    t = int(tot[c]) - (ki if c == a else 0)
                    return float(links.get(c, 0)) - (gk * float(t)) / float(m2)
                best = None
                for c in sorted(links):
                    if (c > a if direction == 0 else c < a) and (best is None or score(c) > score(best)):
                        best = c
                if best is not None and score(best) > score(a):
                    want[i] = best
            assert np.array_equal(got, want), (direction, gamma, np.flatnonzero(got != want))
            assert int((got != lab).sum()) > 20
            if gamma == 1.0:
                assert got[EDGE_TIE_UP] == (70 if direction == 0 else 1)
                assert got[EDGE_TIE_DOWN] == (80 if direction == 0 else 62)
                assert got[EDGE_WRONG_SIDE] == (68 if direction == 0 else 40)
    assert m2 < 2 ** 62 and int(tot.max()) > 2 ** 58 and got[2] == lab[2]


def test_m2_beyond_2_62_is_refused():
    g = {"indptr": torch.tensor([0, 1, 2]), "indices": torch.tensor([1, 0], dtype=torch.int32),
         "wq": torch.tensor([2 ** 61, 2 ** 61])}
    with pytest.raises(ValueError, match="2\\^62"):
        _solve(g)
    g["wq"] = torch.tensor([2 ** 60, 2 ** 60])
    assert _solve(g)["labels"].tolist() == [0, 0]


def test_every_argument_check_raises_before_a_library_call(monkeypatch):
    m = cpu_model()[0]
    no_library(monkeypatch)
    g = {n: t for n, t in two_rings().items() if n in ("indptr", "indices", "weights")}
    nan, inf = float("nan"), float("inf")
    for kw, what in ((dict(resolution=0.0), "resolution"), (dict(resolution=-1.0), "resolution"),
                     (dict(resolution=nan), "resolution"), (dict(resolution=inf), "resolution"),
                     (dict(resolution="1"), "resolution"), (dict(resolution=True), "resolution"),
                     (dict(max_levels=0), "max_levels"), (dict(max_levels=1.5), "max_levels"),
                     (dict(max_sweeps=0), "max_sweeps"), (dict(max_sweeps=True), "max_sweeps"),
                     (dict(tol=-1e-9), "tol"), (dict(tol=nan), "tol"), (dict(tol=None), "tol")):
        with pytest.raises(ValueError, match="communities: " + what):
            m.communities(g, **kw)
        with pytest.raises(ValueError, match="communities: " + what):
            communities.solve(None, **kw)
    for bad in (None, {}, {"indptr": g["indptr"], "indices": g["indices"]}):
        with pytest.raises(ValueError, match="communities: graph must be a dict"):
            m.communities(bad)
    for name, t in (("indptr", g["indptr"].to(torch.int32)), ("indices", g["indices"].to(torch.int64)),
                    ("weights", g["weights"].double()), ("weights", g["weights"].numpy())):
        with pytest.raises(ValueError, match="communities: .*" + name):
            m.communities(dict(g, **{name: t}))
    with pytest.raises(ValueError, match="entries"):
        m.communities(dict(g, weights=g["weights"][:-1]))
    ptr = g["indptr"].clone()
    ptr[-1] += 1
    with pytest.raises(ValueError, match="rise from 0"):
        m.communities(dict(g, indptr=ptr))
    ind = g["indices"].clone()
    ind[3] = 400
    with pytest.raises(ValueError, match="must lie in"):
        m.communities(dict(g, indices=ind))
    with pytest.raises(ValueError, match="communities: .*device"):      # host memory is never handed to the library
        m.communities(g)
    lab = np.zeros(400, dtype=np.int64)
    with pytest.raises(ValueError, match="one entry per row"):
        communities.modularity(lab[:-1], g)
    lab[3] = -1
    with pytest.raises(ValueError, match="negative label"):
        communities.modularity(lab, g)
