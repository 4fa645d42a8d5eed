"""CPU-side tests of PAGA (PoissonFactorization.paga / paga_init, spmf_amd/paga.py, spmf_graph_group_edges,
csrc/graph_groups.hip): the entry point's declaration, size function and error contract on dummy addresses; the numpy
backend against a plain Python double loop on the hand-made edge graph; ``connectivity`` on the worked example of its
docstring; ``tree`` with a tie; ``layout_init``'s boxes, scale and seed; every argument check with the library
unloadable; and the script's refusal of --paga without labels.  (The valid calls of the library:
tests/test_gpu_paga.py.)  No result of the reduction has a tolerance: every compared value is an integer, or an fp64
made from integers by one function; only the float32 positions of a layout start are compared within their own
rounding."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from _communities_cases import edge_graph
from _paga_cases import (HEADER_ARGS, MAX_GROUPS, assert_errors, assert_scratch_sizes, chain, edge_labellings,
                         host_good, loop_group_edges, path_order)
from _stream_cases import ROOT, assert_declared_exported_bound, cpu_model, host_ctx, library, no_library
from spmf_amd import paga


def test_entry_point_is_declared_exported_and_bound():
    lib = library()
    for name, nargs in HEADER_ARGS.items():
        assert_declared_exported_bound(name, nargs)
        assert callable(getattr(lib, name)), name
    hdr = open(os.path.join(ROOT, "include", "spmf_hip.h")).read()
    assert f"#define SPMF_GROUP_EDGES_MAX_GROUPS {MAX_GROUPS}" in hdr and paga.MAX_GROUPS == MAX_GROUPS


def test_methods_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    empty = inspect.Parameter.empty
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        got = [(p.name, p.default) for p in list(inspect.signature(cls.paga).parameters.values())[1:]]
        assert got == [("graph", empty), ("labels", empty), ("n_groups", None)], (cls.__name__, got)
        got = [(p.name, p.default) for p in list(inspect.signature(cls.paga_init).parameters.values())[1:6]]
        assert got == [("graph", empty), ("labels", empty), ("n_groups", None), ("seed", 0), ("threshold", 0.0)]


def test_raw_errors_and_sizes_before_any_device_call():
    """A context of spmf_ctx_create and dummy addresses: no call here is valid, so nothing may be launched, filled or
    dereferenced."""
    lib = library()
    h = host_ctx(lib, 3)
    try:
        assert_scratch_sizes(lib, h)
        assert_errors(lib, host_good(lib, h))
    finally:
        lib.spmf_ctx_destroy(h)


def test_numpy_backend_follows_the_definition_on_the_edge_graph():
    """NumpyOps.group_edges against a plain Python double loop: rows of 0 .. 600 entries, columns -1 and N, wq of 0 and
    negative, a falling indptr, self entries, a repeated column and wq near 2^50."""
    e = edge_graph()
    ops = paga.NumpyOps(e)
    assert ops.n == 83
    for name, labels, G in edge_labellings():
        count, weight, size = ops.group_edges(torch.from_numpy(labels), G)
        want = loop_group_edges(e, labels, G)
        for got, ref, what in zip((count, weight, size), want, ("count", "weight", "size")):
            assert got.dtype == torch.int64 and np.array_equal(got.numpy(), ref), (name, what)
        assert int(count.sum()) > 0 and int(weight.max()) > 2 ** 50
    # the folded labelling does skip rows at both ends, and keeps an empty group
    _, folded, G = edge_labellings()[1]
    count, _, size = ops.group_edges(torch.from_numpy(folded), G)
    every = ops.group_edges(torch.from_numpy(np.where((folded < 0) | (folded >= G), 0, folded).astype(np.int32)), G)[0]
    assert int(count.sum()) < int(every.sum()) and int(size[3]) == 0 and int(size.sum()) == 83 - 9
    assert not count[3].any() and not count[:, 3].any()


def test_the_worked_example():
    g = {"indptr": torch.tensor([0, 1, 3, 5, 6]), "indices": torch.tensor([1, 0, 2, 3, 1, 2], dtype=torch.int32),
         "weights": torch.ones(6)}
    res = paga.solve(paga.NumpyOps(g), np.array([0, 0, 1, 1]))
    assert res["edge_count"].tolist() == [[2, 1], [1, 2]] and res["sizes"].tolist() == [2, 2]
    assert res["edge_weight"].tolist() == [[2 << 24, 1 << 24], [1 << 24, 2 << 24]]
    assert res["expected"].tolist() == [[0.0, 4.0], [4.0, 0.0]]
    assert res["connectivities"].tolist() == [[0.0, 0.5], [0.5, 0.0]]
    assert res["connectivities_tree"].tolist() == [[0.0, 0.5], [0.5, 0.0]] and res["n_groups"] == 2
    assert res["connectivities"].dtype == torch.float64
    # int32 labels, negative = no group, an explicit G with an empty group
    res = paga.solve(paga.NumpyOps(g), torch.tensor([0, -7, 1, 1], dtype=torch.int32), n_groups=3)
    assert res["edge_count"].tolist() == [[0, 0, 0], [0, 2, 0], [0, 0, 0]] and res["sizes"].tolist() == [1, 2, 0]
    assert not res["connectivities"].any()
    # the clip at 1, the rule for n <= 1, and numbers beyond int64 in the numerator
    conn, expected = paga.connectivity(np.array([[0, 50], [50, 0]]), np.array([1, 1]))
    assert conn.tolist() == [[0.0, 1.0], [1.0, 0.0]] and expected[0, 1] == 100.0
    assert not paga.connectivity(np.array([[3]]), np.array([1]))[0].any()
    big = np.array([[0, 2 ** 61], [2 ** 61, 0]], dtype=np.int64)
    conn, expected = paga.connectivity(big, np.array([2 ** 30, 2 ** 30]))
    assert expected[0, 1] == float(2 * 2 ** 61 * 2 ** 30) / float(2 ** 31 - 1)
    assert conn[0, 1] == 1.0                                   # 2^62 / expected is about 2: clipped


def test_both_integer_paths_of_connectivity_agree():
    rng = np.random.default_rng(2)
    count = rng.integers(0, 1000, size=(7, 7))
    size = rng.integers(1, 50, size=7)
    small = paga.connectivity(count, size)
    es = count.sum(1)
    n = int(size.sum())
    for a in range(7):
        for b in range(7):
            if a == b:
                assert small[0][a, b] == 0 and small[1][a, b] == 0
                continue
            expected = float(int(es[a]) * int(size[b]) + int(es[b]) * int(size[a])) / float(n - 1)
            sym = int(count[a, b] + count[b, a])
            assert small[1][a, b] == expected
            assert small[0][a, b] == (min(1.0, sym / expected) if sym > 0 else 0.0)


def test_tree_with_a_tie():
    """4 groups: the pairs (0, 1) and (2, 3) tie at 0.5 and come first, (0, 1) before (2, 3); then (0, 2) and (1, 3)
    tie at 0.3 and only the first joins two trees; (1, 2) at 0.2 closes a cycle."""
    c = np.zeros((4, 4))
    for (a, b), v in {(0, 1): 0.5, (2, 3): 0.5, (0, 2): 0.3, (1, 3): 0.3, (1, 2): 0.2}.items():
        c[a, b] = c[b, a] = v
    t = paga.tree(c)
    want = np.zeros((4, 4))
    for (a, b), v in {(0, 1): 0.5, (2, 3): 0.5, (0, 2): 0.3}.items():
        want[a, b] = want[b, a] = v
    assert np.array_equal(t, want) and np.array_equal(t, t.T)
    # a forest: an isolated group stays alone; an empty matrix gives an empty forest
    c2 = np.zeros((5, 5))
    c2[:4, :4] = c
    assert np.array_equal(paga.tree(c2)[:4, :4], want) and not paga.tree(c2)[4].any()
    assert not paga.tree(np.zeros((3, 3))).any()


def test_group_start():
    assert paga.group_start(1).tolist() == [[0.0, 0.0]]
    p = paga.group_start(4)
    assert p.dtype == torch.float32 and tuple(p.shape) == (4, 2)
    assert torch.allclose(p, torch.tensor([[10.0, 0.0], [0.0, 10.0], [-10.0, 0.0], [0.0, -10.0]]), atol=1e-5)
    assert torch.allclose(paga.group_start(7).norm(dim=1), torch.full((7,), 10.0), atol=1e-5)
    with pytest.raises(ValueError, match="group_start: n_groups"):
        paga.group_start(0)


def test_layout_init_boxes_scale_and_seed():
    """Groups 0, 1, 2 on a line with 1 nearest to 0 and 2; group 3 has no neighbour; some rows have no group."""
    pos = torch.tensor([[0.0, 0.0], [4.0, 2.0], [6.0, -2.0], [-3.0, 5.0]])
    conn = torch.zeros(4, 4, dtype=torch.float64)
    for (a, b), v in {(0, 1): 0.3, (1, 2): 0.3, (0, 2): 0.1}.items():
        conn[a, b] = conn[b, a] = v
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 4, size=500)
    labels[[5, 17]] = -1
    labels[[40]] = 4
    out = paga.layout_init(labels, pos, conn, seed=9)
    assert out.dtype == torch.float32 and tuple(out.shape) == (500, 2)
    assert float(out.abs().max()) == 10.0
    assert torch.equal(out, paga.layout_init(torch.from_numpy(labels), pos, conn, seed=9)), "the same seed, the same bits"
    assert not torch.equal(out, paga.layout_init(labels, pos, conn, seed=10))
    assert out[[5, 17, 40]].abs().max() == 0, "a row without a group starts at the origin"
    # an isolated group sits on its position, which gives the scale
    alone = out[torch.from_numpy(labels == 3)].double()
    assert len(alone) > 50 and bool((alone == alone[0]).all())
    f = float(alone[0, 1]) / 5.0
    assert abs(float(alone[0, 0]) + 3.0 * f) <= 1e-5 and 0 < f
    # every row of a group lies inside its group's box: pos[a] -+ |pos[a] - pos[nb]| / 2, nb the strongest neighbour
    # (group 1 ties between 0 and 2: the smaller label)
    for a, nb in ((0, 1), (1, 0), (2, 1)):
        rows = out[torch.from_numpy(labels == a)].double() / f
        half = (pos[a] - pos[nb]).abs().double() / 2
        assert len(rows) > 50 and bool(((rows - pos[a].double()).abs() <= half + 1e-5).all()), a
        assert float((rows - pos[a].double()).abs().max()) > 0.8 * float(half.max()), "the rows fill their box"
    for bad, what in ((dict(positions=pos[:, :1]), "positions"), (dict(conn=conn[:3]), "conn"),
                      (dict(labels=labels.astype(np.float64)), "labels"), (dict(seed=-1), "seed")):
        with pytest.raises(ValueError, match="layout_init: " + what):
            paga.layout_init(**dict(dict(labels=labels, positions=pos, conn=conn, seed=0), **bad))


def test_knn_graph_keeps_padding_that_does_not_count():
    idx = torch.tensor([[1, 2], [0, -1], [1, 0]])
    g = paga.knn_graph(idx)
    assert g["indptr"].tolist() == [0, 2, 4, 6] and g["indptr"].dtype == torch.int64
    assert g["indices"].tolist() == [1, 2, 0, -1, 1, 0] and g["indices"].dtype == torch.int32
    assert g["weights"].tolist() == [1.0] * 6 and g["weights"].dtype == torch.float32
    res = paga.solve(paga.NumpyOps(g), [0, 1, 1])
    assert res["edge_count"].tolist() == [[0, 2], [2, 1]] and int(res["edge_count"].sum()) == 5
    with pytest.raises(ValueError, match="knn_graph"):
        paga.knn_graph(torch.zeros(3, 2))


def test_the_chain_of_blobs_is_a_path_on_the_numpy_backend():
    """With the true labels and the centres 4.0 apart the coarse graph is the path 0 - 1 - 2 - 3 exactly."""
    g, _, truth = chain(4.0)
    res = paga.solve(paga.NumpyOps(g), truth)
    conn = res["connectivities"].numpy()
    assert path_order(conn) == [0, 1, 2, 3]
    assert np.array_equal(res["connectivities_tree"].numpy() > 0, conn > 0)
    assert res["sizes"].tolist() == [80] * 4 and np.array_equal(res["edge_count"].numpy(), res["edge_count"].numpy().T)
    again = paga.solve(paga.NumpyOps(g), truth.to(torch.int32))
    assert all(torch.equal(res[k], again[k]) for k in res if isinstance(res[k], torch.Tensor))


def test_solve_refuses_too_many_groups_and_too_much_weight():
    g = {"indptr": torch.tensor([0, 1, 2]), "indices": torch.tensor([1, 0], dtype=torch.int32),
         "wq": torch.tensor([2 ** 61, 2 ** 61])}
    with pytest.raises(ValueError, match="2\\^62"):
        paga.solve(paga.NumpyOps(g), [0, 1])
    g["wq"] = torch.tensor([2 ** 60, 2 ** 60])
    assert paga.solve(paga.NumpyOps(g), [0, 1])["edge_weight"].tolist() == [[0, 2 ** 60], [2 ** 60, 0]]
    with pytest.raises(ValueError, match="limit of 1024"):
        paga.solve(paga.NumpyOps(g), [0, 1024])
    with pytest.raises(ValueError, match="limit of 1024"):
        paga.solve(paga.NumpyOps(g), [0, 1], n_groups=1025)
    with pytest.raises(ValueError, match="below n_groups"):
        paga.solve(paga.NumpyOps(g), [0, 2], n_groups=2)
    with pytest.raises(ValueError, match="one entry per row"):
        paga.solve(paga.NumpyOps(g), [0, 1, 1])
    big = {"indptr": torch.arange(1026), "indices": torch.zeros(1025, dtype=torch.int32), "weights": torch.ones(1025)}
    assert paga.solve(paga.NumpyOps(big), np.arange(1025) % 1024)["n_groups"] == 1024


def test_every_argument_check_raises_before_a_library_call(monkeypatch):
    m = cpu_model()[0]
    no_library(monkeypatch)
    g = {n: t for n, t in chain()[0].items() if n in ("indptr", "indices", "weights")}
    lab = np.zeros(320, dtype=np.int64)
    for call, name in ((m.paga, "paga"), (m.paga_init, "paga_init")):
        for bad in (None, {}, {"indptr": g["indptr"], "indices": g["indices"]}):
            with pytest.raises(ValueError, match=name + ": graph must be a dict"):
                call(bad, lab)
        for key, t in (("indptr", g["indptr"].to(torch.int32)), ("indices", g["indices"].to(torch.int64)),
                       ("weights", g["weights"].double())):
            with pytest.raises(ValueError, match=name + ": .*" + key):
                call(dict(g, **{key: t}), lab)
        ind = g["indices"].clone()
        ind[3] = -1
        with pytest.raises(ValueError, match="must lie in"):
            call(dict(g, indices=ind), lab)
        with pytest.raises(ValueError, match=name + ": labels must have one entry per row"):
            call(g, lab[:-1])
        with pytest.raises(ValueError, match=name + ": labels"):
            call(g, lab.astype(np.float32))
        with pytest.raises(ValueError, match=name + ": labels"):
            call(g, lab.reshape(4, 80))
        for G in (0, -1, 2.0, True):
            with pytest.raises(ValueError, match=name + ": n_groups"):
                call(g, lab, n_groups=G)
        with pytest.raises(ValueError, match=name + ": .*limit of 1024"):
            call(g, lab, n_groups=1025)
        with pytest.raises(ValueError, match=name + ": .*limit of 1024"):
            call(g, np.arange(320) * 4)
        with pytest.raises(ValueError, match=name + ": .*below n_groups"):
            call(g, lab + 2, n_groups=2)
        with pytest.raises(ValueError, match=name + ": .*device"):          # host memory is never handed to the library
            call(g, lab)
    for kw, what in ((dict(seed=-1), "seed"), (dict(seed=1.5), "seed"), (dict(threshold=-0.1), "threshold"),
                     (dict(threshold=float("nan")), "threshold"), (dict(n_epochs=-1), "n_epochs"),
                     (dict(n_negatives=0), "n_negatives"), (dict(a=1.0), "a and b")):
        with pytest.raises(ValueError, match="paga_init: " + what):
            m.paga_init(g, lab, **kw)


def test_the_script_refuses_paga_without_labels(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location(
        "factorize_scrnaseq_counts", os.path.join(ROOT, "bin", "factorize_scrnaseq_counts.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    np.save(tmp_path / "toy_counts.npy", np.ones((4, 3), dtype=np.int64))
    base = ["--counts", str(tmp_path / "toy_counts.npy")]
    for flags in (["--paga"], ["--umap", "--umap-init", "paga"], ["--paga", "--umap", "--spectral", "2"]):
        with pytest.raises(SystemExit) as err:
            cli.main(base + flags)
        assert err.value.code == 2
        assert "--paga needs --communities, --clusters or --labels" in capsys.readouterr().err
    args = cli.build_parser().parse_args(base + ["--communities", "--umap-init", "paga"])
    assert args.umap_init == "paga" and args.paga is False      # (main sets --paga behind the parser)
