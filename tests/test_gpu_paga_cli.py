"""GPU: bin/factorize_scrnaseq_counts.py --communities --paga --umap --umap-init paga (the script called in-process on
a toy matrix, three steps): the three PAGA files have the right shapes and hold the arrays of the method on the run's
graph and labels; the map starts from the PAGA start; the step run twice writes equal files.  (Training is not
bit-reproducible from run to run, so a run is held against its own model and the second run of the step is made on
that model.)"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    spec = importlib.util.spec_from_file_location(
        "factorize_scrnaseq_counts", os.path.join(ROOT, "bin", "factorize_scrnaseq_counts.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_paga_files_twice_and_the_map_from_their_start(tmp_path, capsys, monkeypatch):
    from spmf_amd import paga
    cli = _cli()
    rng = np.random.default_rng(4)
    N, D, P, G = 130, 30, 2, 3
    types = rng.integers(0, G, size=N)
    prog = rng.gamma(0.3, 1.0, size=(G, D)) * (rng.random((G, D)) < 0.3) * 6.0 + 0.2
    X = rng.poisson(prog[types] * rng.lognormal(0.0, 0.4, size=(N, 1))).astype(np.int64)
    np.save(tmp_path / "toy_counts.npy", X)
    base = ["--counts", str(tmp_path / "toy_counts.npy"), "-d", str(P), "-b", "64", "-e", "3", "--seed", "3",
            "--top", "4", "--cluster-seed", "7", "--cluster-draws", "4", "--umap-neighbors", "9", "--umap-epochs", "40"]
    files = [tmp_path / f"toy_paga_{what}_{P}.npy" for what in ("connectivities", "tree", "pos")]
    seen = {}
    inner, graphs = cli.paga_cells, cli._cell_graph

    def recorded(factor, graph, labels, n_groups, *paths_and_args):
        seen.update(factor=factor, graph=graph, labels=labels, n_groups=n_groups, rest=paths_and_args)
        seen["start"] = inner(factor, graph, labels, n_groups, *paths_and_args)
        return seen["start"]

    def counted(*a, **k):
        seen["graphs"] = seen.get("graphs", 0) + 1
        return graphs(*a, **k)
    monkeypatch.setattr(cli, "paga_cells", recorded)
    monkeypatch.setattr(cli, "_cell_graph", counted)
    cli.main(base + ["--communities", "--paga", "--umap", "--umap-init", "paga"])
    out = capsys.readouterr().out
    assert seen["graphs"] == 1, "the graph is built once"
    for tag in ("communities: ", "paga: ", "umap: "):
        assert len([ln for ln in out.splitlines() if ln.startswith(tag)]) == 1, out
    lab = np.load(tmp_path / f"toy_communities_{P}.npy")
    n_groups = int(lab.max()) + 1
    assert seen["n_groups"] == n_groups >= 1 and np.array_equal(seen["labels"].cpu().numpy(), lab)
    conn, tree, pos = (np.load(f) for f in files)
    assert conn.shape == tree.shape == (n_groups, n_groups) and conn.dtype == tree.dtype == np.float64
    assert pos.shape == (n_groups, 2) and pos.dtype == np.float32 and np.isfinite(pos).all()
    assert np.array_equal(conn, conn.T) and (conn >= 0).all() and (conn <= 1).all() and not np.diag(conn).any()
    assert ((tree == conn) | (tree == 0)).all() and np.array_equal(tree, paga.tree(conn))
    # the method on the run's graph and labels, and the numpy backend's bits
    factor, g = seen["factor"], seen["graph"]
    want = factor.paga(g, seen["labels"], n_groups=n_groups)
    assert np.array_equal(conn, want["connectivities"].cpu().numpy())
    host = paga.solve(paga.NumpyOps({n: g[n].cpu() for n in ("indptr", "indices", "weights")}), lab, n_groups=n_groups)
    assert np.array_equal(conn, host["connectivities"].numpy()) and np.array_equal(tree, host["connectivities_tree"].numpy())
    # the map is the layout of the same graph from the PAGA start
    y = np.load(tmp_path / f"toy_UMAP_{P}.npy")
    assert y.shape == (N, 2) and tuple(seen["start"].shape) == (N, 2)
    again = factor.graph_layout(g, init=seen["start"], n_epochs=40, min_dist=0.1, seed=7)["embedding"].cpu().numpy()
    assert np.array_equal(y.view(np.int32), again.view(np.int32))
    # the step a second time on the run's model: equal files
    second = [tmp_path / f"second_{i}.npy" for i in range(3)]
    start2 = inner(factor, g, seen["labels"], n_groups, *second, seen["rest"][-1])
    assert torch.equal(start2, seen["start"])
    for a, b in zip(files, second):
        assert open(a, "rb").read() == open(b, "rb").read(), a
    capsys.readouterr()
    # --clusters labels where there are no communities asked for; --umap-init paga alone implies --paga
    for f in files:
        os.remove(f)
    cli.main(base + ["--clusters", "3", "--umap", "--umap-init", "paga"])
    conn = np.load(files[0])
    assert conn.shape == (3, 3) and seen["n_groups"] == 3 and seen["labels"].dtype == torch.int32
    assert np.load(tmp_path / f"toy_UMAP_{P}.npy").shape == (N, 2)
