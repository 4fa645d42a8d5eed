"""GPU: bin/factorize_scrnaseq_counts.py --communities with --resolution R (the script called in-process on a toy
matrix, three steps): the file holds one label per cell, the bits of the method on the run's graph and of the numpy
backend; the step run twice writes equal files; --silhouette takes the labels; with --umap the graph is built once;
the flags' own refusals.  (Training is not bit-reproducible from run to run, so a run is held against its own model
and the second run of the step is made on that model.)"""
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


def test_communities_file_twice_and_the_graph_once(tmp_path, capsys, monkeypatch):
    from spmf_amd import communities
    cli = _cli()
    rng = np.random.default_rng(4)
    N, D, P, G = 130, 30, 2, 3
    types = rng.integers(0, G, size=N)
    prog = rng.gamma(0.3, 1.0, size=(G, D)) * (rng.random((G, D)) < 0.3) * 6.0 + 0.2
    X = rng.poisson(prog[types] * rng.lognormal(0.0, 0.4, size=(N, 1))).astype(np.int64)
    np.save(tmp_path / "toy_counts.npy", X)
    base = ["--counts", str(tmp_path / "toy_counts.npy"), "-d", str(P), "-b", "64", "-e", "3", "--seed", "3",
            "--top", "4", "--cluster-seed", "7", "--cluster-draws", "4", "--umap-neighbors", "9", "--umap-epochs", "40"]
    path = tmp_path / f"toy_communities_{P}.npy"
    seen = {}
    inner = cli.community_cells

    def recorded(factor, X_run, graph, out_path, args):
        seen.update(factor=factor, X=X_run, graph=graph, args=args)
        return inner(factor, X_run, graph, out_path, args)
    monkeypatch.setattr(cli, "community_cells", recorded)
    cli.main(base + ["--communities", "--silhouette"])
    out = capsys.readouterr().out
    lab = np.load(path)
    assert lab.shape == (N,) and lab.dtype == np.int64 and lab.min() >= -1
    assert seen["graph"] is None and not os.path.exists(tmp_path / f"toy_UMAP_{P}.npy")
    assert len([ln for ln in out.splitlines() if ln.startswith("communities: ")]) == 1, out
    assert len([ln for ln in out.splitlines() if ln.startswith("silhouette: ")]) == 1, out
    # the method on the same graph: the seed of the draws, the flags' values; and the numpy backend's bits
    factor = seen["factor"]
    torch.manual_seed(7)
    emb = factor.embed({factor.count_key: seen["X"]}, nsamples=4)["mean"]
    nn = factor.knn(emb, k=9)
    g = factor.fuzzy_graph(nn["indices"], nn["distances"])
    want = factor.communities(g)
    np.testing.assert_array_equal(lab, want["labels"].cpu().numpy())
    host = communities.solve(communities.NumpyOps({n: g[n].cpu() for n in ("indptr", "indices", "weights")}))
    np.testing.assert_array_equal(lab, host["labels"].numpy())
    assert np.array_equal(np.bincount(lab[lab >= 0]), want["sizes"].cpu().numpy()) and want["n_communities"] >= 1
    # the labels are what --silhouette scored
    sil = factor.silhouette(emb, want["labels"], want["n_communities"])["silhouette"].cpu().numpy()
    np.testing.assert_array_equal(np.load(tmp_path / f"toy_silhouette_{P}.npy").view(np.int32), sil.view(np.int32))
    # the step a second time on the run's model: an equal file
    second = tmp_path / "second.npy"
    inner(factor, seen["X"], None, second, seen["args"])
    assert open(path, "rb").read() == open(second, "rb").read()
    capsys.readouterr()
    # with --umap the graph is the layout's: built once, clustered at the flag's resolution
    os.remove(path)

    def never(*a, **k):
        raise AssertionError("the graph was built a second time")
    monkeypatch.setattr(cli, "_cell_graph", never)
    cli.main(base + ["--umap", "--communities", "--resolution", "2.5"])
    out = capsys.readouterr().out
    assert len([ln for ln in out.splitlines() if ln.startswith("umap: ")]) == 1, out
    y = np.load(tmp_path / f"toy_UMAP_{P}.npy")
    assert y.shape == (N, 2) and seen["graph"] is not None and seen["args"].resolution == 2.5
    want = seen["factor"].communities(seen["graph"], resolution=2.5)
    np.testing.assert_array_equal(np.load(path), want["labels"].cpu().numpy())
    # the flags' refusals
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            cli.main(base + ["--communities", "--resolution", bad])
    with pytest.raises(SystemExit):
        cli.main(base + ["--silhouette"])
