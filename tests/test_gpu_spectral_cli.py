"""GPU: bin/factorize_scrnaseq_counts.py --spectral N and --umap-init {pca,spectral} (the script called in-process on
a toy matrix, three steps): the files of the stated shapes, whose bits are the methods' on the run's graph; --umap-init
pca writes the bits of the call --umap alone makes; the flags' own refusals."""
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


def test_spectral_files_and_the_spectral_start(tmp_path, capsys, monkeypatch):
    from spmf_amd import spectral
    cli = _cli()
    rng = np.random.default_rng(4)
    N, D, P, G = 130, 30, 2, 3
    types = rng.integers(0, G, size=N)
    prog = rng.gamma(0.3, 1.0, size=(G, D)) * (rng.random((G, D)) < 0.3) * 6.0 + 0.2
    X = rng.poisson(prog[types] * rng.lognormal(0.0, 0.4, size=(N, 1))).astype(np.int64)
    np.save(tmp_path / "toy_counts.npy", X)
    base = ["--counts", str(tmp_path / "toy_counts.npy"), "-d", str(P), "-b", "64", "-e", "3", "--seed", "3",
            "--top", "4", "--cluster-seed", "7", "--cluster-draws", "4", "--umap-neighbors", "9", "--umap-epochs", "40"]
    umap_file = tmp_path / f"toy_UMAP_{P}.npy"
    # --umap-init pca is --umap: the same arguments, and the file holds the bits of the call --umap has always made
    # (training is not bit-reproducible from run to run, so one run is held against its own model)
    parser = cli.build_parser()
    assert parser.parse_args(base + ["--umap"]) == parser.parse_args(base + ["--umap", "--umap-init", "pca"])
    seen = {}
    inner_umap = cli.umap_cells

    def recorded_umap(factor, X_run, path, args):
        seen.update(factor=factor, X=X_run)
        return inner_umap(factor, X_run, path, args)
    monkeypatch.setattr(cli, "umap_cells", recorded_umap)
    cli.main(base + ["--umap", "--umap-init", "pca"])
    monkeypatch.setattr(cli, "umap_cells", inner_umap)
    factor = seen["factor"]
    torch.manual_seed(7)
    want = factor.umap({factor.count_key: seen["X"]}, k=9, nsamples=4, n_epochs=40, min_dist=0.1, seed=7)
    plain = np.load(umap_file)
    np.testing.assert_array_equal(plain.view(np.int32), want["embedding"].cpu().numpy().view(np.int32))
    os.remove(umap_file)
    assert not os.path.exists(tmp_path / f"toy_spectral_{P}.npy")
    capsys.readouterr()
    # --spectral 3 and the spectral start, with the run's model and counts recorded
    seen = {}
    inner = cli.spectral_cells

    def recorded(factor, X_run, path, values_path, args):
        seen.update(factor=factor, X=X_run)
        return inner(factor, X_run, path, values_path, args)
    monkeypatch.setattr(cli, "spectral_cells", recorded)
    cli.main(base + ["--umap", "--umap-init", "spectral", "--spectral", "3"])
    out = capsys.readouterr().out
    vec = np.load(tmp_path / f"toy_spectral_{P}.npy")
    val = np.load(tmp_path / f"toy_spectral_values_{P}.npy")
    y = np.load(umap_file)
    assert vec.shape == (N, 3) and vec.dtype == np.float32 and np.isfinite(vec).all()
    assert val.shape == (4,) and val.dtype == np.float64 and (np.diff(val) <= 0).all() and abs(val[0] - 1.0) <= 1e-4
    assert y.shape == (N, 2) and y.dtype == np.float32 and np.isfinite(y).all()
    assert len([ln for ln in out.splitlines() if ln.startswith("spectral: 3 eigenvectors")]) == 1, out
    assert len([ln for ln in out.splitlines() if ln.startswith("umap: spectral start")]) == 1, out
    # the methods on the same graph: the seed of the draws, the flags' values
    factor = seen["factor"]
    torch.manual_seed(7)
    emb = factor.embed({factor.count_key: seen["X"]}, nsamples=4)["mean"]
    nn = factor.knn(emb, k=9)
    g = factor.fuzzy_graph(nn["indices"], nn["distances"])
    want = factor.spectral(g, n_components=3, seed=7)
    np.testing.assert_array_equal(vec.view(np.int32), want["embedding"].cpu().numpy().view(np.int32))
    np.testing.assert_array_equal(val, want["values"])
    start = spectral.layout_init(factor.spectral(g, n_components=2, seed=7)["embedding"], seed=7)
    lay = factor.graph_layout(g, init=start, n_epochs=40, seed=7)["embedding"]
    np.testing.assert_array_equal(y.view(np.int32), lay.cpu().numpy().view(np.int32))
    # the flag's range
    for bad in ("0", "13"):
        with pytest.raises(SystemExit):
            cli.main(base + ["--spectral", bad])
    with pytest.raises(SystemExit):
        cli.main(base + ["--umap", "--umap-init", "random"])
