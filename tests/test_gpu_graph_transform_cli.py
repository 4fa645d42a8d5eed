"""GPU: bin/factorize_scrnaseq_counts.py --umap --clusters G --map-counts FILE: the coordinates of the new cells and
their voted labels as files, whose bits are the method's on the map of the run (the script called in-process on a toy
matrix, three steps), the printed line, and the flag's own refusals."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_map_counts_writes_the_new_cells_on_the_map(tmp_path, capsys, monkeypatch):
    spec = importlib.util.spec_from_file_location(
        "factorize_scrnaseq_counts", os.path.join(ROOT, "bin", "factorize_scrnaseq_counts.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    rng = np.random.default_rng(4)
    N, N_new, D, P, G = 130, 23, 30, 2, 3
    types = rng.integers(0, G, size=N + N_new)
    prog = rng.gamma(0.3, 1.0, size=(G, D)) * (rng.random((G, D)) < 0.3) * 6.0 + 0.2
    X = rng.poisson(prog[types] * rng.lognormal(0.0, 0.4, size=(N + N_new, 1))).astype(np.int64)
    np.save(tmp_path / "toy_counts.npy", X[:N])
    np.save(tmp_path / "new_counts.npy", X[N:])
    base = ["--counts", str(tmp_path / "toy_counts.npy"), "-d", str(P), "-b", "64", "-e", "3", "--seed", "3",
            "--top", "4", "--cluster-seed", "7", "--cluster-draws", "4", "--umap", "--umap-neighbors", "9",
            "--umap-epochs", "40"]
    seen = {}
    inner = cli.map_cells

    def recorded(factor, X_new, reference, labels, n_classes, path, label_path, args):
        seen.update(factor=factor, X=X_new, reference=reference, labels=labels, n_classes=n_classes)
        return inner(factor, X_new, reference, labels, n_classes, path, label_path, args)
    monkeypatch.setattr(cli, "map_cells", recorded)
    cli.main(base + ["--clusters", str(G), "--map-counts", str(tmp_path / "new_counts.npy")])
    out = capsys.readouterr().out
    y = np.load(tmp_path / f"toy_UMAP_map_{P}.npy")
    lab = np.load(tmp_path / f"toy_label_map_{P}.npy")
    assert y.shape == (N_new, 2) and y.dtype == np.float32 and np.isfinite(y).all()
    assert lab.shape == (N_new,) and lab.dtype == np.int64 and lab.min() >= 0 and lab.max() < G
    # the map itself is the file of --umap, and the clusters are the voters
    ref = np.load(tmp_path / f"toy_UMAP_{P}.npy")
    np.testing.assert_array_equal(ref.view(np.int32), seen["reference"]["embedding"].cpu().numpy().view(np.int32))
    np.testing.assert_array_equal(np.load(tmp_path / f"toy_cluster_{P}.npy"), seen["labels"].cpu().numpy())
    assert seen["n_classes"] == G
    # the method on the same map: the seed of the draws, the flags' values
    factor = seen["factor"]
    torch.manual_seed(7)
    want = factor.umap_transform({factor.count_key: seen["X"]}, seen["reference"], k=9, nsamples=4,
                                 labels=seen["labels"], n_classes=G, seed=7)
    np.testing.assert_array_equal(y.view(np.int32), want["embedding"].cpu().numpy().view(np.int32))
    np.testing.assert_array_equal(lab, want["labels"].cpu().numpy())
    line = [ln for ln in out.splitlines() if ln.startswith("umap map: ")]
    assert len(line) == 1 and f"{N_new} new cells on {N}" in line[0] and "100 epochs" in line[0], out
    assert f"{N_new} labelled" in line[0]
    # without labels: the coordinates alone
    os.remove(tmp_path / f"toy_label_map_{P}.npy")
    cli.main(base + ["--map-counts", str(tmp_path / "new_counts.npy")])
    assert np.load(tmp_path / f"toy_UMAP_map_{P}.npy").shape == (N_new, 2)
    assert not os.path.exists(tmp_path / f"toy_label_map_{P}.npy")
    # the flag needs --umap, an existing file and the genes of --counts
    with pytest.raises(SystemExit):
        cli.main([a for a in base if a != "--umap"] + ["--map-counts", str(tmp_path / "new_counts.npy")])
    with pytest.raises(SystemExit):
        cli.main(base + ["--map-counts", str(tmp_path / "missing.npy")])
    np.save(tmp_path / "narrow_counts.npy", X[N:, :D - 1])
    with pytest.raises(SystemExit):
        cli.main(base + ["--map-counts", str(tmp_path / "narrow_counts.npy")])
