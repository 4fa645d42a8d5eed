"""GPU: bin/factorize_scrnaseq_counts.py --clusters G --silhouette: the per-cell file, whose values are the
method's on the encoding and the labels of the run (the script called in-process on a toy matrix, three steps), the
printed score, and the flag's refusal without --clusters or --labels."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_silhouette_flag_writes_the_per_cell_file_of_the_method(tmp_path, capsys, monkeypatch):
    spec = importlib.util.spec_from_file_location(
        "factorize_scrnaseq_counts", os.path.join(ROOT, "bin", "factorize_scrnaseq_counts.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    rng = np.random.default_rng(4)
    N, D, P, G = 130, 30, 2, 3
    types = rng.integers(0, G, size=N)
    prog = rng.gamma(0.3, 1.0, size=(G, D)) * (rng.random((G, D)) < 0.3) * 6.0 + 0.2
    X = rng.poisson(prog[types] * rng.lognormal(0.0, 0.4, size=(N, 1))).astype(np.int64)
    np.save(tmp_path / "toy_counts.npy", X)
    base = ["--counts", str(tmp_path / "toy_counts.npy"), "-d", str(P), "-b", "64", "-e", "3", "--seed", "3",
            "--top", "4", "--group-draws", "5", "--cluster-seed", "7", "--cluster-draws", "4"]
    with pytest.raises(SystemExit):
        cli.main(base + ["--silhouette"])                  # neither --clusters nor --labels
    capsys.readouterr()
    seen = {}
    inner = cli.silhouette_cells

    def recorded(factor, X_, labels, n_clusters, path, args):
        seen.update(factor=factor, X=X_, labels=labels, n_clusters=n_clusters, args=args)
        return inner(factor, X_, labels, n_clusters, path, args)
    monkeypatch.setattr(cli, "silhouette_cells", recorded)
    cli.main(base + ["--clusters", str(G), "--silhouette"])
    out = capsys.readouterr().out
    sil = np.load(tmp_path / f"toy_silhouette_{P}.npy")
    labels = np.load(tmp_path / f"toy_cluster_{P}.npy")
    assert sil.shape == (N,) and sil.dtype == np.float32
    assert seen["n_clusters"] == G and np.array_equal(seen["labels"].cpu().numpy(), labels)
    # the method on the same encoding: the seed of the draws, the draws, the labels of the run
    factor = seen["factor"]
    torch.manual_seed(7)
    emb = factor.embed({factor.count_key: seen["X"]}, nsamples=4)["mean"]
    want = factor.silhouette(emb, labels, G)
    np.testing.assert_array_equal(sil.view(np.int32), want["silhouette"].cpu().numpy().view(np.int32))
    line = [ln for ln in out.splitlines() if ln.startswith("silhouette: ")]
    means = ", ".join(f"{v:.3f}" for v in want["cluster_mean"].tolist())
    assert line == [f"silhouette: {want['score']:.4f} over {want['n_scored']} cells; per cluster {means}"], out
    scored = labels >= 0
    assert np.isfinite(sil[scored]).all() or int((np.bincount(labels[scored], minlength=G) > 0).sum()) < 2
    # with --labels alone the file's labels are scored
    given = types.copy()
    given[:5] = -1
    np.save(tmp_path / "toy_labels.npy", given)
    cli.main(base + ["--labels", str(tmp_path / "toy_labels.npy"), "--silhouette"])
    capsys.readouterr()
    sil = np.load(tmp_path / f"toy_silhouette_{P}.npy")
    assert seen["n_clusters"] is None and np.isnan(sil[:5]).all() and np.isfinite(sil[5:]).all()
    assert ((sil[5:] >= -1) & (sil[5:] <= 1)).all()
