"""GPU: bin/factorize_scrnaseq_counts.py --umap: the coordinate file, whose bits are the method's on the encoding of
the run (the script called in-process on a toy matrix, three steps), and the printed line."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_umap_flag_writes_the_coordinates_of_the_method(tmp_path, capsys, monkeypatch):
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
            "--top", "4", "--cluster-seed", "7", "--cluster-draws", "4"]
    seen = {}
    inner = cli.umap_cells

    def recorded(factor, X_, path, args):
        seen.update(factor=factor, X=X_, args=args)
        return inner(factor, X_, path, args)
    monkeypatch.setattr(cli, "umap_cells", recorded)
    cli.main(base + ["--umap", "--umap-neighbors", "9", "--umap-min-dist", "0.25", "--umap-epochs", "40"])
    out = capsys.readouterr().out
    y = np.load(tmp_path / f"toy_UMAP_{P}.npy")
    assert y.shape == (N, 2) and y.dtype == np.float32 and np.isfinite(y).all()
    # the method on the same encoding: the seed of the draws, the draws, the flags' values
    factor = seen["factor"]
    torch.manual_seed(7)
    want = factor.umap({factor.count_key: seen["X"]}, k=9, nsamples=4, n_epochs=40, min_dist=0.25, seed=7)
    np.testing.assert_array_equal(y.view(np.int32), want["embedding"].cpu().numpy().view(np.int32))
    # ... which is the encoding --clusters labels
    torch.manual_seed(7)
    emb = factor.embed({factor.count_key: seen["X"]}, nsamples=4)["mean"]
    assert torch.equal(emb.view(torch.int32), want["latent"].view(torch.int32))
    line = [ln for ln in out.splitlines() if ln.startswith("umap: ")]
    assert len(line) == 1 and f"{N} cells" in line[0] and "40 epochs" in line[0], out
    assert f"{int(want['graph']['indices'].numel())} graph entries" in line[0]
    # the defaults: 15 neighbours, min_dist 0.1, 500 epochs at this size
    cli.main(base + ["--umap"])
    out = capsys.readouterr().out
    assert "500 epochs" in out and "a = 1.5769" in out
    assert np.load(tmp_path / f"toy_UMAP_{P}.npy").shape == (N, 2)
