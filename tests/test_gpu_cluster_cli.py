"""GPU: bin/factorize_scrnaseq_counts.py --clusters: the label and centroid files, the group table written from
these labels when no --labels file is given, the file winning when one is, and the same seed giving the same
files (the script called in-process on a toy matrix, three steps).  The fit behind a run adds its gradients with
float atomics (tests/test_gpu_groups_cli.py), so two runs of the script do not share the bits of their encodings:
the same-seed comparison is made where the flag's own work starts, on the fitted model of one run."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clusters_write_labels_and_centroids_and_feed_the_group_table(tmp_path, capsys, monkeypatch):
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
    argv = ["--counts", str(tmp_path / "toy_counts.npy"), "-d", str(P), "-b", "64", "-e", "3", "--seed", "3",
            "--top", "4", "--group-draws", "5", "--clusters", str(G), "--cluster-seed", "7", "--cluster-draws", "4"]
    seen = {}
    inner = cli.cluster_cells

    def recorded(factor, X_, labels_path, centroid_path, args):
        seen.update(factor=factor, X=X_, args=args)
        return inner(factor, X_, labels_path, centroid_path, args)
    monkeypatch.setattr(cli, "cluster_cells", recorded)
    cli.main(argv)
    out = capsys.readouterr().out
    labels = np.load(tmp_path / f"toy_cluster_{P}.npy")
    cent = np.load(tmp_path / f"toy_centroid_{P}.npy")
    assert labels.shape == (N,) and labels.dtype == np.int32 and ((labels >= 0) & (labels < G)).all()
    assert cent.shape == (G, P) and cent.dtype == np.float32 and np.isfinite(cent).all()
    count = np.bincount(labels, minlength=G)
    line = [ln for ln in out.splitlines() if ln.startswith("clusters: ")]
    assert len(line) == 1 and line[0].endswith("cells " + ", ".join(str(n) for n in count)), out
    # without --labels the table is written from these labels
    table = [ln for ln in out.splitlines() if ln.startswith("group ")]
    filled = [g for g in range(G) if count[g] > 0]
    assert len(table) == len(filled) and len(filled) >= 2, out
    for ln, g in zip(table, filled):
        assert ln.startswith(f"group {g} ({count[g]} cells): "), ln
    gm = np.load(tmp_path / f"toy_groupmean_{P}.npy")
    assert gm.shape == (G, D) and gm.dtype == np.float64
    # the same seed gives the same files: the flag's work again on the fitted model of this run
    inner(seen["factor"], seen["X"], str(tmp_path / "again_cluster.npy"), str(tmp_path / "again_centroid.npy"),
          seen["args"])
    capsys.readouterr()
    assert (tmp_path / "again_cluster.npy").read_bytes() == (tmp_path / f"toy_cluster_{P}.npy").read_bytes()
    assert (tmp_path / "again_centroid.npy").read_bytes() == (tmp_path / f"toy_centroid_{P}.npy").read_bytes()
    # with --labels the file wins for the table
    given = types.copy()
    given[:5] = -1
    np.save(tmp_path / "toy_labels.npy", given)
    cli.main(argv + ["--labels", str(tmp_path / "toy_labels.npy")])
    out = capsys.readouterr().out
    table = [ln for ln in out.splitlines() if ln.startswith("group ")]
    want = np.bincount(given[given >= 0], minlength=G)
    assert len(table) == G and all(table[g].startswith(f"group {g} ({want[g]} cells): ") for g in range(G)), out
    assert np.load(tmp_path / f"toy_cluster_{P}.npy").shape == (N,)
