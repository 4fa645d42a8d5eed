"""GPU: bin/factorize_scrnaseq_counts.py --pseudotime ROOT (the script called in-process on a toy matrix, three steps):
the file has the documented shape and holds the values of ``model.pseudotime`` on the run's model; with --communities
--paga the groups' means are written too and the neighbours are found once; the step run twice writes equal files.
(Training is not bit-reproducible from run to run, so a run is held against its own model.)"""
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


def test_pseudotime_file_is_the_methods_values(tmp_path, capsys, monkeypatch):
    cli = _cli()
    rng = np.random.default_rng(4)
    N, D, P, G, root = 130, 30, 2, 3, 17
    types = rng.integers(0, G, size=N)
    prog = rng.gamma(0.3, 1.0, size=(G, D)) * (rng.random((G, D)) < 0.3) * 6.0 + 0.2
    X = rng.poisson(prog[types] * rng.lognormal(0.0, 0.4, size=(N, 1))).astype(np.int64)
    np.save(tmp_path / "toy_counts.npy", X)
    base = ["--counts", str(tmp_path / "toy_counts.npy"), "-d", str(P), "-b", "64", "-e", "3", "--seed", "3",
            "--top", "4", "--cluster-seed", "7", "--cluster-draws", "4", "--umap-neighbors", "9", "--umap-epochs", "40"]
    seen = {}
    inner, graphs = cli.pseudotime_cells, cli._cell_graph

    def recorded(factor, nn, *rest):
        seen.update(factor=factor, nn=nn, rest=rest)
        seen["t"] = inner(factor, nn, *rest)
        return seen["t"]

    def counted(*a, **k):
        seen["graphs"] = seen.get("graphs", 0) + 1
        return graphs(*a, **k)
    monkeypatch.setattr(cli, "pseudotime_cells", recorded)
    monkeypatch.setattr(cli, "_cell_graph", counted)
    cli.main(base + ["--pseudotime", str(root)])
    out = capsys.readouterr().out
    assert seen["graphs"] == 1 and len([ln for ln in out.splitlines() if ln.startswith("pseudotime: root 17")]) == 1
    path = tmp_path / f"toy_pseudotime_{P}.npy"
    t = np.load(path)
    assert t.shape == (N,) and t.dtype == np.float32 and t[root] == 0.0
    ok = np.isfinite(t)
    assert ok.sum() > N // 2 and t[ok].min() == 0.0 and t[ok].max() == 1.0
    assert not os.path.exists(tmp_path / f"toy_paga_pseudotime_{P}.npy")
    # the method on the run's model: the same seed, the same draws
    factor = seen["factor"]
    torch.manual_seed(7)
    want = factor.pseudotime({factor.count_key: X}, root, k=9, nsamples=4)
    assert np.array_equal(t.view(np.int32), want["pseudotime"].cpu().numpy().view(np.int32))
    assert torch.equal(want["indices"], seen["nn"]["indices"])
    # the step a second time on the run's model: an equal file
    second = tmp_path / "second.npy"
    inner(factor, seen["nn"], root, str(second))
    assert open(path, "rb").read() == open(second, "rb").read()
    capsys.readouterr()
    # with --communities --paga and --umap: the neighbours are found once, and the groups' means are written
    seen.pop("graphs")
    cli.main(base + ["--communities", "--paga", "--umap", "--umap-init", "paga", "--pseudotime", str(root)])
    assert seen["graphs"] == 1, "the graph is built once"
    lab = np.load(tmp_path / f"toy_communities_{P}.npy")
    t = np.load(path)
    means = np.load(tmp_path / f"toy_paga_pseudotime_{P}.npy")
    n_groups = int(lab.max()) + 1
    assert means.shape == (n_groups,) and means.dtype == np.float64
    for a in range(n_groups):
        sel = (lab == a) & np.isfinite(t)
        assert means[a] == t[sel].astype(np.float64).mean() if sel.any() else np.isnan(means[a])
    # beside a layout from the encoding's axes the layout's own neighbours are used: no graph beside it
    seen.pop("graphs")
    cli.main(base + ["--umap", "--pseudotime", str(root)])
    assert "graphs" not in seen and np.load(path).shape == (N,)
    # refusals
    for bad, code in ((["--pseudotime", "-1"], 2),):
        with pytest.raises(SystemExit) as err:
            cli.main(base + bad)
        assert err.value.code == code
    with pytest.raises(SystemExit, match="--pseudotime must be one of the 130 cells"):
        cli.main(base + ["--pseudotime", "130"])
