"""GPU: bin/factorize_scrnaseq_counts.py --gene-sets: the two score files of a two-set GMT on a toy matrix (the
script called in-process, three steps), and their values: the script's own scoring step is watched for the model
it scores and the state of the random generator in front of its draws, and ``set_scores`` from that state on
that model returns the files' numbers bit for bit."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gene_sets_add_the_two_score_files(tmp_path, capsys):
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
    (tmp_path / "toy.gmt").write_text("FIRST\ta duplicate and an unknown gene\tg3\tg0\tg3\tg77\tg29\n"
                                      "SECOND\tna\t" + "\t".join(f"g{j}" for j in range(5, 25)) + "\n")
    seen = {}
    scoring = cli.gene_set_scores

    def watched(factor, data, *rest):
        seen["factor"], seen["data"] = factor, data
        seen["cpu"], seen["cuda"] = torch.get_rng_state(), torch.cuda.get_rng_state(factor.device)
        return scoring(factor, data, *rest)
    cli.gene_set_scores = watched
    cli.main(["--counts", str(tmp_path / "toy_counts.npy"), "-d", str(P), "-b", "64", "-e", "3", "--seed", "3",
              "--top", "4", "--gene-sets", str(tmp_path / "toy.gmt"), "--set-draws", "5"])
    out = capsys.readouterr().out
    assert "gene sets: 2 sets, 24 members, 1 unknown members dropped" in out, out
    mean = np.load(tmp_path / f"toy_setscore_{P}.npy")
    sd = np.load(tmp_path / f"toy_setscore_sd_{P}.npy")
    for a in (mean, sd):
        assert a.shape == (N, 2) and a.dtype == np.float64 and np.isfinite(a).all()
    assert (mean > 0).all() and (sd > 0).all()
    assert not (tmp_path / f"toy_groupmean_{P}.npy").exists()
    factor = seen["factor"]
    torch.set_rng_state(seen["cpu"])
    torch.cuda.set_rng_state(seen["cuda"], factor.device)
    ref = factor.set_scores({factor.count_key: seen["data"]}, [[3, 0, 3, 29], list(range(5, 25))], nsamples=5,
                            sd=True)
    np.testing.assert_array_equal(ref["mean"].cpu().numpy(), mean)
    np.testing.assert_array_equal(ref["sd"].cpu().numpy(), sd)
    assert ref["sizes"].cpu().tolist() == [4, 20]
