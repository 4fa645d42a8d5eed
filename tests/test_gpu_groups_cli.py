"""GPU: bin/factorize_scrnaseq_counts.py --labels: the group-mean file and the marker table, and without the flag
the same output as with it up to the table (the script called in-process on a toy matrix, three steps).  The fit
behind both runs adds its gradients with float atomics (it is not the deterministic mode), so the numbers printed
by two runs may differ in their last digits and a near-tie between two genes may swap: every line that is not
part of the table is compared with its numbers masked, and the decoding matrix of both runs to 2e-3, the
comparison test_gpu_driver.test_scrnaseq_cli_end_to_end makes between two runs."""
import importlib.util
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_labels_add_the_group_means_and_the_marker_table(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location(
        "factorize_scrnaseq_counts", os.path.join(ROOT, "bin", "factorize_scrnaseq_counts.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    rng = np.random.default_rng(4)
    N, D, P, G = 130, 30, 2, 3
    types = rng.integers(0, G, size=N)
    prog = rng.gamma(0.3, 1.0, size=(G, D)) * (rng.random((G, D)) < 0.3) * 6.0 + 0.2
    X = rng.poisson(prog[types] * rng.lognormal(0.0, 0.4, size=(N, 1))).astype(np.int64)
    labels = types.copy()
    labels[:5] = -1
    np.save(tmp_path / "toy_counts.npy", X)
    np.save(tmp_path / "toy_labels.npy", labels)
    argv = ["--counts", str(tmp_path / "toy_counts.npy"), "-d", str(P), "-b", "64", "-e", "3", "--seed", "3",
            "--top", "4", "--group-draws", "5"]
    names = ("U", "V", "W", "Z", "cellscore", "genescore", "interceptscore")
    cli.main(argv)
    plain = capsys.readouterr().out
    files = {n: np.load(tmp_path / f"toy_{n}_{P}.npy") for n in names}
    assert "group " not in plain and not (tmp_path / f"toy_groupmean_{P}.npy").exists()
    cli.main(argv + ["--labels", str(tmp_path / "toy_labels.npy")])
    out = capsys.readouterr().out
    table = [ln for ln in out.splitlines() if ln.startswith("group ")]
    assert len(table) == G and all(ln.count("g") >= 4 and "+-" in ln for ln in table), out
    count = np.bincount(labels[labels >= 0], minlength=G)
    for g in range(G):
        assert table[g].startswith(f"group {g} ({count[g]} cells): "), table[g]
    def masked(text):
        return [re.sub(r"[-+]?\d[\d.]*(e[-+]?\d+)?", "#", ln) for ln in text.splitlines()
                if not ln.startswith("group ")]
    rest = [ln for ln in out.splitlines() if not ln.startswith("group ")]
    assert rest[:2] == plain.splitlines()[:2] and masked(out) == masked(plain)
    assert out.splitlines()[len(rest):] == table, "the table comes last"
    for n in names:
        assert np.load(tmp_path / f"toy_{n}_{P}.npy").shape == files[n].shape, n
    np.testing.assert_allclose(np.load(tmp_path / f"toy_V_{P}.npy"), files["V"], rtol=2e-3, atol=1e-6)
    gm = np.load(tmp_path / f"toy_groupmean_{P}.npy")
    assert gm.shape == (G, D) and gm.dtype == np.float64 and np.isfinite(gm).all()
