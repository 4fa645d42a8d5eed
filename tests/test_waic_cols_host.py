"""CPU-side tests of the per-column WAIC (waic_streaming(col_scores=True), spmf_waic_accumulate_cols):
spmf_amd.waic.combine_columns against numpy on synthetic per-cell values, and the declarations -- the entry in the
header, the export list and the binding, the keyword on the three classes, the two flags of the scRNA script.
The valid call is tests/test_gpu_waic_cols.py's."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from _stream_cases import assert_declared_exported_bound, library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _synthetic(seed=11, B=300, D=12):
    """Per-cell lppd, pwaic [B,D] fp64 and the mask of counted cells: column 0 has one counted cell, column 1
    none, columns 2 and 3 lose a few cells, the rest are whole."""
    rng = np.random.default_rng(seed)
    lp = -rng.gamma(2.0, 1.5, size=(B, D))
    pw = rng.gamma(1.5, 0.05, size=(B, D))
    ok = np.ones((B, D), dtype=bool)
    ok[:, 0] = False
    ok[17, 0] = True
    ok[:, 1] = False
    ok[rng.random(B) < 0.1, 2] = False
    ok[5, 3] = False
    return lp, pw, ok


def _sums(lp, pw, ok):
    e = lp - pw
    return np.stack([ok.sum(0).astype(np.float64), np.where(ok, lp, 0.0).sum(0), np.where(ok, pw, 0.0).sum(0),
                     np.where(ok, e * e, 0.0).sum(0), (~ok).sum(0).astype(np.float64)], axis=1)


def test_combine_columns_matches_numpy():
    from spmf_amd import waic as W
    lp, pw, ok = _synthetic()
    B, D = lp.shape
    sums = _sums(lp, pw, ok)
    out = W.combine_columns(torch.as_tensor(sums))
    assert set(out) == {"col_n", "col_n_excluded", "col_lppd", "col_pwaic", "col_waic", "col_se"}
    for k, v in out.items():
        assert tuple(v.shape) == (D,) and v.device.type == "cpu", k
        assert v.dtype == (torch.int64 if k in ("col_n", "col_n_excluded") else torch.float64), k
    np.testing.assert_array_equal(out["col_n"].numpy(), ok.sum(0))
    np.testing.assert_array_equal(out["col_n_excluded"].numpy(), (~ok).sum(0))
    assert out["col_n"].tolist()[:2] == [1, 0] and ((out["col_n"] + out["col_n_excluded"]) == B).all()
    e = lp - pw
    want_waic = np.array([-2.0 * e[ok[:, d], d].sum() for d in range(D)])
    np.testing.assert_allclose(out["col_lppd"].numpy(), sums[:, 1], rtol=0, atol=0)
    np.testing.assert_allclose(out["col_pwaic"].numpy(), sums[:, 2], rtol=0, atol=0)
    np.testing.assert_allclose(out["col_waic"].numpy(), want_waic, rtol=1e-12, atol=0)
    assert out["col_waic"][1] == 0.0
    se = out["col_se"].numpy()
    assert np.isnan(se[0]) and np.isnan(se[1]), "n = 1 and n = 0 have no deviation"
    for d in range(2, D):
        col = e[ok[:, d], d]
        n = col.size
        # the cancellation in sum e^2 - (sum e)^2 / n costs about 2^-52 n mean^2 / var: far inside 1e-9 here
        assert col.var(ddof=1) >= 1e-4 * col.mean() ** 2, d
        np.testing.assert_allclose(se[d], 2.0 * np.sqrt(n * col.var(ddof=1)), rtol=1e-9, err_msg=str(d))
        # and it is combine()'s number for the column's own sums
        assert abs(se[d] - W.combine(np.concatenate([sums[d], [0.0]]))["se"]) <= 1e-12 * se[d], d


def test_combine_columns_refuses_other_shapes_and_takes_numpy():
    from spmf_amd import waic as W
    lp, pw, ok = _synthetic(seed=12, B=40, D=5)
    sums = _sums(lp, pw, ok)
    a, b = W.combine_columns(sums), W.combine_columns(torch.as_tensor(sums))
    for k in a:
        assert torch.equal(a[k].nan_to_num(-1.0), b[k].nan_to_num(-1.0)), k
    for bad in (np.zeros(5), np.zeros((4, 6)), np.zeros((2, 3, 5))):
        with pytest.raises(ValueError, match="column sums"):
            W.combine_columns(bad)
    added = W.combine_columns(torch.as_tensor(sums + sums))       # two batches add
    assert added["col_n"].tolist() == (2 * a["col_n"]).tolist()
    np.testing.assert_allclose(added["col_waic"].numpy(), 2.0 * a["col_waic"].numpy(), rtol=1e-15)


def test_entry_point_is_declared_exported_and_bound():
    assert_declared_exported_bound("spmf_waic_accumulate_cols", 11)
    assert_declared_exported_bound("spmf_waic_accumulate", 10)
    hdr = open(os.path.join(ROOT, "include", "spmf_hip.h")).read()
    assert "sum_d col_out[d][j]" in hdr and "[D][5]" in hdr


def test_library_exports_the_entry():
    from spmf_amd import _lib
    lib = library()
    assert callable(lib.spmf_waic_accumulate_cols) and callable(lib.spmf_waic_accumulate)
    assert lib.spmf_version() == 6
    assert lib.spmf_waic_accumulate_cols(None, None, 2, _lib.PtrArray(), None, None, None, None, None, 0, None) == -1


def test_col_scores_is_a_keyword_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        p = inspect.signature(cls.waic_streaming).parameters
        assert "col_scores" in p and p["col_scores"].default is False, cls.__name__
        assert list(p)[:6] == ["self", "data", "nsamples", "draws", "row_scores", "max_rows"], cls.__name__


def test_cli_flags_parse():
    spec = importlib.util.spec_from_file_location(
        "factorize_scrnaseq_counts", os.path.join(ROOT, "bin", "factorize_scrnaseq_counts.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    p = cli.build_parser()
    a = p.parse_args(["--counts", "x_counts.npy"])
    assert a.gene_waic is False and a.waic_draws == 32
    a = p.parse_args(["--counts", "x_counts.npy", "--gene-waic", "--waic-draws", "7"])
    assert a.gene_waic is True and a.waic_draws == 7
    with pytest.raises(SystemExit):
        p.parse_args(["--counts", "x_counts.npy", "--waic-draws", "1"])
    assert callable(cli.gene_waic)
