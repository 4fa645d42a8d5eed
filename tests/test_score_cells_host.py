"""CPU-side tests of score_cells: the two entry points in the header, the export list and the
binding, the method on the class surface, the argument checks that need no device and the
summary of spmf_amd.heldout."""
import fnmatch
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spmf_cells_scratch_bytes", "spmf_score_cells")


def _header_args(hdr, name):
    """Number of arguments of the declaration of `name` in the header."""
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/spmf_hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_entry_points_are_declared_exported_and_bound():
    from spmf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spmf_hip.h")).read(), flags=re.S)
    exports = open(os.path.join(ROOT, "spmf_amd", "csrc", "exports.map")).read()
    exports = re.sub(r"/\*.*?\*/", "", exports, flags=re.S)
    globs = re.search(r"global:\s*([^}]*?)local:", exports, re.S).group(1)
    patterns = [p.strip() for p in globs.split(";") if p.strip()]
    for name in NAMES:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == _header_args(hdr, name), name
    assert _header_args(hdr, "spmf_cells_scratch_bytes") == 3 and _header_args(hdr, "spmf_score_cells") == 14
    assert "define SPMF_ABI_VERSION 6" in hdr and _lib.ABI_VERSION == 6


def test_score_cells_is_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        assert callable(getattr(cls, "score_cells", None)), cls.__name__


def _cpu_model():
    from spmf_amd import PoissonFactorization
    m = PoissonFactorization(latent_dim=2, feature_dim=6, initialize_distributions=False, device="cpu")
    rng = np.random.default_rng(0)
    x = rng.poisson(1.0, size=(8, 6)).astype(np.float64)
    draws = {"u": rng.random((2, 6, 2)), "v": rng.random((2, 2, 6)), "w": rng.random((2, 1, 6)),
             "s": rng.random((2, 2, 6))}
    return m, x, draws


def test_score_cells_on_a_cpu_model_fails_like_top_k():
    m, x, draws = _cpu_model()
    with pytest.raises(Exception) as e_topk:
        m.top_k({"counts": x}, k=3, draws=draws)
    with pytest.raises(Exception) as e_cells:
        m.score_cells({"counts": x}, [0, 3], [1, 5], values=[0.0, 2.0], draws=draws)
    assert type(e_cells.value) is type(e_topk.value), (e_cells.value, e_topk.value)
    assert not isinstance(e_cells.value, ValueError)


def test_unequal_lengths_and_an_iterable_raise_value_error():
    m, x, draws = _cpu_model()
    with pytest.raises(ValueError):
        m.score_cells({"counts": x}, [0, 3], [1], draws=draws)
    with pytest.raises(ValueError):
        m.score_cells({"counts": x}, [0, 3], [1, 5], values=[1.0], draws=draws)
    with pytest.raises(ValueError):
        m.score_cells({"counts": x}, np.zeros((2, 1), dtype=np.int64), [1, 5], draws=draws)
    with pytest.raises(ValueError):
        m.score_cells([{"counts": x}], [0], [1], draws=draws)
    with pytest.raises(ValueError):
        m.score_cells(lambda: iter([{"counts": x}]), [0], [1], draws=draws)


def _summary_numpy(l):
    """fp64 restatement of heldout.summarize."""
    l = np.asarray(l, dtype=np.float64).reshape(-1)
    x = l[np.isfinite(l)]
    n = x.size
    return {"lppd_sum": float(x.sum()) if n else 0.0, "lppd_mean": float(x.mean()) if n else float("nan"),
            "se": float(np.sqrt(n * x.var(ddof=1))) if n >= 2 else 0.0, "n": n, "n_excluded": l.size - n}


def _same(got, want):
    assert set(got) == {"lppd_sum", "lppd_mean", "se", "n", "n_excluded"}
    assert got["n"] == want["n"] and got["n_excluded"] == want["n_excluded"]
    for k in ("lppd_sum", "lppd_mean", "se"):
        if math.isnan(want[k]):
            assert math.isnan(got[k]), k
        else:
            assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), (k, got[k], want[k])


def test_summarize_agrees_with_numpy_on_a_vector_with_nans():
    from spmf_amd.heldout import summarize
    rng = np.random.default_rng(7)
    l = (-5.0 * rng.gamma(2.0, 1.0, size=1000)).astype(np.float32)
    l[::7] = np.nan
    l[3] = -np.inf
    want = _summary_numpy(l)
    assert want["n_excluded"] == 144 and want["n"] == 856 and want["se"] > 0
    _same(summarize(torch.as_tensor(l)), want)
    _same(summarize(l), want)                                   # numpy in
    # n = 0 (empty, and nothing finite) and n = 1
    for v in (np.zeros(0, np.float32), np.array([np.nan, np.nan], np.float32),
              np.array([np.nan, -2.5], np.float32), np.array([-1.25], np.float32)):
        want = _summary_numpy(v)
        assert want["n"] in (0, 1) and want["se"] == 0.0
        _same(summarize(torch.as_tensor(v)), want)
    assert summarize(torch.zeros(0))["lppd_sum"] == 0.0 and math.isnan(summarize(torch.zeros(0))["lppd_mean"])
    assert summarize(torch.tensor([-1.25]))["lppd_mean"] == -1.25


def test_summary_does_not_depend_on_the_order_of_the_list():
    """The finite entries are sorted before they are reduced: a permuted list gives the same bits."""
    from spmf_amd.heldout import summarize
    rng = np.random.default_rng(11)
    l = (-40.0 * rng.gamma(2.0, 1.0, size=26_000)).astype(np.float32)
    l[::13] = np.nan
    l[5], l[6] = 0.0, -0.0
    one = summarize(torch.as_tensor(l))
    for seed in (1, 2, 3):
        p = np.random.default_rng(seed).permutation(l.size)
        assert summarize(torch.as_tensor(l[p])) == one
