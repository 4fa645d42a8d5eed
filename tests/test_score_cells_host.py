"""CPU-side tests of score_cells: the argument checks that need no device and the summary of
spmf_amd.heldout.  (The entry points and the method on the class surface: test_stream_host.py.)"""
import math

import numpy as np
import pytest
import torch

from _stream_cases import cpu_model


def test_score_cells_on_a_cpu_model_fails_like_top_k():
    m, x, draws = cpu_model()
    with pytest.raises(Exception) as e_topk:
        m.top_k({"counts": x}, k=3, draws=draws)
    with pytest.raises(Exception) as e_cells:
        m.score_cells({"counts": x}, [0, 3], [1, 5], values=[0.0, 2.0], draws=draws)
    assert type(e_cells.value) is type(e_topk.value), (e_cells.value, e_topk.value)
    assert not isinstance(e_cells.value, ValueError)


def test_unequal_lengths_and_an_iterable_raise_value_error():
    m, x, draws = cpu_model()
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
