"""CPU-side tests of the streaming WAIC: the combination of the six sums.  (The entry points and the
method on the class surface: test_stream_host.py.)"""
import math

import numpy as np


def _sums(lppd, pwaic, n_excluded=0):
    e = lppd - pwaic
    return np.array([lppd.size, lppd.sum(), pwaic.sum(), (e * e).sum(), n_excluded, 0.0])


def test_combine_matches_the_pointwise_definition():
    from spmf_amd.waic import combine
    rng = np.random.default_rng(5)
    lppd = -rng.gamma(2.0, 3.0, size=4000)
    pwaic = rng.gamma(1.5, 0.05, size=4000)
    out = combine(_sums(lppd, pwaic, 3))
    e = lppd - pwaic
    assert set(out) == {"waic", "se", "lppd", "pwaic", "n", "n_excluded"}
    assert out["n"] == 4000 and out["n_excluded"] == 3
    assert math.isclose(out["lppd"], lppd.sum(), rel_tol=1e-13)
    assert math.isclose(out["pwaic"], pwaic.sum(), rel_tol=1e-13)
    assert math.isclose(out["waic"], -2.0 * e.sum(), rel_tol=1e-13)
    assert math.isclose(out["se"], 2.0 * math.sqrt(e.size * e.var(ddof=1)), rel_tol=1e-10)


def test_sums_of_two_parts_combine_to_the_whole():
    import torch
    from spmf_amd.waic import combine
    rng = np.random.default_rng(6)
    lppd = -rng.gamma(2.0, 3.0, size=1500)
    pwaic = rng.gamma(1.5, 0.05, size=1500)
    whole = combine(_sums(lppd, pwaic, 2))
    merged = combine(torch.as_tensor(_sums(lppd[:400], pwaic[:400], 2) + _sums(lppd[400:], pwaic[400:])))
    assert merged["n"] == whole["n"] == 1500 and merged["n_excluded"] == 2
    for k in ("waic", "se", "lppd", "pwaic"):
        assert math.isclose(merged[k], whole[k], rel_tol=1e-11), k
