"""CPU-side tests of the streaming WAIC: the combination of the six sums, the two
entry points in the header and the binding, the method on the class surface."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_entry_points_are_declared_and_bound():
    from spmf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "spmf_hip.h")).read()
    declared = set(re.findall(r"\b(spmf_[a-z0-9_]+)\s*\(", hdr))
    for name in ("spmf_waic_scratch_bytes", "spmf_waic_accumulate"):
        assert name in declared and name in _lib.SIGNATURES, name
    assert "define SPMF_ABI_VERSION 6" in hdr


def test_waic_streaming_is_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        assert callable(getattr(cls, "waic_streaming", None)), cls.__name__
