"""CPU-side tests of top_k: the two entry points in the header, the export list and the
binding, the method on the class surface."""
import fnmatch
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spmf_topk_scratch_bytes", "spmf_topk_rows")


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
    assert _header_args(hdr, "spmf_topk_scratch_bytes") == 3 and _header_args(hdr, "spmf_topk_rows") == 12
    assert "define SPMF_ABI_VERSION 6" in hdr


def test_top_k_is_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        assert callable(getattr(cls, "top_k", None)), cls.__name__


def test_top_k_on_a_cpu_model_fails_like_waic_streaming():
    import numpy as np
    from spmf_amd import PoissonFactorization
    m = PoissonFactorization(latent_dim=2, feature_dim=6, initialize_distributions=False, device="cpu")
    rng = np.random.default_rng(0)
    x = rng.poisson(1.0, size=(8, 6)).astype(np.float64)
    draws = {"u": rng.random((2, 6, 2)), "v": rng.random((2, 2, 6)), "w": rng.random((2, 1, 6)),
             "s": rng.random((2, 2, 6))}
    with pytest.raises(Exception) as e_waic:
        m.waic_streaming({"counts": x}, draws=draws)
    with pytest.raises(Exception) as e_topk:
        m.top_k({"counts": x}, k=3, draws=draws)
    assert type(e_topk.value) is type(e_waic.value), (e_topk.value, e_waic.value)
    for k in (0, 65):
        with pytest.raises(ValueError):
            m.top_k({"counts": x}, k=k, draws=draws)
