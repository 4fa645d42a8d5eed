"""CPU-side tests of top_k: what the method raises without a device.  (The entry points and the
method on the class surface: test_stream_host.py.)"""
import pytest


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
