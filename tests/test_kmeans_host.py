"""CPU-side tests of k-means (PoissonFactorization.kmeans / cluster, spmf_kmeans_step, csrc/kmeans.hip,
spmf_amd/cluster.py): the two entry points in the header, the export list and the binding, the methods on the
class surface, every argument check of the methods before a library call, the raw entry's refusals through a
ctypes call with dummy aligned addresses, the scratch size, and the centroid update against numpy.
(The valid calls: tests/test_gpu_kmeans.py.)"""
import inspect

import numpy as np
import pytest
import torch

from _stream_cases import (K, assert_declared_exported_bound, assert_kmeans_errors, cpu_model, host_ctx, library,
                           no_library)

HEADER_ARGS = {"spmf_kmeans_scratch_bytes": 4, "spmf_kmeans_step": 15}


def test_entry_points_are_declared_exported_and_bound():
    lib = library()
    for name, nargs in HEADER_ARGS.items():
        assert_declared_exported_bound(name, nargs)
        assert callable(getattr(lib, name)), name
    assert lib.spmf_version() == 6


def test_methods_and_signatures_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    E = inspect.Parameter.empty
    want = {"kmeans": [("points", E), ("n_clusters", E), ("init", "k-means++"), ("max_iter", 100), ("seed", 0)],
            "cluster": [("data", E), ("n_clusters", E), ("nsamples", 32), ("draws", None), ("max_rows", None),
                        ("init", "k-means++"), ("max_iter", 100), ("seed", 0)]}
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        for name, params in want.items():
            fn = getattr(cls, name, None)
            assert callable(fn), (cls.__name__, name)
            got = [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]
            assert got == params, (cls.__name__, name, got)


# ---- the methods' argument checks ----------------------------------------------------------------

def test_every_argument_check_raises_before_a_library_call(monkeypatch):
    m, x, draws = cpu_model()
    no_library(monkeypatch)
    pts = torch.zeros(9, 3)
    data = {"counts": x}
    for g in (True, 0, -1, 65537, 2.0, None, "3"):
        with pytest.raises(ValueError, match="n_clusters"):
            m.kmeans(pts, g)
        with pytest.raises(ValueError, match="n_clusters"):
            m.cluster(data, g, draws=draws)
    for it in (0, -3, 1.5, True, None):
        with pytest.raises(ValueError, match="max_iter"):
            m.kmeans(pts, 2, max_iter=it)
        with pytest.raises(ValueError, match="max_iter"):
            m.cluster(data, 2, draws=draws, max_iter=it)
    for init in ("random", "kmeans++", None, 3, np.zeros((2, 3), dtype=np.float32)):
        with pytest.raises(ValueError, match="init"):
            m.kmeans(pts, 2, init=init)
        with pytest.raises(ValueError, match="init"):
            m.cluster(data, 2, draws=draws, init=init)
    with pytest.raises(ValueError, match="shape"):
        m.kmeans(pts, 2, init=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="shape"):
        m.kmeans(pts, 2, init=torch.zeros(2, 4))
    with pytest.raises(ValueError, match="shape"):
        m.kmeans(pts, 2, init=torch.zeros(6))
    with pytest.raises(ValueError, match="shape"):
        m.cluster(data, 2, draws=draws, init=torch.zeros(2, 3))       # latent_dim is 2
    with pytest.raises(ValueError, match="float32"):
        m.kmeans(pts, 2, init=torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        m.cluster(data, 2, draws=draws, init=torch.zeros(2, 2, dtype=torch.float64))    # before the embedding
    with pytest.raises(ValueError, match="device"):
        m.kmeans(pts, 2, init=torch.zeros(2, 3, device="meta"))
    with pytest.raises(ValueError, match="torch tensor"):
        m.kmeans(np.zeros((9, 3), dtype=np.float32), 2)
    with pytest.raises(ValueError, match="2-D"):
        m.kmeans(torch.zeros(9), 2)
    with pytest.raises(ValueError, match="float32"):
        m.kmeans(pts.double(), 2)
    with pytest.raises(ValueError, match="width"):
        m.kmeans(torch.zeros(4, 257), 2)
    with pytest.raises(ValueError, match="width"):
        m.kmeans(torch.zeros(4, 0), 2)
    with pytest.raises(ValueError, match="device"):
        m.kmeans(pts, 2)                         # host memory is never handed to the library
    with pytest.raises(ValueError, match="device"):
        m.kmeans(pts, 2, init=torch.zeros(2, 3))


def test_custom_codec_raises_in_cluster_as_in_embed(monkeypatch):
    m, x, draws = cpu_model(encoder_function=lambda t: t, decoder_function=lambda t: t)
    no_library(monkeypatch)
    with pytest.raises(ValueError, match="n_clusters"):
        m.cluster({"counts": x}, 0, draws=draws)
    with pytest.raises(NotImplementedError) as e_embed:
        m.embed({"counts": x}, draws=draws)
    with pytest.raises(NotImplementedError) as e_cluster:
        m.cluster({"counts": x}, 2, draws=draws)
    assert str(e_cluster.value) == str(e_embed.value)


# ---- spmf_amd.cluster on the CPU -----------------------------------------------------------------

def test_centroid_update_and_the_empty_cluster_rule_against_numpy():
    from spmf_amd.cluster import update_centroids
    rng = np.random.default_rng(5)
    G, W = 7, 5
    counts = np.array([3, 0, 1, 10 ** 6, 0, 2, 17], dtype=np.int64)
    sums = rng.standard_normal((G, W)) * np.maximum(counts, 1)[:, None]
    sums[1] = 123.0                              # whatever the sums of an empty cluster hold, its centroid stays
    old = rng.standard_normal((G, W)).astype(np.float32)
    got = update_centroids(torch.as_tensor(sums), torch.as_tensor(counts), torch.as_tensor(old))
    assert got.dtype == torch.float32 and tuple(got.shape) == (G, W)
    want = np.where(counts[:, None] > 0, (sums / np.maximum(counts, 1)[:, None]).astype(np.float32), old)
    np.testing.assert_array_equal(got.numpy(), want)
    np.testing.assert_array_equal(got.numpy()[[1, 4]], old[[1, 4]])


def test_named_inits_on_the_cpu():
    from spmf_amd.cluster import init_first, init_plus_plus
    rng = np.random.default_rng(9)
    pts = rng.standard_normal((40, 3)).astype(np.float32)
    pts[0, 1] = np.nan
    pts[3] = np.inf
    t = torch.as_tensor(pts)
    np.testing.assert_array_equal(init_first(t, 3).numpy(), pts[[1, 2, 4]])
    with pytest.raises(ValueError, match="finite rows"):
        init_first(t, 39)
    c = init_plus_plus(t, 12, seed=4).numpy()
    assert c.dtype == np.float32 and c.shape == (12, 3) and np.isfinite(c).all()
    rows = [int(np.flatnonzero((pts == r).all(1))[0]) for r in c]
    assert len(set(rows)) == 12, "distinct points give distinct centres"
    np.testing.assert_array_equal(init_plus_plus(t, 12, seed=4).numpy(), c)
    assert not np.array_equal(init_plus_plus(t, 12, seed=5).numpy(), c)
    with pytest.raises(ValueError, match="finite"):
        init_plus_plus(torch.full((4, 2), float("nan")), 2, seed=0)
    same = init_plus_plus(torch.ones(5, 2), 3, seed=0)               # all rows coincide: still rows of the points
    np.testing.assert_array_equal(same.numpy(), np.ones((3, 2), dtype=np.float32))


# ---- the C-ABI's argument errors -----------------------------------------------------------------

def test_step_errors_return_before_any_device_call():
    """A context of spmf_ctx_create and dummy aligned addresses: no call here is valid, so nothing may be
    launched or dereferenced."""
    lib = library()
    h = host_ctx(lib, K)
    try:
        n, G, row_len = 70, 5, 33
        need = int(lib.spmf_kmeans_scratch_bytes(h, n, G, row_len))
        assert need > 0 and need % 256 == 0
        good = dict(h=h, x=0x1000000, n=n, row_len=row_len, cent=0x2000000, G=G, prev=0x3000000, labels=0x4000000,
                    dist=0x5000000, sums=0x6000000, counts=0x7000000, stats=0x9000000, ptr=0x8000000, nbytes=need,
                    stream=None)
        assert_kmeans_errors(lib, good, need)
    finally:
        lib.spmf_ctx_destroy(h)


def test_scratch_size():
    """0 for arguments the call refuses, else a positive multiple of 256 that holds the working rows and the
    ordering, and does not shrink as the rows grow (knn's own scratch does, where its slices drop to one)."""
    lib = library()
    h = host_ctx(lib, K)
    try:
        for bad in ((-1, 5, 8), (2 ** 31 - 63, 5, 8), (5, 0, 8), (5, 65537, 8), (5, 5, 0), (5, 5, 257)):
            assert int(lib.spmf_kmeans_scratch_bytes(h, *bad)) == 0, bad
        assert int(lib.spmf_kmeans_scratch_bytes(None, 5, 5, 8)) == 0
        assert int(lib.spmf_kmeans_scratch_bytes(h, 0, 1, 1)) > 0
        for G, row_len, kp in ((1, 1, 4), (5, 33, 64), (64, 8, 8), (1000, 256, 256), (65536, 16, 16)):
            last = 0
            for n in (0, 1, 63, 64, 65, 1000, 4096, 32704, 32768, 32769, 65536, 10 ** 6, 10 ** 6 + 1, 2 ** 31 - 64):
                need = int(lib.spmf_kmeans_scratch_bytes(h, n, G, row_len))
                assert need % 256 == 0 and need >= (n + G) * kp * 4 + n * 4 * 8 + (n + 64 * G) * 4, (n, G, row_len)
                assert need >= last, (n, G, row_len, need, last)
                last = need
    finally:
        lib.spmf_ctx_destroy(h)
