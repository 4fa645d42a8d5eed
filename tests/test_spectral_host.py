"""CPU-side tests of the spectral calls (PoissonFactorization.spectral / spectral_cluster, spmf_amd/spectral.py,
spmf_graph_scale / spmf_graph_spmm / spmf_block_gram / spmf_block_rotate, csrc/spectral.hip): the entry points'
declarations, the size function and the error contract on dummy addresses, the solver on its float32 numpy backend
against the fp64 reference, the helpers, and every argument check with the library unloadable.  (The valid calls of
the library: tests/test_gpu_spectral.py.)

Measured here with the numpy backend at tol = 1e-5 (outer iterations / products / largest residual):
cycle of 64 rows, m = 2: 5 / 44 / 1.3e-7; blobs' graph, m = 7: 4 / 32 / 4.9e-7; two rings, m = 1: 5 / 70 / 3.9e-6;
the sines 7.8e-7, 1.9e-6 and 1.1e-4 against the bounds 3.0e-5, 5.9e-6 and 5.6e-3."""
import inspect
import os

import numpy as np
import pytest
import torch

from _spectral_cases import (BLOCK, CHUNK, HEADER_ARGS, agreement, assert_criteria, assert_errors, assert_sign_rule,
                             cycle_graph, end_to_end_graphs, host_good, many_components, raw_call, rings)
from _stream_cases import ROOT, assert_declared_exported_bound, cpu_model, host_ctx, library, no_library
from spmf_amd import spectral

TOL = 1e-5


def test_entry_points_are_declared_exported_and_bound():
    lib = library()
    for name, nargs in HEADER_ARGS.items():
        assert_declared_exported_bound(name, nargs)
        assert callable(getattr(lib, name)), name
    hdr = open(os.path.join(ROOT, "include", "spmf_hip.h")).read()
    assert f"#define SPMF_BLOCK_COLS {BLOCK}" in hdr and f"#define SPMF_GRAM_CHUNK_ROWS {CHUNK}" in hdr
    assert spectral.BLOCK == BLOCK


def test_methods_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    E = inspect.Parameter.empty
    want = {"spectral": [("graph", E), ("n_components", 2), ("tol", 1e-4), ("max_iter", 100), ("seed", 0)],
            "spectral_cluster": [("graph", E), ("n_clusters", E), ("tol", 1e-4), ("max_iter", 100), ("seed", 0),
                                 ("kmeans_init", "k-means++"), ("kmeans_max_iter", 100)]}
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        for name, params in want.items():
            got = [(p.name, p.default) for p in list(inspect.signature(getattr(cls, name)).parameters.values())[1:]]
            assert got == params, (cls.__name__, name, got)


def test_scratch_size():
    """0 for arguments the call refuses, else a positive multiple of 256 that holds 256 doubles per chunk of rows
    and does not shrink as the rows grow."""
    lib = library()
    h = host_ctx(lib, 3)
    try:
        for bad in (-1, 2 ** 31 - 63, 2 ** 40):
            assert int(lib.spmf_block_gram_scratch_bytes(h, bad)) == 0, bad
        assert int(lib.spmf_block_gram_scratch_bytes(None, 5)) == 0
        last = 0
        for n in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 5000, 10 ** 6, 2 ** 31 - 64):
            need = int(lib.spmf_block_gram_scratch_bytes(h, n))
            chunks = max(1, -(-n // CHUNK))
            assert need > 0 and need % 256 == 0 and need >= 8 * BLOCK * BLOCK * chunks and need >= last, (n, need)
            last = need
    finally:
        lib.spmf_ctx_destroy(h)


@pytest.mark.parametrize("entry", ["graph_scale", "graph_spmm", "block_gram", "block_rotate"])
def test_raw_errors_return_before_any_device_call(entry):
    """A context of spmf_ctx_create and dummy aligned addresses: no call here is valid, so nothing may be launched
    or dereferenced; the empty calls return SPMF_OK without touching anything either."""
    lib = library()
    h = host_ctx(lib, 3)
    try:
        good, need = host_good(entry, h, lib)
        assert_errors(lib, entry, good, need)
        call = raw_call(entry, good)
        if entry != "block_gram":                              # (its empty call zero-fills g on the stream)
            assert call(n=0) == 0                              # no row: nothing to do
            assert call(n=0, indptr=None, indices=None, weights=None, scale=None, x=None, y=None, z=None) == 0
    finally:
        lib.spmf_ctx_destroy(h)


@pytest.mark.parametrize("name", ["cycle", "blobs", "rings"])
def test_solver_on_the_numpy_backend_against_the_reference(name):
    g, m = {n: (gr, mm) for n, gr, mm in end_to_end_graphs()}[name]
    res = spectral.solve(spectral.NumpyOps(g), m, tol=TOL)
    assert_criteria(name, res, m, TOL)
    assert_sign_rule(res["vectors"])
    assert res["vectors"].dtype == torch.float32 and res["values"].dtype == np.float64
    assert torch.equal(res["embedding"], res["vectors"][:, 1:])
    again = spectral.solve(spectral.NumpyOps(g), m, tol=TOL)
    assert torch.equal(res["vectors"].view(torch.int32), again["vectors"].view(torch.int32)), "the same bits twice"
    assert np.array_equal(res["values"], again["values"]) and res["n_products"] == again["n_products"]
    if name == "cycle":
        want = np.cos(2.0 * np.pi * np.array([0, 1, 1]) / 64.0)
        assert np.abs(res["values"] - want).max() <= 1e-6, res["values"]
        assert res["n_unit"] == 1
    if name == "blobs":
        assert res["n_unit"] == 7
    if name == "rings":
        assert res["n_unit"] == 2
        other = spectral.solve(spectral.NumpyOps(g), m, tol=TOL, seed=1)
        assert not torch.equal(res["vectors"], other["vectors"]), "a degenerate space: the basis is the seed's"
        assert_criteria(name, other, m, TOL)


def test_rows_without_an_edge_stay_exactly_zero():
    """The blobs' graph with two rows cut out of it (their lists emptied, their entries in the other rows given
    weight 0): scale 0, the rows of the vectors exactly 0, and the rest still an eigenbasis."""
    g = {n: t.clone() for n, t in end_to_end_graphs()[1][1].items() if n in ("indptr", "indices", "weights")}
    dead = (5, 300)
    row = torch.repeat_interleave(torch.arange(480), torch.diff(g["indptr"]))
    for d in dead:
        g["weights"][(row == d) | (g["indices"] == d)] = 0.0
    res = spectral.solve(spectral.NumpyOps(g), 3, tol=TOL)
    assert res["converged"]
    assert (res["scale"][list(dead)] == 0).all() and int((res["scale"] == 0).sum()) == 2
    assert (res["vectors"][list(dead)] == 0).all()
    S = spectral.normalized_dense(g)
    V = res["vectors"].double().numpy()
    assert np.abs(np.linalg.norm(S @ V - V * res["values"][None, :], axis=0) - res["residuals"]).max() <= 1e-6


def test_more_components_than_columns_do_not_stall(monkeypatch):
    """20 components: every Ritz value of the block goes to 1, and a filter cut at the smallest of them gains
    nothing.  With the cut lowered on a stalled iteration the residuals reach 1e-5 in 5 outer iterations (67
    products, 1.6e-7); without that rule they stay at 2.1e-5 through 30 (617 products)."""
    g = many_components()
    val, _ = spectral.reference(g, 2)
    assert int((val > 1 - 1e-9).sum()) == 20 and val[20] < 0.8
    res = spectral.solve(spectral.NumpyOps(g), 2, tol=TOL, max_iter=30)
    assert res["converged"] and res["n_iter"] <= 10 and res["n_unit"] == 3, (res["n_iter"], res["residuals"])
    S = spectral.normalized_dense(g)
    V = res["vectors"].double().numpy()
    assert np.abs(np.linalg.norm(S @ V - V * res["values"][None, :], axis=0) - res["residuals"]).max() <= 1e-6
    monkeypatch.setattr(spectral, "MIN_GAIN", 0.0)
    assert not spectral.solve(spectral.NumpyOps(g), 2, tol=TOL, max_iter=30)["converged"]


def test_too_small_a_graph_names_dense_eigh():
    with pytest.raises(ValueError, match="eigh"):
        spectral.solve(spectral.NumpyOps(cycle_graph(31)), 2)
    assert spectral.solve(spectral.NumpyOps(cycle_graph(32)), 2, tol=TOL)["converged"]
    val, vec = spectral.reference(cycle_graph(31), 2)
    assert np.abs(val[:3] - np.cos(2.0 * np.pi * np.array([0, 1, 1]) / 31.0)).max() <= 1e-12


def test_an_asymmetric_graph_does_not_converge_and_is_not_refused():
    n = 64
    g = {"indptr": torch.arange(0, n + 1, dtype=torch.int64), "indices": ((torch.arange(n) + 1) % n).to(torch.int32),
         "weights": torch.ones(n)}                              # the directed cycle
    res = spectral.solve(spectral.NumpyOps(g), 2, tol=TOL, max_iter=3)
    assert not res["converged"] and res["n_iter"] == 3


def test_diffusion_map_is_the_random_walks_eigenbasis():
    g, _, _ = rings()
    res = spectral.solve(spectral.NumpyOps(g), 3, tol=TOL)
    S = spectral.normalized_dense(g)
    d = spectral.degrees(g)
    P = S * np.sqrt(d)[None, :] / np.sqrt(d)[:, None]          # D^-1 A = D^-1/2 S D^1/2
    for t in (1, 3):
        psi = spectral.diffusion_map(res, t=t).numpy()
        assert psi.dtype == np.float64 and psi.shape == (400, 4)
        lam = res["values"]
        unit = psi / lam[None, :] ** t
        off = np.linalg.norm(P @ unit - unit * lam[None, :], axis=0)
        # |D^-1/2 r| <= max(s) |r|, plus the float32 rounding of the scale
        assert (off <= res["scale"].max().item() * (res["residuals"] + 1e-6)).all(), (off, res["residuals"])


def test_layout_init_extent_and_seed():
    g, _, _ = rings()
    res = spectral.solve(spectral.NumpyOps(g), 2, tol=TOL)
    y = spectral.layout_init(res["embedding"], seed=3)
    assert y.dtype == torch.float32 and tuple(y.shape) == (400, 2)
    assert abs(float(y.abs().max()) - 10.0) <= 1e-3
    assert torch.equal(y, spectral.layout_init(res["embedding"], seed=3))
    other = spectral.layout_init(res["embedding"], seed=4)
    assert not torch.equal(y, other) and float((y - other).abs().max()) <= 2e-3
    exact = res["embedding"].double() * (10.0 / float(res["embedding"].abs().max()))
    noise = (y.double() - exact).flatten()
    assert 0.5e-4 <= float(noise.std()) <= 2e-4
    one = spectral.layout_init(res["embedding"][:, :1], seed=0)
    assert tuple(one.shape) == (400, 2) and float(one[:, 1].abs().max()) <= 1e-3
    for bad in (torch.zeros(5), torch.zeros(5, 0)):
        with pytest.raises(ValueError, match="embedding"):
            spectral.layout_init(bad)
    with pytest.raises(ValueError, match="seed"):
        spectral.layout_init(res["embedding"], seed=-1)


def test_cluster_features_put_the_rings_on_two_orthogonal_points():
    g, x, truth = rings()
    res = spectral.solve(spectral.NumpyOps(g), 1, tol=TOL)
    f = spectral.cluster_features(res, 2).double()
    assert tuple(f.shape) == (400, 2) and float((f.norm(dim=1) - 1).abs().max()) <= 1e-6
    a, b = f[truth == 0], f[truth == 1]
    assert float((a - a[0]).abs().max()) <= 1e-3 and float((b - b[0]).abs().max()) <= 1e-3
    assert abs(float(a[0] @ b[0])) <= 1e-3
    labels = (f @ a[0] < 0.5).long().numpy()
    assert agreement(labels, truth.numpy()) == 1.0
    # a row without an edge has no direction
    res0 = dict(res, vectors=res["vectors"].clone())
    res0["vectors"][7] = 0
    assert bool(torch.isnan(spectral.cluster_features(res0, 2)[7]).all())
    for bad in (0, 3, 2.0, True):
        with pytest.raises(ValueError, match="n_clusters"):
            spectral.cluster_features(res, bad)


def test_every_argument_check_raises_before_a_library_call(monkeypatch):
    m = cpu_model()[0]
    no_library(monkeypatch)
    g = {n: t for n, t in rings()[0].items() if n in ("indptr", "indices", "weights")}
    nan = float("nan")
    for kw, what in ((dict(n_components=0), "n_components"), (dict(n_components=13), "n_components"),
                     (dict(n_components=2.0), "n_components"), (dict(n_components=True), "n_components"),
                     (dict(tol=0.0), "tol"), (dict(tol=nan), "tol"), (dict(tol="1"), "tol"), (dict(tol=-1e-3), "tol"),
                     (dict(max_iter=0), "max_iter"), (dict(max_iter=1.5), "max_iter"), (dict(seed=-1), "seed"),
                     (dict(seed=2 ** 63), "seed")):
        with pytest.raises(ValueError, match=what):
            m.spectral(g, **kw)
        with pytest.raises(ValueError, match=what):
            spectral.solve(None, **kw)
    for kw, what in ((dict(n_clusters=1), "n_clusters"), (dict(n_clusters=14), "n_clusters"),
                     (dict(n_clusters=2.0), "n_clusters"), (dict(n_clusters=2, tol=0.0), "tol"),
                     (dict(n_clusters=2, kmeans_init="best"), "init"), (dict(n_clusters=2, kmeans_max_iter=0), "max_iter")):
        with pytest.raises(ValueError, match=what):
            m.spectral_cluster(g, **kw)
    # the graph, as graph_layout checks it
    for bad in (None, {}, {"indptr": g["indptr"], "indices": g["indices"]}):
        with pytest.raises(ValueError, match="dict"):
            m.spectral(bad)
    for name, t in (("indptr", g["indptr"].to(torch.int32)), ("indices", g["indices"].to(torch.int64)),
                    ("weights", g["weights"].double()), ("weights", g["weights"].numpy())):
        with pytest.raises(ValueError, match=name):
            m.spectral(dict(g, **{name: t}))
    with pytest.raises(ValueError, match="entries"):
        m.spectral(dict(g, weights=g["weights"][:-1]))
    ptr = g["indptr"].clone()
    ptr[-1] += 1
    with pytest.raises(ValueError, match="rise from 0"):
        m.spectral(dict(g, indptr=ptr))
    ind = g["indices"].clone()
    ind[3] = 400
    with pytest.raises(ValueError, match="must lie in"):
        m.spectral(dict(g, indices=ind))
    # too few rows with a valid edge: dense eigh is named, before the device is asked for
    with pytest.raises(ValueError, match="eigh"):
        m.spectral(cycle_graph(31))
    w = g["weights"].clone()
    w[g["indptr"][20]:] = float("nan")
    with pytest.raises(ValueError, match="eigh"):
        m.spectral(dict(g, weights=w))
    # host memory is never handed to the library
    with pytest.raises(ValueError, match="device"):
        m.spectral(g)
    with pytest.raises(ValueError, match="device"):
        m.spectral_cluster(g, 2)
