"""CPU-side tests of the neighbour calls (PoissonFactorization.embed / knn / neighbors, spmf_embed_rows,
spmf_knn, csrc/knn.hip): the two entry points of knn in the header, the export list and the binding (those of
embed: the "embed" row of tests/test_stream_host.py), the methods' signatures on the class surface, the
argument checks of the methods that need no device, the host helpers of spmf_amd.neighbors, and the argument errors of the two calls -- all refused before anything touches a device.
(The valid calls: tests/test_gpu_knn.py.)"""
import inspect

import numpy as np
import pytest
import torch

from _stream_cases import (B, K, S, ENTRIES, abi_call, assert_declared_exported_bound, assert_embed_own_errors,
                           assert_knn_errors, assert_shared_errors, cpu_model, host_ctx, host_good_call, knn_raw_call,
                           library)

# spmf_knn is no draw-stage call: it is not in the contract table
HEADER_ARGS = {"spmf_knn_scratch_bytes": 4, "spmf_knn": 14}


def test_entry_points_are_declared_exported_and_bound():
    for name, nargs in HEADER_ARGS.items():
        assert_declared_exported_bound(name, nargs)


def test_symbols_are_in_the_built_library():
    lib = library()
    for name in (*HEADER_ARGS, ENTRIES["embed"].size, ENTRIES["embed"].call):
        assert callable(getattr(lib, name)), name


def test_methods_and_signatures_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    want = {"embed": [("data", inspect.Parameter.empty), ("nsamples", 32), ("draws", None), ("sd", False),
                      ("max_rows", None)],
            "knn": [("points", inspect.Parameter.empty), ("k", 15), ("queries", None), ("metric", "euclidean"),
                    ("include_self", False)],
            "neighbors": [("data", inspect.Parameter.empty), ("k", 15), ("query", None), ("metric", "euclidean"),
                          ("include_self", False), ("nsamples", 32), ("draws", None), ("max_rows", None)]}
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        for name, params in want.items():
            fn = getattr(cls, name, None)
            assert callable(fn), (cls.__name__, name)
            got = [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]
            assert got == params, (cls.__name__, name, got)


# ---- the methods' argument checks ----------------------------------------------------------------

@pytest.mark.parametrize("k", [0, 65, -1, 2.5, True])
def test_bad_k_raises_value_error(k):
    m, x, draws = cpu_model()
    pts = torch.zeros(9, 3)
    with pytest.raises(ValueError, match="k"):
        m.knn(pts, k=k)
    with pytest.raises(ValueError, match="k"):
        m.neighbors({"counts": x}, k=k, draws=draws)


def test_bad_metric_and_inputs_raise_value_error():
    m, x, draws = cpu_model()
    pts = torch.zeros(9, 3)
    with pytest.raises(ValueError, match="metric"):
        m.knn(pts, k=3, metric="manhattan")
    with pytest.raises(ValueError, match="metric"):
        m.neighbors({"counts": x}, k=3, metric="manhattan", draws=draws)
    with pytest.raises(ValueError, match="2-D"):
        m.knn(torch.zeros(9), k=3)
    with pytest.raises(ValueError, match="2-D"):
        m.knn(pts, k=3, queries=torch.zeros(3))
    with pytest.raises(ValueError, match="float32"):
        m.knn(pts.double(), k=3)
    with pytest.raises(ValueError, match="float32"):
        m.knn(pts, k=3, queries=torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="width"):
        m.knn(pts, k=3, queries=torch.zeros(4, 2))
    with pytest.raises(ValueError, match="width"):
        m.knn(torch.zeros(4, 257), k=3)
    with pytest.raises(ValueError, match="torch tensor"):
        m.knn(np.zeros((4, 3), dtype=np.float32), k=3)
    with pytest.raises(ValueError, match="device"):
        m.knn(pts, k=3)                      # host memory is never handed to the library


def test_sd_needs_two_draws():
    m, x, draws = cpu_model()
    one = {n: v[:1] for n, v in draws.items()}
    with pytest.raises(ValueError, match="at least 2 draws"):
        m.embed({"counts": x}, draws=one, sd=True)
    with pytest.raises(ValueError, match="nsamples >= 2"):
        m.embed({"counts": x}, nsamples=1, sd=True)


def test_a_valid_embed_on_a_cpu_model_fails_like_top_k():
    m, x, draws = cpu_model()
    with pytest.raises(Exception) as e_topk:
        m.top_k({"counts": x}, k=3, draws=draws)
    with pytest.raises(Exception) as e_embed:
        m.embed({"counts": x}, draws=draws)
    assert type(e_embed.value) is type(e_topk.value) and not isinstance(e_embed.value, ValueError)


# ---- spmf_amd.neighbors --------------------------------------------------------------------------

def _double_loop(q, r, k, metric, off):
    """The reference of the reference: plain Python over fp64 numpy rows."""
    q, r = np.asarray(q, dtype=np.float64), np.asarray(r, dtype=np.float64)
    idx = np.full((len(q), k), -1, dtype=np.int64)
    dist = np.full((len(q), k), np.inf)
    for i, a in enumerate(q):
        found = []
        for j, b in enumerate(r):
            if off is not None and j == i + off:
                continue
            if not (np.isfinite(a).all() and np.isfinite(b).all()):
                continue
            if metric == "cosine":
                na, nb = np.sqrt((a * a).sum()), np.sqrt((b * b).sum())
                if na == 0 or nb == 0:
                    continue
                d = 0.5 * (((a / na) - (b / nb)) ** 2).sum()
            else:
                d = np.sqrt(((a - b) ** 2).sum())
            found.append((d, j))
        found.sort()
        for s, (d, j) in enumerate(found[:k]):
            idx[i, s], dist[i, s] = j, d
    return idx, dist


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("self_case", [False, True])
def test_brute_force_against_a_double_loop(metric, self_case):
    from spmf_amd.neighbors import brute_force
    rng = np.random.default_rng(11)
    r = rng.standard_normal((23, 5)).astype(np.float32)
    r[4] = r[9]                              # a tie: ascending index
    r[6, 2] = np.nan
    r[12] = 0.0                              # no direction under cosine
    q = r if self_case else rng.standard_normal((7, 5)).astype(np.float32)
    if not self_case:
        q[3, 0] = np.inf
    for k in (1, 4, 30):
        idx, dist = brute_force(torch.as_tensor(q), torch.as_tensor(r), k, metric, self_case, max_elements=300)
        ridx, rdist = _double_loop(q, r, k, metric, 0 if self_case else None)
        assert idx.dtype == torch.int64 and dist.dtype == torch.float64 and idx.shape == (len(q), k)
        np.testing.assert_array_equal(idx.numpy(), ridx)
        np.testing.assert_allclose(dist.numpy(), rdist, rtol=1e-14, atol=1e-15)
    assert (idx.numpy()[:, -1] == -1).all(), "k above the row count leaves padding"
    if self_case:
        assert (idx.numpy()[6] == -1).all(), "a non-finite query has no neighbour"
        assert not (idx.numpy() == 6).any(), "a non-finite row is nobody's neighbour"
        assert (idx.numpy()[4, 0] == 9 and dist.numpy()[4, 0] == 0.0) or metric == "cosine"
    one, _ = brute_force(torch.as_tensor(q), torch.as_tensor(r), 4, metric, self_case)
    np.testing.assert_array_equal(one.numpy(), ridx[:, :4])     # the chunking changes nothing
    with pytest.raises(ValueError):
        brute_force(torch.zeros(3, 2), torch.zeros(3, 3), 2)
    with pytest.raises(ValueError):
        brute_force(torch.zeros(3, 2), torch.zeros(3, 2), 2, "manhattan")


def test_brute_force_self_offset_and_empty_sets():
    from spmf_amd.neighbors import brute_force
    r = torch.arange(12, dtype=torch.float32).reshape(6, 2)
    idx, dist = brute_force(r[2:4], r, 2, "euclidean", 2)          # queries ARE rows 2 and 3
    assert idx.tolist() == [[1, 3], [2, 4]]
    idx, dist = brute_force(r[2:4], r, 2, "euclidean", False)
    assert idx.tolist() == [[2, 1], [3, 2]] and dist[:, 0].tolist() == [0.0, 0.0]
    idx, dist = brute_force(r, r[:0], 3)
    assert idx.shape == (6, 3) and (idx == -1).all() and torch.isinf(dist).all()
    idx, dist = brute_force(r[:0], r, 3)
    assert idx.shape == (0, 3) and dist.shape == (0, 3)


def test_to_csr_drops_the_padding():
    from spmf_amd.neighbors import to_csr
    idx = torch.tensor([[3, 1, -1], [-1, -1, -1], [0, 2, 4]], dtype=torch.int32)
    dist = torch.tensor([[0.5, 1.5, np.inf], [np.inf] * 3, [0.0, 0.25, 2.0]], dtype=torch.float32)
    indptr, indices, data = to_csr(idx, dist, n_ref=5)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
    assert indptr.tolist() == [0, 2, 2, 5], "the middle row is all padding"
    assert indices.tolist() == [3, 1, 0, 2, 4] and data.tolist() == [0.5, 1.5, 0.0, 0.25, 2.0]
    indptr, indices, data = to_csr(idx.numpy(), dist.numpy())
    assert indptr.tolist() == [0, 2, 2, 5]
    e = to_csr(torch.zeros(0, 4, dtype=torch.int32), torch.zeros(0, 4))
    assert e[0].tolist() == [0] and e[1].size == 0 and e[2].size == 0
    with pytest.raises(ValueError, match="outside"):
        to_csr(idx, dist, n_ref=4)
    with pytest.raises(ValueError, match="one shape"):
        to_csr(idx, dist[:, :2])
    with pytest.raises(ValueError, match="integers"):
        to_csr(dist, dist)


def test_recall():
    from spmf_amd.neighbors import recall
    truth = torch.tensor([[1, 2, 3], [4, 5, -1], [-1, -1, -1]])
    assert recall(truth, truth) == 1.0
    assert recall(torch.tensor([[3, 9, 1], [5, 4, 7], [0, 1, 2]]), truth) == 4 / 5      # the order does not count
    assert recall(torch.tensor([[7, 8, 9], [7, 8, 9], [7, 8, 9]]), truth) == 0.0
    assert recall(torch.full((2, 3), -1), torch.full((2, 3), -1)) == 1.0
    with pytest.raises(ValueError):
        recall(torch.zeros(2, 3), torch.zeros(3, 3))


# ---- the C-ABI's argument errors -----------------------------------------------------------------

def test_knn_errors_return_before_any_device_call():
    """A context of spmf_ctx_create and dummy aligned addresses: nothing here is a valid call with queries, so
    nothing may be launched or dereferenced."""
    lib = library()
    h = host_ctx(lib, K)
    try:
        nq, nr, row_len = 70, 333, 33
        need = int(lib.spmf_knn_scratch_bytes(h, nq, nr, row_len))
        assert need > 0 and need % 256 == 0
        good = dict(h=h, q=0x1000000, nq=nq, r=0x2000000, nr=nr, row_len=row_len, k=5, flags=0, self_offset=-1,
                    idx=0x3000000, dist=0x4000000, ptr=0x8000000, nbytes=need, stream=None)
        assert_knn_errors(lib, good, need)
        call = knn_raw_call(good)
        # no query: served without a launch, no pointer here could be dereferenced
        assert call(nq=0) == 0 and call(nq=0, q=None, idx=None, dist=None) == 0
        assert call(nq=0, nr=0, r=None) == 0
    finally:
        lib.spmf_ctx_destroy(h)


def test_knn_scratch_size():
    """A multiple of 256 that holds the padded working rows of both sets and the biases; it does not depend on
    k (the call has no k) and is 0 for arguments the call refuses."""
    lib = library()
    h = host_ctx(lib, K)
    try:
        for nq, nr, row_len, kp in ((70, 70, 3, 4), (5, 333, 33, 64), (197, 197, 70, 128), (1000, 20000, 256, 256)):
            need = int(lib.spmf_knn_scratch_bytes(h, nq, nr, row_len))
            assert need % 256 == 0 and need >= (nq + nr) * kp * 4 + nr * 4
        assert int(lib.spmf_knn_scratch_bytes(h, 0, 0, 8)) > 0
        for bad in ((-1, 5, 8), (5, -1, 8), (5, 2 ** 31, 8), (5, 5, 0), (5, 5, 257)):
            assert int(lib.spmf_knn_scratch_bytes(h, *bad)) == 0, bad
        assert int(lib.spmf_knn_scratch_bytes(None, 5, 5, 8)) == 0
    finally:
        lib.spmf_ctx_destroy(h)


def test_embed_errors_return_before_any_device_call():
    lib = library()
    good, need, no_u, raw, cleanup = host_good_call(lib, "embed")
    h, cs = good["h"], good["ct"]
    try:
        assert need == int(lib.spmf_cells_scratch_bytes(h, B, S)), "the draw carve alone"
        assert int(lib.spmf_embed_scratch_bytes(h, B, 0)) == 0 and int(lib.spmf_embed_scratch_bytes(h, B, 1)) > 0
        call = assert_shared_errors(lib, "embed", good, need, no_u, raw)
        assert_embed_own_errors(lib, call, good)
        empty = type(cs).from_buffer_copy(cs)
        empty.n_rows = 0
        assert abi_call("embed", good)(ct=empty) == 0, "an empty batch launches nothing"
    finally:
        cleanup()
