"""What the test files of the transform share (test_graph_transform_host.py, test_gpu_graph_transform.py): the
argument list of spmf_graph_transform, its raw call and its error contract, asserted without a device on dummy
addresses and with one on real buffers; the one-epoch cases with the float32 restatement their error bar is measured
with; and the split of the blobs into reference and query rows with the reference's layout for the quality tests."""
import ctypes as C
import functools
import itertools

import numpy as np
import torch

from _graph_layout_cases import blobs, clip_distance, error_units

GT_ARGS = (("n", C.c_int64), ("k", C.c_int), ("idx", C.c_void_p), ("w", C.c_void_p), ("y_ref", C.c_void_p),
           ("n_ref", C.c_int64), ("y_in", C.c_void_p), ("y_out", C.c_void_p), ("row0", C.c_int64),
           ("epoch0", C.c_int), ("n_epochs", C.c_int), ("total", C.c_int), ("lr", C.c_double), ("a", C.c_double),
           ("b", C.c_double), ("gamma", C.c_double), ("rate", C.c_double), ("M", C.c_int), ("seed", C.c_uint64),
           ("stream", C.c_void_p))
N_HEADER_ARGS = len(GT_ARGS) + 1


def graph_transform_raw_call(good):
    """-> call(**overrides): spmf_graph_transform through a binding of its own with the arguments of ``good``."""
    from spmf_amd import _lib
    fn = C.CDLL(_lib.LIB_PATH).spmf_graph_transform
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [t for _, t in GT_ARGS]

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], *[a[n] for n, _ in GT_ARGS])
    return call


def assert_graph_transform_errors(lib, good, after=lambda: None):
    """The error contract of spmf_graph_transform; every call here returns before a launch or a copy, and ``after``
    is run behind each (the GPU file checks its sentinels there)."""
    call, h = graph_transform_raw_call(good), good["h"]
    nan, inf = float("nan"), float("inf")

    def refused(**kw):
        assert call(**kw) == -1, kw
        msg = lib.spmf_last_error(h).decode()
        assert msg.startswith("graph_transform: "), msg
        after()
        return msg
    for k in (0, -1, 65):
        assert "k must" in refused(k=k)
    for m in (0, -1, 65):
        assert "n_negatives" in refused(M=m)
    assert "n_query" in refused(n=-1)
    for n_ref in (-1, 2 ** 31, 2 ** 40):
        assert "n_ref" in refused(n_ref=n_ref)
    for kw in (dict(row0=-1), dict(row0=2 ** 32 - good["n"] + 1), dict(row0=2 ** 32 + 1, n=0), dict(row0=2 ** 62),
               dict(row0=2 ** 63 - 1, n=2 ** 63 - 1)):
        assert "row0" in refused(**kw)
    for kw in (dict(epoch0=-1), dict(n_epochs=-1), dict(epoch0=3, n_epochs=2, total=4), dict(n_epochs=1, total=0),
               dict(epoch0=2 ** 31 - 1, n_epochs=2 ** 31 - 1, total=2 ** 31 - 1)):
        assert "epoch" in refused(**kw)
    for name in ("a", "b"):
        for v in (0.0, -1.0, nan, inf):
            assert "a and b" in refused(**{name: v})
    for name in ("lr", "gamma", "rate"):
        for v in (-1e-9, nan, inf, -inf):
            assert "finite" in refused(**{name: v})
    for name in ("idx", "w", "y_out", "y_ref"):
        assert "null" in refused(**{name: None})
    assert "continued" in refused(y_in=None, epoch0=1, n_epochs=1)
    assert "continued" in refused(y_in=None, epoch0=1, n_epochs=0)
    refused(n=0, k=0)                        # errors come before the empty return
    refused(n=0, y_ref=None)
    assert call(h=None) == -1


# ---- the one-epoch cases ---------------------------------------------------------------------------------------
EPOCH, TOTAL = 2, 10
QS = (1, 2, 15, 16, 17, 64, 65, 257)
KS = (1, 15, 16, 17, 48, 64)
MS = (1, 8, 16, 17, 64)
N_REFS = (1, 2, 300)
MIN_DISTS = (0.1, 0.5)
LRS = (1.0, 0.01)


@functools.lru_cache(maxsize=None)
def curve(min_dist):
    from spmf_amd import graph
    return graph.find_ab(min_dist, 1.0)


def one_epoch_cases(Q):
    """Every (k, M, n_ref, min_dist) of the one-epoch test at ``Q`` query rows."""
    return list(itertools.product(KS, MS, N_REFS, MIN_DISTS))


def transform_case(Q, k, M, n_ref, min_dist=0.1, seed=0, epoch=EPOCH, row0=0):
    """``Q`` query rows with ``k`` entries each among ``n_ref`` reference rows at uniform positions in [-10, 10]^2,
    every entry valid, the weights uniform in (0.05, 1), with starting positions that reach every branch of an
    epoch -> dict(idx int32 [Q,k], w, y_ref, y_in: float32 numpy).  Row i starts, by i mod 7: 1 -- on its first
    neighbour (d^2 = 0); 3 -- 1000 away from it (d^2 = 2e6, the clip inactive); 5 -- at 0.9, 1.0 or 1.1 times the
    distance from its first negative (known from (seed, row0 + i, epoch)) where the repulsive step is 4; else
    uniform in [-10, 10]^2."""
    from spmf_amd import graph
    a, b = curve(min_dist)
    rng = np.random.default_rng(5200 + 1000 * Q + 10 * k + n_ref)
    idx = rng.integers(0, n_ref, size=(Q, k)).astype(np.int32)
    w = rng.uniform(0.05, 1.0, size=(Q, k)).astype(np.float32)
    y_ref = rng.uniform(-10, 10, size=(n_ref, 2)).astype(np.float32)
    y_in = rng.uniform(-10, 10, size=(Q, 2)).astype(np.float32)
    neg = graph.transform_negatives(row0, Q, n_ref, epoch, M, seed)
    d4 = clip_distance(a, b)
    for i in range(Q):
        if i % 7 == 1:
            y_in[i] = y_ref[idx[i, 0]]
        elif i % 7 == 3:
            y_in[i] = y_ref[idx[i, 0]] + np.float32(1000.0)
        elif i % 7 == 5:
            y_in[i] = y_ref[neg[i, 0]] + np.array([d4 * (0.9, 1.0, 1.1)[(i // 7) % 3], 0.0], dtype=np.float32)
    return dict(idx=idx, w=w, y_ref=y_ref, y_in=y_in)


def restate32(idx, w, y_ref, y_in, row0, epoch, total_epochs, lr, a, b, gamma, rate, M, seed):
    """One epoch of include/spmf_hip.h spmf_graph_transform in float32 numpy on clean inputs (every entry valid,
    every position finite, n_ref > 0): the formulas of the kernel in its number format, the sums sequential in list
    order.  What the error bar of the GPU test is measured with."""
    from spmf_amd import graph
    f = np.float32
    y = np.asarray(y_in, dtype=f)
    y_ref = np.asarray(y_ref, dtype=f)
    w = np.asarray(w, dtype=f)
    Q, k = w.shape
    alpha = f(float(lr) * (1.0 - epoch / float(total_epochs)))
    a32, b32, neg2b, tgb, rom = f(a), f(b), f(-2.0 * b), f(2.0 * gamma * b), f(rate / M)

    def terms(other, coef):
        d = y - other
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        live = d2 > 0
        s = np.where(live, d2, f(1))
        q = np.minimum(a32 * np.exp2(b32 * np.log2(s)), f(2.0 ** 60))
        c = np.where(live, coef(s, q), f(0))
        return np.clip(c[:, None] * d, f(-4), f(4)).astype(f)
    W = np.zeros(Q, dtype=f)
    F = np.zeros((Q, 2), dtype=f)
    for t in range(k):
        W = W + w[:, t]
        F = F + w[:, t, None] * terms(y_ref[idx[:, t]], lambda s, q: neg2b * q / (s * (f(1) + q)))
    neg = graph.transform_negatives(row0, Q, y_ref.shape[0], epoch, M, seed)
    G = np.zeros((Q, 2), dtype=f)
    for m in range(M):
        G = G + terms(y_ref[neg[:, m]], lambda s, q: tgb / ((f(0.001) + s) * (f(1) + q)))
    step = (alpha / np.maximum(f(1), W)).astype(f)
    out = (y + step[:, None] * (F + (rom * W)[:, None] * G)).astype(f)
    assert out.dtype == f
    return out


def one_epoch_reference(c, M, min_dist, lr, seed=0, row0=0):
    """-> (fp64 reference of the case's one epoch, A, W, alpha)."""
    from spmf_amd import graph
    a, b = curve(min_dist)
    ref, A, W = graph.transform_reference(c["idx"], c["w"], c["y_ref"], c["y_in"], row0, EPOCH, 1, TOTAL, lr, a, b,
                                          1.0, 5.0, M, seed, details=True)
    return ref, A, W, float(np.float32(lr * (1.0 - EPOCH / TOTAL)))


def restatement_units(Q):
    """The largest error of the float32 restatement against the fp64 reference over the one-epoch cases at ``Q``
    rows, in the units of ``error_units`` -> (units, the case)."""
    worst = (-1.0, None)
    for k, M, n_ref, md in one_epoch_cases(Q):
        a, b = curve(md)
        c = transform_case(Q, k, M, n_ref, md)
        for lr in LRS:
            ref, A, W, alpha = one_epoch_reference(c, M, md, lr)
            soft = restate32(c["idx"], c["w"], c["y_ref"], c["y_in"], 0, EPOCH, TOTAL, lr, a, b, 1.0, 5.0, M, 0)
            u = error_units(soft, ref, c["y_in"], alpha, A, W)
            if u > worst[0]:
                worst = (u, (Q, k, M, n_ref, md, lr))
    return worst


# ---- the quality case ------------------------------------------------------------------------------------------
QUALITY_K = 10


@functools.lru_cache(maxsize=None)
def blob_split():
    """The 480 blob rows split into 80 query rows (i % 6 == 5) and 400 reference rows, the reference rows laid out
    by the fp64 restatement of the layout (exact kNN k = 10 -> fuzzy_graph -> 500 epochs of ``layout_reference``
    from ``init_pca``, lr 1, min_dist 0.1, rounded to fp32) and the queries' exact kNN among the reference rows
    with their memberships -> dict of read-only arrays; computed once on the CPU."""
    from spmf_amd import graph, neighbors
    x, labels = blobs()
    query = torch.arange(x.shape[0]) % 6 == 5
    xr, xq = x[~query], x[query]
    idx, dist = neighbors.brute_force(xr, xr, QUALITY_K, exclude_self=True)
    indptr, indices, wts = graph.to_csr(graph.fuzzy_graph(idx, dist))
    a, b = graph.find_ab(0.1, 1.0)
    y_ref = graph.layout_reference(indptr, indices, wts, graph.init_pca(xr).numpy(), 0, 500, 500, 1.0, a, b, 1.0, 5.0,
                                   8, 0).astype(np.float32)
    qi, qd = neighbors.brute_force(xq, xr, QUALITY_K)
    qw = graph.query_weights(qi, qd)
    return dict(y_ref=y_ref, labels_ref=labels[~query].numpy(), labels_query=labels[query].numpy(),
                idx=qi.numpy().astype(np.int32), dist=qd.numpy(), w=qw["weights"].numpy(), a=a, b=b)


def transform_quality(y, s):
    """-> (purity, spacing ratio) of query positions ``y`` [80, 2] on the split ``s``: the share of a query's 10
    nearest reference rows in the plane that carry its label, and the median distance from a query to its nearest
    reference row over the reference rows' own median nearest-neighbour spacing."""
    from spmf_amd import neighbors
    y = torch.as_tensor(np.asarray(y, dtype=np.float64))
    ref = torch.as_tensor(s["y_ref"].astype(np.float64))
    idx, dist = neighbors.brute_force(y, ref, 10)
    pure = float((torch.as_tensor(s["labels_ref"])[idx] == torch.as_tensor(s["labels_query"])[:, None]).double().mean())
    _, own = neighbors.brute_force(ref, ref, 1, exclude_self=True)
    return pure, float(dist[:, 0].median() / own[:, 0].median())
