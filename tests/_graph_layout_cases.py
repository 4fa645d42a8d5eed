"""What the test files of the layout share (test_graph_host.py, test_gpu_graph_layout.py): the argument list of
spmf_graph_layout, its raw call and its error contract, asserted without a device on dummy addresses and with one on
real buffers; the blobs of the quality tests with their neighbour graph, and neighbour purity; the graphs and
positions of the one-epoch cases, the float32 restatement their error bar is measured with, and the bar's unit."""
import ctypes as C
import functools

import numpy as np
import torch

GL_ARGS = (("n", C.c_int64), ("nnz", C.c_int64), ("indptr", C.c_void_p), ("indices", C.c_void_p),
           ("weights", C.c_void_p), ("y_in", C.c_void_p), ("y_out", C.c_void_p), ("epoch0", C.c_int),
           ("n_epochs", C.c_int), ("total", C.c_int), ("lr", C.c_double), ("a", C.c_double), ("b", C.c_double),
           ("gamma", C.c_double), ("rate", C.c_double), ("M", C.c_int), ("seed", C.c_uint64), ("ptr", C.c_void_p),
           ("nbytes", C.c_size_t), ("stream", C.c_void_p))


def graph_layout_raw_call(good):
    """-> call(**overrides): spmf_graph_layout through a binding of its own with the arguments of ``good``."""
    from spmf_amd import _lib
    fn = C.CDLL(_lib.LIB_PATH).spmf_graph_layout
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [t for _, t in GL_ARGS]

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], *[a[n] for n, _ in GL_ARGS])
    return call


def assert_graph_layout_errors(lib, good, need, after=lambda: None):
    """The error contract of spmf_graph_layout; every call here returns before a launch or a copy, and ``after``
    is run behind each (the GPU file checks its sentinels there)."""
    call, h = graph_layout_raw_call(good), good["h"]
    nan, inf = float("nan"), float("inf")

    def refused(code, **kw):
        assert call(**kw) == code, kw
        msg = lib.spmf_last_error(h).decode()
        assert msg.startswith("graph_layout: "), msg
        after()
        return msg
    for rows in (-1, 2 ** 31 - 63, 2 ** 40):
        assert "n_rows" in refused(-1, n=rows)
    assert "nnz" in refused(-1, nnz=-1)
    for m in (0, -1, 65):
        assert "n_negatives" in refused(-1, M=m)
    for kw in (dict(epoch0=-1), dict(n_epochs=-1), dict(epoch0=3, n_epochs=2, total=4), dict(n_epochs=1, total=0),
               dict(epoch0=2 ** 31 - 1, n_epochs=2 ** 31 - 1, total=2 ** 31 - 1)):
        assert "epoch" in refused(-1, **kw)
    for name in ("a", "b"):
        for v in (0.0, -1.0, nan, inf):
            assert "a and b" in refused(-1, **{name: v})
    for name in ("lr", "gamma", "rate"):
        for v in (-1e-9, nan, inf, -inf):
            assert "finite" in refused(-1, **{name: v})
    for name in ("indptr", "indices", "weights", "y_in", "y_out", "ptr"):
        assert "null" in refused(-1, **{name: None})
    refused(-1, n=0, ptr=None)
    assert "aligned" in refused(-1, ptr=good["ptr"] + 4)
    assert str(need) in refused(-3, nbytes=need - 256)
    refused(-3, n=0, nbytes=0)               # errors come before the empty return
    refused(-3, n_epochs=0, nbytes=0)
    assert call(h=None) == -1


# ---- the quality case ------------------------------------------------------------------------------------------
BLOB_SEED = 1


@functools.lru_cache(maxsize=None)
def blobs(seed=BLOB_SEED, n_blobs=8, per=60, dim=16):
    """8 Gaussian blobs of 60 points in 16 dimensions, unit variance, centres N(0, 2^2 I) -> (float32 [480, 16],
    labels int64 [480]); read-only."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    centres = 2.0 * torch.randn(n_blobs, dim, generator=gen, dtype=torch.float64)
    labels = torch.arange(n_blobs).repeat_interleave(per)
    x = centres[labels] + torch.randn(n_blobs * per, dim, generator=gen, dtype=torch.float64)
    return x.to(torch.float32), labels


@functools.lru_cache(maxsize=None)
def blob_graph(k=10):
    """The blobs' exact kNN (fp64, ``neighbors.brute_force``) and its fuzzy graph on the CPU, computed once."""
    from spmf_amd import graph, neighbors
    x, _ = blobs()
    idx, dist = neighbors.brute_force(x, x, k, exclude_self=True)
    return graph.fuzzy_graph(idx, dist)


def purity(y, labels, k=10):
    """Neighbour purity: the share of each point's ``k`` nearest neighbours in the plane that carry its own label."""
    from spmf_amd import neighbors
    y = torch.as_tensor(y).detach().cpu().double()
    labels = torch.as_tensor(labels).cpu()
    idx, _ = neighbors.brute_force(y, y, k, exclude_self=True)
    return float((labels[idx] == labels[:, None]).double().mean())


# ---- the one-epoch cases ---------------------------------------------------------------------------------------
def clip_distance(a, b, gamma=1.0):
    """The distance d at which the repulsive step |c_r d| = 2 gamma b d / ((0.001 + d^2)(1 + a d^2b)) falls
    through 4 (the larger root: the step rises from 0, peaks near d = 0.03 and falls), by bisection in fp64."""
    def step(d):
        return 2.0 * gamma * b * d / ((0.001 + d * d) * (1.0 + a * d ** (2.0 * b)))
    lo, hi = 0.04, 10.0
    assert step(lo) > 4.0 > step(hi)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if step(mid) > 4.0 else (lo, mid)
    return lo


@functools.lru_cache(maxsize=None)
def layout_case(N, hub=0, seed=0, epoch=2, M=8, a=1.576943, b=0.895061):
    """A random symmetric graph of ``N`` rows and mean degree about 12 with positions that reach every branch of
    an epoch -> dict(indptr, indices, weights, y: numpy).  Row N // 2 is empty and row N // 2 + 1 has one edge
    (N >= 8); ``hub``: row 0 is joined to rows 1 .. hub (a list longer than any single pass of a lane group).
    Positions: uniform in [-10, 10]^2; some edges' endpoints coincide (d^2 = 0); some rows sit 1000 away from
    their neighbours (d^2 about 1e6, the clip inactive); and the first negative of some rows, known from
    (seed, row, epoch), is placed at 0.9, 1.0 and 1.1 times the distance where the repulsive step is 4."""
    from spmf_amd import graph
    rng = np.random.default_rng(4100 + N + hub)
    pairs = set()
    want = 6 * N if N >= 8 else N * (N - 1) // 2
    while len(pairs) < want:
        i, j = (int(v) for v in rng.integers(0, N, size=2))
        if i != j:
            pairs.add((min(i, j), max(i, j)))
    pairs |= {(0, j) for j in range(1, hub + 1)}
    if N >= 8:
        e, one = N // 2, N // 2 + 1
        pairs = {p for p in pairs if e not in p and one not in p} | {(one, N - 1) if one != N - 1 else (0, one)}
    und = np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2)
    wts = rng.uniform(0.05, 1.0, size=len(und)).astype(np.float32)
    rows = np.concatenate([und[:, 0], und[:, 1]])
    cols = np.concatenate([und[:, 1], und[:, 0]])
    order = np.argsort(rows * N + cols, kind="stable")
    rows, cols, w = rows[order], cols[order], np.concatenate([wts, wts])[order]
    indptr = np.searchsorted(rows, np.arange(N + 1)).astype(np.int64)
    y = rng.uniform(-10, 10, size=(N, 2)).astype(np.float32)
    if N >= 8:
        picks = rng.choice(len(und), size=min(6, len(und)), replace=False)
        for p in picks[:3]:
            y[und[p, 1]] = y[und[p, 0]]                       # coincident endpoints
        for p in picks[3:]:
            y[und[p, 1]] = y[und[p, 0]] + np.float32(1000.0)  # d^2 = 2e6
        neg = graph.negatives(N, epoch, M, seed)
        d4 = clip_distance(a, b)
        moved = set(int(v) for p in picks for v in und[p])
        for t, i in enumerate(int(v) for v in rng.choice(N, size=min(9, N), replace=False)):
            r = int(neg[i, 0])
            if r != i and r not in moved and i not in moved:
                y[r] = y[i] + np.array([d4 * (0.9, 1.0, 1.1)[t % 3], 0.0], dtype=np.float32)
                moved |= {i, r}
    return dict(indptr=indptr, indices=cols.astype(np.int32), weights=w, y=y)


def restate32(indptr, indices, weights, y, epoch, total_epochs, lr, a, b, gamma, rate, M, seed):
    """One epoch of include/spmf_hip.h spmf_graph_layout in float32 numpy on a clean graph (every entry valid,
    every position finite): the formulas of the kernel in its number format, the sums sequential in list order.
    What the error bar of the GPU test is measured with."""
    from spmf_amd import graph
    f = np.float32
    y = np.asarray(y, dtype=f)
    n = y.shape[0]
    row = np.repeat(np.arange(n), np.diff(indptr))
    col, w = np.asarray(indices, dtype=np.int64), np.asarray(weights, dtype=f)
    alpha = f(float(lr) * (1.0 - epoch / float(total_epochs)))
    a32, b32, neg2b, tgb, rom = f(a), f(b), f(-2.0 * b), f(2.0 * gamma * b), f(rate / M)

    def terms(i, j, coef):
        d = y[i] - y[j]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        live = d2 > 0
        s = np.where(live, d2, f(1))
        q = np.minimum(a32 * np.exp2(b32 * np.log2(s)), f(2.0 ** 60))
        c = np.where(live, coef(s, q), f(0))
        return np.clip(c[:, None] * d, f(-4), f(4)).astype(f)
    W = np.zeros(n, dtype=f)
    np.add.at(W, row, w)
    F = np.zeros((n, 2), dtype=f)
    np.add.at(F, row, w[:, None] * terms(row, col, lambda s, q: neg2b * q / (s * (f(1) + q))))
    neg = graph.negatives(n, epoch, M, seed)
    i_, r_ = np.repeat(np.arange(n), M), neg.reshape(-1)
    t = terms(i_, r_, lambda s, q: tgb / ((f(0.001) + s) * (f(1) + q)))
    t[r_ == i_] = 0
    G = np.zeros((n, 2), dtype=f)
    np.add.at(G, i_, t)
    out = y.copy()
    mv = W > 0
    step = (alpha / np.maximum(f(1), W)).astype(f)
    out[mv] = (y + step[:, None] * (F + (rom * W)[:, None] * G))[mv]
    return out


def error_units(got, ref, y, alpha, A, W):
    """max over the rows of |got - ref|_inf / (2^-24 (|y_i|_inf + alpha A_i / max(1, W_i))): the error in units
    of the per-row bar of the one-epoch tests."""
    scale = 2.0 ** -24 * (np.abs(np.asarray(y, dtype=np.float64)).max(1) + alpha * A / np.maximum(1.0, W))
    err = np.abs(np.asarray(got, dtype=np.float64) - ref).max(1)
    ok = scale > 0
    assert (err[~ok] == 0).all()
    return float((err[ok] / scale[ok]).max()) if ok.any() else 0.0
