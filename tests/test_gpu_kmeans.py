"""GPU tests of k-means: the Lloyd step of the library (spmf_kmeans_step, csrc/kmeans.hip behind csrc/knn.hip and
the ordering of csrc/groups.hip) and the methods on top of it (PoissonFactorization.kmeans / cluster,
spmf_amd/cluster.py).

The step is held against three references, all from the fp32 inputs alone:
  * ``knn``: labels and distances are the first column of ``knn(centroids, k=min(4, G), queries=points)``, bit for
    bit (the distances through their int32 view);
  * fp64 numpy: counts exact; every entry of ``sums`` within n_g * 2^-52 * sum_{i in g} |x_ik| of the sum in
    extended precision -- the worst case of a sequential fp64 sum of n_g terms is (n_g - 1) * 2^-53 times that
    sum of magnitudes, so the bar leaves a factor 2; ``stats[0]`` within the same bar of the sum of the returned
    fp32 distances squared; ``stats[1]`` and ``stats[2]`` exact;
  * the fp64 argmin with the bar of tests/test_gpu_knn.py, bar_ig = 2e-5 (|x'_i|^2 + |c'_g|^2) on the centred
    rows: a row is clear-cut when its two smallest fp64 d^2 differ by more than 2 max(bar); on clear-cut rows the
    label is the fp64 argmin, on every row d^2(label) <= min d^2 + 2 bar, and at least 95 % of the rows of every
    random case are clear-cut (asserted, so that no case hides behind the condition).
Shapes: the smallest at which the kernels can go wrong -- N in {1, 63, 65, 130, 300}, G in {1, 2, 3, 5, 64, 65,
130}, widths {1, 3, 8, 16, 33, 100, 256} (every padded width), each value once; 64 rows against 2 600 centroids
(reference slices and the merge); 300 rows against 10 centroids shifted by 50 (the centring).
"""
import functools

import numpy as np
import pytest
import torch

from _problems import _dense_model
from _stream_cases import _problem, assert_kmeans_errors, kmeans_raw_call

pytestmark = pytest.mark.gpu
T = torch.as_tensor

# (N, G, width, shift)
CASES = [(1, 3, 8, 0.0), (63, 1, 3, 0.0), (65, 2, 1, 0.0), (130, 65, 16, 0.0), (300, 5, 33, 0.0),
         (300, 130, 100, 0.0), (130, 64, 256, 0.0), (64, 2600, 8, 0.0), (300, 10, 8, 50.0)]


def _bits(t):
    return t.view(torch.int32)


@functools.lru_cache(maxsize=None)
def _model():
    from spmf_amd import PoissonFactorization
    return PoissonFactorization(latent_dim=3, feature_dim=8, initialize_distributions=False, device="cuda")


def _step(x, cent, prev=None, dist=True):
    """One raw spmf_kmeans_step on device tensors, in an exactly sized scratch -> dict of device tensors."""
    from spmf_amd import _lib
    lib, h = _lib.load(), _model()._handle()
    N, W, G = int(x.shape[0]), int(x.shape[1]), int(cent.shape[0])
    need = int(lib.spmf_kmeans_scratch_bytes(h, N, G, W))
    assert need > 0 and need % 256 == 0
    scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    out = {"labels": torch.full((N,), -7, dtype=torch.int32, device="cuda"),
           "distances": torch.full((N,), -7.0, dtype=torch.float32, device="cuda"),
           "sums": torch.full((G, W), -7.0, dtype=torch.float64, device="cuda"),
           "counts": torch.full((G,), -7, dtype=torch.int64, device="cuda"),
           "stats": torch.full((3,), -7.0, dtype=torch.float64, device="cuda")}
    _lib.check(h, lib.spmf_kmeans_step(
        h, x.data_ptr(), N, W, cent.data_ptr(), G, prev.data_ptr() if prev is not None else None,
        out["labels"].data_ptr(), out["distances"].data_ptr() if dist else None, out["sums"].data_ptr(),
        out["counts"].data_ptr(), out["stats"].data_ptr(), scratch.data_ptr() + (-scratch.data_ptr()) % 256, need,
        torch.cuda.current_stream().cuda_stream), "spmf_kmeans_step")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _inputs(N, G, W, shift):
    """Seeded standard-normal points (+ shift) and G centroids: rows of the points where there are enough of them,
    else draws of their own."""
    rng = np.random.default_rng(8100 + N + 7 * G + W)
    X = (rng.standard_normal((N, W)) + shift).astype(np.float32)
    if G <= N:
        Cn = X[rng.choice(N, size=G, replace=False)].copy()
    else:
        Cn = (rng.standard_normal((G, W)) + shift).astype(np.float32)
    return X, Cn


def _oracle(X, Cn):
    """fp64 from the fp32 inputs: d2 and bar of every pair, the candidates, per row the argmin and clear-cut."""
    x, c = X.astype(np.float64), Cn.astype(np.float64)
    x_ok, c_ok = np.isfinite(x).all(1), np.isfinite(c).all(1)
    ctr = c[c_ok].mean(0) if c_ok.any() else np.zeros(c.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        xw, cw = x - ctr, c - ctr
        d2 = np.zeros((len(x), len(c)))
        for k in range(x.shape[1]):
            d2 += (x[:, k][:, None] - c[:, k][None, :]) ** 2
        bar = 2e-5 * ((xw * xw).sum(1)[:, None] + (cw * cw).sum(1)[None, :])
    cand = x_ok[:, None] & c_ok[None, :]
    key = np.where(cand, d2, np.inf)
    order = np.argsort(key, axis=1, kind="stable")
    rows = np.arange(len(x))
    j0 = order[:, 0]
    nc = cand.sum(1)
    if len(c) > 1:
        j1 = order[:, 1]
        with np.errstate(invalid="ignore"):
            gap = key[rows, j1] - key[rows, j0]
            edge = 2 * np.maximum(bar[rows, j0], bar[rows, j1])
            clear = (nc <= 1) | (gap > edge)
    else:
        clear = np.ones(len(x), dtype=bool)
    return dict(d2=d2, bar=bar, cand=cand, nc=nc, argmin=np.where(nc > 0, j0, -1), clear=clear)


def _check_sums(X, labels, out, tag):
    """counts exact, sums and stats[0] / stats[2] against fp64 from the returned labels and distances."""
    G, W = out["sums"].shape
    lab = labels.astype(np.int64)
    counts = out["counts"].cpu().numpy()
    sums = out["sums"].cpu().numpy()
    np.testing.assert_array_equal(counts, np.bincount(lab[lab >= 0], minlength=G), err_msg=tag)
    worst = 0.0
    for g in range(G):
        xg = X[lab == g].astype(np.longdouble)
        ref = xg.sum(0)
        bound = len(xg) * 2.0 ** -52 * np.abs(xg).sum(0)
        err = np.abs(sums[g].astype(np.longdouble) - ref)
        assert (err <= bound).all(), (tag, g, float(err.max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if len(xg) else 0.0)
    print(f"{tag}: largest |sums - ref| / bound {worst:.3e}")
    stats = out["stats"].cpu().numpy()
    d = out["distances"].cpu().numpy().astype(np.longdouble)[lab >= 0]
    ref0 = (d * d).sum()
    err0 = abs(np.longdouble(stats[0]) - ref0)
    print(f"{tag}: |stats[0] - ref| {float(err0):.3e} of {float(ref0):.6e}")
    assert err0 <= len(d) * 2.0 ** -52 * ref0, (tag, float(err0))
    assert stats[2] == (lab < 0).sum(), tag


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"N{c[0]}_G{c[1]}_W{c[2]}_s{c[3]:g}")
def test_step_against_knn_fp64_sums_and_the_fp64_argmin(case):
    N, G, W, shift = case
    X, Cn = _inputs(*case)
    x, c = T(X).cuda(), T(Cn).cuda()
    out = _step(x, c)
    tag = f"N={N} G={G} W={W} shift={shift:g}"
    # knn, bit for bit
    ref = _model().knn(c, k=min(4, G), queries=x)
    assert torch.equal(out["labels"], ref["indices"][:, 0].contiguous()), tag
    assert torch.equal(_bits(out["distances"]), _bits(ref["distances"][:, 0].contiguous())), tag
    labels = out["labels"].cpu().numpy()
    assert ((labels >= 0) & (labels < G)).all(), tag
    # fp64 sums and statistics
    _check_sums(X, labels, out, tag)
    assert out["stats"][1].item() == N, (tag, "prev_labels NULL: every row counts as changed")
    # the fp64 argmin
    o = _oracle(X, Cn)
    share = o["clear"].mean()
    print(f"{tag}: clear-cut rows {int(o['clear'].sum())}/{N}")
    assert share >= 0.95, (tag, share)
    assert (labels[o["clear"]] == o["argmin"][o["clear"]]).all(), (tag, "label on clear-cut rows")
    rows = np.arange(N)
    slack = 2 * np.maximum(o["bar"][rows, labels], o["bar"][rows, o["argmin"]])
    assert (o["d2"][rows, labels] <= o["d2"][rows, o["argmin"]] + slack).all(), (tag, "a nearer centroid was missed")
    dref = np.sqrt(o["d2"][rows, labels])
    assert (np.abs(out["distances"].cpu().numpy() - dref) <= 1e-5 * dref).all(), tag


def test_changed_count_and_a_null_distance_output():
    N, G, W, shift = CASES[4]
    X, Cn = _inputs(*CASES[4])
    x, c = T(X).cuda(), T(Cn).cuda()
    first = _step(x, c)
    same = _step(x, c, prev=first["labels"])
    assert same["stats"][1].item() == 0 and torch.equal(same["labels"], first["labels"])
    prev = first["labels"].clone()
    moved = torch.tensor([0, 63, 64, 255, 256, 299], device="cuda")
    prev[moved] = (prev[moved] + 1) % G
    prev[7] = -1
    out = _step(x, c, prev=prev, dist=False)
    assert out["stats"][1].item() == 7
    assert bool((out["distances"] == -7).all()), "dist_out NULL: nothing is written"
    for key in ("labels", "counts"):
        assert torch.equal(out[key], first[key]), key
    assert torch.equal(out["sums"].view(torch.int64), first["sums"].view(torch.int64))
    assert torch.equal(out["stats"][:1].view(torch.int64), first["stats"][:1].view(torch.int64))


def test_exact_ties_go_to_the_smaller_index():
    # lattice points midway between centroids 1 and 2 (and far from 0 and 3): equal fp32 distances
    cent = np.array([[40, 40, 0], [0, 0, 0], [2, 0, 0], [-40, 7, 1]], dtype=np.float32)
    ys = np.arange(-6, 7)
    X = np.array([[1, y, z] for y in ys for z in (-2, 0, 3)], dtype=np.float32)
    out = _step(T(X).cuda(), T(cent).cuda())
    assert bool((out["labels"] == 1).all())
    nn = _model().knn(T(cent).cuda(), k=4, queries=T(X).cuda())
    assert nn["indices"][:, :2].tolist() == [[1, 2]] * len(X)
    assert torch.equal(_bits(nn["distances"][:, 0]), _bits(nn["distances"][:, 1])), "the distances are equal in fp32"
    want = np.sqrt((X.astype(np.float64) ** 2).sum(1))
    np.testing.assert_allclose(out["distances"].cpu().numpy(), want, rtol=1e-6)
    assert out["counts"].tolist() == [0, len(X), 0, 0]
    # duplicated centroids: the later one stays empty
    Xr, Cr = _inputs(*CASES[4])
    Cd = Cr.copy()
    Cd[4] = Cd[1]
    Cd[3] = Cd[0]
    out = _step(T(Xr).cuda(), T(Cd).cuda())
    labels = out["labels"].cpu().numpy()
    assert not np.isin(labels, (3, 4)).any() and out["counts"][3].item() == 0 and out["counts"][4].item() == 0
    assert bool((out["sums"][3:5] == 0).all())
    assert (labels == 0).any() and (labels == 1).any()


def test_non_finite_rows_and_centroids():
    N, G, W, shift = CASES[4]
    X, Cn = _inputs(*CASES[4])
    X, Cn = X.copy(), Cn.copy()
    bad = [0, 64, 130, 299]
    X[0, 5] = np.nan
    X[64] = np.inf
    X[130, 32] = -np.inf
    X[299, 0] = np.nan
    Cn[2, 7] = np.nan
    out = _step(T(X).cuda(), T(Cn).cuda())
    labels = out["labels"].cpu().numpy()
    assert (labels[bad] == -1).all() and np.isposinf(out["distances"].cpu().numpy()[bad]).all()
    keep = np.setdiff1d(np.arange(N), bad)
    assert (labels[keep] >= 0).all() and not (labels == 2).any(), "a NaN centroid is never chosen"
    assert out["stats"][2].item() == 4 and out["counts"].sum().item() == N - 4 and out["counts"][2].item() == 0
    _check_sums(X, labels, out, "non-finite rows")
    o = _oracle(X, Cn)
    assert (labels[o["clear"]] == o["argmin"][o["clear"]]).all()
    # a finite row's result does not depend on the non-finite ones
    clean = _step(T(X[keep]).cuda(), T(Cn).cuda())
    assert torch.equal(clean["labels"], out["labels"][T(keep).cuda()])
    assert torch.equal(_bits(clean["distances"]), _bits(out["distances"][T(keep).cuda()]))
    # all centroids NaN
    out = _step(T(X).cuda(), torch.full((G, W), float("nan"), device="cuda"))
    assert bool((out["labels"] == -1).all()) and bool(torch.isposinf(out["distances"]).all())
    assert bool((out["sums"] == 0).all()) and bool((out["counts"] == 0).all())
    assert out["stats"].tolist() == [0.0, float(N), float(N)]


def test_bit_properties():
    case = CASES[5]
    N, G, W, shift = case
    X, Cn = _inputs(*case)
    x, c = T(X).cuda(), T(Cn).cuda()
    a, b = _step(x, c), _step(x, c)
    for key in ("labels", "counts"):
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(_bits(a["distances"]), _bits(b["distances"]))
    for key in ("sums", "stats"):
        assert torch.equal(a[key].view(torch.int64), b[key].view(torch.int64)), (key, "two calls, the same bits")
    # a permutation of the rows
    perm = np.random.default_rng(3).permutation(N)
    p = _step(T(X[perm]).cuda(), c)
    pc = T(perm).cuda()
    assert torch.equal(p["labels"], a["labels"][pc]) and torch.equal(_bits(p["distances"]), _bits(a["distances"][pc]))
    assert torch.equal(p["counts"], a["counts"])
    _check_sums(X[perm], p["labels"].cpu().numpy(), p, "permuted rows")
    # a row alone
    for i in (0, 64, 299):
        one = _step(x[i:i + 1].contiguous(), c)
        assert one["labels"].item() == a["labels"][i].item(), i
        assert _bits(one["distances"]).item() == _bits(a["distances"])[i].item(), i


def test_raw_errors_leave_the_outputs_untouched_and_no_rows_zero_fill():
    from spmf_amd import _lib
    lib, h = _lib.load(), _model()._handle()
    N, G, W = 70, 5, 33
    X, Cn = _inputs(N, G, W, 0.0)
    x, c = T(X).cuda(), T(Cn).cuda()
    need = int(lib.spmf_kmeans_scratch_bytes(h, N, G, W))
    scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    outs = {"labels": torch.full((N,), -7, dtype=torch.int32, device="cuda"),
            "dist": torch.full((N,), -7.0, dtype=torch.float32, device="cuda"),
            "sums": torch.full((G, W), -7.0, dtype=torch.float64, device="cuda"),
            "counts": torch.full((G,), -7, dtype=torch.int64, device="cuda"),
            "stats": torch.full((3,), -7.0, dtype=torch.float64, device="cuda")}
    prev = torch.zeros(N, dtype=torch.int32, device="cuda")
    good = dict(h=h, x=x.data_ptr(), n=N, row_len=W, cent=c.data_ptr(), G=G, prev=prev.data_ptr(),
                ptr=scratch.data_ptr() + (-scratch.data_ptr()) % 256, nbytes=need,
                stream=torch.cuda.current_stream().cuda_stream, **{k: v.data_ptr() for k, v in outs.items()})
    call = kmeans_raw_call(good)

    def untouched():
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in outs.values()) and not bool(scratch.any())
    assert_kmeans_errors(lib, good, need, after=untouched)
    # no rows: the zero fills, and nothing else
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((outs["sums"] == 0).all()) and bool((outs["counts"] == 0).all()) and bool((outs["stats"] == 0).all())
    assert bool((outs["labels"] == -7).all()) and bool((outs["dist"] == -7).all()) and not bool(scratch.any())
    # and the valid call is the step
    assert call() == 0
    torch.cuda.synchronize()
    want = _step(x, c, prev=prev)
    assert torch.equal(outs["labels"], want["labels"]) and torch.equal(_bits(outs["dist"]), _bits(want["distances"]))
    assert torch.equal(outs["sums"].view(torch.int64), want["sums"].view(torch.int64))
    assert torch.equal(outs["counts"], want["counts"])


# ---- kmeans ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _blobs():
    """Six blobs of 100 points in 8 dimensions, centres N(0, 10^2), unit noise, shuffled; one true member per
    blob as the init; the fp64 Lloyd iteration from it: the labels of every step and the least relative gap
    between the nearest and the second-nearest centroid, (d2_second - d2_first) / d2_second on the squared
    distances the selection compares.  The seed is one at which that gap, a property of the fp64 iteration alone,
    reaches 0.95."""
    rng = np.random.default_rng(29)
    centres = 10.0 * rng.standard_normal((6, 8))
    truth = rng.permutation(np.repeat(np.arange(6), 100))
    X = (centres[truth] + rng.standard_normal((600, 8))).astype(np.float32)
    init = np.stack([X[np.flatnonzero(truth == g)[0]] for g in range(6)])
    x, c = X.astype(np.float64), init.astype(np.float64)
    steps, gap = [], np.inf
    for _ in range(5):
        d = ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1)
        two = np.sort(d, axis=1)[:, :2]
        gap = min(gap, float(((two[:, 1] - two[:, 0]) / two[:, 1]).min()))
        lab = d.argmin(1)
        if steps and (lab == steps[-1]).all():
            break
        steps.append(lab)
        c = np.stack([x[lab == g].mean(0) for g in range(6)])
    return X, truth, init, steps, gap, c


def test_kmeans_on_blobs_follows_the_fp64_iteration():
    X, truth, init, steps, gap, means = _blobs()
    print(f"fp64 Lloyd: {len(steps)} labellings, least relative gap {gap:.3f}")
    assert gap >= 0.95 and len(steps) == 1 and (steps[0] == truth).all(), "the fp64 iteration itself"
    m = _model()
    x, c0 = T(X).cuda(), T(init).cuda()
    res = m.kmeans(x, 6, init=c0)
    assert res["converged"] is True and res["n_iter"] == 2 and res["n_unassigned"] == 0
    assert res["labels"].dtype == torch.int32 and res["distances"].dtype == torch.float32
    assert res["centroids"].dtype == torch.float32 and res["counts"].dtype == torch.int64
    np.testing.assert_array_equal(res["labels"].cpu().numpy(), truth)
    assert res["counts"].tolist() == [100] * 6
    want = means.astype(np.float32)
    got = res["centroids"].cpu().numpy()
    assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all(), float(np.abs(got - want).max())
    cen = got.astype(np.float64)
    ref = ((X.astype(np.float64) - cen[truth]) ** 2).sum()
    assert abs(res["inertia"] - ref) <= 1e-5 * ref, (res["inertia"], ref)
    # every output refers to the returned centroids
    nn = m.knn(res["centroids"], k=4, queries=x)
    assert torch.equal(res["labels"], nn["indices"][:, 0].contiguous())
    assert torch.equal(_bits(res["distances"]), _bits(nn["distances"][:, 0].contiguous()))
    # bit-reproducible
    again = m.kmeans(x, 6, init=c0)
    assert torch.equal(_bits(again["centroids"]), _bits(res["centroids"])) and again["inertia"] == res["inertia"]
    # max_iter = 1: the labels of the init, not converged, the init returned
    one = m.kmeans(x, 6, init=c0, max_iter=1)
    assert one["converged"] is False and one["n_iter"] == 1
    assert torch.equal(_bits(one["centroids"]), _bits(c0))
    np.testing.assert_array_equal(one["labels"].cpu().numpy(), steps[0])
    nn = m.knn(c0, k=4, queries=x)
    assert torch.equal(one["labels"], nn["indices"][:, 0].contiguous())
    # 'first': the first six rows
    f = m.kmeans(x, 6, init="first", max_iter=1)
    assert torch.equal(_bits(f["centroids"]), _bits(x[:6]))


def test_kmeans_loop_with_large_centroid_arrays_matches_step_by_step():
    """G * width large enough (2 048 x 256: 4 MiB in fp64) that the update's temporaries and the new centroids are
    allocations of the size class of the call's scratch: the loop must own its scratch across the iterations, or a
    later step prepares its working rows over the centroids it reads.  The reference is the same iteration spelled
    out step by step, every step in a scratch of its own that lives through it."""
    from spmf_amd.cluster import update_centroids
    N, G, W, iters = 4096, 2048, 256, 3
    x = torch.randn(N, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(12))
    m = _model()
    a = m.kmeans(x, G, init="first", max_iter=iters)
    b = m.kmeans(x, G, init="first", max_iter=iters)
    assert a["n_iter"] >= 2, "several steps, each behind an update"
    for key in ("labels", "counts"):
        assert torch.equal(a[key], b[key]), key
    for key in ("distances", "centroids"):
        assert torch.equal(_bits(a[key]), _bits(b[key])), (key, "two runs, the same bits")
    assert a["inertia"] == b["inertia"]
    nn = m.knn(a["centroids"], k=4, queries=x)
    assert torch.equal(a["labels"], nn["indices"][:, 0].contiguous())
    assert torch.equal(_bits(a["distances"]), _bits(nn["distances"][:, 0].contiguous()))
    cent, prev = x[:G].contiguous(), None
    for it in range(iters):
        out = _step(x, cent, prev=prev)
        if out["stats"][1].item() == 0:
            break
        if it + 1 < iters:
            cent, prev = update_centroids(out["sums"], out["counts"], cent).contiguous(), out["labels"]
    assert torch.equal(_bits(a["centroids"]), _bits(cent)), "the centroids of the step-by-step iteration"
    assert torch.equal(a["labels"], out["labels"]) and torch.equal(a["counts"], out["counts"])
    assert a["inertia"] == out["stats"][0].item() and a["n_iter"] == it + 1


def test_kmeans_keeps_the_centroid_of_an_empty_cluster():
    X, truth, init, _, _, means = _blobs()
    far = np.full((1, 8), 1e3, dtype=np.float32)
    c0 = T(np.concatenate([init[:3], far, init[3:]])).cuda()
    res = _model().kmeans(T(X).cuda(), 7, init=c0)
    assert res["converged"] and res["counts"][3].item() == 0 and res["counts"].sum().item() == 600
    assert torch.equal(_bits(res["centroids"][3]), _bits(c0[3]))
    lab = res["labels"].cpu().numpy()
    np.testing.assert_array_equal(np.where(lab > 3, lab - 1, lab), truth)


def test_kmeans_plus_plus_centres():
    from spmf_amd.cluster import init_plus_plus
    X = _blobs()[0].copy()
    X[5, 2] = np.nan
    X[17] = np.inf
    x = T(X).cuda()
    c = init_plus_plus(x, 20, seed=11)
    assert c.is_cuda and c.dtype == torch.float32 and tuple(c.shape) == (20, 8) and bool(torch.isfinite(c).all())
    rows = [np.flatnonzero((X == r).all(1)) for r in c.cpu().numpy()]
    assert all(len(r) == 1 for r in rows), "every centre is a row of the points"
    assert len({int(r[0]) for r in rows}) == 20, "distinct points give distinct centres"
    assert torch.equal(_bits(init_plus_plus(x, 20, seed=11)), _bits(c))
    m = _model()
    a, b = m.kmeans(x, 6, seed=3), m.kmeans(x, 6, seed=3)
    assert a["n_unassigned"] == 2 and a["labels"][5].item() == -1 and a["labels"][17].item() == -1
    assert torch.equal(a["labels"], b["labels"]) and torch.equal(_bits(a["centroids"]), _bits(b["centroids"]))
    with pytest.raises(ValueError, match="finite"):
        m.kmeans(torch.full((4, 2), float("nan"), device="cuda"), 2)


# ---- cluster -----------------------------------------------------------------------------------

def test_cluster_is_kmeans_of_embed():
    case = ("poisson", 70, 45, 3, 2)
    lik, B, D, K, S = case
    cfg, x, params, mask, _ = _problem(*case)
    m = _dense_model(lik, cfg, mask, 32)
    e = m.embed({"counts": x}, draws=params)["mean"]
    want = m.kmeans(e, 3, init="first")
    split = [{"counts": np.ascontiguousarray(x[:30])}, {"counts": np.ascontiguousarray(x[30:])}]
    for data in ({"counts": x}, split):
        got = m.cluster(data, 3, draws=params, init="first")
        assert torch.equal(_bits(got["embedding"]), _bits(e))
        for key in ("labels", "counts"):
            assert torch.equal(got[key], want[key]), key
        for key in ("distances", "centroids"):
            assert torch.equal(_bits(got[key]), _bits(want[key])), key
        for key in ("inertia", "n_iter", "converged", "n_unassigned"):
            assert got[key] == want[key], key
    pp = m.cluster({"counts": x}, 4, draws=params, seed=5)
    ref = m.kmeans(e, 4, seed=5)
    assert torch.equal(pp["labels"], ref["labels"]) and torch.equal(_bits(pp["centroids"]), _bits(ref["centroids"]))
    from spmf_amd import PoissonFactorization
    c = PoissonFactorization(latent_dim=K, feature_dim=D, column_norms=cfg.eta_i, initialize_distributions=False,
                             device="cuda", encoder_function=lambda t: t, decoder_function=lambda t: t)
    with pytest.raises(NotImplementedError):
        c.cluster({"counts": x}, 3, draws=params)
