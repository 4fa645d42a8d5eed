"""GPU tests of the silhouette: the library call (spmf_silhouette, csrc/silhouette.hip behind the ordering of
csrc/groups.hip) and the method on top of it (PoissonFactorization.silhouette, also on the result of ``cluster``).

The reference is fp64 numpy from the fp32 inputs: the members (a label in [0, G), a finite row, under cosine a
positive norm), all pairs by squared differences (cosine: half the squared differences of the fp64 unit rows), the
centre as the fp64 mean of the members.

Bars (derived, not tuned).  The kernel forms u_ij = -(bias_i + (<x'_i, x'_j> + bias_j)) = 1/2 |x'_i - x'_j|^2 in
fp32 and d_ij = sqrtf(max(0, 2 u_ij)) (Euclidean) or max(0, u_ij) (cosine), the expression of the issue.
  Euclidean: e_ij = (KP + 32) * 2^-24 * (|x'_i|^2 + |x'_j|^2) is a worst-case forward bound on d^2: the length-KP
fp32 dot product (KP * 2^-24 |x'_i| |x'_j| <= KP * 2^-25 (|x'_i|^2 + |x'_j|^2), doubled by the factor 2 of d^2),
both biases (each a length-KP chain, (KP + 1) * 2^-24 * 1/2 |x'|^2, doubled), the three additions and the rounding
of the centring share the 32.  From d^2 to d: |sqrt(d^2 + e) - d| <= min(sqrt(e), e / d) =: delta_ij.
  Cosine: delta_ij = (KP + 32) * 2^-23 (unit rows: |x'|^2 = 1 in the bound above, and d is linear in u).
  |a - a_ref| <= mean_j delta_ij + 2^-23 a_ref (the fp64 mean's rounding to fp32 and the sqrt's), likewise b against
the reference's nearest cluster.  A row is clear-cut when its two smallest other-cluster means differ by more than
the sum of their bars: there ``nearest`` is the fp64 argmin; on every row mean(nearest) <= min + both bars.  A row
is conditioned when (Da + Db) / max(a_ref, b_ref) <= 1e-3: there |s - s_ref| <= 2 (Da + Db) / max(a_ref, b_ref) +
2^-23 (the first-order error of (b - a) / max(a, b), with a factor 2 for the denominator).  At least 95 % of the
scored rows of every case are clear-cut and conditioned (asserted: no case hides behind the conditions).
"""
import functools

import numpy as np
import pytest
import torch

from _problems import _dense_model
from _silhouette_cases import assert_silhouette_errors, silhouette_raw_call
from _stream_cases import _problem

pytestmark = pytest.mark.gpu
T = torch.as_tensor

# (N, G, width, shift, data, metric); data: "pair" (labels 0, 1), "random" (normal points, random labels), "blobs"
CASES = [(2, 2, 8, 0.0, "pair", "euclidean"), (63, 1, 3, 0.0, "random", "euclidean"),
         (65, 2, 1, 0.0, "random", "euclidean"), (130, 3, 16, 0.0, "blobs", "euclidean"),
         (300, 5, 33, 0.0, "blobs", "euclidean"), (300, 130, 100, 0.0, "random", "euclidean"),
         (130, 65, 256, 0.0, "random", "euclidean"), (200, 3, 8, 50.0, "blobs", "euclidean"),
         (257, 4, 64, 0.0, "blobs", "euclidean"), (300, 2, 16, 0.0, "blobs", "euclidean"),
         (2100, 7, 8, 0.0, "blobs", "euclidean"), (300, 5, 33, 0.0, "blobs", "cosine"),
         (130, 3, 3, 0.0, "random", "cosine")]


def _case_id(c):
    return f"N{c[0]}_G{c[1]}_W{c[2]}_s{c[3]:g}_{c[4]}_{c[5]}"


def _bits(t):
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


@functools.lru_cache(maxsize=None)
def _model():
    from spmf_amd import PoissonFactorization
    return PoissonFactorization(latent_dim=3, feature_dim=8, initialize_distributions=False, device="cuda")


@functools.lru_cache(maxsize=None)
def _inputs(N, G, W, shift, data, metric):
    """Seeded standard-normal points plus the shift, "blobs" plus 4 N(0, I) centres per label; random labels (every
    cluster of "blobs" and "pair" is met); for N >= 63, N / 20 rows get label -1."""
    rng = np.random.default_rng(9200 + N + 7 * G + W)
    if data == "pair":
        lab = np.arange(N) % G
    else:
        lab = rng.integers(0, G, size=N)
    X = rng.standard_normal((N, W)) + shift
    if data == "blobs":
        X = X + (4.0 * rng.standard_normal((G, W)))[lab]
    lab = lab.astype(np.int32)
    if N >= 63:
        lab[rng.choice(N, size=N // 20, replace=False)] = -1
    return X.astype(np.float32), lab


def _padded(W):
    kp = 4
    while kp < W:
        kp *= 2
    return kp


def _reference(X, lab, G, metric):
    """fp64 from the fp32 inputs -> dict: members, counts, per member a, b, nearest, s, their bars, clear-cut and
    conditioned; M / DB [N, G]: the mean distance to every cluster and its bar."""
    x = X.astype(np.float64)
    N, W = x.shape
    KP = _padded(W)
    lab = lab.astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        member = (lab >= 0) & (lab < G) & np.isfinite(x).all(1)
        if metric == "cosine":
            nrm = np.sqrt((x * x).sum(1))
            member &= np.isfinite(nrm) & (nrm > 0)
    idx = np.flatnonzero(member)
    xm, lm = x[idx], lab[idx]
    n = len(idx)
    if metric == "cosine":
        w = xm / np.sqrt((xm * xm).sum(1))[:, None]
    else:
        w = xm - (xm.mean(0) if n else 0.0)
    d2 = np.zeros((n, n))
    for k in range(W):
        d2 += (w[:, k][:, None] - w[:, k][None, :]) ** 2
    if metric == "cosine":
        D = 0.5 * d2
        delta = np.full((n, n), (KP + 32) * 2.0 ** -23)
    else:
        D = np.sqrt(d2)
        nn = (w * w).sum(1)
        e = (KP + 32) * 2.0 ** -24 * (nn[:, None] + nn[None, :])
        with np.errstate(divide="ignore"):
            delta = np.minimum(np.sqrt(e), e / D)
    np.fill_diagonal(D, 0.0)
    np.fill_diagonal(delta, 0.0)                           # d_ii is not added
    onehot = np.zeros((n, G))
    onehot[np.arange(n), lm] = 1.0
    counts = onehot.sum(0).astype(np.int64)
    S, DS = D @ onehot, delta @ onehot                     # [n, G] sums of distances / of bars
    rows = np.arange(n)
    ng = counts[lm]
    own = S[rows, lm]
    a = np.where(ng > 1, own / np.maximum(ng - 1, 1), 0.0)
    Da = np.where(ng > 1, DS[rows, lm] / np.maximum(ng - 1, 1), 0.0) + 2.0 ** -23 * a
    with np.errstate(invalid="ignore", divide="ignore"):
        M = np.where(counts[None, :] > 0, S / counts[None, :], np.inf)
        DB = np.where(counts[None, :] > 0, DS / counts[None, :] + 2.0 ** -23 * M, 0.0)
    other = M.copy()
    other[rows, lm] = np.inf
    order = np.argsort(other, axis=1, kind="stable")
    two = int((counts > 0).sum()) >= 2
    if two:
        h0 = order[:, 0]
        b, Db = other[rows, h0], DB[rows, h0]
        if G > 1:
            h1 = order[:, 1]
            clear = ~np.isfinite(other[rows, h1]) | (other[rows, h1] - b > Db + DB[rows, h1])
        else:
            clear = np.ones(n, dtype=bool)
        mx = np.maximum(a, b)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where((ng > 1) & (mx > 0), (b - a) / mx, 0.0)
            cond = (Da + Db) / mx
        cond = np.where(mx > 0, cond, 0.0)
    else:
        h0 = np.full(n, -1)
        b, Db = np.full(n, np.inf), np.zeros(n)
        clear = np.ones(n, dtype=bool)
        s = np.full(n, np.nan)
        cond = np.zeros(n)
    return dict(idx=idx, member=member, counts=counts, lab=lm, a=a, Da=Da, b=b, Db=Db, nearest=h0, s=s, clear=clear,
                cond=cond, M=M, DB=DB, two=two)


@functools.lru_cache(maxsize=None)
def _case_reference(case):
    X, lab = _inputs(*case)
    return _reference(X, lab, case[1], case[5])


def _raw(x, lab, G, metric="euclidean", a=True, b=True, nearest=True):
    """One raw spmf_silhouette on device tensors, in an exactly sized scratch -> dict of device tensors (sentinel
    -7 where the call writes nothing)."""
    from spmf_amd import _lib
    lib, h = _lib.load(), _model()._handle()
    N, W = int(x.shape[0]), int(x.shape[1])
    need = int(lib.spmf_silhouette_scratch_bytes(h, N, G, W))
    assert need > 0 and need % 256 == 0
    scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    out = {"silhouette": torch.full((N,), -7.0, dtype=torch.float32, device="cuda"),
           "a": torch.full((N,), -7.0, dtype=torch.float32, device="cuda"),
           "b": torch.full((N,), -7.0, dtype=torch.float32, device="cuda"),
           "nearest": torch.full((N,), -7, dtype=torch.int32, device="cuda"),
           "cluster_sum": torch.full((G,), -7.0, dtype=torch.float64, device="cuda"),
           "counts": torch.full((G,), -7, dtype=torch.int64, device="cuda")}
    _lib.check(h, lib.spmf_silhouette(
        h, x.data_ptr(), N, W, lab.data_ptr(), G, 1 if metric == "cosine" else 0, out["silhouette"].data_ptr(),
        out["a"].data_ptr() if a else None, out["b"].data_ptr() if b else None,
        out["nearest"].data_ptr() if nearest else None, out["cluster_sum"].data_ptr(), out["counts"].data_ptr(),
        scratch.data_ptr() + (-scratch.data_ptr()) % 256, need, torch.cuda.current_stream().cuda_stream),
        "spmf_silhouette")
    torch.cuda.synchronize()
    return out


def _check(tag, ref, N, G, out):
    """The assertions of the module's docstring on numpy outputs ``out`` (silhouette, a, b, nearest, cluster_sum,
    counts)."""
    idx, rows = ref["idx"], np.arange(len(ref["idx"]))
    non = ~ref["member"]
    for key in ("silhouette", "a", "b"):
        assert np.isnan(out[key][non]).all(), (tag, key, "a non-member is NaN")
    assert (out["nearest"][non] == -1).all(), tag
    np.testing.assert_array_equal(out["counts"], ref["counts"], err_msg=tag)
    s, a, b, near = (out[k][idx] for k in ("silhouette", "a", "b", "nearest"))
    a64, b64, s64 = a.astype(np.float64), b.astype(np.float64), s.astype(np.float64)
    # a
    err_a = np.abs(a64 - ref["a"])
    ratio_a = float((err_a / np.maximum(ref["Da"], 1e-300)).max()) if len(idx) else 0.0
    print(f"{tag}: largest |a - ref| / bar {ratio_a:.3e}")
    assert (err_a <= ref["Da"]).all(), (tag, "a", ratio_a)
    # the per-cluster sums against the returned s
    sums = out["cluster_sum"]
    if not ref["two"]:
        assert np.isposinf(b).all() and (near == -1).all() and np.isnan(s).all(), (tag, "fewer than two clusters")
        assert all(np.isnan(sums[g]) for g in range(G) if ref["counts"][g] > 0), tag
        assert all(sums[g] == 0 for g in range(G) if ref["counts"][g] == 0), tag
        return
    assert np.isfinite(s).all() and (s >= -1).all() and (s <= 1).all(), (tag, "s lies in [-1, 1]")
    assert ((near >= 0) & (near < G) & (near != ref["lab"])).all(), tag
    # b against the reference's nearest cluster
    err_b = np.abs(b64 - ref["b"])
    ratio_b = float((err_b / np.maximum(ref["Db"], 1e-300)).max())
    print(f"{tag}: largest |b - ref| / bar {ratio_b:.3e}")
    assert (err_b <= ref["Db"]).all(), (tag, "b", ratio_b)
    # nearest
    clear, cond = ref["clear"], ref["cond"] <= 1e-3
    print(f"{tag}: clear-cut rows {int(clear.sum())}/{len(idx)}, conditioned {int(cond.sum())}/{len(idx)}, largest "
          f"(Da + Db) / max(a, b) {float(ref['cond'].max()):.3e}")
    assert clear.mean() >= 0.95 and cond.mean() >= 0.95, (tag, clear.mean(), cond.mean())
    assert (near[clear] == ref["nearest"][clear]).all(), (tag, "nearest on clear-cut rows")
    assert (ref["M"][rows, near] <= ref["b"] + ref["DB"][rows, near] + ref["Db"]).all(), (tag, "a nearer cluster")
    # s
    err_s = np.abs(s64 - ref["s"])[cond]
    bar_s = (2 * ref["cond"] + 2.0 ** -23)[cond]
    ratio_s = float((err_s / bar_s).max())
    print(f"{tag}: largest |s - ref| / bar {ratio_s:.3e}")
    assert (err_s <= bar_s).all(), (tag, "s", ratio_s)
    single = ref["counts"][ref["lab"]] == 1
    assert (s[single] == 0).all() and (a[single] == 0).all(), (tag, "a singleton cluster")
    # the clusters' sums: sequential fp64 sums of n_g terms, and the rounding of every returned s to fp32
    worst = 0.0
    for g in range(G):
        sg = s[ref["lab"] == g].astype(np.longdouble)
        bound = len(sg) * 2.0 ** -52 * float(np.abs(sg).sum()) + len(sg) * 2.0 ** -24
        err = abs(float(np.longdouble(sums[g]) - sg.sum()))
        assert err <= bound, (tag, g, err, bound)
        worst = max(worst, err / bound if bound else 0.0)
    print(f"{tag}: largest |cluster_sum - sum of s| / bound {worst:.3e}")


def _numpy(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_call_against_fp64(case):
    N, G, W, shift, data, metric = case
    X, lab = _inputs(*case)
    ref = _case_reference(case)
    out = _raw(T(X).cuda(), T(lab).cuda(), G, metric)
    _check(_case_id(case), ref, N, G, _numpy(out))
    # the method: the same bits, the clusters' means and a score consistent with the sums
    res = _model().silhouette(T(X).cuda(), lab, G, metric=metric)
    for key in ("silhouette", "a", "b"):
        assert res[key].dtype == torch.float32 and torch.equal(_bits(res[key]), _bits(out[key])), key
    assert res["nearest"].dtype == torch.int32 and torch.equal(res["nearest"], out["nearest"])
    assert res["counts"].dtype == torch.int64 and torch.equal(res["counts"], out["counts"])
    assert res["n_scored"] == int(ref["counts"].sum())
    sums, counts = out["cluster_sum"].cpu().numpy(), ref["counts"]
    mean = res["cluster_mean"].cpu().numpy()
    assert res["cluster_mean"].dtype == torch.float64 and np.isnan(mean[counts == 0]).all()
    np.testing.assert_allclose(mean[counts > 0], sums[counts > 0] / counts[counts > 0], rtol=2.0 ** -51, atol=0)
    if ref["two"]:
        want = float(sums.astype(np.longdouble).sum()) / counts.sum()
        assert abs(res["score"] - want) <= G * 2.0 ** -52 * np.abs(sums).sum() / counts.sum(), (res["score"], want)
        assert abs(res["score"] - ref["s"].mean()) <= 2 * float(ref["cond"].max()) + 2.0 ** -22
    else:
        assert np.isnan(res["score"])


def test_two_singletons_and_the_hand_case():
    out = _numpy(_raw(*(T(v).cuda() for v in _inputs(*CASES[0])), 2))
    assert (out["silhouette"] == 0).all() and (out["a"] == 0).all() and out["nearest"].tolist() == [1, 0]
    assert out["counts"].tolist() == [1, 1] and out["cluster_sum"].tolist() == [0.0, 0.0]
    # points 0, 1, 10, 11 on a line
    x = T(np.array([[0.0], [1.0], [10.0], [11.0]], dtype=np.float32)).cuda()
    res = _model().silhouette(x, np.array([0, 0, 1, 1]))
    np.testing.assert_allclose(res["a"].cpu().numpy(), [1, 1, 1, 1], rtol=0, atol=1e-6)
    np.testing.assert_allclose(res["b"].cpu().numpy(), [10.5, 9.5, 9.5, 10.5], rtol=0, atol=1e-6)
    np.testing.assert_allclose(res["silhouette"].cpu().numpy(), [19 / 21, 17 / 19, 17 / 19, 19 / 21], rtol=0, atol=1e-6)
    assert res["nearest"].tolist() == [1, 1, 0, 0] and res["counts"].tolist() == [2, 2] and res["n_scored"] == 4
    assert abs(res["score"] - (19 / 21 + 17 / 19) / 2) <= 1e-6
    np.testing.assert_allclose(res["cluster_mean"].cpu().numpy(), [(19 / 21 + 17 / 19) / 2] * 2, rtol=0, atol=1e-6)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_non_members_are_excluded_bit_for_bit(metric):
    """Non-finite rows with a label >= 0, label -1 and the raw labels G and -5 are non-members; dropping them all
    from the input leaves every other row's outputs and both per-cluster outputs bit-identical: the test of the
    exclusion and of the members-only centre."""
    case = CASES[4]
    N, G, W = case[:3]
    X, lab = (v.copy() for v in _inputs(*case))
    assert (lab == -1).sum() == N // 20
    X[0, 5] = np.nan
    X[64] = np.inf
    X[130, 32] = -np.inf
    X[299, 0] = np.nan
    X[77] = 1e30                                           # finite, far away, and labelled out of range below
    lab[[0, 64, 130, 299]] = [1, 2, 0, 4]
    lab[77], lab[78], lab[200] = G, -5, G + 1000
    if metric == "cosine":
        X[150] = 0.0                                       # a zero row has no direction
        lab[150] = 3
    bad = [0, 64, 130, 299, 77, 78, 200] + ([150] if metric == "cosine" else [])
    non = np.zeros(N, dtype=bool)
    non[bad] = True
    non |= lab == -1
    ref = _reference(X, lab, G, metric)
    np.testing.assert_array_equal(ref["member"], ~non)
    out = _raw(T(X).cuda(), T(lab).cuda(), G, metric)
    o = _numpy(out)
    _check(f"non-members {metric}", ref, N, G, o)
    assert o["counts"].sum() == (~non).sum()
    keep = np.flatnonzero(~non)
    clean = _raw(T(X[keep]).cuda(), T(lab[keep]).cuda(), G, metric)
    kc = T(keep).cuda()
    for key in ("silhouette", "a", "b", "nearest"):
        assert torch.equal(_bits(clean[key]), _bits(out[key][kc].contiguous())), key
    assert torch.equal(_bits(clean["cluster_sum"]), _bits(out["cluster_sum"]))
    assert torch.equal(clean["counts"], out["counts"])
    # every row a non-member
    none = _numpy(_raw(T(X).cuda(), torch.full((N,), -1, dtype=torch.int32, device="cuda"), G, metric))
    assert np.isnan(none["silhouette"]).all() and np.isnan(none["a"]).all() and (none["nearest"] == -1).all()
    assert (none["counts"] == 0).all() and (none["cluster_sum"] == 0).all()


def test_two_calls_give_the_same_bits_and_duplicates_stay_in_range():
    case = CASES[5]
    X, lab = _inputs(*case)
    x, l = T(X).cuda(), T(lab).cuda()
    a, b = _raw(x, l, case[1]), _raw(x, l, case[1])
    for key in a:
        assert torch.equal(_bits(a[key]), _bits(b[key])), (key, "two calls, the same bits")
    # duplicated points: distances of exactly coinciding rows, and whole clusters of one point
    rng = np.random.default_rng(77)
    base = rng.standard_normal((20, 5)).astype(np.float32)
    X = np.repeat(base, 8, axis=0)
    lab = rng.integers(0, 3, size=len(X)).astype(np.int32)
    X = np.concatenate([X, np.ones((6, 5), dtype=np.float32)])
    lab = np.concatenate([lab, np.array([3, 3, 3, 4, 4, 4], dtype=np.int32)])   # clusters 3 and 4 coincide
    for metric in ("euclidean", "cosine"):
        o = _numpy(_raw(T(X).cuda(), T(lab).cuda(), 5, metric))
        s = o["silhouette"]
        assert np.isfinite(s).all() and (s >= -1).all() and (s <= 1).all(), metric
        # a = b = 0 up to the expansion's error: s = 0 exactly where both are 0, and nearest the smaller index
        assert o["nearest"][-6:].tolist() == [4, 4, 4, 3, 3, 3], metric


def test_raw_errors_leave_the_outputs_untouched_and_no_rows_zero_fill():
    from spmf_amd import _lib
    lib, h = _lib.load(), _model()._handle()
    N, G, W = 70, 5, 33
    X, lab = _inputs(N, G, W, 0.0, "blobs", "euclidean")
    x, l = T(X).cuda(), T(lab).cuda()
    need = int(lib.spmf_silhouette_scratch_bytes(h, N, G, W))
    scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    outs = {"sil": torch.full((N,), -7.0, dtype=torch.float32, device="cuda"),
            "a": torch.full((N,), -7.0, dtype=torch.float32, device="cuda"),
            "b": torch.full((N,), -7.0, dtype=torch.float32, device="cuda"),
            "nearest": torch.full((N,), -7, dtype=torch.int32, device="cuda"),
            "sums": torch.full((G,), -7.0, dtype=torch.float64, device="cuda"),
            "counts": torch.full((G,), -7, dtype=torch.int64, device="cuda")}
    good = dict(h=h, x=x.data_ptr(), n=N, row_len=W, labels=l.data_ptr(), G=G, flags=0,
                ptr=scratch.data_ptr() + (-scratch.data_ptr()) % 256, nbytes=need,
                stream=torch.cuda.current_stream().cuda_stream, **{k: v.data_ptr() for k, v in outs.items()})
    call = silhouette_raw_call(good)

    def untouched():
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in outs.values()) and not bool(scratch.any())
    assert_silhouette_errors(lib, good, need, after=untouched)
    # no rows: the zero fills of the two per-cluster outputs, and nothing else
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((outs["sums"] == 0).all()) and bool((outs["counts"] == 0).all())
    assert all(bool((outs[k] == -7).all()) for k in ("sil", "a", "b", "nearest")) and not bool(scratch.any())
    # the valid call in the exactly sized scratch is the method's result
    assert call() == 0
    torch.cuda.synchronize()
    want = _model().silhouette(x, lab, G)
    for mine, key in (("sil", "silhouette"), ("a", "a"), ("b", "b"), ("nearest", "nearest"), ("counts", "counts")):
        assert torch.equal(_bits(outs[mine]), _bits(want[key])), key
    full = _raw(x, l, G)
    assert torch.equal(_bits(outs["sums"]), _bits(full["cluster_sum"]))
    # NULL a_out / b_out / nearest_out: nothing is written there, nothing else changes
    part = _raw(x, l, G, a=False, b=False, nearest=False)
    assert bool((part["a"] == -7).all()) and bool((part["b"] == -7).all()) and bool((part["nearest"] == -7).all())
    for key in ("silhouette", "cluster_sum", "counts"):
        assert torch.equal(_bits(part[key]), _bits(full[key])), key


# ---- the surface ---------------------------------------------------------------------------------

CLUSTER_KEYS = {"labels", "distances", "centroids", "counts", "inertia", "n_iter", "converged", "n_unassigned",
                "embedding"}
SILHOUETTE_KEYS = {"silhouette", "a", "b", "nearest", "cluster_mean", "counts", "score", "n_scored"}


def test_silhouette_of_a_clustering_does_not_depend_on_the_batches():
    """``cluster`` keeps its keys; the silhouette of its embedding and labels has the same bits for one batch and
    for a split into two, and its counts are the clustering's."""
    case = ("poisson", 70, 45, 3, 2)
    cfg, x, params, mask, _ = _problem(*case)
    m = _dense_model(case[0], cfg, mask, 32)
    split = [{"counts": np.ascontiguousarray(x[:30])}, {"counts": np.ascontiguousarray(x[30:])}]
    got = []
    for data in ({"counts": x}, split):
        res = m.cluster(data, 3, draws=params, init="first")
        assert set(res) == CLUSTER_KEYS, "cluster's result has exactly the old keys"
        sil = m.silhouette(res["embedding"], res["labels"], 3)
        assert set(sil) == SILHOUETTE_KEYS and sil["n_scored"] == 70
        assert torch.equal(sil["counts"], res["counts"])
        got.append(sil)
    for key in ("silhouette", "a", "b", "nearest", "cluster_mean", "counts"):
        assert torch.equal(_bits(got[0][key]), _bits(got[1][key])), key
    assert got[0]["score"] == got[1]["score"] or (np.isnan(got[0]["score"]) and np.isnan(got[1]["score"]))


@functools.lru_cache(maxsize=None)
def _blobs():
    """Six blobs of 100 points in 8 dimensions, centres N(0, 10^2), unit noise, shuffled (the construction of
    tests/test_gpu_kmeans.py); one true member per blob as the init of the G = 6 run."""
    rng = np.random.default_rng(29)
    centres = 10.0 * rng.standard_normal((6, 8))
    truth = rng.permutation(np.repeat(np.arange(6), 100))
    X = (centres[truth] + rng.standard_normal((600, 8))).astype(np.float32)
    init = np.stack([X[np.flatnonzero(truth == g)[0]] for g in range(6)])
    return X, truth, init


def test_the_score_picks_the_number_of_blobs():
    X, truth, init = _blobs()
    m = _model()
    x = T(X).cuda()
    labels = {6: m.kmeans(x, 6, init=T(init).cuda())["labels"]}
    np.testing.assert_array_equal(labels[6].cpu().numpy(), truth)
    for G in (3, 12):
        labels[G] = m.kmeans(x, G, seed=0)["labels"]
    # the fp64 ordering first: a property of the data and the labellings alone
    full = {G: _reference(X, labels[G].cpu().numpy(), G, "euclidean") for G in (3, 6, 12)}
    ref = {G: float(r["s"].mean()) for G, r in full.items()}
    print("fp64 scores: " + ", ".join(f"G={G}: {v:.4f}" for G, v in ref.items()))
    assert ref[6] > ref[3] + 0.05 and ref[6] > ref[12] + 0.05, ref
    got = {G: m.silhouette(x, labels[G], G)["score"] for G in (3, 6, 12)}
    print("scores: " + ", ".join(f"G={G}: {v:.4f}" for G, v in got.items()))
    assert got[6] > got[3] and got[6] > got[12], got
    for G in (3, 6, 12):
        assert abs(got[G] - ref[G]) <= 2 * float(full[G]["cond"].max()) + 2.0 ** -22, (G, got[G], ref[G])
