"""GPU: embed / knn / neighbors (spmf_embed_rows, spmf_knn, csrc/knn.hip).

The kNN kernels are held against spmf_amd.neighbors.brute_force (fp64, exact differences) on data that owes
nothing to the model: R = standard normal [nr, K] from default_rng(7300 + nq + K), Q = R (a self case) or a
second draw; every shape under both metrics, and the Euclidean ones again with +1000 on every coordinate (the
centring).  Membership is judged in squared working distance d2 = |q' - r'|^2 (fp64 centre / unit rows) with
bar_ij = 2e-5 (|q'_i|^2 + |r'_j|^2), the project's 1e-5 on the three terms of the expansion the selection
uses; a row is clear-cut when it has at most k candidates or d2_(k+1) - d2_(k) > 2 max(bar of the two).  One
helper (_check) holds a result against the oracle:
 (a) shapes, dtypes, device, indices in [0, nr) or -1, distinct, padding -1 / +inf at the tail only,
     min(k, candidates) real slots;
 (b) distances non-decreasing, equal ones by ascending index;
 (c) only candidates are returned;
 (d) every distance within 1e-5 v (cosine: + 1e-6) of the oracle's v for that pair: the refine step works on
     exact differences, so (K + 2) 2^-24 of rounding remains; unit vectors rounded to fp32 leave a few 2^-23;
 (e) no candidate left out has d2 below the row's largest returned d2 minus 2 bar;
 (f) on clear-cut rows the index set is the oracle's.
Each case asserts on the oracle alone that at least 95 % of its rows are clear-cut (measured on the CPU with
this generator: CLEAR below, every case at or above 97 %).

embed is held against the fp64 oracle's encode, entry by entry within 1e-5 of the summed absolute
contributions and within 1e-5 of the array norm (the two bars of _gradcheck); neighbors is held bit for bit
against knn(embed(...)) -- no oracle set comparison there: those embeddings are near-collinear."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import spmf_oracle as O
from _problems import _dense_model
from _stream_cases import (_points, _problem, assert_embed_own_errors, assert_knn_errors, assert_shared_errors,
                           gpu_good_call, knn_raw_call)

pytestmark = pytest.mark.gpu
T = torch.as_tensor

# (nq, nr, K, k, self): ragged blocks, K padded 3 -> 4 and self rows 63 / 64 across a block edge; 32 x 32 tile
# edges; two K chunks, CAP = 80, six slices and the merge on a 256-CU device; KP = 128; dense near-ties
SHAPES = [(70, 70, 3, 5, True), (131, 197, 16, 10, False), (5, 333, 33, 64, False), (197, 197, 70, 15, True),
          (300, 300, 2, 64, True)]
VARIANTS = [("euclidean", 0.0), ("cosine", 0.0), ("euclidean", 1000.0)]
CLEAR = {("euclidean", 0.0): (70, 130, 5, 193, 300), ("cosine", 0.0): (70, 131, 5, 196, 299),
         ("euclidean", 1000.0): (70, 130, 5, 194, 300)}


def _bits(t):
    return t.view(torch.int32)


@functools.lru_cache(maxsize=None)
def _model():
    from spmf_amd import PoissonFactorization
    return PoissonFactorization(latent_dim=3, feature_dim=8, initialize_distributions=False, device="cuda")


def _oracle_view(Q, R, k, metric, self_off):
    """From the fp32 inputs alone, in fp64: candidates, the distance v, d2 and bar of every pair, per row the
    candidate count, the clear-cut flag and the oracle's top-k set."""
    q, r = Q.astype(np.float64), R.astype(np.float64)
    r_ok, q_ok = np.isfinite(r).all(1), np.isfinite(q).all(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        if metric == "cosine":
            rn, qn = np.sqrt((r * r).sum(1)), np.sqrt((q * q).sum(1))
            r_ok, q_ok = r_ok & (rn > 0), q_ok & (qn > 0)
            qw, rw = q / qn[:, None], r / rn[:, None]
        else:
            c = r[r_ok].mean(0) if r_ok.any() else np.zeros(r.shape[1])
            qw, rw = q - c, r - c
        d2 = ((qw[:, None, :] - rw[None, :, :]) ** 2).sum(-1)
        bar = 2e-5 * ((qw * qw).sum(1)[:, None] + (rw * rw).sum(1)[None, :])
        v = 0.5 * d2 if metric == "cosine" else np.sqrt(((q[:, None, :] - r[None, :, :]) ** 2).sum(-1))
    cand = q_ok[:, None] & r_ok[None, :]
    if self_off is not None:
        i = np.arange(len(q))
        ok = (i + self_off >= 0) & (i + self_off < len(r))
        cand[i[ok], i[ok] + self_off] = False
    nq = len(q)
    nc = cand.sum(1)
    key = np.where(cand, d2, np.inf)
    order = np.argsort(key, axis=1, kind="stable")
    pad = np.concatenate([order, np.zeros((nq, k + 1), dtype=order.dtype)], axis=1)
    rows = np.arange(nq)
    jk, jn = pad[:, k - 1], pad[:, k]
    with np.errstate(invalid="ignore"):
        gap = key[rows, jn] - key[rows, jk] if R.shape[0] else np.zeros(nq)
        edge = 2 * np.maximum(bar[rows, jk], bar[rows, jn]) if R.shape[0] else np.zeros(nq)
        clear = (nc <= k) | ((nc > k) & (gap > edge))
    top = np.zeros_like(cand)
    for i in range(nq):
        top[i, order[i, :min(k, nc[i])]] = True
    return cand, v, d2, bar, nc, clear, top


@functools.lru_cache(maxsize=None)
def _case(nq, nr, K, k, self_case, metric, shift):
    Q, R = _points(nq, nr, K, self_case, shift)
    return Q, R, _oracle_view(Q, R, k, metric, 0 if self_case else None)


def _check(out, view, nr, k, metric, min_clear=None, tag=""):
    cand, v, d2, bar, nc, clear, top = view
    nq = cand.shape[0]
    print(f"{tag}: clear-cut rows {int(clear.sum())}/{nq}")
    if min_clear is not None:
        assert clear.sum() >= np.ceil(min_clear * nq - 1e-9), (tag, int(clear.sum()), nq)
    idx, dist = out["indices"], out["distances"]
    # (a)
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32, tag
    assert tuple(idx.shape) == (nq, k) and tuple(dist.shape) == (nq, k), (tag, idx.shape, dist.shape)
    assert idx.is_cuda and dist.is_cuda, tag
    c = idx.cpu().numpy().astype(np.int64)
    s = dist.cpu().numpy().astype(np.float64)
    real = c >= 0
    n = np.minimum(k, nc)
    assert ((c >= -1) & (c < max(nr, 0))).all() or nr == 0 and (c == -1).all(), tag
    assert (real == (np.arange(k)[None, :] < n[:, None])).all(), (tag, "real slots / padding at the tail")
    assert (c[~real] == -1).all() and np.isposinf(s[~real]).all(), tag
    cs = np.sort(np.where(real, c, -1 - np.arange(k)[None, :]), axis=1)
    assert (np.diff(cs, axis=1) != 0).all(), (tag, "distinct indices")
    if nr == 0 or nq == 0:
        return clear
    # (b)
    both = real[:, 1:] & real[:, :-1]
    with np.errstate(invalid="ignore"):
        ds = np.where(both, s[:, 1:] - s[:, :-1], 1.0)
    assert (ds >= 0).all(), (tag, "order")
    assert (c[:, 1:] > c[:, :-1])[both & (ds == 0)].all(), (tag, "ties by index")
    # (c)
    rows = np.broadcast_to(np.arange(nq)[:, None], (nq, k))
    cc = np.where(real, c, 0)
    assert cand[rows, cc][real].all(), (tag, "a returned row is no candidate")
    # (d)
    ref = v[rows, cc]
    err = np.abs(s - ref)[real]
    rel = (err / np.maximum(ref[real], 1e-300)).max() if err.size else 0.0
    print(f"{tag}: max |dist - oracle| {err.max() if err.size else 0.0:.3e} (largest relative {rel:.3e})")
    assert (err <= 1e-5 * ref[real] + (1e-6 if metric == "cosine" else 0.0)).all(), (tag, float(err.max()))
    # (e)
    ret = np.zeros_like(cand)
    ret[rows[real], c[real]] = True
    has = n > 0
    d2r = np.where(ret, d2, -np.inf)
    jl = d2r.argmax(1)                                        # the row's largest returned d2
    last, lbar = d2r[np.arange(nq), jl], bar[np.arange(nq), jl]
    with np.errstate(invalid="ignore"):
        slack = np.where(cand & ~ret, d2 - (last[:, None] - 2 * np.maximum(bar, lbar[:, None])), np.inf)
    print(f"{tag}: least (left-out d2) - (last returned d2 - 2 bar) {slack[has].min() if has.any() else 0.0:.3e}")
    assert (slack[has] >= 0).all(), (tag, "a nearer candidate was missed")
    assert not (cand & ~ret)[~has].any(), tag
    # (f)
    assert (ret[clear] == top[clear]).all(), (tag, "index set on clear-cut rows")
    return clear


def _knn(Q, R, k, metric, self_case, **kw):
    r = T(R).cuda()
    return _model().knn(r, k=k, queries=None if self_case else T(Q).cuda(), metric=metric, **kw)


@pytest.mark.parametrize("metric,shift", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}_K{s[2]}_k{s[3]}")
def test_knn_against_brute_force(shape, metric, shift):
    from spmf_amd.neighbors import brute_force
    nq, nr, K, k, self_case = shape
    Q, R, view = _case(nq, nr, K, k, self_case, metric, shift)
    tag = f"{metric}{'+1000' if shift else ''} {nq}x{nr} K={K} k={k}"
    # the condition on the inputs, on the oracle alone
    clear = view[5]
    print(f"{tag}: clear-cut {int(clear.sum())} (recorded {CLEAR[(metric, shift)][SHAPES.index(shape)]})")
    assert clear.sum() >= np.ceil(0.95 * nq - 1e-9), (tag, int(clear.sum()))
    # the oracle view is brute_force's: same candidates and order on clear-cut rows
    bi, bd = brute_force(T(Q), T(R), k, metric, self_case)
    bset = np.zeros_like(view[0])
    br = np.broadcast_to(np.arange(nq)[:, None], (nq, k))
    bi = bi.numpy()
    bset[br[bi >= 0], bi[bi >= 0]] = True
    assert (bset[clear] == view[6][clear]).all(), tag
    out = _knn(Q, R, k, metric, self_case)
    _check(out, view, nr, k, metric, 0.95, tag)


def test_duplicated_rows_tie_by_index_at_distance_zero():
    rng = np.random.default_rng(3)
    base = rng.standard_normal((40, 6)).astype(np.float32)
    R = np.concatenate([base, base, base[:10]])              # row i = row i + 40 (= row i + 80 for i < 10)
    for metric in ("euclidean", "cosine"):
        out = _knn(R, R, 3, metric, True)
        idx, dist = out["indices"].cpu().numpy(), out["distances"].cpu().numpy()
        assert idx[0].tolist()[:2] == [40, 80] and (dist[0, :2] == 0.0).all(), (metric, idx[0], dist[0])
        assert idx[45, 0] == 5 and idx[45, 1] == 85 and (dist[45, :2] == 0.0).all(), metric
        assert idx[20, 0] == 60 and dist[20, 0] == 0.0 and dist[20, 1] > 0.0, metric
        _check(out, _oracle_view(R, R, 3, metric, 0), len(R), 3, metric, tag=f"duplicates {metric}")


def test_include_self_puts_the_row_first():
    Q, R = _points(131, 131, 16, True)
    for metric in ("euclidean", "cosine"):
        out = _knn(R, R, 4, metric, True, include_self=True)
        assert out["indices"][:, 0].cpu().tolist() == list(range(131)), metric
        assert (out["distances"][:, 0] == 0.0).all(), metric
        _check(out, _oracle_view(R, R, 4, metric, None), 131, 4, metric, tag=f"include_self {metric}")
        rest = _knn(R, R, 3, metric, True)
        assert torch.equal(rest["indices"], out["indices"][:, 1:]), metric


def test_few_rows_and_empty_sets():
    m = _model()
    Q, R = _points(9, 7, 5, False)
    for metric in ("euclidean", "cosine"):
        out = _knn(Q, R, 10, metric, False)                                     # nr < k
        _check(out, _oracle_view(Q, R, 10, metric, None), 7, 10, metric, tag="nr < k")
        assert (out["indices"][:, 7:] == -1).all() and (out["indices"][:, :7] >= 0).all()
        one = _knn(R[:1], R[:1], 3, metric, True)                               # nr = 1, itself excluded
        assert (one["indices"] == -1).all() and torch.isposinf(one["distances"]).all()
        none = m.knn(T(R).cuda(), k=3, queries=torch.empty(0, 5, device="cuda"), metric=metric)   # nq = 0
        assert tuple(none["indices"].shape) == (0, 3) and tuple(none["distances"].shape) == (0, 3)
        void = m.knn(torch.empty(0, 5, device="cuda"), k=3, queries=T(Q).cuda(), metric=metric)   # nr = 0
        assert (void["indices"] == -1).all() and torch.isposinf(void["distances"]).all()
        assert tuple(void["indices"].shape) == (9, 3)


def test_non_finite_and_zero_rows():
    Q, R = (a.copy() for a in _points(131, 197, 16, False))
    R[70, 3] = np.nan
    R[71, 0] = np.inf
    Q[5, 15] = np.nan
    R[100] = 0.0
    Q[9] = 0.0
    for metric in ("euclidean", "cosine"):
        out = _knn(Q, R, 10, metric, False)
        view = _oracle_view(Q, R, 10, metric, None)
        _check(out, view, 197, 10, metric, tag=f"non-finite {metric}")
        idx = out["indices"].cpu().numpy()
        assert (idx[5] == -1).all() and not np.isin(idx, (70, 71)).any(), metric
        if metric == "cosine":
            assert (idx[9] == -1).all() and not (idx == 100).any(), "a zero row has no direction"
        else:
            assert (idx[9] >= 0).all()
    S, _ = _points(70, 70, 3, True)
    S = S.copy()
    S[63] = np.nan                                           # as query and as reference row of a self case
    out = _knn(S, S, 5, "euclidean", True)
    _check(out, _oracle_view(S, S, 5, "euclidean", 0), 70, 5, "euclidean", tag="non-finite self")


def test_bit_properties(monkeypatch):
    m = _model()
    for (nq, nr, K, k, self_case), metric in zip(SHAPES, ("euclidean", "cosine", "euclidean", "cosine", "euclidean")):
        Q, R = _points(nq, nr, K, self_case)
        r, q = T(R).cuda(), T(Q).cuda()
        one = m.knn(r, k=k, queries=None if self_case else q, metric=metric)
        two = m.knn(r, k=k, queries=None if self_case else q, metric=metric)
        assert torch.equal(one["indices"], two["indices"]) and torch.equal(_bits(one["distances"]), _bits(two["distances"]))
        # a subset of the queries in another order: the same bits for the same queries (no self-exclusion here,
        # the queries are a list of their own)
        full = m.knn(r, k=k, queries=q.clone(), metric=metric)
        pick = torch.as_tensor(np.random.default_rng(nq).permutation(nq)[:max(1, nq // 3)].copy(), device="cuda")
        part = m.knn(r, k=k, queries=q[pick].contiguous(), metric=metric)
        assert torch.equal(part["indices"], full["indices"][pick]), (nq, metric)
        assert torch.equal(_bits(part["distances"]), _bits(full["distances"][pick])), (nq, metric)
        if self_case:                                        # queries=points IS the self case
            same = m.knn(r, k=k, queries=r, metric=metric)
            assert torch.equal(same["indices"], one["indices"])
            assert torch.equal(_bits(same["distances"]), _bits(one["distances"]))
        # the two tile functions of the select kernel
        res = {}
        for tile in ("0", "1"):
            monkeypatch.setenv("SPMF_KNN_TILE", tile)
            res[tile] = m.knn(r, k=k, queries=None if self_case else q, metric=metric)
        monkeypatch.delenv("SPMF_KNN_TILE")
        assert torch.equal(res["0"]["indices"], res["1"]["indices"]), (nq, metric)
        assert torch.equal(_bits(res["0"]["distances"]), _bits(res["1"]["distances"])), (nq, metric)
        assert torch.equal(res["0"]["indices"], one["indices"])


def test_raw_knn_errors_leave_the_outputs_untouched():
    from spmf_amd import _lib
    m, lib = _model(), _lib.load()
    h = m._handle()
    nq, nr, K, k = 70, 333, 33, 5
    Q, R = _points(nq, nr, K, False)
    q, r = T(Q).cuda(), T(R).cuda()
    need = int(lib.spmf_knn_scratch_bytes(h, nq, nr, K))
    assert need > 0 and need % 256 == 0
    scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    idx = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
    dist = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
    good = dict(h=h, q=q.data_ptr(), nq=nq, r=r.data_ptr(), nr=nr, row_len=K, k=k, flags=0, self_offset=-1,
                idx=idx.data_ptr(), dist=dist.data_ptr(), ptr=scratch.data_ptr() + (-scratch.data_ptr()) % 256,
                nbytes=need, stream=torch.cuda.current_stream().cuda_stream)

    def untouched():
        torch.cuda.synchronize()
        assert bool((idx == -7).all()) and bool((dist == -7).all()) and not bool(scratch.any())
    assert_knn_errors(lib, good, need, untouched)
    call = knn_raw_call(good)
    assert call(nq=0) == 0
    untouched()
    assert call() == 0                                       # and the valid call is the method's
    torch.cuda.synchronize()
    want = m.knn(r, k=k, queries=q)
    assert torch.equal(idx, want["indices"]) and torch.equal(_bits(dist), _bits(want["distances"]))
    assert call(self_offset=3, nq=nq) == 0                   # query i is reference row 3 + i
    torch.cuda.synchronize()
    assert not bool((idx == torch.arange(3, 3 + nq, device="cuda", dtype=torch.int32)[:, None]).any())


# ---- embed -------------------------------------------------------------------------------------

EMBED = [("poisson", 70, 45, 3, 2), ("poisson_log", 131, 197, 16, 7), ("mixed", 131, 197, 16, 7),
         ("poisson", 40, 90, 65, 1)]


@functools.lru_cache(maxsize=None)
def _embed_oracle(case):
    """fp64: z [S,B,K] of the oracle's encode and the summed absolute contributions to each entry."""
    cfg, x, params, mask, _ = _problem(*case)
    z = O.encode(cfg, T(x), T(params["u"]), T(params["s"]))
    A = O.encoding_matrix(T(params["u"]), T(params["s"]))
    scale = torch.matmul(O.encoder_function(cfg, T(x)).abs(), A.abs())
    if cfg.scale_rows and cfg.likelihood != "bernoulli":
        scale = scale * (T(x).sum(-1, keepdim=True) / float(cfg.xi_u_global)).abs()
    if z.dim() == 2:
        z, scale = z.unsqueeze(0), scale.unsqueeze(0)
    return z.numpy(), scale.numpy()


def _assert_entries(got, ref, scale, tag):
    g = got.cpu().double().numpy()
    assert g.shape == ref.shape, (tag, g.shape, ref.shape)
    err = np.abs(g - ref)
    worst = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0)).max()
    print(f"{tag}: worst |hip - oracle| / contributions {worst:.3e}, max|err| / max|oracle| "
          f"{err.max() / max(np.abs(ref).max(), 1e-300):.3e}")
    assert worst <= 1e-5, (tag, worst)
    assert err.max() <= 1e-5 * np.abs(ref).max(), (tag, float(err.max()), float(np.abs(ref).max()))


@pytest.mark.parametrize("case", EMBED, ids=lambda c: f"{c[0]}_{c[1]}x{c[2]}_K{c[3]}_S{c[4]}")
def test_embed_against_the_oracle_and_encode(case):
    lik, B, D, K, S = case
    cfg, x, params, mask, _ = _problem(*case)
    z, scale = _embed_oracle(case)
    m = _dense_model(lik, cfg, mask, 32)
    out = m.embed({"counts": x}, draws=params, sd=S >= 2)
    assert out["mean"].dtype == torch.float32 and tuple(out["mean"].shape) == (B, K) and out["mean"].is_cuda
    _assert_entries(out["mean"], z.mean(0), scale.mean(0), f"{case} mean")
    # the mean of model.encode per draw (the same bars: two fp32 evaluations of one sum)
    enc = m.encode({"counts": x}, u=T(params["u"]), s=T(params["s"]))
    enc = enc.unsqueeze(0) if enc.dim() == 2 else enc
    want = enc.double().mean(0)
    print(f"{case}: bit-equal to the fp32 mean of encode in draw order: "
          f"{bool(torch.equal(out['mean'], sum(enc[1:], enc[0]) * torch.tensor(1.0 / S, dtype=torch.float32)))}")
    _assert_entries(out["mean"], want.cpu().numpy(), scale.mean(0), f"{case} mean vs encode")
    if S >= 2:
        assert set(out) == {"mean", "sd"} and tuple(out["sd"].shape) == (B, K)
        _assert_entries(out["sd"], z.std(0, ddof=1), scale.mean(0), f"{case} sd")
    else:
        assert set(out) == {"mean"}
        with pytest.raises(ValueError):
            m.embed({"counts": x}, draws=params, sd=True)
    # two batches equal the concatenation; max_rows changes no bit
    cut = 32
    two = m.embed([{"counts": x[:cut]}, {"counts": x[cut:]}], draws=params, sd=S >= 2)
    small = m.embed({"counts": x}, draws=params, sd=S >= 2, max_rows=32)
    for key in out:
        assert torch.equal(_bits(two[key]), _bits(out[key])), (case, key, "two batches")
        assert torch.equal(_bits(small[key]), _bits(out[key])), (case, key, "max_rows")


def test_embed_nan_count_and_custom_codec():
    case = EMBED[0]
    lik, B, D, K, S = case
    cfg, x, params, mask, _ = _problem(*case)
    m = _dense_model(lik, cfg, mask, 32)
    ref = m.embed({"counts": x}, draws=params, sd=True)
    bad = x.copy()
    bad[17, 4] = np.nan
    out = m.embed({"counts": bad}, draws=params, sd=True)
    keep = np.arange(B) != 17
    for key in ("mean", "sd"):
        assert torch.isnan(out[key][17]).all(), key
        assert torch.equal(_bits(out[key][keep]), _bits(ref[key][keep])), key
    from spmf_amd import PoissonFactorization
    c = PoissonFactorization(latent_dim=K, feature_dim=D, column_norms=cfg.eta_i, initialize_distributions=False,
                             device="cuda", encoder_function=lambda t: t, decoder_function=lambda t: t)
    with pytest.raises(NotImplementedError):
        c.embed({"counts": x}, draws=params)
    with pytest.raises(NotImplementedError):
        c.neighbors({"counts": x}, k=3, draws=params)


def test_embed_rows_shared_errors_launch_nothing():
    from spmf_amd import _lib
    lik, B, D, K, S = EMBED[0]
    cfg, x, params, mask, _ = _problem(*EMBED[0])
    m = _dense_model(lik, cfg, mask, 32)
    lib = _lib.load()
    good, need, out, scratch, no_u = gpu_good_call("embed", m, x, params)
    mean, sd = out["mean"], out["sd"]
    raw = _dense_model("mixed", cfg, np.arange(D) % 3 == 1, 32)._new_ctx()

    def untouched():
        torch.cuda.synchronize()
        assert bool((mean == -7).all()) and bool((sd == -7).all()) and not bool(scratch.any())
    try:
        call = assert_shared_errors(lib, "embed", good, need, no_u, raw, untouched)
        assert_embed_own_errors(lib, call, good, untouched)
    finally:
        lib.spmf_ctx_destroy(raw)
    assert call() == 0
    torch.cuda.synchronize()
    want = m.embed({"counts": x}, draws=params, sd=True)
    assert torch.equal(_bits(mean), _bits(want["mean"])) and torch.equal(_bits(sd), _bits(want["sd"]))


# ---- neighbors ---------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("case", EMBED[:2], ids=lambda c: f"{c[0]}_{c[1]}x{c[2]}")
def test_neighbors_is_knn_of_embed(case, metric):
    lik, B, D, K, S = case
    cfg, x, params, mask, _ = _problem(*case)
    m = _dense_model(lik, cfg, mask, 32)
    e = m.embed({"counts": x}, draws=params)["mean"]
    for include_self in (False, True):
        got = m.neighbors({"counts": x}, k=7, metric=metric, include_self=include_self, draws=params)
        want = m.knn(e, k=7, metric=metric, include_self=include_self)
        assert got["indices"].dtype == torch.int32 and tuple(got["indices"].shape) == (B, 7)
        assert torch.equal(got["indices"], want["indices"]), (case, metric)
        assert torch.equal(_bits(got["distances"]), _bits(want["distances"])), (case, metric)
    # a second batch as the query: the draws are shared
    xq = np.ascontiguousarray(x[::-1][:41])
    got = m.neighbors({"counts": x}, k=7, query={"counts": xq}, metric=metric, draws=params)
    eq = m.embed({"counts": xq}, draws=params)["mean"]
    want = m.knn(e, k=7, queries=eq, metric=metric)
    assert tuple(got["indices"].shape) == (41, 7)
    assert torch.equal(got["indices"], want["indices"]) and torch.equal(_bits(got["distances"]), _bits(want["distances"]))


def test_neighbors_samples_once_for_data_and_query():
    """Without ``draws`` the surrogate is sampled once and both embeddings use that sample."""
    lik, B, D, K, S = EMBED[0]
    cfg, x, params, mask, _ = _problem(*EMBED[0])
    m = _dense_model(lik, cfg, mask, 32)
    calls = []

    class Once:
        def sample(self, n):
            calls.append(n)
            return {k: T(v[:1]).repeat(n, *([1] * (np.ndim(v) - 1))) * (1.0 + 0.01 * len(calls)) for k, v in params.items()}
    m.surrogate_distribution = Once()
    got = m.neighbors({"counts": x}, k=5, query={"counts": x[:20]}, nsamples=3)
    assert calls == [3]
    draws = {k: T(v[:1]).repeat(3, *([1] * (np.ndim(v) - 1))) * 1.01 for k, v in params.items()}
    want = m.knn(m.embed({"counts": x}, draws=draws)["mean"], k=5,
                 queries=m.embed({"counts": x[:20]}, draws=draws)["mean"])
    assert torch.equal(got["indices"], want["indices"]) and torch.equal(_bits(got["distances"]), _bits(want["distances"]))
