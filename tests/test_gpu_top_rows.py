"""GPU: top_rows (spmf_toprows_columns, csrc/toprows.hip): per column the k rows with the largest posterior
predictive mean.

1. Exact against predict: the reference is predict's 'mean' with the non-candidates masked (non-finite, or x != 0
   when stored cells are excluded), each column ordered by (score descending, row ascending), the first k taken,
   the rest padded with -1 / -inf.  rows and scores equal it bit for bit in every column: no tolerance.
2. Against the fp64 oracle: test_gpu_topk._check's (a)-(f) with rows and columns exchanged, the bar
   bar(v) = 1e-5 |v| + 1e-5 max|score|:
    (a) shapes, dtypes, rows in [0,B) or -1, distinct within a column, padding -1 / -inf at the tail only,
        min(k, #candidates) real slots;
    (b) scores non-increasing, equal scores in ascending row order;
    (c) only candidates are returned;
    (d) every returned score within bar of the oracle's score of that cell;
    (e) every candidate not returned scores at most the column's last returned one + 2 bar;
    (f) on columns whose oracle gap between the k-th and (k+1)-th candidate exceeds 2 bar ("clear cut") the
        returned row set is the oracle's.
   The clear-cut condition is asserted on the oracle alone before the GPU result is read: CLEAR_COLS below holds
   the counts of the CPU oracle (seed 9100+B+K) at CASES, every case keeps at least half its columns clear-cut and
   the Poisson cases 95 %.  The unclear columns are tied or near-tied scores; 1. covers them exactly.
3. ties, 4. a NaN count, 5. invariance (max_rows, batches, factory, lists, a repeated call), 6. wide K,
7. the C-ABI, 8. memory.

CASES (B, D, K, S, k): ragged 64-blocks and 32-tiles, K padded 3 -> 4, K = 16, K = 33 -> 64 (two K chunks), both
candidate-buffer sizes with real competition ((131, 197) at k = 10 and k = 64), columns with no candidate and with
fewer than k (B = 5 at k = 64; stored cells at B = 70), and one to four column blocks with one to three row blocks:
the rows of (70, 45) and (131, 197) are split into 2 and 3 row slices on a 256-CU device, so the merge runs."""
import functools

import numpy as np
import pytest
import torch

from _stream_cases import _case, _problem, assert_shared_errors, gpu_good_call, host_ctx
from _problems import LIKELIHOODS, _dense_model, _dense_problem

pytestmark = pytest.mark.gpu
T = torch.as_tensor

CASES = [(70, 45, 3, 2, 5), (131, 197, 16, 7, 10), (5, 333, 33, 3, 64), (131, 197, 16, 7, 64)]
# clear-cut columns of the CPU oracle at CASES: (stored cells excluded, all cells)
CLEAR_COLS = {"poisson": ((45, 196, 333, 194), (45, 196, 333, 193)),
              "poisson_log": ((40, 178, 333, 150), (45, 149, 333, 102)),
              "bernoulli": ((43, 192, 333, 189), (45, 197, 333, 182)),
              "bernoulli_log": ((43, 189, 333, 177), (45, 174, 333, 197)),
              "mixed": ((30, 130, 333, 128), (30, 131, 333, 129))}
MIN_CLEAR = {"poisson": 0.95}


def _bar(v, smax):
    return 1e-5 * np.abs(v) + 1e-5 * smax


def _oracle_view(score, x, k, exclude_stored):
    """From the oracle alone, per column: candidates [D,B], max|score|, their number, the clear-cut flag and the
    top-k set."""
    st, xt = score.T, x.T
    C_, B = st.shape
    fin = np.isfinite(st)
    smax = float(np.abs(st[fin]).max()) if fin.any() else 0.0
    cand = fin & (~(xt != 0) if exclude_stored else True)          # (NaN != 0: a NaN count is stored)
    nc = cand.sum(1)
    srt = -np.sort(-np.where(cand, st, -np.inf), axis=1)
    srt = np.concatenate([srt, np.full((C_, k + 1), -np.inf)], axis=1)
    kth, nxt = srt[:, k - 1], srt[:, k]
    with np.errstate(invalid="ignore"):
        clear = (nc <= k) | (kth - nxt > 2 * _bar(kth, smax))
    top = cand & (st >= np.where(nc > k, kth, -np.inf)[:, None])
    return cand, smax, nc, clear, top


def _reference(mean, x, k, exclude_stored):
    """1.'s reference from predict's 'mean' (fp32 [B,C] on the host) and the counts [B,C] of those columns."""
    B, C_ = mean.shape
    cand = np.isfinite(mean) & (~(x != 0) if exclude_stored else True)
    rows = np.full((C_, k), -1, dtype=np.int64)
    scores = np.full((C_, k), -np.inf, dtype=np.float32)
    for j in range(C_):
        b = np.nonzero(cand[:, j])[0]
        b = b[np.lexsort((b, -mean[b, j].astype(np.float64)))][:k]      # score descending, then row ascending
        rows[j, :len(b)], scores[j, :len(b)] = b, mean[b, j]
    return rows, scores


def _assert_exact(out, mean, x, k, exclude_stored, tag):
    rows, scores = out["rows"], out["scores"]
    C_ = mean.shape[1]
    assert rows.dtype == torch.int64 and scores.dtype == torch.float32, tag
    assert tuple(rows.shape) == (C_, k) and tuple(scores.shape) == (C_, k), (tag, rows.shape, scores.shape)
    assert rows.is_cuda and scores.is_cuda, tag
    want_r, want_s = _reference(mean, x, k, exclude_stored)
    got_r, got_s = rows.cpu().numpy(), scores.cpu().numpy()
    bad = np.nonzero((got_r != want_r).any(1) | (got_s.view(np.int32) != want_s.view(np.int32)).any(1))[0]
    assert bad.size == 0, (tag, "columns that differ", bad[:8].tolist(), got_r[bad[:1]], want_r[bad[:1]])


def _check(out, score, x, k, exclude_stored, tag):
    B, D = score.shape
    cand, smax, nc, clear, top = _oracle_view(score, x, k, exclude_stored)
    st = score.T
    rows, scores = out["rows"], out["scores"]
    # (a)
    assert rows.dtype == torch.int64 and scores.dtype == torch.float32, tag
    assert tuple(rows.shape) == (D, k) and tuple(scores.shape) == (D, k), (tag, rows.shape, scores.shape)
    r = rows.cpu().numpy()
    s = scores.cpu().numpy().astype(np.float64)
    real = r >= 0
    n = np.minimum(k, nc)
    assert ((r >= -1) & (r < B)).all(), tag
    assert (real == (np.arange(k)[None, :] < n[:, None])).all(), (tag, "real slots / padding at the tail")
    assert (r[~real] == -1).all() and np.isneginf(s[~real]).all(), tag
    rs = np.sort(np.where(real, r, -1 - np.arange(k)[None, :]), axis=1)
    assert (np.diff(rs, axis=1) != 0).all(), (tag, "distinct rows")
    # (b)
    both = real[:, 1:] & real[:, :-1]
    with np.errstate(invalid="ignore"):
        ds = np.where(both, s[:, 1:] - s[:, :-1], -1.0)
    assert (ds <= 0).all(), (tag, "order")
    assert (r[:, 1:] > r[:, :-1])[both & (ds == 0)].all(), (tag, "ties by row")
    # (c)
    colj = np.broadcast_to(np.arange(D)[:, None], (D, k))
    rr = np.where(real, r, 0)
    assert cand[colj, rr][real].all(), (tag, "a returned cell is no candidate")
    # (d)
    ref = st[colj, rr]
    err = np.abs(s - ref)[real]
    print(f"{tag}: clear-cut columns {int(clear.sum())}/{D}, max|score| {smax:.6g}, "
          f"max |score - oracle| {err.max() if err.size else 0.0:.3e}")
    assert (err <= _bar(ref[real], smax)).all(), (tag, float(err.max()))
    # (e)
    ret = np.zeros((D, B), dtype=bool)
    ret[colj[real], r[real]] = True
    rest = np.where(cand & ~ret, st, -np.inf).max(1)
    has = n > 0
    last = ref[np.arange(D), np.maximum(n - 1, 0)]
    assert (rest[has] <= last[has] + 2 * _bar(last[has], smax)).all(), (tag, "a better candidate was missed")
    assert not (cand & ~ret)[~has].any(), tag
    # (f)
    assert (ret[clear] == top[clear]).all(), (tag, "row set on clear-cut columns")


@functools.lru_cache(maxsize=None)
def _mean(lik, B, D, K, S):
    """predict's 'mean' of the case on the host, computed once (read-only)."""
    return _case(lik, B, D, K, S)["full"]["mean"].cpu().numpy()


@pytest.mark.parametrize("exclude_stored", [True, False])
@pytest.mark.parametrize("B,D,K,S,k", CASES)
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_every_likelihood_exact_against_predict_and_within_bar_of_the_oracle(lik, B, D, K, S, k, exclude_stored):
    c = _case(lik, B, D, K, S)
    tag = f"{lik} {B}x{D} K={K} S={S} k={k} exclude={exclude_stored}"
    # the condition on the inputs, on the oracle alone
    i = CASES.index((B, D, K, S, k))
    clear = int(_oracle_view(c["score"], c["x"], k, exclude_stored)[3].sum())
    assert clear >= CLEAR_COLS[lik][0 if exclude_stored else 1][i], (tag, clear)
    assert clear >= np.ceil(MIN_CLEAR.get(lik, 0.5) * D - 1e-9), (tag, clear, D)
    nc = _oracle_view(c["score"], c["x"], k, exclude_stored)[2]
    if B == 5:
        assert (nc < k).all(), "fewer than k candidates"
    out = c["m"].top_rows({"counts": c["x"]}, k=k, draws=c["params"], exclude_stored=exclude_stored)
    assert set(out) == {"rows", "scores"}
    _assert_exact(out, _mean(lik, B, D, K, S), c["x"], k, exclude_stored, tag)
    _check(out, c["score"], c["x"], k, exclude_stored, tag)


def test_a_column_without_a_candidate_and_one_with_fewer_than_k():
    """Column 3 is stored in every row, column 4 in all rows but 2 and 68: with stored cells excluded the first is
    all padding and the second returns its two rows; without the exclusion both compete as usual."""
    c = _case("poisson", 70, 45, 3, 2)
    x = c["x"].copy()
    x[:, 3] = 1.0
    x[:, 4] = 2.0
    x[[2, 68], 4] = 0.0
    m = c["m"]
    mean = m.predict({"counts": x}, draws=c["params"])["mean"].cpu().numpy()
    for ex in (True, False):
        out = m.top_rows({"counts": x}, k=5, draws=c["params"], exclude_stored=ex)
        _assert_exact(out, mean, x, 5, ex, f"planted columns exclude={ex}")
    out = m.top_rows({"counts": x}, k=5, draws=c["params"])
    assert (out["rows"][3] == -1).all() and torch.isneginf(out["scores"][3]).all()
    assert sorted(out["rows"][4, :2].tolist()) == [2, 68] and (out["rows"][4, 2:] == -1).all()


@pytest.mark.parametrize("B,D,K,S,k", [CASES[0], CASES[3]])
def test_ties_return_the_lowest_rows(B, D, K, S, k):
    """Draws with u = 0: z = 0 in every row, so every row of a column has the same score and a column returns
    rows 0 .. k-1 of its candidates in ascending order; with exclude_stored the stored rows are skipped."""
    c = _case("poisson", B, D, K, S)
    draws = {n: v.copy() for n, v in c["params"].items()}
    draws["u"] = np.zeros_like(draws["u"])
    x, m = c["x"], c["m"]
    mean = m.predict({"counts": x}, draws=draws)["mean"].cpu().numpy()
    assert (mean == mean[:1]).all() and np.isfinite(mean).all(), "one score per column"
    for ex in (True, False):
        out = m.top_rows({"counts": x}, k=k, draws=draws, exclude_stored=ex)
        _assert_exact(out, mean, x, k, ex, f"ties exclude={ex}")
        r = out["rows"].cpu().numpy()
        for j in range(D):
            cand = np.nonzero(x[:, j] == 0)[0] if ex else np.arange(B)
            want = cand[:k].tolist()
            assert r[j].tolist() == want + [-1] * (k - len(want)), (ex, j)


def test_a_nan_count_takes_its_row_out_of_every_column():
    """x[66, 11] = NaN: row 66 is returned for no column, and the result equals, bit for bit, the result of the
    batch without that row (rows above it renumbered)."""
    c = _case("poisson", 131, 197, 16, 7)
    m, draws = c["m"], c["params"]
    x = c["x"].copy()
    x[66, 11] = float("nan")
    rest = np.delete(c["x"], 66, axis=0)
    for ex, k in ((True, 10), (False, 64)):
        out = m.top_rows({"counts": x}, k=k, draws=draws, exclude_stored=ex)
        assert not bool((out["rows"] == 66).any())
        want = m.top_rows({"counts": rest}, k=k, draws=draws, exclude_stored=ex)
        wr = want["rows"]
        wr = torch.where(wr >= 66, wr + 1, wr)
        assert torch.equal(out["rows"], wr), ex
        assert torch.equal(out["scores"], want["scores"]), ex


@pytest.mark.parametrize("lik", ["poisson", "mixed"])
def test_invariance_to_chunks_batches_lists_and_repetition(lik):
    """max_rows = 64 (three chunks), a list of two batches (64 rows + the rest) and a factory against the single
    call, with global rows; cols as a permutation and with a duplicate against cols=None, row by row; a repeated
    call: identical bits everywhere."""
    B, D, K, S = 131, 197, 16, 7
    c = _case(lik, B, D, K, S)
    m, x, draws = c["m"], c["x"], c["params"]
    for k, ex in ((10, True), (64, False)):
        one = m.top_rows({"counts": x}, k=k, draws=draws, exclude_stored=ex)
        parts = [{"counts": x[:64].copy()}, {"counts": x[64:].copy()}]
        for tag, o in (("chunked", m.top_rows({"counts": x}, k=k, draws=draws, exclude_stored=ex, max_rows=64)),
                       ("two batches", m.top_rows(parts, k=k, draws=draws, exclude_stored=ex)),
                       ("factory", m.top_rows(lambda: iter(parts), k=k, draws=draws, exclude_stored=ex)),
                       ("again", m.top_rows({"counts": x}, k=k, draws=draws, exclude_stored=ex))):
            assert torch.equal(o["rows"], one["rows"]), (tag, k)
            assert torch.equal(o["scores"], one["scores"]), (tag, k)
        rng = np.random.default_rng(5)
        perm = rng.permutation(D)
        dup = np.concatenate([[D - 1, 0, 0], rng.integers(0, D, size=62)])      # 65 columns: two blocks
        for tag, cols in (("perm", perm), ("dup", dup), ("one", np.array([D - 1]))):
            o = m.top_rows({"counts": x}, cols=cols, k=k, draws=draws, exclude_stored=ex)
            assert o["columns"].dtype == torch.int32 and o["columns"].tolist() == cols.tolist(), tag
            assert tuple(o["rows"].shape) == (len(cols), k), tag
            sel = T(cols).to("cuda")
            assert torch.equal(o["rows"], one["rows"][sel]), (tag, k)
            assert torch.equal(o["scores"], one["scores"][sel]), (tag, k)
    empty = m.top_rows({"counts": x}, cols=[], k=3, draws=draws)
    assert tuple(empty["rows"].shape) == (0, 3) and tuple(empty["scores"].shape) == (0, 3)


def test_wide_k_runs_four_chunks_per_draw():
    """Poisson / linear K = 100: KP = 128, the wide-K encode sweep and four 32-float K chunks per draw."""
    B, D, K, S, k = 70, 45, 100, 3, 5
    cfg, x, params, mask, _ = _problem("poisson", B, D, K, S)
    m = _dense_model("poisson", cfg, mask, 32)
    mean = m.predict({"counts": x}, draws=params)["mean"].cpu().numpy()
    for ex in (True, False):
        out = m.top_rows({"counts": x}, k=k, draws=params, exclude_stored=ex)
        _assert_exact(out, mean, x, k, ex, f"K=100 exclude={ex}")


def test_c_abi_valid_call_refused_calls_and_empty_calls():
    """A raw valid call on an exactly sized scratch returns 0 and equals the method; every refused call (the draw
    stage's shared cases, _stream_cases.assert_shared_errors, then the entry's own) leaves the sentinel-filled
    outputs and the scratch untouched; n_cols = 0 returns 0 and writes nothing; a batch without rows returns 0 and
    fills both outputs with the padding."""
    from spmf_amd import _lib
    c = _case("poisson", 70, 45, 3, 2)
    m, x, params = c["m"], c["x"], c["params"]
    lib, h, k, D = _lib.load(), m._handle(), 5, 45
    good, need, out, scratch, no_u = gpu_good_call("toprows", m, x, params, k=k)
    rows, scores, cs, listed = out["rows"], out["scores"], good["ct"], good["keep"][-1]["cols"]
    raw = host_ctx(lib, 3, _lib.FLAG_MIXED)        # a mixed context nobody gave column types

    def untouched():
        torch.cuda.synchronize()
        return bool((rows == -7).all()) and bool((scores == -7.0).all()) and not bool(scratch.any())

    def after():
        assert untouched()
    try:
        call = assert_shared_errors(lib, "toprows", good, need, no_u, raw, after=after)
    finally:
        lib.spmf_ctx_destroy(raw)
    for kw in (dict(k=0), dict(k=65), dict(flags=2), dict(n=-1), dict(n=D + 1), dict(cols=None), dict(rows=None),
               dict(scores=None)):
        assert call(**kw) == -1, kw
        assert lib.spmf_last_error(h).decode().startswith("toprows_columns: "), kw
        assert untouched(), kw
    # the empty calls
    assert call(n=0) == 0 and untouched(), "n_cols = 0: nothing launched, nothing written"
    assert call(n=0, k=0) == -1 and untouched(), "errors come before the empty return"
    empty = type(cs).from_buffer_copy(cs)
    empty.n_rows, empty.nnz = 0, 0
    assert call(ct=empty, k=0) == -1 and untouched()
    assert call(ct=empty) == 0
    torch.cuda.synchronize()
    assert bool((rows == -1).all()) and bool(torch.isneginf(scores).all()) and not bool(scratch.any())
    # the valid call
    assert call() == 0
    torch.cuda.synchronize()
    want = m.top_rows({"counts": x}, cols=listed, k=k, draws=params)
    assert torch.equal(rows.long(), want["rows"]) and torch.equal(scores, want["scores"])
    full = m.top_rows({"counts": x}, k=k, draws=params)
    assert torch.equal(want["rows"], full["rows"][listed.long()])


def test_peak_memory_stays_below_the_materialised_block():
    """B = 4096, D = 2048, K = 8, S = 4, all columns: the peak over the call stays below the [B, C] fp32 block
    (32 MiB) plus the call's scratch: no [B, C] array is formed.  The result is 1.'s."""
    from spmf_amd import _lib
    from spmf_amd.sparse import SparseCounts
    B, D, K, S, k = 4096, 2048, 8, 4, 10
    cfg, x, params, mask = _dense_problem("poisson", B, D, K, S, 9700, density=0.05)
    m = _dense_model("poisson", cfg, mask, 256)
    batch = {"counts": SparseCounts.from_any(x, m.device, 256, latent_dim=K)}
    draws = {n: T(params[n]).to("cuda", torch.float32) for n in ("s", "u", "v", "w")}
    m.top_rows({"counts": x[:64].copy()}, k=k, draws=draws)
    scratch = int(_lib.load().spmf_toprows_scratch_bytes(m._handle(), B, S, D))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = m.top_rows(batch, k=k, draws=draws)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"peak above the allocation before the call: {extra / 2**20:.1f} MiB; B*C*4 = {B * D * 4 / 2**20:.1f} MiB, "
          f"scratch {scratch / 2**20:.1f} MiB")
    assert extra < B * D * 4 + scratch, (extra, scratch)
    mean = m.predict(batch, draws=draws)["mean"].cpu().numpy()
    _assert_exact(out, mean, x, k, True, "memory case")
