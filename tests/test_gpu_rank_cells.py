"""GPU: rank_cells (spmf_rank_cells, csrc/rank.hip) against the fp64 oracle and against top_k.

Oracle: _stream_cases._problem's fp64 scores [B,D] (the mean over the draws of the rate, of sigmoid(logit) on a
Bernoulli column).  The candidates of a row are its columns with a finite oracle score that, with stored cells
excluded, hold no count.  A rank is an integer and cannot be held against fp64 scores by a tolerance; it is held
by a bracket: with t the oracle score of the listed cell and s' those of the row's candidates other than the
cell itself,
    lo = #{s' > t + 1e-5 |t|}  <=  rank  <=  hi = #{s' >= t - 1e-5 |t|},
1e-5 being the project's relative bar on a score.  No cell is left out.  So that the bracket says something, the
share of cells with lo == hi is asserted on the oracle alone, before the GPU result is looked at: at least 95 %
in every case without mixed columns (the mixed cases have a third of their columns saturated at score 1.0, true
ties, and are held exactly by the tie and top_k tests).  `candidates` is the oracle's count exactly.  `score` is
within 1e-5 of the oracle relative to the cell's own score, |score - oracle| <= 1e-5 |oracle|, with no absolute
term (the bracket's own tolerance; the largest relative error over the cases is 8.6e-7).  The same float is also
held bit for bit to top_k's score by the link tests.

The link to top_k is exact and is what most tests lean on: for a listed cell that is not stored and has a finite
score, rank < k <=> top_k(k)["columns"][row, rank] is its column, and the two scores are equal bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from _stream_cases import _oracle_scores, _problem
from _problems import _dense_model, build_model, make_problem

pytestmark = pytest.mark.gpu
T = torch.as_tensor

# (lik, B, D, K, S): KP = 4 with ragged last row / column blocks and bitmap words that end inside a block; K = 16;
# K = 40 -> KP = 64 (two K chunks); K = 100 -> KP = 128
CASES = [(lik, 70, 150, 3, 2) for lik in ("poisson", "poisson_log", "bernoulli", "bernoulli_log", "mixed")] + [
    ("poisson", 131, 197, 16, 7), ("bernoulli", 131, 197, 16, 7),
    ("poisson", 65, 130, 40, 3), ("mixed", 65, 130, 40, 3),
    ("poisson", 67, 70, 100, 2)]
KEYS = ("rank", "candidates", "score")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, sel_a=None, sel_b=None):
    for k in KEYS:
        x = a[k] if sel_a is None else a[k][sel_a]
        y = b[k] if sel_b is None else b[k][sel_b]
        assert torch.equal(_bits(x), _bits(y)), k


def _oracle_ranks(score, x, exclude_stored):
    """From the oracle alone, per cell: lo, hi of the bracket and the candidates beside the cell, [B,D] each."""
    B, D = score.shape
    fin = np.isfinite(score)
    cand = fin & (~(x != 0) if exclude_stored else True)           # (NaN != 0: a NaN count is stored)
    lo, hi = np.zeros((B, D), dtype=np.int64), np.zeros((B, D), dtype=np.int64)
    for b in range(B):
        s = np.sort(score[b, cand[b]])
        t = np.where(fin[b], score[b], 0.0)
        tol = 1e-5 * np.abs(t)
        lo[b] = s.size - np.searchsorted(s, t + tol, side="right")
        hi[b] = s.size - np.searchsorted(s, t - tol, side="left") - cand[b]     # (the cell itself is in s)
    beside = cand.sum(1)[:, None] - cand
    return lo, hi, beside, cand, fin


def _cells(B, D, seed, mask=None):
    """The cells of mask [B,D] (None: all) in a seeded random order."""
    cell = np.arange(B * D) if mask is None else np.flatnonzero(mask.reshape(-1))
    cell = np.random.default_rng(seed).permutation(cell)
    return cell // D, cell % D


def _grid(out, rows, cols, B, D):
    """rank / candidates / score of the listed cells as [B,D] arrays (unlisted: -2 / -2 / NaN) on the host."""
    r = np.full((B, D), -2, dtype=np.int64)
    c = np.full((B, D), -2, dtype=np.int64)
    s = np.full((B, D), np.nan, dtype=np.float32)
    r[rows, cols] = out["rank"].cpu().numpy()
    c[rows, cols] = out["candidates"].cpu().numpy()
    s[rows, cols] = out["score"].cpu().numpy()
    return r, c, s


def _assert_link(rank, sc, top, x, exclude_stored, k, all_listed, tag=""):
    """rank / sc [B,D] (unlisted: -2 / NaN) against top_k's result."""
    cols = top["columns"].cpu().numpy().astype(np.int64)
    scores = top["scores"].cpu().numpy()
    B, D = rank.shape
    applies = (rank >= 0) & (~(x != 0) if exclude_stored else np.ones((B, D), dtype=bool))
    bb, dd = np.nonzero(applies & (rank < k))
    # rank < k  =>  entry `rank` of the row's result is the cell, with the same score bits
    assert (cols[bb, rank[bb, dd]] == dd).all(), (tag, "a cell ranked below k is not at its place in top_k")
    assert (scores[bb, rank[bb, dd]].view(np.int32) == sc[bb, dd].view(np.int32)).all(), (tag, "score bits")
    # entry j of the row's result is a listed cell  =>  its rank is j
    real = cols >= 0
    rb, rj = np.nonzero(real)
    got = rank[rb, cols[rb, rj]]
    listed = got != -2
    if all_listed:
        assert listed.all(), tag
        assert ((applies & (rank < k)).sum(1) == real.sum(1)).all(), (tag, "the cells ranked below k are top_k's")
    assert (got[listed] == rj[listed]).all(), (tag, "a cell of top_k has another rank")
    return int(len(bb))


@functools.lru_cache(maxsize=None)
def _every_cell(lik, B, D, K, S):
    """One call per case with every cell listed (shared, read-only): (model, rows, cols, out)."""
    cfg, x, params, mask, score = _problem(lik, B, D, K, S)
    m = _dense_model(lik, cfg, mask, 32)
    rows, cols = _cells(B, D, 700 + B + K)
    return m, rows, cols, m.rank_cells({"counts": x}, rows, cols, draws=params)


# ---- 1. against the oracle --------------------------------------------------------------------

@pytest.mark.parametrize("lik,B,D,K,S", CASES)
def test_every_cell_against_the_oracle_by_bracket(lik, B, D, K, S):
    cfg, x, params, mask, score = _problem(lik, B, D, K, S)
    lo, hi, beside, cand, fin = _oracle_ranks(score, x, True)
    assert fin.all() and (x != 0).any()
    tight = float((lo == hi).mean())
    print(f"{lik} {B}x{D} K={K} S={S}: tight brackets {100 * tight:.2f} %")
    if lik != "mixed":
        assert tight >= 0.95, tight                              # on the oracle alone
    m, rows, cols, out = _every_cell(lik, B, D, K, S)
    for k, dt in (("rank", torch.int32), ("candidates", torch.int32), ("score", torch.float32)):
        assert out[k].dtype == dt and tuple(out[k].shape) == (B * D,) and out[k].is_cuda, k
    rank, nc, sc = _grid(out, rows, cols, B, D)
    assert (nc == beside).all(), "candidates"
    smax = float(np.abs(score).max())
    err = np.abs(sc.astype(np.float64) - score)
    print(f"max |score - oracle| {err.max():.3e} (max|score| {smax:.6g}), relative to the cell's own score "
          f"{(err / np.abs(score)).max():.3e}; "
          f"rank outside its bracket: {int(((rank < lo) | (rank > hi)).sum())}")
    assert (err <= 1e-5 * np.abs(score)).all(), float(err.max())
    assert ((lo <= rank) & (rank <= hi)).all()
    # the summary is rank_summary's of these vectors
    from spmf_amd.heldout import rank_summary
    want = rank_summary(out["rank"], out["candidates"])
    assert out["n"] == B * D and out["n_excluded"] == 0
    assert all(out[k] == want[k] for k in ("n", "n_excluded", "hit_rate", "mrr", "auc"))


def test_a_listed_cell_that_the_batch_stores_is_ranked_against_the_unstored():
    """Every cell of the case is listed, stored ones included: a stored cell has a rank, and all of its row's
    candidates beside it (it is none itself); an unstored one has one fewer."""
    lik, B, D, K, S = CASES[5]
    cfg, x, params, mask, score = _problem(lik, B, D, K, S)
    m, rows, cols, out = _every_cell(lik, B, D, K, S)
    rank, nc, _ = _grid(out, rows, cols, B, D)
    stored = x != 0
    free = (~stored).sum(1)[:, None]
    assert stored.any() and (rank[stored] >= 0).all()
    assert (nc == np.where(stored, free, free - 1)).all()
    assert (rank <= nc).all()


# ---- 2. ties ------------------------------------------------------------------------------------

def test_exact_ties_rank_the_lower_column_first():
    """Column 40 is a copy of column 7 in u, v, w, s, eta and x: bit-equal scores in every row, ranks r and r + 1."""
    cfg, x, params, mask, _ = _problem("poisson", 70, 45, 3, 2, 9600)
    x = x.copy()
    params = {n: v.copy() for n, v in params.items()}
    params["u"][:, 40, :] = params["u"][:, 7, :]
    params["v"][:, :, 40] = params["v"][:, :, 7]
    params["w"][..., 40] = params["w"][..., 7]
    params["s"][..., 40] = params["s"][..., 7]
    eta = cfg.eta_i.clone()
    eta[0, 40] = eta[0, 7]
    cfg.eta_i = eta
    x[:, 40] = x[:, 7]
    x[:, [7, 40]] = 0
    m = _dense_model("poisson", cfg, mask, 32)
    rows = np.repeat(np.arange(70), 2)
    cols = np.tile([40, 7], 70)
    out = m.rank_cells({"counts": x}, rows, cols, draws=params)
    r = out["rank"].cpu().numpy().reshape(70, 2)
    s = out["score"].cpu().numpy().reshape(70, 2)
    assert (s[:, 0].view(np.int32) == s[:, 1].view(np.int32)).all()
    assert (r[:, 1] >= 0).all() and (r[:, 0] == r[:, 1] + 1).all(), r
    assert torch.equal(out["candidates"][0::2], out["candidates"][1::2])


# ---- 3. the link to top_k, exact ------------------------------------------------------------------

@pytest.mark.parametrize("exclude_stored", [True, False])
@pytest.mark.parametrize("lik,B,D,K,S", CASES)
def test_ranks_below_k_are_the_entries_of_top_k(lik, B, D, K, S, exclude_stored):
    cfg, x, params, mask, score = _problem(lik, B, D, K, S)
    m = _dense_model(lik, cfg, mask, 32)
    rows, cols = _cells(B, D, 800 + B + K, mask=(x == 0) if exclude_stored else None)
    out = m.rank_cells({"counts": x}, rows, cols, draws=params, exclude_stored=exclude_stored)
    top = m.top_k({"counts": x}, k=10, draws=params, exclude_stored=exclude_stored)
    rank, _, sc = _grid(out, rows, cols, B, D)
    n = _assert_link(rank, sc, top, x, exclude_stored, 10, True, tag=f"{lik} {B}x{D} K={K}")
    assert n == int((top["columns"] >= 0).sum()) >= B
    # the scores of top_k's entries, as tensors
    real = top["columns"] >= 0
    rb = torch.arange(B, device=real.device).unsqueeze(1).expand(B, 10)[real]
    mine = torch.as_tensor(sc, device=real.device)[rb, top["columns"][real].long()]
    assert torch.equal(_bits(mine), _bits(top["scores"][real]))
    assert out["hit_rate"][10] == n / out["n"]


# ---- 4. invariance ------------------------------------------------------------------------------

def test_order_duplicates_chunks_and_panel_range_give_identical_results():
    from spmf_amd.sparse import SparseCounts
    lik, B, D, K, S = CASES[5]
    cfg, x, params, mask, score = _problem(lik, B, D, K, S)
    m, rows, cols, one = _every_cell(lik, B, D, K, S)
    dev = one["rank"].device
    again = m.rank_cells({"counts": x}, rows, cols, draws=params)
    _same(again, one)
    p = np.random.default_rng(77).permutation(len(rows))
    perm = m.rank_cells({"counts": x}, rows[p], cols[p], draws=params)
    _same(perm, one, sel_b=T(p).to(dev))
    for k in ("n", "n_excluded", "hit_rate", "mrr", "auc"):
        assert perm[k] == one[k], k
    twice = m.rank_cells({"counts": x}, np.concatenate([rows, rows]), np.concatenate([cols, cols]), draws=params)
    _same(twice, one, sel_a=slice(0, len(rows)))
    _same(twice, one, sel_a=slice(len(rows), None))
    chunked = m.rank_cells({"counts": x}, rows, cols, draws=params, max_rows=64)      # 64 + 64 + 3 rows
    _same(chunked, one)
    devin = m.rank_cells({"counts": x}, T(rows).to("cuda", torch.int32), T(cols).cuda(), draws=params)
    _same(devin, one)
    sc = SparseCounts.from_any(x, m.device, 32, latent_dim=K)
    sel = (rows >= 32) & (rows < 96)
    ranged = m.rank_cells({"counts": sc, "panels": (1, 3)}, rows[sel] - 32, cols[sel], draws=params)
    own = m.rank_cells({"counts": x[32:96].copy()}, rows[sel] - 32, cols[sel], draws=params)
    _same(ranged, own)
    _same(ranged, one, sel_b=T(sel).to(dev))


def test_a_row_with_more_listed_cells_than_a_round_takes():
    """Row 5 lists all its 197 columns (seven rounds of 32), every other row one cell: each group alone gives
    the same results, and so does the list of every cell."""
    lik, B, D, K, S = CASES[5]
    cfg, x, params, mask, score = _problem(lik, B, D, K, S)
    m, rows_all, cols_all, every = _every_cell(lik, B, D, K, S)
    others = np.delete(np.arange(B), 5)
    rows = np.concatenate([np.full(D, 5), others])
    cols = np.concatenate([np.arange(D), (others * 37) % D])
    mixed = m.rank_cells({"counts": x}, rows, cols, draws=params)
    full_row = m.rank_cells({"counts": x}, rows[:D], cols[:D], draws=params)
    singles = m.rank_cells({"counts": x}, rows[D:], cols[D:], draws=params)
    _same(mixed, full_row, sel_a=slice(0, D))
    _same(mixed, singles, sel_a=slice(D, None))
    pos = np.empty((B, D), dtype=np.int64)
    pos[rows_all, cols_all] = np.arange(B * D)
    _same(mixed, every, sel_b=T(pos[rows, cols]).to(every["rank"].device))
    r = mixed["rank"][:D].cpu().numpy()
    free = np.flatnonzero(x[5] == 0)
    assert sorted(r[free].tolist()) == list(range(len(free))), "the unstored cells of a row are a permutation"


# ---- 5. edges -------------------------------------------------------------------------------------

def test_empty_list_batch_without_stored_entries_and_a_single_draw():
    cfg, x, params, mask, score = _problem("poisson", 70, 150, 3, 2)
    m = _dense_model("poisson", cfg, mask, 32)
    for e in ([], np.zeros(0, dtype=np.int64)):
        out = m.rank_cells({"counts": x}, e, e, draws=params)
        assert out["rank"].dtype == torch.int32 and out["candidates"].dtype == torch.int32
        assert out["score"].dtype == torch.float32 and out["rank"].is_cuda
        assert all(tuple(out[k].shape) == (0,) for k in KEYS)
        assert out["n"] == 0 and out["n_excluded"] == 0 and out["mrr"] != out["mrr"]
    # nothing stored: z = 0 in every row, every cell a candidate
    B, D = x.shape
    zero = np.zeros_like(x)
    rows, cols = _cells(B, D, 31)
    out = m.rank_cells({"counts": zero}, rows, cols, draws=params)
    rank, nc, sc = _grid(out, rows, cols, B, D)
    assert (nc == D - 1).all() and (np.sort(rank, axis=1) == np.arange(D)[None, :]).all()
    _assert_link(rank, sc, m.top_k({"counts": zero}, k=10, draws=params), zero, True, 10, True, tag="no entries")
    # S = 1, with and without a sample axis
    one = {n: params[n][:1] for n in ("s", "u", "v", "w")}
    a = m.rank_cells({"counts": x}, rows, cols, draws=one)
    b = m.rank_cells({"counts": x}, rows, cols, draws={n: v[0] for n, v in one.items()})
    _same(a, b)
    rank, nc, sc = _grid(a, rows, cols, B, D)
    lo, hi, beside, _, _ = _oracle_ranks(_oracle_scores(cfg, x, one, np.zeros(D, dtype=bool)), x, True)
    assert (nc == beside).all() and ((lo <= rank) & (rank <= hi)).all()
    _assert_link(rank, sc, m.top_k({"counts": x}, k=10, draws=one), x, True, 10, True, tag="S=1")


def test_nan_count_takes_its_rows_cells_out_and_leaves_the_others():
    cfg, x, params = make_problem(37, 23, 3, 3, 913, 0.3)
    clean = x.copy()
    clean[6, 11] = 1.0
    x[6, 11] = float("nan")
    m = build_model(cfg, 16)
    rows, cols = _cells(37, 23, 21)
    out = m.rank_cells({"counts": x}, rows, cols, draws=params)
    ref = m.rank_cells({"counts": clean}, rows, cols, draws=params)
    bad = T(rows == 6).to(out["rank"].device)
    assert bool((out["rank"][bad] == -1).all()) and bool((out["candidates"][bad] == 0).all())
    assert bool(torch.isnan(out["score"][bad]).all())
    _same(out, ref, sel_a=~bad, sel_b=~bad)
    assert bool((ref["rank"] >= 0).all())
    assert out["n_excluded"] == 23 and out["n"] == 36 * 23


def test_custom_codec_raises_after_the_argument_checks():
    from spmf_amd import PoissonFactorization
    cfg, x, params, mask, _ = _problem("poisson", 70, 150, 3, 2)
    mc = PoissonFactorization(latent_dim=3, feature_dim=150, encoder_function=lambda t: t,
                              decoder_function=lambda t: t, initialize_distributions=False,
                              device="cuda", panel_rows=32)
    with pytest.raises(ValueError):
        mc.rank_cells({"counts": x}, [0, 70], [0, 1], draws=params)
    with pytest.raises(NotImplementedError):
        mc.rank_cells({"counts": x}, [0], [0], draws=params)


# ---- 6. one slice -----------------------------------------------------------------------------------

def test_many_row_blocks_take_one_slice():
    """32 832 rows = 513 row blocks >= 2 * 256: one column slice per row block (ragged last block, three column
    blocks).  Two listed cells per row.  The first 64 rows as a batch of their own take the many-slices path."""
    B, D, K, S = 32832, 130, 3, 1
    cfg, x, params, mask, score = _problem("poisson", B, D, K, S)
    m = _dense_model("poisson", cfg, mask, 4096)
    rng = np.random.default_rng(61)
    rows = np.repeat(np.arange(B), 2)
    cols = rng.integers(0, D, size=2 * B)
    out = m.rank_cells({"counts": x}, rows, cols, draws=params)
    top = m.top_k({"counts": x}, k=10, draws=params)
    rank, nc, sc = _grid(out, rows, cols, B, D)
    n = _assert_link(rank, sc, top, x, True, 10, False, tag="one slice")
    assert n > B // 20
    assert bool((out["rank"] >= 0).all())
    lo, hi, beside, _, _ = _oracle_ranks(score[:256], x[:256], True)
    listed = rank[:256] != -2
    assert (nc[:256][listed] == beside[listed]).all()
    assert ((lo <= rank[:256]) & (rank[:256] <= hi))[listed].all()
    head = m.rank_cells({"counts": x[:64].copy()}, rows[:128], cols[:128], draws=params)
    _same(head, out, sel_b=slice(0, 128))


# ---- 7. the C-ABI on the device -----------------------------------------------------------------------

def test_c_abi_valid_call_short_scratch_and_sentinels():
    from spmf_amd import _lib
    from spmf_amd._lib import VAR_ORDER
    lik, B, D, K, S = CASES[0]
    cfg, x, params, mask, _ = _problem(lik, B, D, K, S)
    m, rows, cols, want = _every_cell(lik, B, D, K, S)
    lib, h = _lib.load(), m._handle()
    _, cs = m._batch({"counts": x})
    Sp, P = m._pack_params(params, names=("s", "u", "v", "w"))
    pin = _lib.PtrArray(*[P[n].data_ptr() if n in P else None for n in VAR_ORDER])
    eta = m._eta_device()
    N, pad = B * D, 100
    order = np.argsort(rows, kind="stable")
    r32 = T(rows[order]).to("cuda", torch.int32)
    c32 = T(cols[order]).to("cuda", torch.int32)
    need = int(lib.spmf_rank_scratch_bytes(h, int(cs.n_rows), Sp))
    assert need > 0 and need % 256 == 0
    scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    base = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    rank = torch.full((N + pad,), -7, dtype=torch.int32, device="cuda")
    cand = torch.full((N + pad,), -7, dtype=torch.int32, device="cuda")
    score = torch.full((N + pad,), -7.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(nbytes=need, n=N, flags=1):
        return lib.spmf_rank_cells(h, C.byref(cs), Sp, pin, eta.data_ptr(), n, r32.data_ptr(), c32.data_ptr(), flags,
                                   rank.data_ptr(), cand.data_ptr(), score.data_ptr(), base, nbytes, stream)
    assert call(nbytes=need - 256) == -3
    msg = lib.spmf_last_error(h).decode()
    assert str(need) in msg, msg
    assert call(flags=2) == -1 and call(n=-1) == -1
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((rank == -7).all()) and bool((cand == -7).all()) and bool((score == -7.0).all())
    assert not bool(scratch.any())
    assert call() == 0, lib.spmf_last_error(h).decode()
    torch.cuda.synchronize()
    assert bool((rank[N:] == -7).all()) and bool((cand[N:] == -7).all()) and bool((score[N:] == -7.0).all())
    assert bool((rank[:N] >= 0).all()) and bool((cand[:N] >= 0).all()) and bool((score[:N] != -7.0).all())
    o = T(order).to("cuda")
    assert torch.equal(rank[:N], want["rank"][o]) and torch.equal(cand[:N], want["candidates"][o])
    assert torch.equal(_bits(score[:N]), _bits(want["score"][o]))
    assert not bool(scratch[need + (base - scratch.data_ptr()):].any()), "a write behind the scratch"


def test_peak_memory_stays_below_the_materialised_tensors():
    """(131, 197, 16, 7), every cell listed: the call's peak above what was allocated before it stays below the
    8 S B D bytes of rate[S,B,D] and ll[S,B,D]."""
    from spmf_amd.sparse import SparseCounts
    lik, B, D, K, S = CASES[5]
    cfg, x, params, mask, _ = _problem(lik, B, D, K, S)
    m, rows, cols, want = _every_cell(lik, B, D, K, S)
    batch = {"counts": SparseCounts.from_any(x, m.device, 32, latent_dim=K)}
    draws = {n: T(params[n]).to("cuda", torch.float32) for n in ("s", "u", "v", "w")}
    r, c = T(rows).to("cuda", torch.int32), T(cols).to("cuda", torch.int32)
    m.rank_cells(batch, r[:10], c[:10], draws=draws)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = m.rank_cells(batch, r, c, draws=draws)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"peak above the allocation before the call: {extra} B; 8 S B D = {8 * S * B * D} B")
    assert extra < 8 * S * B * D, extra
    _same(out, want)
