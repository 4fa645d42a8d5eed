"""GPU: top_k (spmf_topk_rows, csrc/topk.hip) against the fp64 oracle.

Oracle: O.log_likelihood_components(...)["rate"] [S,B,D] fp64 (the logit on a Bernoulli
column: test_oracle_rate_is_the_logit_on_bernoulli_columns), sigmoid on the Bernoulli columns,
mean over the draws.  Bar: bar(v) = 1e-5 |v| + 1e-5 max|score|, the per-cell bar on 'rate' of
test_gpu_dense._assert_cells.  One helper (_check) holds a result against the oracle:
 (a) shapes, dtypes, columns in [0,D) or -1, distinct within a row, padding -1 / -inf at the
     tail only, min(k, #candidates) real slots;
 (b) scores non-increasing, equal scores in ascending column order;
 (c) only candidates are returned (finite score; not stored when stored cells are excluded);
 (d) every returned score within bar of the oracle's score of that cell;
 (e) every candidate not returned scores at most the row's last returned one + 2 bar;
 (f) on rows whose oracle gap between the k-th and (k+1)-th candidate exceeds 2 bar ("clear
     cut") the returned column set is the oracle's.
The share of clear-cut rows is asserted on the oracle alone before the GPU result is looked at.

Bernoulli damping: with the parameters of _dense_problem the Bernoulli probabilities saturate
and tie, so u and w of the two Bernoulli cases are scaled by _stream_cases.BERN_DAMP (a power of
two: the values stay fp32-exact).  Clear-cut rows on the CPU oracle with seed 9100+B+K at the three
shapes of SHAPES: CLEAR_ROWS below (asserted on the oracle in the test)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import spmf_oracle as O
from _stream_cases import _bern_cols, _oracle_scores, _problem
from _problems import LIKELIHOODS, _dense_model, build_model, make_problem

pytestmark = pytest.mark.gpu
T = torch.as_tensor

# (B, D, K, S, k): ragged 64 x 64 blocks and 32 x 32 tiles, K padded 3 -> 4, K = 16, K = 33 -> 64 (two K
# chunks), k = 5 / 10 / 64 (both candidate-buffer sizes), D = 333 = six column blocks.  Column slices the
# host rule picks on a 256-CU device (2 * 256 workgroups wanted, at most 16 slices, at most one per column
# block): 1, 4 and, for the 5-row batch, 6.  The rule is a static function of the library, not reachable
# from Python.
SHAPES = [(70, 45, 3, 2, 5), (131, 197, 16, 7, 10), (5, 333, 33, 3, 64)]
# Clear-cut rows of the CPU oracle at SHAPES (seed 9100+B+K): the counts recorded for poisson, mixed and
# poisson_log when the cases were set, and for the two Bernoulli cases when their damping was chosen.  A case
# asserts, on the oracle alone, that its shape has at least its recorded count and that the likelihood's share
# over the rows of the three shapes together is at least MIN_CLEAR (poisson_log: 192/206 = 93 %; its 5-row shape
# alone is 4/5).
CLEAR_ROWS = {"poisson": (70, 131, 5), "mixed": (70, 131, 5), "poisson_log": (62, 126, 4),
              "bernoulli": (65, 130, 5), "bernoulli_log": (70, 129, 5)}
MIN_CLEAR = {"poisson": 1.0, "mixed": 1.0, "poisson_log": 0.85, "bernoulli": 0.90, "bernoulli_log": 0.90}


def _bar(v, smax):
    return 1e-5 * np.abs(v) + 1e-5 * smax


def _oracle_view(score, x, k, exclude_stored):
    """From the oracle alone: candidates, max|score|, per row the clear-cut flag and the top-k set."""
    B, D = score.shape
    fin = np.isfinite(score)
    smax = float(np.abs(score[fin]).max()) if fin.any() else 0.0
    cand = fin & (~(x != 0) if exclude_stored else True)          # (NaN != 0: a NaN count is stored)
    nc = cand.sum(1)
    srt = -np.sort(-np.where(cand, score, -np.inf), axis=1)
    srt = np.concatenate([srt, np.full((B, k + 1), -np.inf)], axis=1)
    kth, nxt = srt[:, k - 1], srt[:, k]
    with np.errstate(invalid="ignore"):
        clear = (nc <= k) | (kth - nxt > 2 * _bar(kth, smax))
    top = cand & (score >= np.where(nc > k, kth, -np.inf)[:, None])
    return cand, smax, nc, clear, top


def _check(out, score, x, k, exclude_stored=True, min_clear=None, tag=""):
    B, D = score.shape
    cand, smax, nc, clear, top = _oracle_view(score, x, k, exclude_stored)
    print(f"{tag}: clear-cut rows {int(clear.sum())}/{B}, max|score| {smax:.6g}")
    if min_clear is not None:
        assert clear.sum() >= np.ceil(min_clear * B - 1e-9), (tag, int(clear.sum()), B)
    cols, scores = out["columns"], out["scores"]
    # (a)
    assert cols.dtype == torch.int32 and scores.dtype == torch.float32, tag
    assert tuple(cols.shape) == (B, k) and tuple(scores.shape) == (B, k), (tag, cols.shape, scores.shape)
    assert cols.is_cuda and scores.is_cuda, tag
    c = cols.cpu().numpy().astype(np.int64)
    s = scores.cpu().numpy().astype(np.float64)
    real = c >= 0
    n = np.minimum(k, nc)
    assert ((c >= -1) & (c < D)).all(), tag
    assert (real == (np.arange(k)[None, :] < n[:, None])).all(), (tag, "real slots / padding at the tail")
    assert (c[~real] == -1).all() and np.isneginf(s[~real]).all(), tag
    cs = np.sort(np.where(real, c, -1 - np.arange(k)[None, :]), axis=1)
    assert (np.diff(cs, axis=1) != 0).all(), (tag, "distinct columns")
    # (b)
    both = real[:, 1:] & real[:, :-1]
    with np.errstate(invalid="ignore"):                    # (-inf) - (-inf) between two padding slots
        ds = np.where(both, s[:, 1:] - s[:, :-1], -1.0)
    assert (ds <= 0).all(), (tag, "order")
    assert (c[:, 1:] > c[:, :-1])[both & (ds == 0)].all(), (tag, "ties by column")
    # (c)
    rows = np.broadcast_to(np.arange(B)[:, None], (B, k))
    cc = np.where(real, c, 0)
    assert cand[rows, cc][real].all(), (tag, "a returned cell is no candidate")
    # (d)
    ref = score[rows, cc]
    err = np.abs(s - ref)[real]
    print(f"{tag}: max |score - oracle| {err.max() if err.size else 0.0:.3e}")
    assert (err <= _bar(ref[real], smax)).all(), (tag, float(err.max()))
    # (e)
    ret = np.zeros((B, D), dtype=bool)
    ret[rows[real], c[real]] = True
    rest = np.where(cand & ~ret, score, -np.inf).max(1)
    has = n > 0
    last = ref[np.arange(B), np.maximum(n - 1, 0)]
    assert (rest[has] <= last[has] + 2 * _bar(last[has], smax)).all(), (tag, "a better candidate was missed")
    assert not (cand & ~ret)[~has].any(), tag
    # (f)
    assert (ret[clear] == top[clear]).all(), (tag, "column set on clear-cut rows")
    return clear


def _run(lik, B, D, K, S, k, exclude_stored=True, seed=None, min_clear=None, panel_rows=32, tag=""):
    cfg, x, params, mask, score = _problem(lik, B, D, K, S, seed)
    min_clear = MIN_CLEAR[lik] if min_clear is None else min_clear
    # the condition on the inputs, on the oracle alone
    clear = _oracle_view(score, x, k, exclude_stored)[3]
    assert clear.sum() >= np.ceil(min_clear * B - 1e-9), (tag, int(clear.sum()), B)
    m = _dense_model(lik, cfg, mask, panel_rows)
    out = m.top_k({"counts": x}, k=k, draws=params, exclude_stored=exclude_stored)
    _check(out, score, x, k, exclude_stored, min_clear, tag or f"{lik} {B}x{D} K={K} S={S} k={k}")
    return m, out


def test_oracle_rate_is_the_logit_on_bernoulli_columns():
    """The oracle's 'rate' on a Bernoulli column is the logit: ll = x * rate - softplus(rate)."""
    for lik in ("bernoulli", "bernoulli_log", "mixed"):
        cfg, x, params, mask, _ = _problem(lik, 70, 45, 3, 2)
        r = O.log_likelihood_components(cfg, T(x), T(params["s"]), T(params["u"]), T(params["v"]),
                                        T(params["w"]))
        b = T(_bern_cols(lik, mask, 45))
        rate, ll = r["rate"][..., b], r["log_likelihood"][..., b]
        want = T(x)[:, b] * rate - torch.nn.functional.softplus(rate)
        assert torch.allclose(ll, want, rtol=1e-12, atol=1e-12), lik


@functools.lru_cache(maxsize=None)
def _clear_counts(lik):
    """Clear-cut rows of the oracle at each of SHAPES."""
    out = []
    for B, D, K, S, k in SHAPES:
        _, x, _, _, score = _problem(lik, B, D, K, S)
        out.append(int(_oracle_view(score, x, k, True)[3].sum()))
    return tuple(out)


@pytest.mark.parametrize("B,D,K,S,k", SHAPES)
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_every_likelihood_at_ragged_tiles(lik, B, D, K, S, k):
    """Every likelihood code at SHAPES (module docstring).  Bernoulli: u and w damped by 1/64, clear-cut
    rows on the CPU oracle 65/70, 130/131, 5/5 (undamped 0 at the two larger shapes; 1/16 gives 78/131 and
    0/5, 1/32 still 0/5).  Bernoulli + log_transform: damped by 1/8, 70/70, 129/131, 5/5 (1/16: 3/5 at
    the last shape).  The condition on the inputs is asserted on the oracle alone, before the GPU runs:
    the shape's recorded count (CLEAR_ROWS) and the likelihood's share over the three shapes.  B = 5 runs
    the few-rows column split: 6 slices on a 256-CU device; (131, 197): 4 slices; (70, 45): one column
    block, the kernel writes the result itself."""
    counts = _clear_counts(lik)
    i = SHAPES.index((B, D, K, S, k))
    assert counts[i] >= CLEAR_ROWS[lik][i], (lik, counts)
    assert sum(counts) >= MIN_CLEAR[lik] * sum(sh[0] for sh in SHAPES), (lik, counts)
    _run(lik, B, D, K, S, k, min_clear=CLEAR_ROWS[lik][i] / B)


def test_wide_k_runs_four_chunks_per_draw():
    """Poisson K = 128: the wide-K encode sweep and four 32-float K chunks per draw."""
    _run("poisson", 40, 70, 128, 3, 7)


def test_a_slice_sweeps_several_column_blocks():
    """D = 2100 is 33 column blocks: 11 slices of three blocks each on a 256-CU device, so the
    threshold and the candidate buffer of a row are carried from block to block (both buffer sizes:
    k = 7 and k = 20).  Clear-cut rows on the CPU oracle: 20/20 in both."""
    _run("poisson", 20, 2100, 4, 2, 7)
    _run("poisson_log", 20, 2100, 4, 2, 20)


def test_many_row_blocks_take_one_slice():
    """32 832 rows = 513 row blocks >= 2 * 256: one slice sweeps all three column blocks and
    writes the final result, no merge.  Clear-cut rows on the CPU oracle: 32758/32832."""
    _run("poisson", 32832, 130, 3, 2, 5, min_clear=0.99, panel_rows=4096)


def test_stored_cells_may_be_returned_when_not_excluded():
    _run("poisson", 70, 45, 3, 2, 5, exclude_stored=False)
    _run("poisson", 131, 197, 16, 7, 10, exclude_stored=False)


def _edge_problem():
    cfg, x, params = make_problem(70, 45, 5, 4, 77, 0.25)
    x[5, :] = 1 + (np.arange(45) % 4)
    x[5, 2] = 0
    return cfg, x, params


def test_empty_rows_an_empty_column_and_a_nearly_full_row():
    """make_problem leaves rows 1, B-1 and column 2 empty; row 5 is stored in all but column 2:
    with k = 5 it has one real result and four padding slots."""
    cfg, x, params = _edge_problem()
    assert (x[1] == 0).all() and (x[69] == 0).all() and (x[:, 2] == 0).all() and (x[5] != 0).sum() == 44
    score = _oracle_scores(cfg, x, params, np.zeros(45, dtype=bool))
    out = build_model(cfg, 32).top_k({"counts": x}, k=5, draws=params)
    _check(out, score, x, 5, tag="edges")
    c = out["columns"].cpu().numpy()
    assert c[5].tolist() == [2, -1, -1, -1, -1]
    assert (c[1] >= 0).all() and (c[69] >= 0).all()


@pytest.mark.parametrize("B,k,S", [(1, 5, 3), (70, 1, 2), (70, 5, 1)])
def test_single_row_single_result_single_draw(B, k, S):
    cfg, x, params, mask, score = _problem("poisson", B, 45, 3, S, 9500 + B + k + S)
    m = _dense_model("poisson", cfg, mask, 32)
    out = m.top_k({"counts": x}, k=k, draws=params)
    _check(out, score, x, k, tag=f"B={B} k={k} S={S}")
    if S == 1:   # a point estimate without a sample axis
        one = m.top_k({"counts": x}, k=k, draws={n: params[n][0] for n in ("s", "u", "v", "w")})
        assert torch.equal(one["columns"], out["columns"]) and torch.equal(one["scores"], out["scores"])


def test_nan_count_takes_its_row_out():
    """x[6, 11] = NaN: z of row 6 is NaN in every draw, so the row has no candidates (checked on
    the oracle first); every other row matches the oracle."""
    cfg, x, params = make_problem(37, 23, 3, 3, 913, 0.3)
    x[6, 11] = float("nan")
    score = _oracle_scores(cfg, x, params, np.zeros(23, dtype=bool))
    assert not np.isfinite(score[6]).any() and np.isfinite(np.delete(score, 6, axis=0)).all()
    out = build_model(cfg, 16).top_k({"counts": x}, k=4, draws=params)
    _check(out, score, x, 4, tag="NaN row")
    assert (out["columns"][6] == -1).all() and torch.isneginf(out["scores"][6]).all()


def test_exact_ties_return_the_lower_column_first():
    """Column 40 is a copy of column 7 in u, v, w, s, eta and x: bit-equal scores in every row.
    Unstored, the two are neighbours in the result, 7 before 40."""
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
    x[:, [7, 40]] = 0                         # candidates in every row
    score = _oracle_scores(cfg, x, params, np.zeros(45, dtype=bool))
    # (the fp64 matrix products of the oracle may order a column's sums differently: equal to rounding there,
    # bit-equal on the device, which is what the test is about)
    np.testing.assert_allclose(score[:, 40], score[:, 7], rtol=1e-13)
    score[:, 40] = score[:, 7]
    m = _dense_model("poisson", cfg, mask, 32)
    k = 45
    out = m.top_k({"counts": x}, k=k, draws=params)
    _check(out, score, x, k, tag="ties")
    c, s = out["columns"].cpu().numpy(), out["scores"].cpu().numpy()
    for b in range(70):
        i7, i40 = int(np.where(c[b] == 7)[0][0]), int(np.where(c[b] == 40)[0][0])
        assert i40 == i7 + 1 and s[b, i7] == s[b, i40], (b, i7, i40)


def test_row_chunks_batches_factory_and_panel_minibatch():
    """max_rows = 32 at panel_rows = 32 (five chunks), an iterable of two batches and a factory
    against the single call: identical bits.  A panels minibatch with p0 > 0 is rows
    p0 * panel_rows ... of the full result."""
    from spmf_amd.sparse import SparseCounts
    cfg, x, params, mask, score = _problem("poisson", 131, 197, 16, 7)
    m = _dense_model("poisson", cfg, mask, 32)
    one = m.top_k({"counts": x}, k=10, draws=params)
    _check(one, score, x, 10, tag="single call")
    parts = [{"counts": x[:64].copy()}, {"counts": x[64:].copy()}]
    for tag, o in (("chunked", m.top_k({"counts": x}, k=10, draws=params, max_rows=32)),
                   ("two batches", m.top_k(parts, k=10, draws=params)),
                   ("factory", m.top_k(lambda: iter(parts), k=10, draws=params))):
        assert torch.equal(o["columns"], one["columns"]), tag
        assert torch.equal(o["scores"], one["scores"]), tag
    sc = SparseCounts.from_any(x, m.device, 32, latent_dim=16)
    mini = m.top_k({"counts": sc, "panels": (1, 3)}, k=10, draws=params)
    assert torch.equal(mini["columns"], one["columns"][32:96])
    assert torch.equal(mini["scores"], one["scores"][32:96])


def test_two_calls_return_identical_bits():
    for lik, shape in (("poisson", SHAPES[1]), ("mixed", SHAPES[2])):
        B, D, K, S, k = shape
        cfg, x, params, mask, _ = _problem(lik, B, D, K, S)
        m = _dense_model(lik, cfg, mask, 32)
        a = m.top_k({"counts": x}, k=k, draws=params)
        b = m.top_k({"counts": x}, k=k, draws=params)
        assert torch.equal(a["columns"], b["columns"]) and torch.equal(a["scores"], b["scores"]), lik


def test_agrees_with_the_materialising_path():
    """log_likelihood_components -> mean over the draws -> torch.topk on a clear-cut Poisson
    problem: the same column sets."""
    B, D, K, S, k = SHAPES[1]
    cfg, x, params, mask, score = _problem("poisson", B, D, K, S)
    assert _oracle_view(score, x, k, True)[3].all()
    m = _dense_model("poisson", cfg, mask, 32)
    rate = m.log_likelihood_components(s=params["s"], u=params["u"], v=params["v"], w=params["w"],
                                       data={"counts": x})["rate"]
    dense = rate.mean(0).masked_fill(T(x != 0).to(rate.device), float("-inf"))
    want = torch.topk(dense, k, dim=1).indices.sort(1).values
    got = m.top_k({"counts": x}, k=k, draws=params)["columns"].long().sort(1).values
    assert torch.equal(got, want)


def test_peak_memory_stays_far_below_the_materialised_tensor():
    """B = 1024, D = 2048, K = 16, S = 32, k = 10: the streaming call may take a quarter of one
    [S,B,D] fp32 tensor (268 MB)."""
    from spmf_amd.sparse import SparseCounts
    B, D, K, S, k = 1024, 2048, 16, 32, 10
    cfg, x, params, mask, score = _problem("poisson", B, D, K, S, 9700, 0.05)
    m = _dense_model("poisson", cfg, mask, 256)
    batch = {"counts": SparseCounts.from_any(x, m.device, 256, latent_dim=K)}
    draws = {n: T(params[n]).to("cuda", torch.float32) for n in ("s", "u", "v", "w")}
    m.top_k({"counts": x[:64].copy()}, k=k, draws=draws)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = m.top_k(batch, k=k, draws=draws)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"peak above the allocation before the call: {extra / 2**20:.1f} MiB; "
          f"S*B*D*4 = {S * B * D * 4 / 2**20:.1f} MiB")
    assert extra < 0.25 * S * B * D * 4, extra
    _check(out, score, x, k, tag="memory case")


def test_a_step_is_undisturbed_by_a_top_k_call():
    """The call uses its own scratch: a deterministic step before and after it gives identical
    parts and gradients."""
    from spmf_amd import PoissonFactorization
    cfg, x, params = make_problem(200, 150, 16, 2, 5000, 0.05)
    m = PoissonFactorization(latent_dim=16, feature_dim=150, u_tau_scale=cfg.u_tau_scale,
                             column_norms=cfg.eta_i, initialize_distributions=False, device="cuda",
                             panel_rows=64, deterministic=True)
    m.xi_u_global = cfg.xi_u_global
    batch = {"counts": x}
    p1, g1, n1 = m.energy_and_grads(batch, params)
    p1 = {n: v.clone() for n, v in p1.items()}
    g1 = {n: v.clone() for n, v in g1.items()}
    out = m.top_k(batch, k=10, draws=params)
    assert tuple(out["columns"].shape) == (200, 10)
    p2, g2, n2 = m.energy_and_grads(batch, params)
    for n in p1:
        assert torch.equal(p1[n], p2[n]), n
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    assert torch.equal(n1, n2)


def test_bad_k_and_custom_codec_raise_before_any_launch():
    cfg, x, params, mask, _ = _problem("poisson", 70, 45, 3, 2)
    m = _dense_model("poisson", cfg, mask, 32)
    for k in (0, 65):
        with pytest.raises(ValueError):
            m.top_k({"counts": x}, k=k, draws=params)
    from spmf_amd import PoissonFactorization
    mc = PoissonFactorization(latent_dim=3, feature_dim=45, encoder_function=lambda t: t,
                              decoder_function=lambda t: t, initialize_distributions=False,
                              device="cuda", panel_rows=32)
    with pytest.raises(NotImplementedError):
        mc.top_k({"counts": x}, k=5, draws=params)
    with pytest.raises(NotImplementedError):
        mc.waic_streaming({"counts": x}, draws=params)


def test_c_abi_errors_launch_nothing():
    """Through ctypes: S = 0 and a misaligned scratch are SPMF_E_ARG (-1), a short scratch is
    SPMF_E_WORKSPACE (-3) and names the need; the outputs keep their sentinel."""
    from spmf_amd import _lib
    from spmf_amd._lib import VAR_ORDER
    cfg, x, params, mask, _ = _problem("poisson", 70, 45, 3, 2)
    m = _dense_model("poisson", cfg, mask, 32)
    lib, h = _lib.load(), m._handle()
    _, cs = m._batch({"counts": x})
    S, P = m._pack_params(params, names=("s", "u", "v", "w"))
    pin = _lib.PtrArray(*[P[n].data_ptr() if n in P else None for n in VAR_ORDER])
    eta = m._eta_device()
    k = 5
    need = int(lib.spmf_topk_scratch_bytes(h, int(cs.n_rows), S))
    assert need > 0 and need % 256 == 0
    assert int(lib.spmf_topk_scratch_bytes(h, int(cs.n_rows), 0)) == 0
    scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    base = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    cols = torch.full((70, k), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((70, k), -7.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(S_, ptr, nbytes, k_=k, flags=1):
        return lib.spmf_topk_rows(h, C.byref(cs), S_, pin, eta.data_ptr(), k_, flags, cols.data_ptr(),
                                  scores.data_ptr(), ptr, nbytes, stream)
    assert call(0, base, need) == -1
    assert call(S, base + 4, need) == -1
    assert call(S, base, need, k_=0) == -1 and call(S, base, need, k_=65) == -1
    assert call(S, base, need, flags=2) == -1
    assert call(S, base, need - 256) == -3
    msg = lib.spmf_last_error(h).decode()
    assert str(need) in msg, msg
    torch.cuda.synchronize()
    assert bool((cols == -7).all()) and bool((scores == -7.0).all()) and not bool(scratch.any())
    assert call(S, base, need) == 0
    torch.cuda.synchronize()
    want = m.top_k({"counts": x}, k=k, draws=params)
    assert torch.equal(cols, want["columns"]) and torch.equal(scores, want["scores"])
