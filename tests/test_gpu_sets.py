"""GPU: set_scores (spmf_set_scores, csrc/sets.hip).

Two references.  (1) The fp64 oracle: per draw m_s = rate | sigmoid(rate) of test_gpu_predict._per_draw (the
'ms' of test_gpu_predict._case), score_s(b, g) = sum_j w_j m_s(b, c_j) in numpy.  Every cell carries the bar of
test_gpu_predict._bar, bar(v) = 1e-5 |v| + 1e-5 max|m| with the maximum over all per-draw cells of the problem --
on a mixed problem over the cells of the column's own type, as test_gpu_groups does; the bars are summed with
|w_j| over the set and averaged over the draws: mean lies within that.  sd lies within 2 max_s of the summed
bars (each score_s is off by at most its summed bar, and the deviation moves by at most sqrt(S / (S - 1)) <=
sqrt 2 times the largest perturbation).  That the comparison says something is asserted on the oracle first:
every non-empty set with weight 1 has a mean above ten times its bar, and on the set of all columns at least
0.4 of the rows have an oracle sd above ten times the sd bound.  (2) The cells of predict: predict(draws = draw s
alone)["mean"] has the fp32 bits of m_s; their weighted sums in numpy fp64.  mean equals it within
1e-12 (1/S) sum_s sum_j |w_j m_s| -- at most 333 + S addends reordered at 2^-53 each is 4e-14, any fp32
accumulation shows at 1e-7 -- and sd within 1e-9 max_s sum_j |w_j m_s|: the fp64 variance error S eps max^2 over
2 sd stays below that for sd >= 1e-6 max, an fp32 fold is again 1e-7.
Everything else is bit for bit: a repeat, a set alone, a set at another position, row chunks, runs of sets.
The weights are drawn as fp64 and rounded to fp32 once, so that the references use the numbers the kernel
sees."""
import functools

import numpy as np
import pytest
import torch

from _problems import LIKELIHOODS, _dense_model, _dense_problem, build_model, make_problem
from _stream_cases import SHAPES, _bar, _case, assert_shared_errors, gpu_good_call, host_ctx

pytestmark = pytest.mark.gpu
T = torch.as_tensor
REL, REL_SD = 1e-12, 1e-9
# test_gpu_predict's shapes and one draw above a draw chunk (csrc/kernels.h kSetDrawChunk = 8)
SET_SHAPES = SHAPES + [(70, 45, 3, 9)]
NAMES = ("all", "last", "empty", "dup", "three", "dup_reversed")


def _sets(D):
    """The six sets of a shape: all columns; the last column; the empty set; 65 entries that start D-1, 0, 0 (a
    duplicate, a block edge crossed); 130 entries (three blocks, more listed columns than D = 45 has); the
    fourth reversed."""
    rng = np.random.default_rng(1300 + D)
    dup = np.concatenate([[D - 1, 0, 0], rng.integers(0, D, 62)]).astype(np.int64)
    three = rng.integers(0, D, 130).astype(np.int64)
    return [np.arange(D, dtype=np.int64), np.array([D - 1], dtype=np.int64), np.zeros(0, dtype=np.int64), dup,
            three, dup[::-1].copy()]


def _weights(D, sets):
    """Signed weights, |w| in [0.25, 2), fp32-exact; the reversed set carries the reversed weights of its twin."""
    rng = np.random.default_rng(1400 + D)
    w = [(rng.uniform(0.25, 2.0, len(s)) * rng.choice([-1.0, 1.0], len(s))).astype(np.float32).astype(np.float64)
         for s in sets]
    w[5] = w[3][::-1].copy()
    return w


def _scores(cells, sets, weights):
    """cells [S,B,D] fp64 -> (score_s [S,B,G], sum_j |w_j cell| [S,B,G]) in numpy fp64."""
    S, B = cells.shape[:2]
    sc, mag = np.zeros((S, B, len(sets))), np.zeros((S, B, len(sets)))
    for g, cols in enumerate(sets):
        w = np.ones(len(cols)) if weights is None else weights[g]
        sc[:, :, g] = (cells[:, :, cols] * w).sum(-1)
        mag[:, :, g] = np.abs(cells[:, :, cols] * w).sum(-1)
    return sc, mag


def _oracle_view(ms, bern, sets, weights):
    """From the oracle alone: (score_s [S,B,G], the summed bar of every score_s [S,B,G])."""
    mmax = np.full(ms.shape[2], float(np.abs(ms).max()))
    if bern.any() and not bern.all():
        mmax = np.where(bern, np.abs(ms[:, :, bern]).max(), np.abs(ms[:, :, ~bern]).max())
    ref, _ = _scores(ms, sets, weights)
    _, bar = _scores(_bar(ms, mmax), sets, weights)
    return ref, bar


def _route(m, x, params):
    """predict one draw at a time: fp64 [S,B,D] with the bits of the fp32 cells m_s."""
    S = int(params["u"].shape[0])
    return np.stack([m.predict({"counts": x}, draws={n: params[n][s:s + 1] for n in ("s", "u", "v", "w")})["mean"]
                     .cpu().double().numpy() for s in range(S)])


@functools.lru_cache(maxsize=None)
def _scase(lik, B, D, K, S):
    """test_gpu_predict._case plus predict's per-draw cells, the sets and the full set_scores with and without
    weights; computed once and shared (read-only)."""
    c = dict(_case(lik, B, D, K, S))
    c["cells"] = _route(c["m"], c["x"], c["params"])
    c["sets"] = _sets(D)
    c["weights"] = _weights(D, c["sets"])
    data = {"counts": c["x"]}
    c["res"] = {"ones": c["m"].set_scores(data, c["sets"], draws=c["params"], sd=True),
                "signed": c["m"].set_scores(data, c["sets"], c["weights"], draws=c["params"], sd=True)}
    return c


def _i64(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float64 and torch.equal(_i64(a), _i64(b))


def _check_oracle(c, S):
    sets = c["sets"]
    filled = np.array([len(s) > 0 for s in sets])
    for kind, weights in (("ones", None), ("signed", c["weights"])):
        res = c["res"][kind]
        ref_s, bar_s = _oracle_view(c["ms"], c["bern"], sets, weights)
        ref, bar = ref_s.mean(0), bar_s.mean(0)
        _, mag = _scores(np.abs(c["ms"]), sets, weights)
        print(f"{kind}: smallest sum|w m| / bar {float((mag.mean(0)[:, filled] / bar[:, filled]).min()):.1f}")
        if weights is None:        # on the oracle alone
            assert (ref[:, filled] > 10.0 * bar[:, filled]).all(), float((ref[:, filled] / bar[:, filled]).min())
        got = res["mean"].cpu().numpy()
        assert res["mean"].dtype == torch.float64 and got.shape == ref.shape
        err = np.abs(got - ref)
        print(f"{kind}: max |mean - oracle| {err.max():.3e}, worst err/bar "
              f"{float((err[:, filled] / bar[:, filled]).max()):.3f}")
        assert (err <= bar).all(), (kind, float(err.max()))
        assert (got[:, ~filled] == 0).all(), kind
        ref_sd, bound = ref_s.std(axis=0, ddof=1), 2.0 * bar_s.max(axis=0)
        share = float((ref_sd[:, 0] > 10.0 * bound[:, 0]).mean())
        print(f"{kind}: share of rows with sd > 10 bound on the set of all columns {share:.3f}")
        if weights is None:        # on the oracle alone
            assert share >= 0.4, share
        got_sd = res["sd"].cpu().numpy()
        err = np.abs(got_sd - ref_sd)
        print(f"{kind}: max |sd - oracle| {err.max():.3e}, worst err/bound "
              f"{float((err[:, filled] / bound[:, filled]).max()):.3f}")
        assert np.isfinite(got_sd).all() and (err <= bound).all(), (kind, float(err.max()))
        assert (got_sd[:, ~filled] == 0).all(), kind
        assert res["sizes"].dtype == torch.int64 and res["sizes"].cpu().tolist() == [len(s) for s in sets]


def _check_cells(c, S):
    for kind, weights in (("ones", None), ("signed", c["weights"])):
        res = c["res"][kind]
        ref_s, mag_s = _scores(c["cells"], c["sets"], weights)
        got, got_sd = res["mean"].cpu().numpy(), res["sd"].cpu().numpy()
        err, mag = np.abs(got - ref_s.mean(0)), mag_s.mean(0)
        print(f"{kind}: max |mean - sum of predict's cells| / mean sum|w m| "
              f"{float((err / np.maximum(mag, 1e-300)).max()):.3e}")
        assert np.isfinite(got).all() and (err <= REL * mag).all(), (kind, float(err.max()))
        err, top = np.abs(got_sd - ref_s.std(axis=0, ddof=1)), mag_s.max(axis=0)
        print(f"{kind}: max |sd - sd of the sums of predict's cells| / max sum|w m| "
              f"{float((err / np.maximum(top, 1e-300)).max()):.3e}")
        assert (err <= REL_SD * top).all(), (kind, float(err.max()))


@pytest.mark.parametrize("B,D,K,S", SET_SHAPES)
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_mean_and_sd_against_the_oracle(lik, B, D, K, S):
    _check_oracle(_scase(lik, B, D, K, S), S)


@pytest.mark.parametrize("B,D,K,S", SET_SHAPES)
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_scores_are_the_fp64_sums_of_predicts_cells(lik, B, D, K, S):
    _check_cells(_scase(lik, B, D, K, S), S)


@pytest.mark.parametrize("B,D,K,S", SET_SHAPES)
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_repeats_and_variants_give_the_same_bits(lik, B, D, K, S):
    c = _scase(lik, B, D, K, S)
    m, params, sets, weights = c["m"], c["params"], c["sets"], c["weights"]
    data = {"counts": c["x"]}
    for kind, wts in (("ones", None), ("signed", weights)):
        full = c["res"][kind]

        def run(idx, **kw):
            return m.set_scores(data, [sets[g] for g in idx], None if wts is None else [wts[g] for g in idx],
                                draws=params, **kw)
        again = run(range(6), sd=True)
        for n in ("mean", "sd"):
            assert _same(again[n], full[n]), (kind, n)
        assert "sd" not in run(range(6)) and _same(run(range(6))["mean"], full["mean"]), "a mean-only call"
        for g in range(6):                 # alone
            out = run([g], sd=True)
            for n in ("mean", "sd"):
                assert _same(out[n], full[n][:, g:g + 1].contiguous()), (kind, NAMES[g], n)
        order = [4, 2, 0, 5, 1, 3]         # at another position, beside other neighbours
        moved = run(order, sd=True)
        chunked = run(range(6), sd=True, max_rows=64)
        one_per_run = run(range(6), sd=True, max_listed=64)
        for n in ("mean", "sd"):
            assert _same(moved[n], full[n][:, order].contiguous()), (kind, n, "moved")
            assert _same(chunked[n], full[n]), (kind, n, "max_rows")
            assert _same(one_per_run[n], full[n]), (kind, n, "max_listed")
        # the same multiset in reverse order: the same sum up to the fp64 reordering
        _, mag_s = _scores(c["cells"], sets, wts)
        mean, sd = full["mean"].cpu().numpy(), full["sd"].cpu().numpy()
        assert (np.abs(mean[:, 3] - mean[:, 5]) <= REL * mag_s.mean(0)[:, 3]).all(), kind
        assert (np.abs(sd[:, 3] - sd[:, 5]) <= REL_SD * mag_s.max(0)[:, 3]).all(), kind


def test_more_sets_than_one_fill_launch_takes():
    """300 sets of 0 .. 5 columns in one library call: the fill kernel takes the offsets of 128 sets per launch
    (csrc/kernels.h kSetFillChunk), so three launches lay out the list.  Against the sums of predict's cells, and
    bit for bit against runs of one non-empty set each."""
    B, D, K, S = 70, 45, 3, 2
    c = _scase("poisson", B, D, K, S)
    rng = np.random.default_rng(1500)
    sets = [rng.integers(0, D, int(n)).astype(np.int64) for n in rng.integers(0, 6, 300)]
    wts = [(rng.uniform(0.25, 2.0, len(s)) * rng.choice([-1.0, 1.0], len(s))).astype(np.float32).astype(np.float64)
           for s in sets]
    assert sum(len(s) == 0 for s in sets) > 10 and max(len(s) for s in sets) == 5
    data = {"counts": c["x"]}
    out = c["m"].set_scores(data, sets, wts, draws=c["params"], sd=True)
    runs = c["m"].set_scores(data, sets, wts, draws=c["params"], sd=True, max_listed=64)
    ref_s, mag_s = _scores(c["cells"], sets, wts)
    assert (np.abs(out["mean"].cpu().numpy() - ref_s.mean(0)) <= REL * mag_s.mean(0)).all()
    assert (np.abs(out["sd"].cpu().numpy() - ref_s.std(axis=0, ddof=1)) <= REL_SD * mag_s.max(0)).all()
    for n in ("mean", "sd"):
        assert tuple(out[n].shape) == (B, 300) and _same(out[n], runs[n]), n


def test_a_nan_row_is_nan_in_every_set_and_touches_no_other_row():
    cfg, x, params = make_problem(37, 23, 3, 3, 913, 0.3)
    m = build_model(cfg, 16)
    sets = _sets(23)
    xn = x.copy()
    xn[6, 11] = float("nan")
    others = T([b for b in range(37) if b != 6], device="cuda")
    filled = T([g for g, s in enumerate(sets) if len(s)], device="cuda")
    for wts in (None, _weights(23, sets)):
        clean = m.set_scores({"counts": x}, sets, wts, draws=params, sd=True)
        dirty = m.set_scores({"counts": xn}, sets, wts, draws=params, sd=True)
        for n in ("mean", "sd"):
            assert bool(torch.isfinite(clean[n]).all()), n
            assert bool(torch.isnan(dirty[n][6][filled]).all()), n
            assert _same(dirty[n][others], clean[n][others]), n
            assert bool((dirty[n][others][:, 2] == 0).all()) and bool((clean[n][:, 2] == 0).all()), n


def test_c_abi_errors_an_outside_column_the_row_stride_and_the_empty_calls():
    """Through ctypes with an exactly sized scratch of zeros and outputs filled with the sentinel -7: every
    refused call (the draw stage's shared cases, _stream_cases.assert_shared_errors, then the entry's own) and
    every empty call leaves both untouched; a listed column D makes its set NaN and no other; ld = n_sets + 2
    leaves the two gap columns of every row untouched; the valid sets have the bits of the Python call."""
    from spmf_amd import _lib
    B, D, K, S = 70, 45, 3, 2
    c = _scase("mixed", B, D, K, S)
    m, x, params = c["m"], c["x"], c["params"]
    lib, h = _lib.load(), m._handle()
    lists = [[3, D, 7], [0, 44], [], [4, 4], list(range(D)) + [9]]
    wlists = [[1.0, 1.0, 1.0], [0.5, -1.25], [], [2.0, 1.0], [1.0] * (D + 1)]
    G = len(lists)
    good, need, outs, scratch, no_u = gpu_good_call("sets", m, x, params, sets=(lists, wlists, G + 2))
    cs, set_ptr, off = good["ct"], good["keep"][-1]["set_ptr"], good["ptr"] - scratch.data_ptr()
    assert good["S"] == S and good["ld"] == G + 2
    raw = host_ctx(lib, K, _lib.FLAG_MIXED)        # a mixed context nobody gave column types

    def untouched():
        torch.cuda.synchronize()
        assert all(bool((t == -7.0).all()) for t in outs.values()) and not bool(scratch.any())
    try:
        call = assert_shared_errors(lib, "sets", good, need, no_u, raw, after=untouched)

        def refused(code, **kw):
            assert call(**kw) == code, kw
            untouched()
        # the entry's own
        down = set_ptr.copy()
        down[2] = 1
        shifted = set_ptr + 1
        refused(-1, set_ptr=down.ctypes.data)
        refused(-1, set_ptr=shifted.ctypes.data)
        refused(-1, set_ptr=None)
        refused(-1, n_sets=-1)
        refused(-1, ld=G - 1)
        refused(-1, mean=None)
        refused(-1, cols=None)
        refused(-1, S=1)                   # sd with one draw (the first of the two)
        assert "S >= 2" in lib.spmf_last_error(h).decode()
        # the empty calls launch nothing
        empty = type(cs).from_buffer_copy(cs)
        empty.n_rows = 0
        refused(0, n_sets=0)
        refused(0, n_sets=0, set_ptr=None, cols=None, weights=None, mean=None, sd=None)
        refused(0, ct=empty)
        # the valid call
        assert call() == 0
        torch.cuda.synchronize()
        assert not bool(scratch[off + need:].any()) and not bool(scratch[:off].any())
        ref = m.set_scores({"counts": x}, lists[1:], wlists[1:], draws=params, sd=True)
        for n in ("mean", "sd"):
            t = outs[n]
            assert bool((t[:, G:] == -7.0).all()), (n, "the gap columns")
            assert bool(torch.isnan(t[:, 0]).all()), (n, "the set with column D")
            assert bool(torch.isfinite(t[:, 1:G]).all()) and _same(t[:, 1:G].contiguous(), ref[n]), n
            assert bool((t[:, 2] == 0).all()), n
        # every set empty: zeros, mean alone, the gap untouched
        zeros = np.zeros(4, dtype=np.int64)
        for t in outs.values():
            t.fill_(-7.0)
        assert call(n_sets=3, set_ptr=zeros.ctypes.data, cols=None, weights=None, sd=None) == 0
        torch.cuda.synchronize()
        assert bool((outs["mean"][:, :3] == 0).all()) and bool((outs["mean"][:, 3:] == -7.0).all())
        assert bool((outs["sd"] == -7.0).all())
    finally:
        lib.spmf_ctx_destroy(raw)


def test_wide_k_runs_four_chunks_per_draw():
    """Poisson K = 70 (KP = 128): the wide-K encode sweep and four 32-float K chunks per draw."""
    B, D, K, S = 40, 70, 70, 2
    c = _scase("poisson", B, D, K, S)
    _check_oracle(c, S)
    _check_cells(c, S)


def test_peak_memory_stays_below_the_materialised_rates():
    """B = 4096, D = 1024, K = 8, S = 16, one set of all columns: the peak over the call stays below S*B*D*4
    bytes (256 MiB), the [S,B,D] fp32 rates alone; the score is the row sum of predict's mean (fp32 cells, their
    fp32 mean over the draws: 1e-5 relative leaves room for the 16 roundings)."""
    from spmf_amd.sparse import SparseCounts
    B, D, K, S = 4096, 1024, 8, 16
    cfg, x, params, mask = _dense_problem("poisson", B, D, K, S, 9700, density=0.05)
    m = _dense_model("poisson", cfg, mask, 256)
    batch = {"counts": SparseCounts.from_any(x, m.device, 256, latent_dim=K)}
    draws = {n: T(params[n]).to("cuda", torch.float32) for n in ("s", "u", "v", "w")}
    sets = [np.arange(D)]
    m.set_scores({"counts": x[:64].copy()}, sets, draws=draws, sd=True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = m.set_scores(batch, sets, draws=draws, sd=True)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"peak above the allocation before the call: {extra / 2**20:.1f} MiB; "
          f"S*B*D*4 = {S * B * D * 4 / 2**20:.1f} MiB")
    assert extra < S * B * D * 4, extra
    assert tuple(out["mean"].shape) == (B, 1) and bool(torch.isfinite(out["sd"]).all())
    ref = m.predict(batch, draws=draws)["mean"].double().sum(1)
    torch.testing.assert_close(out["mean"][:, 0], ref, rtol=1e-5, atol=0)
