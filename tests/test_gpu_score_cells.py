"""GPU: score_cells (spmf_score_cells, csrc/cells.hip) against the fp64 oracle.

Oracle: O.log_likelihood_components(cfg, x_train, ...)["rate"] [S,B,D] fp64 (the logit on a
Bernoulli column), read at the listed cells.  m_s = sigmoid(rate) on a Bernoulli column, the rate
elsewhere; with the held-out value v: ll_s = v log r - r - lgamma(v+1) (0 log 0 := 0) on a Poisson
column, v rate - softplus(rate) on a Bernoulli one; mean = mean_s m_s, lppd = logsumexp_s ll_s -
log S, all in fp64.

Bars, both from the per-cell contract of test_gpu_dense._assert_cells (rtol 1e-5, atol 1e-5 of the
largest reference value):
  |mean - ref| <= 1e-5 |ref| + 1e-5 max|mean_ref|                (max over the case's cells)
  |lppd - ref| <= 1e-5 max_s|ll_s| + 1e-5 max|ll|                (max over the case's cells and draws)
The second carries the bar on each ll_s over because log-mean-exp is 1-Lipschitz in the sup norm.
_check asserts on the oracle alone what the case expects to be finite before the GPU result is
looked at, and prints the largest observed error of each output before asserting.

Bernoulli damping as in test_gpu_topk (_stream_cases._problem is shared: same seeds, same cached inputs)."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import spmf_oracle as O
from _stream_cases import _bern_cols, _problem, assert_shared_errors
from _problems import LIKELIHOODS, _dense_model, _dense_problem, build_model, make_problem

pytestmark = pytest.mark.gpu
T = torch.as_tensor

# (B, D, K, S): K padded 3 -> 4 (one lane per cell), K = 16 (4-lane groups), K = 33 -> KP = 64 (16-lane
# groups); 70 * 45 + 50 = 3200 cells is 12.5 workgroups of 256, 5 * 333 + 50 cells end inside a wave
SHAPES = [(70, 45, 3, 2), (131, 197, 16, 7), (5, 333, 33, 3)]


def _rates(cfg, x, params):
    r = O.log_likelihood_components(cfg, T(x), T(params["s"]), T(params["u"]), T(params["v"]), T(params["w"]))["rate"]
    return r.unsqueeze(0) if r.dim() == 2 else r


def _oracle(rate, bern, rows, cols, vals):
    """fp64: mean [N], lppd [N], ll [S,N] at the listed cells of rate [S,B,D]."""
    r = rate[:, T(rows).long(), T(cols).long()]
    b = T(np.asarray(bern, dtype=bool)[cols])
    mean = torch.where(b, torch.sigmoid(r), r).mean(0)
    if vals is None:
        return mean.numpy(), None, None
    v = T(np.asarray(vals, dtype=np.float64))
    ll = torch.where(b, v * r - torch.nn.functional.softplus(r), torch.xlogy(v, r) - r - torch.lgamma(v + 1.0))
    lppd = torch.logsumexp(ll, 0) - math.log(ll.shape[0])
    return mean.numpy(), lppd.numpy(), ll.numpy()


def _all_cells(B, D, seed, ndup=50):
    """All B*D cells in a seeded random order, then ndup duplicates; dup[j] = position of the first copy."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(B * D)
    dup = rng.integers(0, B * D, size=min(ndup, B * D)) if ndup else np.zeros(0, dtype=np.int64)
    cell = np.concatenate([perm, perm[dup]])
    return (cell // D).astype(np.int64), (cell % D).astype(np.int64), dup


def _heldout_values(B, D, bern, seed):
    """A fresh draw of small counts [B,D], 0/1 on the Bernoulli columns, zeros included."""
    rng = np.random.default_rng(seed)
    v = rng.poisson(1.2, size=(B, D)).astype(np.float64)
    v[:, bern] = (rng.random((B, int(bern.sum()))) < 0.4)
    return v


def _check(m, rate, bern, rows, cols, vals, data, expect_finite=True, tag="", **kw):
    """One call against the oracle.  Returns (out, mean_ref, lppd_ref, ok_mean, ok_lppd)."""
    mref, lref, ll = _oracle(rate, bern, rows, cols, vals)
    ok_m = np.isfinite(mref)
    ok_l = np.isfinite(ll).all(0) if ll is not None else None
    if expect_finite:                                    # on the oracle alone
        assert ok_m.all(), tag
        assert ok_l is None or (ok_l.all() and np.isfinite(lref).all()), tag
    out = m.score_cells(data, rows, cols, values=vals, **kw)
    N = len(rows)
    mean = out["mean"]
    assert mean.dtype == torch.float32 and tuple(mean.shape) == (N,) and mean.is_cuda, tag
    g = mean.cpu().double().numpy()
    assert (np.isnan(g) == ~ok_m).all(), (tag, "NaN means")
    mmax = float(np.abs(mref[ok_m]).max()) if ok_m.any() else 0.0
    err = np.abs(g - mref)[ok_m]
    print(f"{tag}: N={N} max|mean - ref| {err.max() if err.size else 0.0:.3e} (max|mean_ref| {mmax:.6g})")
    assert (err <= 1e-5 * np.abs(mref[ok_m]) + 1e-5 * mmax).all(), (tag, float(err.max()))
    if vals is None:
        assert set(out) == {"mean"}, tag
        return out, mref, None, ok_m, None
    assert set(out) == {"mean", "lppd", "lppd_sum", "lppd_mean", "se", "n", "n_excluded"}, tag
    lp = out["lppd"]
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (N,) and lp.is_cuda, tag
    gl = lp.cpu().double().numpy()
    assert (np.isnan(gl) == ~ok_l).all(), (tag, "NaN lppd", int(np.isnan(gl).sum()), int((~ok_l).sum()))
    assert out["n_excluded"] == int((~ok_l).sum()) and out["n"] == int(ok_l.sum()), tag
    fin = np.isfinite(ll)
    lmax = float(np.abs(ll[fin]).max()) if fin.any() else 0.0
    errl = np.abs(gl - lref)[ok_l]
    bar = 1e-5 * np.abs(ll[:, ok_l]).max(0) + 1e-5 * lmax
    print(f"{tag}: max|lppd - ref| {errl.max() if errl.size else 0.0:.3e} (max|ll| {lmax:.6g}), "
          f"excluded {out['n_excluded']}")
    assert (errl <= bar).all(), (tag, float((errl - bar).max()))
    assert abs(out["lppd_sum"] - lref[ok_l].sum()) <= bar.sum() + 1e-300, tag       # the sum of the cells' bars
    return out, mref, lref, ok_m, ok_l


@functools.lru_cache(maxsize=None)
def _case(lik, B, D, K, S, seed=None):
    """Problem (shared with test_gpu_topk), oracle rates, Bernoulli columns, the cell list and the held-out values."""
    cfg, x, params, mask, score = _problem(lik, B, D, K, S, seed)
    bern = _bern_cols(lik, mask, D)
    rows, cols, dup = _all_cells(B, D, 300 + B + K)
    V = _heldout_values(B, D, bern, 400 + B + K)
    return cfg, x, params, mask, score, _rates(cfg, x, params), bern, rows, cols, dup, V[rows, cols]


def _bits(t):
    return t.view(torch.int32)


def _same_bits(a, b, keys=("mean", "lppd")):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in keys)


@pytest.mark.parametrize("B,D,K,S", SHAPES)
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_every_likelihood_all_cells_and_duplicates(lik, B, D, K, S):
    """All B*D cells in a random order plus 50 duplicates, held-out values that differ from the stored
    counts, panel rows 32; 'mean' without values has the bits of 'mean' with them."""
    cfg, x, params, mask, _, rate, bern, rows, cols, dup, vals = _case(lik, B, D, K, S)
    assert (vals == 0).any() and (vals != x[rows, cols]).mean() > 0.25
    m = _dense_model(lik, cfg, mask, 32)
    tag = f"{lik} {B}x{D} K={K} S={S}"
    out, *_ = _check(m, rate, bern, rows, cols, vals, {"counts": x}, tag=tag, draws=params)
    assert out["n"] == len(rows) and out["n_excluded"] == 0
    only, *_ = _check(m, rate, bern, rows, cols, None, {"counts": x}, tag=tag + " mean only", draws=params)
    assert torch.equal(_bits(only["mean"]), _bits(out["mean"]))
    n0 = B * D
    for k in ("mean", "lppd"):
        assert torch.equal(_bits(out[k][n0:]), _bits(out[k][:n0][T(dup).to(out[k].device)])), (k, "duplicates")


@pytest.mark.parametrize("B,D,K,S", [(40, 70, 128, 2), (9, 33, 256, 2)])
def test_wide_k_runs_32_and_64_lane_groups(B, D, K, S):
    """Poisson K = 128 / 256: the wide-K encode sweep, a cell per half wave and per wave."""
    cfg, x, params, mask = _dense_problem("poisson", B, D, K, S, 9300 + K)
    rows, cols, _ = _all_cells(B, D, 9301 + K)
    vals = _heldout_values(B, D, np.zeros(D, dtype=bool), 9302 + K)[rows, cols]
    m = _dense_model("poisson", cfg, mask, 32)
    _check(m, _rates(cfg, x, params), np.zeros(D, dtype=bool), rows, cols, vals, {"counts": x}, tag=f"K={K}",
           draws=params)


@pytest.mark.parametrize("lik", ["poisson", "mixed"])
def test_sum_agrees_with_waic_streaming_on_the_batchs_own_counts(lik):
    """Every cell once with its stored count as the value: sum lppd_i is waic_streaming's 'lppd'."""
    B, D, K, S = SHAPES[1]
    cfg, x, params, mask, _, rate, bern, *_ = _case(lik, B, D, K, S)
    rows, cols, _ = _all_cells(B, D, 511, ndup=0)
    m = _dense_model(lik, cfg, mask, 32)
    out, *_ = _check(m, rate, bern, rows, cols, x[rows, cols], {"counts": x}, tag=f"{lik} own counts", draws=params)
    w = m.waic_streaming({"counts": x}, draws=params)
    tol = 1e-5 * float(out["lppd"].double().abs().sum())
    print(f"{lik}: sum lppd {out['lppd_sum']!r} waic_streaming lppd {w['lppd']!r} tol {tol:.3e}")
    assert out["n"] == w["n"] == B * D and out["n_excluded"] == w["n_excluded"] == 0
    assert abs(out["lppd_sum"] - w["lppd"]) <= tol


@pytest.mark.parametrize("lik", ["poisson", "bernoulli", "mixed"])
def test_mean_agrees_with_the_scores_of_top_k(lik):
    """The real slots of top_k's (row, column) output, scored: each mean within the mean bar of top_k's score."""
    B, D, K, S = SHAPES[1]
    cfg, x, params, mask, score, *_ = _case(lik, B, D, K, S)
    m = _dense_model(lik, cfg, mask, 32)
    top = m.top_k({"counts": x}, k=10, draws=params)
    real = top["columns"] >= 0
    assert int(real.sum()) > B
    rows = torch.arange(B, device=real.device).unsqueeze(1).expand(B, 10)[real]
    out = m.score_cells({"counts": x}, rows, top["columns"][real], draws=params)
    want = top["scores"][real].double()
    err = (out["mean"].double() - want).abs()
    smax = float(np.abs(score).max())
    print(f"{lik}: max|mean - top_k score| {float(err.max()):.3e} (max|score| {smax:.6g})")
    assert bool((err <= 1e-5 * want.abs() + 1e-5 * smax).all())


def test_order_duplicates_chunks_panels_and_repeat_give_identical_bits():
    from spmf_amd.sparse import SparseCounts
    B, D, K, S = SHAPES[1]
    cfg, x, params, mask, _, rate, bern, rows, cols, dup, vals = _case("poisson", B, D, K, S)
    m = _dense_model("poisson", cfg, mask, 32)
    one = m.score_cells({"counts": x}, rows, cols, values=vals, draws=params)
    again = m.score_cells({"counts": x}, rows, cols, values=vals, draws=params)
    assert _same_bits(one, again), "two identical calls"
    p = np.random.default_rng(77).permutation(len(rows))
    perm = m.score_cells({"counts": x}, rows[p], cols[p], values=vals[p], draws=params)
    pt = T(p).to(one["mean"].device)
    assert all(torch.equal(_bits(perm[k]), _bits(one[k][pt])) for k in ("mean", "lppd")), "permutation"
    chunked = m.score_cells({"counts": x}, rows, cols, values=vals, draws=params, max_rows=32)
    assert _same_bits(chunked, one), "max_rows=32 (five chunks)"
    for k in ("lppd_sum", "lppd_mean", "se", "n", "n_excluded"):
        assert chunked[k] == one[k] == perm[k], k
    # torch tensors on the device and int32 indices are the same list
    dev = m.score_cells({"counts": x}, T(rows).to("cuda", torch.int32), T(cols).cuda(), values=T(vals).cuda(),
                        draws=params)
    assert _same_bits(dev, one), "device inputs"
    sc = SparseCounts.from_any(x, m.device, 32, latent_dim=K)
    sel = (rows >= 32) & (rows < 96)
    mini = m.score_cells({"counts": sc, "panels": (1, 3)}, rows[sel] - 32, cols[sel], values=vals[sel], draws=params)
    st = T(sel).to(one["mean"].device)
    assert all(torch.equal(_bits(mini[k]), _bits(one[k][st])) for k in ("mean", "lppd")), "panel range"
    assert mini["n"] == int(sel.sum())
    # a subset of the list scores as it did inside the full list
    few = np.flatnonzero(cols % 17 == 3)
    sub = m.score_cells({"counts": x}, rows[few], cols[few], values=vals[few], draws=params)
    ft = T(few).to(one["mean"].device)
    assert all(torch.equal(_bits(sub[k]), _bits(one[k][ft])) for k in ("mean", "lppd")), "subset"


def test_empty_list_one_cell_and_a_row_without_stored_entries():
    """make_problem leaves rows 1 and B-1 without stored entries (z = 0 there: the rate is phi)."""
    cfg, x, params = make_problem(70, 45, 5, 4, 77, 0.25)
    assert (x[1] == 0).all() and (x[69] == 0).all()
    bern = np.zeros(45, dtype=bool)
    rate = _rates(cfg, x, params)
    m = build_model(cfg, 32)
    e = np.zeros(0, dtype=np.int64)
    out = m.score_cells({"counts": x}, e, e, values=np.zeros(0), draws=params)
    assert out["mean"].dtype == torch.float32 and out["lppd"].dtype == torch.float32
    assert tuple(out["mean"].shape) == (0,) and tuple(out["lppd"].shape) == (0,) and out["mean"].is_cuda
    assert out["n"] == 0 and out["n_excluded"] == 0 and out["lppd_sum"] == 0.0 and out["se"] == 0.0
    assert set(m.score_cells({"counts": x}, e, e, draws=params)) == {"mean"}
    _check(m, rate, bern, np.array([33]), np.array([7]), np.array([2.0]), {"counts": x}, tag="one cell", draws=params)
    rows = np.repeat([1, 69, 0], 45)
    cols = np.tile(np.arange(45), 3)
    vals = _heldout_values(3, 45, bern, 5).reshape(-1)
    _check(m, rate, bern, rows, cols, vals, {"counts": x}, tag="empty rows", draws=params)
    # a single draw, with and without a sample axis
    one = {n: params[n][:1] for n in ("s", "u", "v", "w")}
    a, *_ = _check(m, rate[:1], bern, rows, cols, vals, {"counts": x}, tag="S=1", draws=one)
    b = m.score_cells({"counts": x}, rows, cols, values=vals, draws={n: v[0] for n, v in one.items()})
    assert _same_bits(a, b)


def test_single_row_batch_and_single_column_model():
    cfg, x, params, mask = _dense_problem("poisson", 1, 45, 3, 3, 9400)
    rows, cols, _ = _all_cells(1, 45, 9401, ndup=5)
    vals = _heldout_values(1, 45, np.zeros(45, dtype=bool), 9402)[rows, cols]
    _check(_dense_model("poisson", cfg, mask, 32), _rates(cfg, x, params), np.zeros(45, dtype=bool), rows, cols, vals,
           {"counts": x}, tag="B=1", draws=params)
    cfg, x, params = make_problem(9, 1, 1, 3, 914, 1.0)
    rows, cols, _ = _all_cells(9, 1, 9403, ndup=3)
    vals = _heldout_values(9, 1, np.zeros(1, dtype=bool), 9404)[rows, cols]
    _check(build_model(cfg, 4), _rates(cfg, x, params), np.zeros(1, dtype=bool), rows, cols, vals, {"counts": x},
           tag="D=1", draws=params)


def test_nan_count_in_the_batch_takes_its_rows_cells_out():
    """x[6, 11] = NaN: z of row 6 is NaN in every draw, so mean and lppd of the row's cells are NaN (on the
    oracle too); every other cell stays within its bar and n_excluded counts exactly the row's cells."""
    cfg, x, params = make_problem(37, 23, 3, 3, 913, 0.3)
    x[6, 11] = float("nan")
    bern = np.zeros(23, dtype=bool)
    rows, cols, _ = _all_cells(37, 23, 21, ndup=20)
    vals = _heldout_values(37, 23, bern, 22)[rows, cols]
    out, mref, lref, ok_m, ok_l = _check(build_model(cfg, 16), _rates(cfg, x, params), bern, rows, cols, vals,
                                         {"counts": x}, expect_finite=False, tag="NaN count", draws=params)
    assert (ok_m == (rows != 6)).all() and (ok_l == (rows != 6)).all()
    assert out["n_excluded"] == int((rows == 6).sum()) >= 23


def test_nan_value_and_rate_zero_under_a_positive_value_give_nan_lppd_and_a_finite_mean():
    """The batch of test_gpu_waic_streaming's rate-0 case with the cell held out instead of stored: row 0
    stores nothing (z = 0), column 0 has phi = 0 in draw 0, so its rate there is 0 and a held-out 3 has
    log-pmf -inf in that draw; a held-out 0 in the same cell is finite.  Two values are NaN."""
    cfg, x, params = make_problem(24, 15, 2, 3, 3, 0.3, empty=False)
    params["w"][0, 0, 0] = 0.0
    params["u"][0, 0, :] = 0.0
    x[:, 0] = 0
    x[0, :] = 0
    bern = np.zeros(15, dtype=bool)
    rate = _rates(cfg, x, params)
    assert float(rate[0, 0, 0]) == 0.0 and float(rate[1, 0, 0]) > 0.0
    rows, cols, _ = _all_cells(24, 15, 31, ndup=0)
    vals = _heldout_values(24, 15, bern, 32)[rows, cols]
    at = int(np.flatnonzero((rows == 0) & (cols == 0))[0])
    vals[at] = 3.0
    rows, cols, vals = np.append(rows, 0), np.append(cols, 0), np.append(vals, 0.0)   # the same cell, value 0
    nan_at = [5, 200]
    assert at not in nan_at
    vals[nan_at] = float("nan")
    out, mref, lref, ok_m, ok_l = _check(build_model(cfg, 8), rate, bern, rows, cols, vals, {"counts": x},
                                         expect_finite=False, tag="rate 0 / NaN value", draws=params)
    assert ok_m.all(), "every mean is finite"
    assert sorted(np.flatnonzero(~ok_l).tolist()) == sorted(nan_at + [at])
    assert out["n_excluded"] == 3 and out["n"] == len(rows) - 3
    assert bool(torch.isfinite(out["lppd"][-1])) and bool(torch.isfinite(out["mean"][at]))


def test_an_index_out_of_range_raises_before_the_library_is_reached(monkeypatch):
    from spmf_amd import _lib
    cfg, x, params, mask, *_ = _case("poisson", 70, 45, 3, 2)
    m = _dense_model("poisson", cfg, mask, 32)
    m.score_cells({"counts": x}, [0], [0], draws=params)         # context, batch and library are set up

    def reached(*a, **k):
        raise AssertionError("spmf_score_cells was called")
    monkeypatch.setattr(_lib.load(), "spmf_score_cells", reached)
    for rows, cols in (([0, 70], [0, 1]), ([0, -1], [0, 1]), ([0, 1], [45, 1]), ([0, 1], [3, -1])):
        with pytest.raises(ValueError):
            m.score_cells({"counts": x}, rows, cols, values=[1.0, 0.0], draws=params)
    from spmf_amd.sparse import SparseCounts
    sc = SparseCounts.from_any(x, m.device, 32, latent_dim=3)
    with pytest.raises(ValueError):                               # rows are relative to the panel range
        m.score_cells({"counts": sc, "panels": (1, 2)}, [32], [0], draws=params)


def test_custom_codec_raises():
    from spmf_amd import PoissonFactorization
    cfg, x, params, mask, *_ = _case("poisson", 70, 45, 3, 2)
    mc = PoissonFactorization(latent_dim=3, feature_dim=45, encoder_function=lambda t: t,
                              decoder_function=lambda t: t, initialize_distributions=False,
                              device="cuda", panel_rows=32)
    with pytest.raises(NotImplementedError):
        mc.score_cells({"counts": x}, [0], [0], draws=params)


def test_c_abi_errors_launch_nothing():
    """Through ctypes, with valid or empty cell lists only: every SPMF_E_ARG (-1) case of the header and a short
    scratch (SPMF_E_WORKSPACE, -3, names the need); outputs and scratch keep their sentinel.  Then the valid
    call returns what the method returns."""
    from spmf_amd import _lib
    from spmf_amd._lib import VAR_ORDER
    cfg, x, params, mask, _, rate, bern, rows, cols, dup, vals = _case("poisson", 70, 45, 3, 2)
    m = _dense_model("poisson", cfg, mask, 32)
    lib, h = _lib.load(), m._handle()
    _, cs = m._batch({"counts": x})
    S, P = m._pack_params(params, names=("s", "u", "v", "w"))
    pin = _lib.PtrArray(*[P[n].data_ptr() if n in P else None for n in VAR_ORDER])
    eta = m._eta_device()
    N = len(rows)
    r32, c32 = T(rows).to("cuda", torch.int32), T(cols).to("cuda", torch.int32)
    v32 = T(vals).to("cuda", torch.float32)
    need = int(lib.spmf_cells_scratch_bytes(h, int(cs.n_rows), S))
    assert need > 0 and need % 256 == 0
    assert need == int(lib.spmf_waic_scratch_bytes(h, int(cs.n_rows), max(S, 2)))
    assert int(lib.spmf_cells_scratch_bytes(h, int(cs.n_rows), 0)) == 0
    assert int(lib.spmf_cells_scratch_bytes(h, int(cs.n_rows), 1)) > 0
    scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    base = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    mean = torch.full((N,), -7.0, dtype=torch.float32, device="cuda")
    lppd = torch.full((N,), -7.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(h=h, ct=cs, S=S, pin=pin, eta=eta.data_ptr(), n=N, row=r32.data_ptr(), col=c32.data_ptr(),
                val=v32.data_ptr(), mean=mean.data_ptr(), lppd=lppd.data_ptr(), ptr=base, nbytes=need,
                stream=stream)
    no_u = _lib.PtrArray(*[P[n].data_ptr() if n in P and n != "u" else None for n in VAR_ORDER])
    raw = _dense_model("mixed", cfg, np.arange(45) % 3 == 1, 32)._new_ctx()   # mixed, and no column types given
    try:
        call = assert_shared_errors(lib, "cells", good, need, no_u, raw)      # the draw stage's list
    finally:
        lib.spmf_ctx_destroy(raw)
    assert call(row=None) == -1 and call(col=None) == -1 and call(mean=None) == -1
    assert call(val=None) == -1 and call(lppd=None) == -1          # one of the pair without the other
    assert call(n=-1) == -1
    assert call(n=0, nbytes=need - 256) == -3                      # errors come before the empty-list return
    assert call(n=0) == 0 and call(n=0, row=None, col=None, mean=None) == 0
    torch.cuda.synchronize()
    assert bool((mean == -7.0).all()) and bool((lppd == -7.0).all()) and not bool(scratch.any())
    assert call(val=None, lppd=None) == 0                          # the mean only
    torch.cuda.synchronize()
    assert bool((lppd == -7.0).all())
    want = m.score_cells({"counts": x}, rows, cols, values=vals, draws=params)
    assert torch.equal(_bits(mean), _bits(want["mean"]))
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(mean), _bits(want["mean"])) and torch.equal(_bits(lppd), _bits(want["lppd"]))


def test_peak_memory_is_the_scratch_and_a_few_vectors_of_the_list():
    """(131, 197, 16, 7), every cell listed: the call's peak above what was allocated before it stays below
    scratch + 64 N bytes + 1 MiB, and below the 8 S B D bytes of rate[S,B,D] and ll[S,B,D]."""
    from spmf_amd import _lib
    from spmf_amd.sparse import SparseCounts
    B, D, K, S = SHAPES[1]
    cfg, x, params, mask, _, rate, bern, *_ = _case("poisson", B, D, K, S)
    rows, cols, _ = _all_cells(B, D, 611, ndup=0)
    vals = _heldout_values(B, D, bern, 612)[rows, cols]
    N = B * D
    m = _dense_model("poisson", cfg, mask, 32)
    batch = {"counts": SparseCounts.from_any(x, m.device, 32, latent_dim=K)}
    draws = {n: T(params[n]).to("cuda", torch.float32) for n in ("s", "u", "v", "w")}
    r, c, v = T(rows).to("cuda", torch.int32), T(cols).to("cuda", torch.int32), T(vals).to("cuda", torch.float32)
    m.score_cells(batch, r[:10], c[:10], values=v[:10], draws=draws)
    scratch = int(_lib.load().spmf_cells_scratch_bytes(m._handle(), B, S))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = m.score_cells(batch, r, c, values=v, draws=draws)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"peak above the allocation before the call: {extra} B; scratch {scratch} B, 64 N = {64 * N} B, "
          f"8 S B D = {8 * S * B * D} B")
    assert extra < scratch + 64 * N + (1 << 20), extra
    assert extra < 8 * S * B * D, extra
    assert out["n"] == N and out["n_excluded"] == 0


def test_empty_python_lists_and_the_row_count_read_off_the_shape():
    """[] has no integer dtype of its own and is an empty list all the same; the row count the index check uses
    is the one of the library's descriptor, for whole batches and panel ranges."""
    from spmf_amd.sparse import SparseCounts
    cfg, x, params, mask, *_ = _case("poisson", 70, 45, 3, 2)
    m = _dense_model("poisson", cfg, mask, 32)
    out = m.score_cells({"counts": x}, [], [], values=[], draws=params)
    assert tuple(out["mean"].shape) == (0,) and tuple(out["lppd"].shape) == (0,) and out["n"] == 0
    sc = SparseCounts.from_any(x, m.device, 32, latent_dim=3)
    for batch in ({"counts": x}, {"counts": sc}, {"counts": sc, "panels": (1, 2)}, {"counts": sc, "panels": (2, 3)},
                  {"counts": sc, "panels": (1, None)}, {"counts": sc, "panels": (0, 9)}):
        assert m._batch_rows(batch) == int(m._batch(batch)[1].n_rows), batch.get("panels")
    assert m._batch_rows({"counts": sc, "panels": (2, 3)}) == 6
