"""GPU: predict (spmf_predict_columns, csrc/panel.hip) against the fp64 oracle.

Oracle: O.log_likelihood_components(...)["rate"] [S,B,D] fp64 (the logit on a Bernoulli column), per draw
m_s = rate | sigmoid(rate); mean = mean_s m_s, sd = std_s(m_s, ddof=1), p_nonzero = mean_s -expm1(-rate_s) on
a Poisson column.  Bars (bar(v) = 1e-5 |v| + 1e-5 max|score|, the bar of test_gpu_topk._bar):
  mean       every cell within bar(mean);
  sd         within 2 max_s bar(m_s): each m_s is off by at most its bar, the standard deviation moves by at
             most sqrt(S/(S-1)) <= sqrt 2 times the largest perturbation, and the fp32 Welford rounding for
             S <= 7 is below the remainder.  The share of cells whose oracle sd exceeds ten times that bound is
             asserted on the oracle first (SD_FLOOR), so that the comparison says something;
  p_nonzero  within mean_s[exp(-r_s) (1e-5 |r_s| + 1e-5 max|r|)] + 2^-22: the per-cell bar on the rate through
             the derivative of 1 - exp(-r), plus the fp32 rounding of a value <= 1.  With the parameters of
             _dense_problem every Poisson rate is above 2 and P(x > 0) is 1 to working precision, so the
             poisson and mixed cases scale u and w by PNZ_DAMP (powers of two: the values stay fp32-exact);
             the oracle then has rates within 0.010 .. 2.8, every Poisson cell's P(x > 0) inside (0.01, 0.99)
             and a bound of at most 2.4e-5, all asserted on the oracle before the GPU result is looked at.
             poisson_log runs the formula on its undamped problem (a loose bound, up to 0.027).
Everything else is bit for bit: against rank_cells, between column lists, between the outputs asked for,
between row chunkings, and beside a NaN row."""
import ctypes as C

import numpy as np
import pytest
import torch

from _problems import LIKELIHOODS, _dense_model, _dense_problem, build_model, make_problem
from _stream_cases import OUTS, SHAPES, _bar, _case, _damped_case, _lists

pytestmark = pytest.mark.gpu
T = torch.as_tensor

# share of cells whose oracle sd exceeds ten times the sd bound; measured minimum over SHAPES on the CPU oracle:
# poisson 0.993, mixed 0.662, poisson_log 0.484, bernoulli 0.892, bernoulli_log 0.984
SD_FLOOR = {"poisson": 0.99, "mixed": 0.65, "poisson_log": 0.45, "bernoulli": 0.85, "bernoulli_log": 0.95}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _sd_view(c):
    """From the oracle alone: sd, its bound and the share of cells the comparison resolves."""
    smax = float(np.abs(c["score"]).max())
    ref = c["ms"].std(axis=0, ddof=1)
    bound = 2.0 * _bar(np.abs(c["ms"]).max(axis=0), smax)
    return ref, bound, float((ref > 10.0 * bound).mean())


def _pnz_view(c):
    """From the oracle alone, on the Poisson columns: P(x > 0), its bound, the smallest and largest rate."""
    r = c["rate"][:, :, ~c["bern"]]
    rmax = float(np.abs(r).max())
    ref = (-np.expm1(-r)).mean(axis=0)
    bound = (np.exp(-r) * (1e-5 * np.abs(r) + 1e-5 * rmax)).mean(axis=0) + 2.0 ** -22
    return ref, bound, float(r.min()), float(r.max())


@pytest.mark.parametrize("B,D,K,S", SHAPES)
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_mean_against_the_oracle(lik, B, D, K, S):
    c = _case(lik, B, D, K, S)
    score = c["score"]
    assert np.isfinite(score).all()
    smax = float(np.abs(score).max())
    got = c["full"]["mean"].cpu().double().numpy()
    err = np.abs(got - score)
    print(f"{lik} {B}x{D} K={K} S={S}: max |mean - oracle| {err.max():.3e}, max|score| {smax:.6g}, "
          f"worst err/bar {float((err / _bar(score, smax)).max()):.3f}")
    assert (err <= _bar(score, smax)).all(), float(err.max())


@pytest.mark.parametrize("B,D,K,S", SHAPES)
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_sd_against_the_oracle(lik, B, D, K, S):
    c = _case(lik, B, D, K, S)
    ref, bound, share = _sd_view(c)
    print(f"{lik} {B}x{D} K={K} S={S}: share of cells with sd > 10 bound {share:.3f}")
    assert share >= SD_FLOOR[lik], share                       # on the oracle alone
    got = c["full"]["sd"].cpu().double().numpy()
    err = np.abs(got - ref)
    print(f"{lik} {B}x{D} K={K} S={S}: max |sd - oracle| {err.max():.3e}, worst err/bound "
          f"{float((err / bound).max()):.3f}")
    assert (err <= bound).all(), float(err.max())


@pytest.mark.parametrize("B,D,K,S", SHAPES)
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_p_nonzero(lik, B, D, K, S):
    c = _case(lik, B, D, K, S)
    bern = c["bern"]
    if bern.any():      # on every Bernoulli column p_nonzero is the mean, bit for bit
        sel = torch.as_tensor(np.flatnonzero(bern), device="cuda")
        assert _same(c["full"]["p_nonzero"][:, sel], c["full"]["mean"][:, sel])
    if lik.startswith("bernoulli"):
        return
    if lik == "poisson_log":
        ref, bound, rlo, rhi = _pnz_view(c)
        got = c["full"]["p_nonzero"]
    else:
        dc = _damped_case(lik, B, D, K, S)
        ref, bound, rlo, rhi = _pnz_view(dc)
        # the condition on the inputs, on the oracle alone
        assert 0.010 <= rlo and rhi <= 2.8, (rlo, rhi)
        assert 0.01 < ref.min() and ref.max() < 0.99, (float(ref.min()), float(ref.max()))
        assert bound.max() <= 2.4e-5, float(bound.max())
        m = _dense_model(lik, dc["cfg"], dc["mask"], 32)
        out = m.predict({"counts": dc["x"]}, draws=dc["params"], p_nonzero=True)
        assert set(out) == {"mean", "p_nonzero"}
        got = out["p_nonzero"]
        if bern.any():
            sel = torch.as_tensor(np.flatnonzero(bern), device="cuda")
            assert _same(got[:, sel], out["mean"][:, sel])
    got = got.cpu().double().numpy()[:, ~bern]
    err = np.abs(got - ref)
    print(f"{lik} {B}x{D} K={K} S={S}: rates {rlo:.4g} .. {rhi:.4g}, P(x>0) {ref.min():.4g} .. {ref.max():.4g}, "
          f"largest bound {bound.max():.3e}, max |p_nonzero - oracle| {err.max():.3e}, worst err/bound "
          f"{float((err / bound).max()):.3f}")
    assert (err <= bound).all(), float(err.max())


def _every_cell(B, D):
    cell = torch.arange(B * D)
    return cell // D, cell % D


@pytest.mark.parametrize("B,D,K,S", SHAPES[:2])
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_mean_has_the_bits_of_the_ranking(lik, B, D, K, S):
    c = _case(lik, B, D, K, S)
    rows, cols = _every_cell(B, D)
    rk = c["m"].rank_cells({"counts": c["x"]}, rows, cols, draws=c["params"], exclude_stored=False)
    assert _same(rk["score"].view(B, D), c["full"]["mean"])


@pytest.mark.parametrize("B,D,K,S", SHAPES)
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_lists_outputs_and_chunks_give_the_same_bits(lik, B, D, K, S):
    from spmf_amd.sparse import SparseCounts
    c = _case(lik, B, D, K, S)
    m, x, params, full = c["m"], c["x"], c["params"], c["full"]
    lists = _lists(D)
    assert len(lists["dup"]) == min(D, 65) and lists["dup"][:3].tolist() == [D - 1, 0, 0]
    if lik == "mixed":   # Bernoulli and Poisson columns side by side inside one 32-lane tile
        for name in ("perm", "dup"):
            b = c["bern"][lists[name]]
            j = np.flatnonzero(b[1:] != b[:-1])
            assert (j // 32 == (j + 1) // 32).any(), name
    for name, cols in lists.items():
        out = m.predict({"counts": x}, cols, draws=params, sd=True, p_nonzero=True)
        if cols is None:
            assert set(out) == set(OUTS)
            sel = slice(None)
        else:
            assert out["columns"].dtype == torch.int32 and out["columns"].cpu().tolist() == cols.tolist(), name
            sel = torch.as_tensor(cols, device="cuda")
        for n in OUTS:
            assert _same(out[n], full[n][:, sel]), (name, n)
        # torch on the device and numpy int32 are the same list
        if name == "dup":
            again = m.predict({"counts": x}, torch.as_tensor(cols, dtype=torch.int32, device="cuda"), draws=params)
            assert set(again) == {"mean", "columns"} and _same(again["mean"], out["mean"])
    # the outputs asked for
    assert _same(m.predict({"counts": x}, draws=params)["mean"], full["mean"])
    only_sd = m.predict({"counts": x}, lists["dup"], draws=params, sd=True)
    only_pz = m.predict({"counts": x}, lists["dup"], draws=params, p_nonzero=True)
    sel = torch.as_tensor(lists["dup"], device="cuda")
    assert set(only_sd) == {"mean", "sd", "columns"} and set(only_pz) == {"mean", "p_nonzero", "columns"}
    for out in (only_sd, only_pz):
        for n in set(out) - {"columns"}:
            assert _same(out[n], full[n][:, sel]), n
    # row chunks and a panel range
    if B > 32:
        chunked = m.predict({"counts": x}, lists["dup"], draws=params, sd=True, p_nonzero=True, max_rows=32)
        sc = SparseCounts.from_any(x, m.device, 32, latent_dim=K)
        mini = m.predict({"counts": sc, "panels": (1, 2)}, lists["dup"], draws=params, sd=True, p_nonzero=True)
        for n in OUTS:
            assert _same(chunked[n], full[n][:, sel]), n
            assert _same(mini[n], full[n][32:64][:, sel]), n


def test_a_nan_count_makes_its_row_nan_and_no_other():
    cfg, x, params = make_problem(37, 23, 3, 3, 913, 0.3)
    m = build_model(cfg, 16)
    cols = np.array([22, 11, 0, 11, 5])
    clean = m.predict({"counts": x}, cols, draws=params, sd=True, p_nonzero=True)
    clean_all = m.predict({"counts": x}, draws=params, sd=True, p_nonzero=True)
    xn = x.copy()
    xn[6, 11] = float("nan")
    keep = torch.as_tensor(np.delete(np.arange(37), 6), device="cuda")
    for ref, out in ((clean, m.predict({"counts": xn}, cols, draws=params, sd=True, p_nonzero=True)),
                     (clean_all, m.predict({"counts": xn}, draws=params, sd=True, p_nonzero=True))):
        for n in OUTS:
            assert bool(torch.isnan(out[n][6]).all()), n
            assert bool(torch.isfinite(ref[n]).all()), n
            assert _same(out[n][keep], ref[n][keep]), n


def test_argument_errors_raise_before_any_launch():
    from spmf_amd import PoissonFactorization
    c = _case("poisson", 70, 45, 3, 2)
    m, x, params = c["m"], c["x"], c["params"]
    one = {n: params[n][:1] for n in ("s", "u", "v", "w")}
    with pytest.raises(ValueError, match="at least 2 draws"):
        m.predict({"counts": x}, draws=one, sd=True)
    assert _same(m.predict({"counts": x}, [3], draws=one)["mean"],
                 m.predict({"counts": x}, draws=one, p_nonzero=True)["mean"][:, 3:4])
    for cols in ([0, 45], [-1], np.zeros((2, 2), dtype=np.int64), list(range(45)) + [0]):
        with pytest.raises(ValueError):
            m.predict({"counts": x}, cols, draws=params)
    mc = PoissonFactorization(latent_dim=3, feature_dim=45, encoder_function=lambda t: t,
                              decoder_function=lambda t: t, initialize_distributions=False,
                              device="cuda", panel_rows=32)
    with pytest.raises(ValueError):
        mc.predict({"counts": x}, [0, 45], draws=params)
    with pytest.raises(NotImplementedError):
        mc.predict({"counts": x}, [0, 44], draws=params)
    empty = m.predict({"counts": x}, [], draws=params, sd=True)
    assert tuple(empty["mean"].shape) == (70, 0) and tuple(empty["sd"].shape) == (70, 0)


def test_c_abi_margins_an_outside_column_and_errors():
    """Through ctypes with an exactly sized scratch and outputs one row and one column larger than needed,
    pre-filled with -7: the margin keeps the sentinel.  A list holding the index D gives NaN in that output
    column and the right neighbours.  A short scratch is SPMF_E_WORKSPACE (-3) and names the need; sd_out with
    S = 1 is SPMF_E_ARG (-1); neither writes anything."""
    from spmf_amd import _lib
    from spmf_amd._lib import VAR_ORDER
    B, D, K, S = 70, 45, 3, 2
    c = _case("mixed", B, D, K, S)
    m, x, params, full = c["m"], c["x"], c["params"], c["full"]
    lib, h = _lib.load(), m._handle()
    _, cs = m._batch({"counts": x})
    S_, P = m._pack_params(params, names=("s", "u", "v", "w"))
    assert S_ == S
    pin = _lib.PtrArray(*[P[n].data_ptr() if n in P else None for n in VAR_ORDER])
    eta = m._eta_device()
    need = int(lib.spmf_predict_scratch_bytes(h, int(cs.n_rows), S))
    assert need > 0 and need % 256 == 0 and int(lib.spmf_predict_scratch_bytes(h, int(cs.n_rows), 0)) == 0
    scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    off = (-scratch.data_ptr()) % 256
    base = scratch.data_ptr() + off
    listed = [3, D, 7, 0, 44, 4, 4]              # columns 3 | 4 | 7 of the mask: Poisson, Bernoulli, Bernoulli
    assert c["bern"][[3, 4, 7]].tolist() == [False, True, True]
    Cn = len(listed)
    cols = torch.tensor(listed, dtype=torch.int32, device="cuda")
    outs = {n: torch.full(((B + 1) * (Cn + 1),), -7.0, dtype=torch.float32, device="cuda") for n in OUTS}
    stream = torch.cuda.current_stream().cuda_stream

    def call(S_=S, nbytes=need, n=Cn, lst=cols.data_ptr(), o=outs):
        return lib.spmf_predict_columns(h, C.byref(cs), S_, pin, eta.data_ptr(), n, lst, o["mean"].data_ptr(),
                                        o["sd"].data_ptr(), o["p_nonzero"].data_ptr(), base, nbytes, stream)
    assert call(nbytes=need - 256) == -3
    msg = lib.spmf_last_error(h).decode()
    assert str(need) in msg, msg
    assert call(S_=1) == -1
    assert call(n=D + 1) == -1 and call(n=-1) == -1 and call(lst=None) == -1
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in outs.values()) and not bool(scratch.any())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool(scratch[off + need:].any()) and not bool(scratch[:off].any())
    good = [j for j, d in enumerate(listed) if d < D]
    sel = torch.tensor([listed[j] for j in good], device="cuda")
    for n in OUTS:
        body, margin = outs[n][:B * Cn].view(B, Cn), outs[n][B * Cn:]
        assert bool((margin == -7.0).all()), n
        assert bool(torch.isnan(body[:, 1]).all()), n
        assert _same(body[:, good], full[n][:, sel]), n
    # all columns, no list, the mean only: no gather, the other outputs untouched
    wide = {n: torch.full(((B + 1) * (D + 1),), -7.0, dtype=torch.float32, device="cuda") for n in OUTS}
    assert lib.spmf_predict_columns(h, C.byref(cs), S, pin, eta.data_ptr(), D, None, wide["mean"].data_ptr(), None,
                                    None, base, need, stream) == 0
    torch.cuda.synchronize()
    assert _same(wide["mean"][:B * D].view(B, D), full["mean"]) and bool((wide["mean"][B * D:] == -7.0).all())
    assert bool((wide["sd"] == -7.0).all()) and bool((wide["p_nonzero"] == -7.0).all())


def test_peak_memory_stays_below_the_materialised_rates():
    """B = 2048, D = 1024, K = 16, S = 8 and 64 listed columns: the peak over the call stays below S*B*D*4
    bytes (64 MiB), the [S,B,D] fp32 rates alone; the panel has the bits of those columns of the full call."""
    from spmf_amd.sparse import SparseCounts
    B, D, K, S = 2048, 1024, 16, 8
    cfg, x, params, mask = _dense_problem("poisson", B, D, K, S, 9800, density=0.05)
    m = _dense_model("poisson", cfg, mask, 256)
    batch = {"counts": SparseCounts.from_any(x, m.device, 256, latent_dim=K)}
    draws = {n: T(params[n]).to("cuda", torch.float32) for n in ("s", "u", "v", "w")}
    cols = torch.as_tensor(np.random.default_rng(3).permutation(D)[:64].copy(), device="cuda")
    m.predict({"counts": x[:64].copy()}, cols, draws=draws, sd=True, p_nonzero=True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = m.predict(batch, cols, draws=draws, sd=True, p_nonzero=True)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"peak above the allocation before the call: {extra / 2**20:.1f} MiB; "
          f"S*B*D*4 = {S * B * D * 4 / 2**20:.1f} MiB")
    assert extra < S * B * D * 4, extra
    full = m.predict(batch, draws=draws, sd=True, p_nonzero=True)
    for n in OUTS:
        assert tuple(out[n].shape) == (B, 64) and _same(out[n], full[n][:, cols]), n


def test_wide_k_runs_four_chunks_per_draw():
    """Poisson K = 65 (KP = 128): the wide-K encode sweep and four 32-float K chunks per draw, against the
    oracle and against the ranking's bits."""
    B, D, K, S = 40, 70, 65, 2
    c = _case("poisson", B, D, K, S)
    score = c["score"]
    smax = float(np.abs(score).max())
    err = np.abs(c["full"]["mean"].cpu().double().numpy() - score)
    print(f"wide K: max |mean - oracle| {err.max():.3e}, worst err/bar {float((err / _bar(score, smax)).max()):.3f}")
    assert (err <= _bar(score, smax)).all(), float(err.max())
    rows, cols = _every_cell(B, D)
    rk = c["m"].rank_cells({"counts": c["x"]}, rows, cols, draws=c["params"], exclude_stored=False)
    assert _same(rk["score"].view(B, D), c["full"]["mean"])
