"""GPU: waic_streaming (spmf_waic_accumulate, csrc/waic.hip) against the fp64 oracle's
per-cell log-likelihood, reduced on the CPU by the pointwise definition exactly as
test_gpu_dense.py::test_waic_matches_pointwise_definition does it.

Tolerances are that test's: lppd and waic 1e-5 relative, pwaic 1e-3 relative; row scores the
same plus an atol of that fraction of the largest row value.  se: the larger of twice the error
of the materialising path (log_likelihood_components -> fp64 -> logsumexp / var, the lines of
waic()) against the oracle on the same batch and draws, and 1e-5 relative."""
import math

import numpy as np
import pytest
import torch

from oracle import spmf_oracle as O
from _problems import LIKELIHOODS, _dense_model, _dense_problem, build_model, make_problem

pytestmark = pytest.mark.gpu
T = torch.as_tensor


def _cells(cfg, x, params):
    """Oracle: per-cell (lppd_i, pwaic_i) [B,D] fp64 and the mask of cells finite in every draw."""
    ll = O.log_likelihood_components(cfg, T(x), T(params["s"]), T(params["u"]), T(params["v"]),
                                     T(params["w"]))["log_likelihood"]
    S = ll.shape[0]
    ok = torch.isfinite(ll).all(0)
    lp = torch.logsumexp(ll, 0) - math.log(S)
    pw = ll.var(0, unbiased=True)
    return lp, pw, ok


def _totals(lp, pw, ok):
    e = (lp - pw)[ok]
    n = int(ok.sum())
    return {"lppd": float(lp[ok].sum()), "pwaic": float(pw[ok].sum()), "waic": float(-2.0 * e.sum()),
            "se": float(2.0 * torch.sqrt(n * e.var(unbiased=True))), "n": n,
            "n_excluded": int((~ok).sum())}


def _materialised_se(m, batch, params):
    """se as waic() computes it, with the draws passed through log_likelihood_components."""
    ll = m.log_likelihood_components(s=params["s"], u=params["u"], v=params["v"], w=params["w"],
                                     data=batch)["log_likelihood"].double()
    e = torch.logsumexp(ll, 0) - math.log(ll.shape[0]) - ll.var(0, unbiased=True)
    return float(2.0 * torch.sqrt(e.numel() * e.var(unbiased=True)))


def _assert_totals(out, ref, se_old=None, tag=""):
    print(f"{tag} got lppd={out['lppd']!r} pwaic={out['pwaic']!r} waic={out['waic']!r} se={out['se']!r} "
          f"n={out['n']} excl={out['n_excluded']} | ref lppd={ref['lppd']!r} pwaic={ref['pwaic']!r} "
          f"waic={ref['waic']!r} se={ref['se']!r} | se materialised={se_old!r}")
    assert out["n"] == ref["n"] and out["n_excluded"] == ref["n_excluded"], tag
    assert math.isfinite(out["lppd"]) and math.isfinite(ref["lppd"]), tag
    assert abs(out["lppd"] - ref["lppd"]) <= 1e-5 * abs(ref["lppd"]), tag
    assert abs(out["pwaic"] - ref["pwaic"]) <= 1e-3 * max(abs(ref["pwaic"]), 1e-9) + 1e-9, tag
    assert abs(out["waic"] - ref["waic"]) <= 1e-5 * abs(ref["waic"]), tag
    if se_old is not None:
        tol = max(2.0 * abs(se_old - ref["se"]), 1e-5 * abs(ref["se"]))
        assert abs(out["se"] - ref["se"]) <= tol, (tag, out["se"], ref["se"], se_old)


def _assert_rows(out, lp, pw, ok, tag=""):
    rl = torch.where(ok, lp, torch.zeros_like(lp)).sum(1).numpy()
    rp = torch.where(ok, pw, torch.zeros_like(pw)).sum(1).numpy()
    gl, gp = out["row_lppd"].cpu().numpy(), out["row_pwaic"].cpu().numpy()
    assert gl.dtype == np.float64 and gl.shape == rl.shape and gp.shape == rp.shape, tag
    np.testing.assert_allclose(gl, rl, rtol=1e-5, atol=1e-5 * np.abs(rl).max(), err_msg=tag)
    np.testing.assert_allclose(gp, rp, rtol=1e-3, atol=1e-3 * np.abs(rp).max(), err_msg=tag)


def _run(lik, cfg, x, params, mask, panel_rows=32, se=True, tag=""):
    lp, pw, ok = _cells(cfg, x, params)
    m = _dense_model(lik, cfg, mask, panel_rows)
    batch = {"counts": x}
    out = m.waic_streaming(batch, draws=params, row_scores=True)
    se_old = _materialised_se(m, batch, params) if se and bool(ok.all()) else None
    _assert_totals(out, _totals(lp, pw, ok), se_old, tag)
    _assert_rows(out, lp, pw, ok, tag)
    return m, out, (lp, pw, ok)


@pytest.mark.parametrize("B,D,K,S", [(70, 45, 3, 2), (131, 97, 16, 7)])
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_every_likelihood_at_ragged_tiles(lik, B, D, K, S):
    """Rows and columns that are no multiple of the 64 x 64 block or the 32 x 32 wave tile,
    K padded 3 -> 4 (half a K chunk) and K = 16, two and seven draws."""
    cfg, x, params, mask = _dense_problem(lik, B, D, K, S, 4100 + B + K)
    _, out, (lp, pw, ok) = _run(lik, cfg, x, params, mask, tag=f"{lik} {B}x{D} K={K} S={S}")
    assert bool(ok.all()) and out["n"] == B * D and out["n_excluded"] == 0


@pytest.mark.parametrize("B,D,K,S", [(70, 45, 64, 5), (40, 70, 128, 3)])
def test_wide_k_runs_several_chunks_per_draw(B, D, K, S):
    """KP = 64 and 128: two and four 32-float K chunks per draw through the LDS tiles, the
    K = 128 encode sweep on the wide-K row kernel."""
    cfg, x, params, mask = _dense_problem("poisson", B, D, K, S, 4300 + K)
    _run("poisson", cfg, x, params, mask, tag=f"K={K}")


def test_empty_row_empty_column_and_a_full_row():
    """make_problem leaves rows 1, B-1 and column 2 empty; row 5 is stored in every other
    column (a fully stored row and an empty column exclude each other in that one cell)."""
    cfg, x, params = make_problem(70, 45, 5, 4, 77, 0.25)
    x[5, :] = 1 + (np.arange(45) % 4)
    x[5, 2] = 0
    assert (x[1] == 0).all() and (x[:, 2] == 0).all() and (x[5] != 0).sum() == 44
    _run("poisson", cfg, x, params, None, tag="edges")


def test_single_row_batch():
    cfg, x, params, mask = _dense_problem("poisson", 1, 45, 3, 3, 4500)
    _run("poisson", cfg, x, params, mask, tag="B=1")


def test_large_count_cell_needs_the_stable_log_mean_exp():
    """A count of 400 under rates of order 1: every ll_s of the cell is below -1000, where a
    plain exp underflows in fp32 and fp64.  The count sits in a column that feeds nothing into
    z (u = 0 there, rows unscaled), so the rates stay where they were."""
    cfg, x, params = make_problem(37, 23, 3, 4, 811, 0.3, scale_rows=False)
    params["u"][:, 7, :] = 0.0
    x[4, 7] = 400.0
    ll = O.log_likelihood_components(cfg, T(x), T(params["s"]), T(params["u"]), T(params["v"]),
                                     T(params["w"]))["log_likelihood"]
    assert bool(torch.isfinite(ll).all()), "n_excluded == 0 is the expected answer"
    assert float(ll[:, 4, 7].max()) < -1000.0
    lp, pw, ok = _cells(cfg, x, params)
    m = build_model(cfg, 16)
    out = m.waic_streaming({"counts": x}, draws=params, row_scores=True)
    assert out["n_excluded"] == 0 and math.isfinite(out["lppd"])
    _assert_totals(out, _totals(lp, pw, ok), _materialised_se(m, {"counts": x}, params), "x=400")
    _assert_rows(out, lp, pw, ok, "x=400")
    assert abs(float(out["row_lppd"][4]) - float(lp[4].sum())) <= 1e-5 * abs(float(lp[4].sum()))


def test_nan_count_is_excluded_and_counted():
    """One NaN count.  The encoder sums the counts of a row into z_b, so the oracle's per-cell
    values are NaN in every cell of that row, not in one: with D > 1 the expected answer is D
    excluded cells (checked on the oracle first).  With D = 1 the row is the cell, and
    n_excluded == 1, n == B*D - 1 hold as stated; the other sums are the oracle's over the
    remaining cells in both."""
    cfg, x, params = make_problem(37, 23, 3, 3, 913, 0.3)
    x[6, 11] = float("nan")
    lp, pw, ok = _cells(cfg, x, params)
    assert int((~ok).sum()) == 23 and not bool(ok[6].any())
    m = build_model(cfg, 16)
    out = m.waic_streaming({"counts": x}, draws=params, row_scores=True)
    assert out["n_excluded"] == 23 and out["n"] == 37 * 23 - 23
    _assert_totals(out, _totals(lp, pw, ok), None, "NaN row")
    _assert_rows(out, lp, pw, ok, "NaN row")

    cfg, x, params = make_problem(9, 1, 1, 3, 914, 1.0)
    x[3, 0] = float("nan")
    lp, pw, ok = _cells(cfg, x, params)
    assert int((~ok).sum()) == 1
    out = build_model(cfg, 4).waic_streaming({"counts": x}, draws=params)
    assert out["n_excluded"] == 1 and out["n"] == 9 * 1 - 1
    _assert_totals(out, _totals(lp, pw, ok), None, "NaN cell D=1")


def test_rate_zero_under_a_positive_count_excludes_that_one_cell():
    """The other cause the kernel names (the case of test_non_finite_rule_matches_reference_semantics):
    log-pmf -inf in draw 0 of one stored cell; n_excluded == 1 and n == B*D - 1."""
    cfg, x, params = make_problem(24, 15, 2, 3, 3, 0.3, empty=False)
    params["w"][0, 0, 0] = 0.0
    params["u"][0, 0, :] = 0.0
    x[:, 0] = 0
    x[0, :] = 0
    x[0, 0] = 3.0
    lp, pw, ok = _cells(cfg, x, params)
    assert int((~ok).sum()) == 1 and not bool(ok[0, 0])
    out = build_model(cfg, 8).waic_streaming({"counts": x}, draws=params, row_scores=True)
    assert out["n_excluded"] == 1 and out["n"] == 24 * 15 - 1
    _assert_totals(out, _totals(lp, pw, ok), None, "rate 0")
    _assert_rows(out, lp, pw, ok, "rate 0")


def test_row_chunks_and_several_batches_add_up():
    """max_rows below B (five chunks of one 32-row panel), an iterable of two batches and a
    data factory against the same rows as one batch: only the fp64 addition order differs."""
    cfg, x, params, mask = _dense_problem("poisson", 131, 97, 16, 4, 4700)
    m = _dense_model("poisson", cfg, mask, 32)
    one = m.waic_streaming({"counts": x}, draws=params, row_scores=True)
    chunked = m.waic_streaming({"counts": x}, draws=params, row_scores=True, max_rows=32)
    parts = [{"counts": x[:64].copy()}, {"counts": x[64:].copy()}]
    two = m.waic_streaming(parts, draws=params, row_scores=True)
    fac = m.waic_streaming(lambda: iter(parts), draws=params, row_scores=True)
    for tag, o in (("chunked", chunked), ("two batches", two), ("factory", fac)):
        assert o["n"] == one["n"] == 131 * 97 and o["n_excluded"] == 0
        for k in ("lppd", "pwaic", "waic", "se"):
            assert abs(o[k] - one[k]) <= 1e-12 * abs(one[k]), (tag, k, o[k], one[k])
        for k in ("row_lppd", "row_pwaic"):
            np.testing.assert_allclose(o[k].cpu().numpy(), one[k].cpu().numpy(), rtol=1e-12, err_msg=tag)


def test_fewer_than_two_draws_is_an_error():
    cfg, x, params, mask = _dense_problem("poisson", 8, 9, 2, 1, 4800)
    m = _dense_model("poisson", cfg, mask, 8)
    with pytest.raises(ValueError):
        m.waic_streaming({"counts": x}, nsamples=1)
    with pytest.raises(ValueError):
        m.waic_streaming({"counts": x}, draws=params)


def test_agrees_with_waic_on_the_surrogate_draws():
    """The 200 x 12 problem of test_waic_matches_pointwise_definition, same seed, both paths."""
    from spmf_amd import PoissonFactorization
    rng = np.random.default_rng(2)
    x = rng.poisson(1.0, size=(200, 12)).astype(np.float64)
    m = PoissonFactorization(latent_dim=2, feature_dim=12, u_tau_scale=1 / math.sqrt(2400),
                             device="cuda", panel_rows=64)
    torch.manual_seed(4)
    old = m.waic({"counts": x}, nsamples=50)
    torch.manual_seed(4)
    new = m.waic_streaming({"counts": x}, nsamples=50)
    torch.manual_seed(4)
    th = m.surrogate_distribution.sample(50)
    cfg = O.OracleConfig(latent_dim=2, feature_dim=12)
    lp, pw, ok = _cells(cfg, x, {k: th[k].double().cpu().numpy() for k in ("s", "u", "v", "w")})
    ref = _totals(lp, pw, ok)
    print("waic()", old, "waic_streaming()", new, "oracle", ref)
    assert set(new) == {"waic", "se", "lppd", "pwaic", "n", "n_excluded"}
    assert new["n"] == 2400 and new["n_excluded"] == 0
    assert abs(new["lppd"] - old["lppd"]) <= 1e-5 * abs(old["lppd"])
    assert abs(new["waic"] - old["waic"]) <= 1e-5 * abs(old["waic"])
    assert abs(new["pwaic"] - old["pwaic"]) <= 1e-3 * max(abs(old["pwaic"]), 1e-9) + 1e-9
    assert abs(new["se"] - ref["se"]) <= max(2.0 * abs(old["se"] - ref["se"]), 1e-5 * abs(ref["se"]))


def test_peak_memory_stays_far_below_the_materialised_tensor():
    """B = 1024, D = 2048, K = 16, S = 32: the [S,B,D] fp32 tensor is 268 MB and the
    materialising path holds four of them; the streaming call may take a quarter of one."""
    from spmf_amd.sparse import SparseCounts
    B, D, K, S = 1024, 2048, 16, 32
    cfg, x, params, mask = _dense_problem("poisson", B, D, K, S, 4900, density=0.05)
    m = _dense_model("poisson", cfg, mask, 256)
    batch = {"counts": SparseCounts.from_any(x, m.device, 256, latent_dim=K)}
    draws = {k: T(params[k]).to("cuda", torch.float32) for k in ("s", "u", "v", "w")}
    m.waic_streaming({"counts": x[:64].copy()}, draws=draws)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = m.waic_streaming(batch, draws=draws)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"peak above the allocation before the call: {extra / 2**20:.1f} MiB; "
          f"S*B*D*4 = {S * B * D * 4 / 2**20:.1f} MiB")
    assert extra < 0.25 * S * B * D * 4, extra
    lp, pw, ok = _cells(cfg, x, params)
    _assert_totals(out, _totals(lp, pw, ok), _materialised_se(m, batch, params), "memory case")


def test_a_step_is_undisturbed_by_a_streaming_call():
    """The call uses its own scratch: a deterministic step before and after it gives
    identical parts and gradients."""
    from spmf_amd import PoissonFactorization
    cfg, x, params = make_problem(200, 150, 16, 2, 5000, 0.05)
    m = PoissonFactorization(latent_dim=16, feature_dim=150, u_tau_scale=cfg.u_tau_scale,
                             column_norms=cfg.eta_i, initialize_distributions=False, device="cuda",
                             panel_rows=64, deterministic=True)
    m.xi_u_global = cfg.xi_u_global
    batch = {"counts": x}
    p1, g1, n1 = m.energy_and_grads(batch, params)
    p1 = {k: v.clone() for k, v in p1.items()}
    g1 = {k: v.clone() for k, v in g1.items()}
    out = m.waic_streaming(batch, draws=params)
    assert out["n"] == 200 * 150
    p2, g2, n2 = m.energy_and_grads(batch, params)
    for k in p1:
        assert torch.equal(p1[k], p2[k]), k
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    assert torch.equal(n1, n2)
