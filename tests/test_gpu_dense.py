"""GPU: dense per-cell outputs (log_likelihood_components,
poisson.py:156-184) and the non-finite replacement rule (:606-616) vs the
fp64 oracle."""
import math

import numpy as np
import pytest
import torch

from oracle import spmf_oracle as O
from _problems import LIKELIHOODS, _dense_model, _dense_problem, build_model, make_problem

pytestmark = pytest.mark.gpu
T = torch.as_tensor


@pytest.mark.parametrize("K,logt", [(3, False), (16, False), (8, True)])
def test_log_likelihood_components_dense(K, logt):
    cfg, x, params = make_problem(70, 45, K, 2, 91 + K, 0.25)
    cfg.log_transform = logt
    if logt:
        params["v"] *= 0.05
    from spmf_amd import PoissonFactorization
    m = PoissonFactorization(latent_dim=K, feature_dim=45, u_tau_scale=cfg.u_tau_scale,
                             log_transform=logt, column_norms=cfg.eta_i,
                             initialize_distributions=False, device="cuda", panel_rows=32)
    m.xi_u_global = cfg.xi_u_global
    ref = O.log_likelihood_components(cfg, T(x), T(params["s"]), T(params["u"]),
                                      T(params["v"]), T(params["w"]))
    got = m.log_likelihood_components(s=params["s"], u=params["u"], v=params["v"],
                                      w=params["w"], data={"counts": x})
    for k in ("rate", "log_likelihood"):
        g = got[k].cpu().double().numpy()
        r = ref[k].numpy()
        assert g.shape == r.shape == (2, 70, 45)
        np.testing.assert_allclose(g, r, rtol=1e-5, atol=1e-5 * np.abs(r).max(), err_msg=k)
    pred = m.predictive_distribution(s=params["s"], u=params["u"], v=params["v"],
                                     w=params["w"], data={"counts": x})
    np.testing.assert_allclose(pred["ll"].cpu().double().numpy(),
                               ref["log_likelihood"].sum(-1).numpy(), rtol=1e-4)
    one = {k: T(v[0]) for k, v in params.items()}
    g1 = m.log_likelihood_components(s=one["s"], u=one["u"], v=one["v"], w=one["w"],
                                     data={"counts": x})
    assert tuple(g1["rate"].shape) == (70, 45)


def _assert_cells(got, ref, shape, tag=""):
    """The bar of test_log_likelihood_components_dense on 'rate' and 'log_likelihood'; the
    reference must be finite everywhere (NaN == NaN would pass assert_allclose)."""
    for k in ("rate", "log_likelihood"):
        g = got[k].cpu().double().numpy()
        r = ref[k].numpy()
        assert g.shape == r.shape == shape, (tag, k, g.shape, r.shape)
        assert np.isfinite(r).all(), (tag, k)
        np.testing.assert_allclose(g, r, rtol=1e-5, atol=1e-5 * np.abs(r).max(), err_msg=f"{tag} {k}")


def _check_dense(lik, cfg, x, params, mask, panel_rows, data=None, rows=slice(None)):
    S = params["u"].shape[0]
    xr = x[rows]
    ref = O.log_likelihood_components(cfg, T(xr), T(params["s"]), T(params["u"]), T(params["v"]),
                                      T(params["w"]))
    m = _dense_model(lik, cfg, mask, panel_rows)
    data = {"counts": x} if data is None else data
    got = m.log_likelihood_components(s=params["s"], u=params["u"], v=params["v"], w=params["w"],
                                      data=data)
    _assert_cells(got, ref, (S,) + xr.shape, lik)
    return m, ref


# K just inside and just across every padded width KP = 4 ... 64 on every likelihood, and the
# K > 64 widths (128, 256) on Poisson/linear, the only context the library admits there.  D walks
# 63, 64, 65, 130, 333 (one, exactly one, two, three and six 64-column blocks with a ragged last
# one), B walks 1, 3, 5, 70 (the kernel takes four rows per block), S alternates 1 and 3.
_DS = (63, 64, 65, 130, 333)
_BS = (1, 3, 5, 70)
SHAPE_GRID = [(lik, K, _DS[(i + j) % 5], _BS[(i + 2 * j) % 4], (1, 3)[(i + j) % 2])
              for i, lik in enumerate(LIKELIHOODS) for j, K in enumerate((4, 5, 16, 17, 32, 33, 64))]
SHAPE_GRID += [("poisson", K, _DS[j % 5], _BS[(j + 1) % 4], (3, 1)[j % 2])
               for j, K in enumerate((65, 128, 129, 200, 256))]


def test_shape_grid_reaches_every_size_the_kernels_branch_on():
    """The grid above is arithmetic: spell out what it has to contain."""
    for lik in LIKELIHOODS:
        assert {c[1] for c in SHAPE_GRID if c[0] == lik} >= {4, 5, 16, 17, 32, 33, 64}
    assert {c[1] for c in SHAPE_GRID if c[0] == "poisson"} >= {65, 128, 129, 200, 256}
    assert {c[2] for c in SHAPE_GRID} == set(_DS) and {c[3] for c in SHAPE_GRID} == set(_BS)
    assert {c[4] for c in SHAPE_GRID} == {1, 3}
    assert any(c[0] == "mixed" and c[2] > 64 for c in SHAPE_GRID)


@pytest.mark.parametrize("lik,K,D,B,S", SHAPE_GRID)
def test_per_cell_outputs_over_k_d_b_and_likelihood(lik, K, D, B, S):
    """dense_rate_kernel<KP> at every KP, blockIdx.x > 0 with the d0 + dl < D edge, ragged row
    blocks, and all five likelihood codes -- each cell against the fp64 oracle."""
    cfg, x, params, mask = _dense_problem(lik, B, D, K, S, 7000 + 13 * K + D + B)
    _check_dense(lik, cfg, x, params, mask, panel_rows=32)


def _long_rows(B, D, lengths, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((B, D))
    for b in range(B):
        n = lengths[b % len(lengths)]
        cols = rng.choice(D, size=n, replace=False)
        x[b, cols] = 1 + rng.poisson(1.5, size=n)
    return x


@pytest.mark.parametrize("lik,K", [("poisson", 16), ("poisson_log", 8), ("bernoulli_log", 5),
                                   ("mixed", 33), ("poisson", 200)])
def test_per_cell_outputs_on_rows_longer_than_one_wave(lik, K):
    """Rows of 65 to 300 stored entries: dense_fix_kernel's lanes stride the row in steps of 64."""
    B, D = 10, 333
    x = _long_rows(B, D, [65, 127, 128, 129, 192, 193, 257, 300, 1, 64], 31 + K)
    cfg, x, params, mask = _dense_problem(lik, B, D, K, 2, 8100 + K, x=x)
    assert (x > 0).sum(1).max() >= 250
    _check_dense(lik, cfg, x, params, mask, panel_rows=4)


@pytest.mark.parametrize("lik", ["poisson", "bernoulli"])
def test_per_cell_outputs_of_a_tall_batch(lik):
    """B > 16 384: dense_fix_kernel has 4096 blocks of four waves, so its row loop strides."""
    B, D, K = 20011, 6, 3
    cfg, x, params, mask = _dense_problem(lik, B, D, K, 1, 8200, density=0.5)
    _check_dense(lik, cfg, x, params, mask, panel_rows=4096)


def test_per_cell_outputs_with_large_and_fractional_counts():
    """Counts up to 60 000 (lgammaf far from its small-argument branch, x log r of order 1e5)
    and fractional counts (no packed-entry stream, lgamma off the integers)."""
    B, D, K = 70, 130, 8
    rng = np.random.default_rng(5)
    big = ((rng.random((B, D)) < 0.3) * rng.integers(1, 60001, size=(B, D))).astype(np.float64)
    big[0, 0] = 60000.0
    cfg, x, params, mask = _dense_problem("poisson", B, D, K, 1, 8300, x=big)
    _check_dense("poisson", cfg, x, params, mask, panel_rows=32)
    frac = (rng.random((B, D)) < 0.3) * np.round(rng.gamma(2.0, 1.5, size=(B, D)) + 0.125, 3)
    frac = frac.astype(np.float32).astype(np.float64)
    assert ((frac != np.floor(frac)) & (frac > 0)).sum() > 100
    for lik in ("poisson", "poisson_log"):
        cfg, x, params, mask = _dense_problem(lik, B, D, K, 3, 8301, x=frac.copy())
        _check_dense(lik, cfg, x, params, mask, panel_rows=32)


@pytest.mark.parametrize("lik", ["poisson", "poisson_log", "mixed"])
def test_per_cell_outputs_of_a_panel_range_minibatch(lik):
    """{"counts": sc, "panels": (p0, p1)} with p0 > 0: row_ptr, row scales and the outputs all
    start at row_base."""
    from spmf_amd import SparseCounts
    B, D, K, P = 150, 130, 17, 16
    cfg, x, params, mask = _dense_problem(lik, B, D, K, 3, 8400)
    sc = SparseCounts.from_any(x, "cuda", P)
    m, _ = _check_dense(lik, cfg, x, params, mask, P, data={"counts": sc, "panels": (2, 7)},
                        rows=slice(2 * P, 7 * P))
    # the last, ragged panel of the same resident matrix through the same model
    ref = O.log_likelihood_components(cfg, T(x[9 * P:]), T(params["s"]), T(params["u"]),
                                      T(params["v"]), T(params["w"]))
    got = m.log_likelihood_components(s=params["s"], u=params["u"], v=params["v"], w=params["w"],
                                      data={"counts": sc, "panels": (9, 10)})
    _assert_cells(got, ref, (3, B - 9 * P, D), "last panel")


@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_per_cell_outputs_without_a_sample_axis(lik):
    B, D, K = 5, 65, 5
    cfg, x, params, mask = _dense_problem(lik, B, D, K, 1, 8500)
    m, ref = _check_dense(lik, cfg, x, params, mask, panel_rows=32)
    one = {k: T(v[0]) for k, v in params.items()}
    got = m.log_likelihood_components(s=one["s"], u=one["u"], v=one["v"], w=one["w"], data={"counts": x})
    _assert_cells(got, {k: v[0] for k, v in ref.items()}, (B, D), lik)


def test_per_cell_outputs_of_a_batch_taller_than_a_grid_extent():
    """B = 270 000 rows of 5 columns: four rows per block put 67 500 blocks on the grid's y extent
    (dense_ll.hip launch_dense_t), past the 65 535 of a CUDA launch.  The HIP runtime bounds
    grid * block per dimension by 2^32 instead and takes the launch; a refusal would surface as an
    SpmfError (api_step.hip checks hipGetLastError), a wrong row mapping as a value mismatch here."""
    B, D, K = 270000, 5, 2
    cfg, x, params, mask = _dense_problem("poisson", B, D, K, 1, 8600, density=0.5)
    _check_dense("poisson", cfg, x, params, mask, panel_rows=None)


def test_non_finite_rule_matches_reference_semantics():
    """A stored cell with rate 0 has log-pmf -inf: the reference replaces it by
    (global min over [S,B,D] - 10) (poisson.py:606-616)."""
    cfg, x, params = make_problem(24, 15, 2, 2, 3, 0.3, empty=False)
    params["w"][0, 0, 0] = 0.0          # phi = 0 for draw 0, column 0
    params["u"][0, 0, :] = 0.0          # column 0 feeds nothing into z
    x[:, 0] = 0
    x[0, :] = 0
    x[0, 0] = 3.0                       # row 0: only column 0 -> z_0 = 0 -> rate 0, x = 3
    ref = O.unormalized_log_prob_parts(cfg, x, params)
    ll = O.log_likelihood_components(cfg, T(x), T(params["s"]), T(params["u"]),
                                     T(params["v"]), T(params["w"]))["log_likelihood"]
    assert torch.isinf(ll[0, 0, 0]) and torch.isfinite(ll[1]).all()
    m = build_model(cfg, 8)
    got = m.unormalized_log_prob_parts({"counts": x}, **params)
    np.testing.assert_allclose(got["x"].cpu().numpy(), ref["x"].numpy(), rtol=1e-5)
    np.testing.assert_allclose(got["z"].cpu().numpy(), ref["z"].numpy(), rtol=1e-5)
    # and the energy/grad entry point reports the cell instead of hiding it
    _, _, nnf = m.energy_and_grads({"counts": x}, params)
    assert nnf.cpu().tolist() == [1.0, 0.0]


def test_waic_matches_pointwise_definition():
    from spmf_amd import PoissonFactorization
    rng = np.random.default_rng(2)
    x = rng.poisson(1.0, size=(200, 12)).astype(np.float64)
    m = PoissonFactorization(latent_dim=2, feature_dim=12, u_tau_scale=1 / math.sqrt(2400),
                             device="cuda", panel_rows=64)
    torch.manual_seed(4)
    out = m.waic({"counts": x}, nsamples=50)
    assert set(out) == {"waic", "se", "lppd", "pwaic"}
    torch.manual_seed(4)
    th = m.surrogate_distribution.sample(50)
    cfg = O.OracleConfig(latent_dim=2, feature_dim=12)
    ll = O.log_likelihood_components(cfg, T(x), th["s"].double().cpu(), th["u"].double().cpu(),
                                     th["v"].double().cpu(), th["w"].double().cpu())["log_likelihood"]
    lppd = (torch.logsumexp(ll, 0) - math.log(50)).sum().item()
    pw = ll.var(0, unbiased=True).sum().item()
    assert abs(out["lppd"] - lppd) <= 1e-5 * abs(lppd)
    assert abs(out["pwaic"] - pw) <= 1e-3 * max(abs(pw), 1e-9) + 1e-9
    assert abs(out["waic"] + 2 * (lppd - pw)) <= 1e-5 * abs(out["waic"])
