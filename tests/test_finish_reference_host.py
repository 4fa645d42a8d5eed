"""CPU: the references and inputs of tests/test_gpu_finish_edges.py, pinned without a GPU.

  * oracle/sparse_exact.prior_term against fp64 autograd of oracle.prior_log_prob_parts, on the magnitude regimes
    the GPU test feeds the finish kernels;
  * oracle/sparse_exact.shard_accumulators + finish_from_acc (and the yardsticks tests/_finish_table.py puts beside
    it) against oracle.energy_and_grads, at the shape edges;
  * the input condition of the regimes: after the redraw every yardstick is below 1e37 and at most 2 % of any
    variable's entries were redrawn;
  * the fp32 formulas of the prior's scale gradients restated in numpy: the order the kernel used to take
    ((q^2 - 1) / sig first) overflows on entries whose gradient is in range, the order it takes now does not.
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _finish_table as F
from oracle import sparse_exact as SE
from oracle import spmf_oracle as O

REGIME_CASES = F.REGIME_CASES


def _cfg(K, D=33, decay=0.99, **kw):
    return O.OracleConfig(latent_dim=K, feature_dim=D, u_tau_scale=1.0 / math.sqrt(40 * D), s_tau_scale=0.7,
                          symmetry_breaking_decay=decay, **kw)


@pytest.mark.parametrize("regime,K,decay", REGIME_CASES)
def test_regime_inputs_meet_the_condition(regime, K, decay):
    cfg = _cfg(K, decay=decay)
    p, share = F.draw_regime(cfg, 2, regime, F.SEEDS[regime])
    sc = F.prior_scales(cfg, p)
    for n in F.VAR_ORDER:
        assert (p[n].astype(np.float32).astype(np.float64) == p[n]).all() and (p[n] > 0).all()
        assert sc[n].max() < F.FP32_RANGE, (n, sc[n].max())
        assert share[n] <= 0.02, (regime, n, share[n])
    print(regime, K, decay, {n: round(v, 4) for n, v in share.items() if v})


@pytest.mark.parametrize("regime,K,decay", REGIME_CASES)
def test_prior_term_equals_autograd_of_the_oracle(regime, K, decay):
    cfg = _cfg(K, decay=decay)
    p, _ = F.draw_regime(cfg, 2, regime, F.SEEDS[regime])
    parts, grads, yard = F.prior_reference(cfg, p)
    pg = {k: torch.as_tensor(v).clone().requires_grad_(True) for k, v in p.items()}
    pp = O.prior_log_prob_parts(cfg, pg)
    g = torch.autograd.grad(sum(v.sum() for v in pp.values()), [pg[n] for n in pg])
    sc = F.prior_scales(cfg, p)
    for n, gi in zip(pg, g):
        assert (np.abs(grads[n] - gi.numpy()) <= 1e-12 * sc[n]).all(), n
        assert np.abs(parts[n] - pp[n].detach().numpy()).max() <= 1e-13 * yard[n].max(), n
        assert np.isfinite(yard[n]).all() and (yard[n] > 0).all()


def test_abs_horseshoe_reference_is_finite_over_its_range():
    for K in (3, 16):
        cfg = _cfg(K, horseshoe_plus=False)
        p = F.draw_abs_horseshoe(cfg, 2, 31 + K)
        parts, grads, yard = F.prior_reference(cfg, p)
        sc = F.prior_scales(cfg, p)
        assert set(parts) == {"v", "w", "u", "s"}
        for n in parts:
            assert np.isfinite(parts[n]).all() and np.isfinite(grads[n]).all() and np.isfinite(yard[n]).all()
            assert np.abs(grads[n]).max() < F.FP32_RANGE
            assert (np.abs(grads[n]) <= sc[n] * (1 + 1e-12)).all()


def _problem(B, D, K, seed):
    rng = np.random.default_rng(seed)
    x = ((rng.random((B, D)) < 0.3) * (1 + rng.poisson(2.0, size=(B, D)))).astype(np.float64)
    x[0, 0] = 2.0
    if D > 2:
        x[:, D // 2] = 0
    cfg = O.OracleConfig(latent_dim=K, feature_dim=D, u_tau_scale=1.0 / math.sqrt(B * D))
    cfg.eta_i = torch.as_tensor(F.f32(rng.uniform(0.5, 3.0, size=(1, D))))
    cfg.xi_u_global = 4.0
    return cfg, x, O.random_params(cfg, 1, seed + 1, fp32_exact=True)


@pytest.mark.parametrize("D,K", [(1, 1), (7, 3), (9, 4), (33, 5), (65, 8), (33, 17)])
def test_finish_from_acc_and_its_yardsticks_against_the_oracle(D, K):
    """shard_accumulators rounds every accumulator to fp32 (2^-24 of its magnitude, the (hi, lo) scalars to 2^-48):
    the chain from them must agree with the dense oracle to a few 2^-24 of the data yardstick, parts to 1e-12."""
    cfg, x, params = _problem(12, D, K, 500 + D + K)
    pref, _, groups = O.energy_and_grads(cfg, x, params)
    one = {k: v[0] for k, v in params.items()}
    eta = cfg.eta_i.numpy().reshape(-1)
    acc = SE.shard_accumulators(sp.csr_matrix(x), eta, cfg.xi_u_global, True, one["u"], one["v"], one["w"], one["s"])
    lg = float(torch.lgamma(torch.as_tensor(x) + 1.0).sum())
    ref, sc, yard = F.data_reference(acc, x.shape[0], lg, eta, one)
    for n in ("u", "v", "w", "s"):
        err = np.abs(ref["grads"][n] - groups["data"][n][0].numpy())
        assert (err <= 4 * 2.0 ** -24 * sc[n] + 1e-300).all(), (n, float((err / np.maximum(sc[n], 1e-300)).max()))
    for n in ("x", "z"):
        assert abs(ref[n] - float(pref[n][0])) <= 1e-12 * yard[n], n
    # the column split is a permutation of the same numbers
    if D == 65:
        KP = SE.padded_k(K)
        sa = F.split_layout(acc, D, K, 32)
        assert sa.size == acc.size and sorted(sa.tolist()) == sorted(acc.tolist())
        h0 = 32 * (2 * KP + 1)
        assert (sa[:32 * KP] == acc[:32 * KP]).all()                                          # gA', lower half
        assert (sa[h0:h0 + 33 * KP] == acc[32 * KP:D * KP]).all()                             # gA', upper half
        assert (sa[h0 + 2 * 33 * KP:h0 + 2 * 33 * KP + 33] == acc[2 * D * KP + 32:2 * D * KP + D]).all()   # gphi


def test_pack_acc_keeps_what_fp32_cannot_hold():
    rng = np.random.default_rng(5)
    D, K = 9, 3
    acc = F.random_acc(D, K, 1_000_003, rng)
    KP = SE.padded_k(K)
    tail = acc[2 * D * KP + D:].astype(np.float64).reshape(-1, 2)
    assert tail.shape[0] == SE.TAIL_HEAD + KP
    assert (tail[:2, 1] != 0).all()                       # llx, sum z^2: the low word is used
    assert tail[2].sum() == 3.0 and tail[4].sum() == 7.0
    assert (acc[:D * KP].reshape(D, KP)[:, K:] == 0).all() and (tail[SE.TAIL_HEAD + K:] == 0).all()
    assert (acc[:D * KP].reshape(D, KP)[:, :K] == 0).all(1).any()        # the empty column


def _scale_grads_fp32(y, s1, s2, reordered):
    """d/ds1, d/ds2 of HalfNormal(s1 * s2)(y) in fp32 arithmetic, both orders of finish_body.h."""
    f = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        y, s1, s2 = f(y), f(s1), f(s2)
        i = f(1) / (s1 * s2)
        q = y * i
        if reordered:
            i1, i2 = f(1) / s1, f(1) / s2
            return q * (q * i1) - i1, q * (q * i2) - i2
        gs = (q * q - f(1)) * i
        return gs * s2, gs * s1


@pytest.mark.parametrize("regime", ["shrunk", "wide"])
def test_scale_gradient_order_in_fp32(regime):
    """Suspect 1 of the issue on the CPU: entry by entry over 200 000 draws of one regime whose fp64 gradients are
    all below 1e37, (q^2 - 1) / sig multiplied back overflows on some; q (q / s) - 1 / s on none, and stays within
    1e-5 of the yardstick (q^2 + 1) / s."""
    rng = np.random.default_rng(77)
    n = 200_000
    R = F.REGIMES[regime]
    lu = lambda r: F.f32(10.0 ** rng.uniform(math.log10(r[0]), math.log10(r[1]), n))
    for y, s1, s2 in ((lu(R["uvw"]), lu(R["eta"]), lu(R["u_tau"]) * 0.99 ** rng.integers(0, 256, n)),
                      (lu(R["s"]), lu(R["eta"]), lu(R["s_tau"]))):
        s2 = F.f32(s2)
        q = y / (s1 * s2)
        ref1, ref2 = (q * q - 1) / s1, (q * q - 1) / s2
        y1, y2 = (q * q + 1) / s1, (q * q + 1) / s2
        ok = (y1 < F.FP32_RANGE) & (y2 < F.FP32_RANGE)
        old = _scale_grads_fp32(y, s1, s2, False)
        new = _scale_grads_fp32(y, s1, s2, True)
        bad_old = ok & ~(np.isfinite(old[0]) & np.isfinite(old[1]))
        print(regime, "entries in range:", int(ok.sum()), "old order non-finite:", int(bad_old.sum()))
        assert np.isfinite(new[0][ok]).all() and np.isfinite(new[1][ok]).all()
        assert (np.abs(new[0].astype(np.float64) - ref1)[ok] <= 1e-5 * y1[ok]).all()
        assert (np.abs(new[1].astype(np.float64) - ref2)[ok] <= 1e-5 * y2[ok]).all()
        if regime == "wide":
            assert bad_old.any()
