"""GPU: the finish kernels (spmf_amd/csrc/finish_body.h, finish.hip, the prior half inside prep.hip's begin_kernel)
against fp64 references, at the value and shape edges -- not through whole-model parity.

  * the prior's twelve gradients over three magnitude regimes (a shrunk horseshoe reaches 1e-8 in u and 1e-6 in
    u_tau) at the project's entry-wise 1e-5, and its twelve parts at fp64 accuracy: 1e-12 of the sum of their
    absolute additive terms;
  * the AbsHorseshoe branch over u in [1e-30, 1e6];
  * the data half on accumulators the test chose (cancelling gphi - B, (hi, lo) scalars an fp32 cannot hold,
    empty columns, per-draw strides, the column split), parts 'x' and 'z' at 1e-12 as well;
  * every tile edge of D and every KP instantiation of K; the other likelihood codes; the three call routes.

The harness is tests/_finish_table.py: every output lives between canary margins and starts as NaN.
tests/test_finish_reference_host.py pins the references and the input condition on the CPU.

Largest error observed on an MI355X over the whole file, as a share of its bound:
  gradients (1e-5 x yardstick, entry-wise): v 0.015, w 0.015, u 0.036, u_eta 0.042, u_tau 0.080, s_eta 0.031,
    s_tau 0.028, s 0.026, u_eta_a 0.028, u_tau_a 0.026, s_eta_a 0.029, s_tau_a 0.027;
  parts (1e-12 x sum of |terms|): v 1.9e-4, w 4.4e-4, u 2.8e-3, u_eta 5.4e-4, u_tau 1.7e-4, s_eta 2.1e-4,
    s_tau 1.7e-4, s 3.8e-4, u_eta_a 4.1e-4, u_tau_a 3.7e-4, s_eta_a 3.5e-4, s_tau_a 3.2e-4, z 0, x 0.
On the kernels before this file existed: parts v 2.1e4, u (AbsHorseshoe) 2.3e3, s 5.8e4, u_tau_a 9.8e4,
s_tau_a 9.2e3, x 5.1e2 times the bound, and non-finite G[u_eta] entries in the wide regime and at the domain's edge.
"""
import math

import numpy as np
import pytest
import torch

import _finish_table as F
from _gradcheck import assert_grads_entrywise, worst_entry
from oracle import spmf_oracle as O
from _problems import bernoulli_problem, mixed_problem, poisson_log_problem

pytestmark = pytest.mark.gpu

RATIOS = {}
PART_TOL = 1e-12
IDX = {n: i for i, n in enumerate(O.VAR_ORDER + ("z", "x"))}


def _note(key, val):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(val))
    print(f"[ratio] {key}: {float(val):.3e} of its bound (largest so far {RATIOS[key]:.3e})")


def _cfg(K, D, decay=0.99, eta=None, **kw):
    cfg = O.OracleConfig(latent_dim=K, feature_dim=D, u_tau_scale=1.0 / math.sqrt(40 * D), s_tau_scale=0.7,
                         symmetry_breaking_decay=decay, **kw)
    if eta is not None:
        cfg.eta_i = torch.as_tensor(np.asarray(eta).reshape(1, D))
    return cfg


def _model(cfg, split=0):
    from spmf_amd import PoissonFactorization
    m = PoissonFactorization(latent_dim=cfg.latent_dim, feature_dim=cfg.feature_dim, u_tau_scale=cfg.u_tau_scale,
                             s_tau_scale=cfg.s_tau_scale, symmetry_breaking_decay=cfg.symmetry_breaking_decay,
                             column_norms=cfg.eta_i, initialize_distributions=False, device="cuda", panel_rows=32,
                             horshoe_plus=cfg.horseshoe_plus)
    m.xi_u_global = 4.0
    if split:
        m.enable_column_split(split)
    return m


def _check_parts(tag, got, ref, yard, names):
    """|part - ref| <= 1e-12 x (sum of the absolute additive terms), per draw."""
    bad = []
    for n in names:
        g = got[:, IDX[n]]
        assert np.isfinite(g).all(), (tag, n, g)
        share = float((np.abs(g - ref[n]) / (PART_TOL * yard[n])).max())
        _note(f"part {n}", share)
        if not share <= 1.0:
            bad.append(f"{n}: |hip - ref| = {share:.3e} x its bound")
    assert not bad, (tag, bad)


def _check_grads(tag, got, ref, scales, note=True):
    for n in ref:
        assert np.isfinite(got[n]).all(), (tag, n, "non-finite gradient entries", int((~np.isfinite(got[n])).sum()))
        if note:
            _note(f"grad {n}", worst_entry(got[n], ref[n], scales[n])[0] / 1e-5)
    assert_grads_entrywise(got, ref, scales, 1e-5, tag)


def _zero_acc(run):
    return np.zeros((run.S, run.n_acc), dtype=np.float32)


# ---- 3.1 / 3.2: the prior over magnitude regimes -----------------------------------------------------------------
@pytest.mark.parametrize("route", ["a", "c"])
@pytest.mark.parametrize("regime,K,decay", F.REGIME_CASES)
def test_prior_gradients_and_parts_over_regimes(regime, K, decay, route):
    """Zero accumulators, no rows: the data half adds exactly nothing, what comes back is the prior alone.  Every
    gradient entry finite and within 1e-5 of its yardstick (entry-wise and in the array norm), every part within
    1e-12 of the sum of its absolute terms."""
    D, S = 33, 2
    cfg = _cfg(K, D, decay)
    p, share = F.draw_regime(cfg, S, regime, F.SEEDS[regime])
    assert max(share.values()) <= 0.02
    parts, grads, yard = F.prior_reference(cfg, p)
    scales = F.prior_scales(cfg, p)
    run = F.FinishRun(_model(cfg), p, F.tiny_batch(D, np.random.default_rng(1)))
    out = run.run(route, acc=_zero_acc(run), rows=0, lgamma=0.0)
    tag = f"{regime} K={K} decay={decay} route {route}"
    _check_grads(tag, out["grads"], grads, scales)
    _check_parts(tag, out["parts"], parts, yard, O.VAR_ORDER)
    assert (out["parts"][:, 12:] == 0).all() and (out["nnf"] == 0).all()


@pytest.mark.parametrize("route", ["a", "c"])
def test_scale_gradients_at_the_edge_of_the_domain(route):
    """The stated domain (include/spmf_hip.h, spmf_finish): a gradient entry is returned whenever its yardstick is
    below 1e37.  Exactly there: sigma = 1e-8, q = 3e16 in the u chain at (0, 0) and in the s chain at row 0 of
    column 0 put d/d u_eta, d/d u_tau[0], d/d s_eta, d/d s_tau[0] at 9e36 ((q^2 - 1) / sigma would be 9e40)."""
    D, K, S = 33, 5, 2
    cfg = _cfg(K, D, 1.0)
    p, _ = F.draw_regime(cfg, S, "benign", 29)
    for y, e, t in (("u", "u_eta", "u_tau"), ("s", "s_eta", "s_tau")):
        p[y][:, 0, 0], p[e][:, 0, 0], p[t][:, 0, 0] = F.f32(3e8), F.f32(1e-4), F.f32(1e-4)
    parts, grads, yard = F.prior_reference(cfg, p)
    scales = F.prior_scales(cfg, p)
    for n in ("u_eta", "u_tau", "s_eta", "s_tau"):
        assert 5e36 < scales[n][:, 0, 0].min() and scales[n].max() < F.FP32_RANGE, (n, scales[n][:, 0, 0])
    run = F.FinishRun(_model(cfg), p, F.tiny_batch(D, np.random.default_rng(3)))
    out = run.run(route, acc=_zero_acc(run), rows=0, lgamma=0.0)
    _check_grads(f"domain edge route {route}", out["grads"], grads, scales, note=False)
    _check_parts(f"domain edge route {route}", out["parts"], parts, yard, O.VAR_ORDER)


@pytest.mark.parametrize("pw", [0.0, 0.37, 1.0])
def test_prior_weight(pw):
    """grads = data + prior_weight * prior on injected accumulators; at 0 the prior contributes exactly nothing:
    the gradients of the eight variables the likelihood does not see are exactly 0.  The parts are unweighted."""
    D, K, S = 33, 5, 2
    rng = np.random.default_rng(41)
    eta = F.f32(rng.uniform(0.5, 3.0, D))
    cfg = _cfg(K, D, eta=eta)
    p, _ = F.draw_regime(cfg, S, "benign", 17)
    run = F.FinishRun(_model(cfg), p, F.tiny_batch(D, rng))
    B, lg = 1_000_003, 12345.678
    acc = np.stack([F.random_acc(D, K, B, rng) for _ in range(S)])
    out = run.run("a", acc=acc, prior_weight=pw, rows=B, lgamma=lg)
    parts, grads, yard = F.prior_reference(cfg, p)
    psc = F.prior_scales(cfg, p)
    ref = {n: pw * grads[n] for n in grads}
    sc = {n: pw * psc[n] for n in grads}
    for s in range(S):
        dref, dsc, _ = F.data_reference(acc[s], B, lg, eta, {k: v[s] for k, v in p.items()})
        for n in ("u", "v", "w", "s"):
            ref[n][s] += dref["grads"][n]
            sc[n][s] += dsc[n]
    _check_grads(f"prior_weight {pw}", out["grads"], ref, sc)
    _check_parts(f"prior_weight {pw}", out["parts"], parts, yard, O.VAR_ORDER)
    if pw == 0.0:
        for n in O.VAR_ORDER:
            if n not in ("u", "v", "w", "s"):
                assert (out["grads"][n] == 0).all(), n


# ---- 3.3: the AbsHorseshoe branch --------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["a", "c"])
@pytest.mark.parametrize("K", [3, 16])
def test_abs_horseshoe_branch(K, route):
    D, S = 33, 2
    cfg = _cfg(K, D, horseshoe_plus=False)
    p = F.draw_abs_horseshoe(cfg, S, 31 + K)
    parts, grads, yard = F.prior_reference(cfg, p)
    scales = F.prior_scales(cfg, p)
    run = F.FinishRun(_model(cfg), p, F.tiny_batch(D, np.random.default_rng(2)))
    out = run.run(route, acc=_zero_acc(run), rows=0, lgamma=0.0)
    tag = f"abs_horseshoe K={K} route {route}"
    _check_grads(tag, out["grads"], grads, scales)
    _check_parts(tag, out["parts"], parts, yard, ("v", "w", "u", "s"))
    gone = [IDX[n] for n in O.VAR_ORDER if n not in ("v", "w", "u", "s")]
    assert (out["parts"][:, gone] == 0).all()            # the variables this model does not have


# ---- 3.4: the data half on injected accumulators -----------------------------------------------------------------
def _data_case(D, K, S, B, route, split=0, seed=0, with_nnf=True, rows_local=False):
    rng = np.random.default_rng(1000 + 7 * D + K + seed)
    eta = F.f32(rng.uniform(0.5, 3.0, D))
    cfg = _cfg(K, D, eta=eta)
    p, _ = F.draw_regime(cfg, S, "benign", 19 + seed)
    run = F.FinishRun(_model(cfg, split), p, F.tiny_batch(D, rng))
    if rows_local:
        B = run.rows
    lg = float(rng.uniform(1e3, 1e6)) + 0.0625
    acc = np.stack([F.random_acc(D, K, B, rng) for _ in range(S)])
    dev = np.stack([F.split_layout(a, D, K, split) for a in acc]) if split else acc
    out = run.run(route, acc=dev, rows=B, lgamma=lg, with_nnf=with_nnf)
    parts, grads, yard = F.prior_reference(cfg, p)
    sc = F.prior_scales(cfg, p)
    x_ref, z_ref, x_y, z_y = (np.zeros(S) for _ in range(4))
    for s in range(S):
        dref, dsc, dy = F.data_reference(acc[s], B, lg, eta, {k: v[s] for k, v in p.items()})
        for n in ("u", "v", "w", "s"):
            grads[n][s] += dref["grads"][n]
            sc[n][s] += dsc[n]
        x_ref[s], z_ref[s], x_y[s], z_y[s] = dref["x"], dref["z"], dy["x"], dy["z"]
    parts.update(x=x_ref, z=z_ref)
    yard.update(x=x_y, z=z_y)
    tag = f"data half D={D} K={K} S={S} B={B} route {route} split {split}"
    _check_grads(tag, out["grads"], grads, sc)
    _check_parts(tag, out["parts"], parts, yard, O.VAR_ORDER + ("z", "x"))
    if with_nnf:
        assert (out["nnf"][:S] == 3).all() and (out["nnf"][S:] == 7).all(), out["nnf"]
    return run, dev, out, (B, lg)


@pytest.mark.parametrize("route,rows_local,split", [("a", False, 0), ("a", True, 0), ("c", False, 0), ("a", False, 32),
                                                    ("c", True, 32)])
def test_data_half_on_injected_accumulators(route, rows_local, split):
    """S = 3 draws with their own accumulators (the per-draw strides), n_rows_global the batch's own or 1 000 003,
    D = 65 with and without the column split Dh = 32."""
    _data_case(65, 5, 3, 1_000_003, route, split=split, rows_local=rows_local)


def test_data_half_without_n_nonfinite():
    _data_case(65, 5, 3, 1_000_003, "a", with_nnf=False, seed=1)


# ---- 3.5: shapes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 7, 8, 9, 31, 32, 33, 65])
def test_shapes_D(D):
    """The FTD = 32 tile edges of the finish and the kPrepSeg = 8 segment edges of the prep sums (part 'x')."""
    _data_case(D, 5, 2, 1_000_003, "a")


def test_shapes_more_than_64_finish_blocks():
    """D = 2049: 65 finish blocks, the second reduce stage loops."""
    _data_case(2049, 2, 1, 1_000_003, "a")


@pytest.mark.parametrize("K", [1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256])
def test_shapes_K(K):
    """Every KP instantiation at K = KP and at K = KP / 2 + 1 (D = 33: two blocks, the second with one column)."""
    _data_case(33, K, 1, 1_000_003, "a")


# ---- 3.6: the other likelihood codes (their own data pass, shrunk prior variables) ---------------------------------
def _shrunk_prior_variables(cfg, params, seed):
    """u, v, w, s as the problem has them; the eight scale variables from the shrunk regime."""
    S = params["u"].shape[0]
    sh, _ = F.draw_regime(_cfg(cfg.latent_dim, cfg.feature_dim), S, "shrunk", seed)
    for n in O.VAR_ORDER:
        if n not in ("u", "v", "w", "s"):
            params[n] = sh[n]
    sc = F.prior_scales(cfg, params)
    assert max(float(v.max()) for v in sc.values()) < F.FP32_RANGE
    return params


@pytest.mark.parametrize("kind", ["log_transform", "bernoulli", "mixed"])
def test_other_likelihood_codes(kind):
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    B, D, K, S = 40, 33, 5, 2
    if kind == "log_transform":
        cfg, x, params = poisson_log_problem((B, D, 0.3), K, S, 71)
        params["v"] = F.f32(params["v"])
        m = PoissonFactorization(latent_dim=K, feature_dim=D, u_tau_scale=cfg.u_tau_scale, log_transform=True,
                                 column_norms=cfg.eta_i, initialize_distributions=False, device="cuda", panel_rows=32)
    elif kind == "bernoulli":
        cfg, x, params = bernoulli_problem((B, D, 0.3), K, S, 72)
        assert (params["v"] < 0).any() and (params["w"] < 0).all()
        m = BernoulliFactorization(latent_dim=K, feature_dim=D, u_tau_scale=cfg.u_tau_scale, column_norms=cfg.eta_i,
                                   device="cuda", panel_rows=32)
    else:
        cfg, x, params, mask = mixed_problem((B, D, 0.3), K, S, 73)
        assert (mask == (np.arange(D) % 2 == 1)).all() and (params["w"][..., mask] < 0).all()
        assert (params["v"][..., mask] < 0).any()
        m = MixedFactorization(mask, latent_dim=K, u_tau_scale=cfg.u_tau_scale, column_norms=cfg.eta_i,
                               device="cuda", panel_rows=32)
    m.xi_u_global = cfg.xi_u_global
    params = _shrunk_prior_variables(cfg, params, 23)
    pref, gref, _ = O.energy_and_grads(cfg, x, params)
    parts, grads, nnf = m.energy_and_grads({"counts": x}, params)
    assert float(nnf.sum()) == 0
    for k, r in pref.items():
        np.testing.assert_allclose(parts[k].cpu().numpy(), r.numpy(), rtol=1e-5, atol=1e-5, err_msg=k)
    got = {n: g.cpu().double().numpy() for n, g in grads.items()}
    _check_grads(kind, got, {n: g.numpy() for n, g in gref.items()},
                 {n: v.numpy() for n, v in O.energy_grad_scales(cfg, x, params).items()}, note=False)


# ---- 3.7: the routes ---------------------------------------------------------------------------------------------
def test_routes_on_identical_accumulators():
    """(a) spmf_finish alone and (b) spmf_prior_async + spmf_finish run the same kernels (finish_kernel<KP, 1>,
    then the data half: inside end_kernel for (a), as finish_kernel<KP, 2> + finish_reduce_kernel for (b), both
    finish_body<KP, 2> and finish_reduce_slot): parts and gradients bit for bit.  (c) runs the prior half inside
    begin_kernel; it is held to the reference (every test above with route "c") and compared here for the record."""
    run, dev, out_a, (B, lg) = _data_case(65, 5, 3, 1_000_003, "a", seed=2)
    out_b = run.run("b", acc=dev, rows=B, lgamma=lg)
    out_c = run.run("c", acc=dev, rows=B, lgamma=lg)
    assert (out_a["parts"].view(np.int64) == out_b["parts"].view(np.int64)).all()
    for n in out_a["bits"]:
        assert (out_a["bits"][n] == out_b["bits"][n]).all(), n
    same = all((out_a["bits"][n] == out_c["bits"][n]).all() for n in out_a["bits"]) and \
        (out_a["parts"].view(np.int64) == out_c["parts"].view(np.int64)).all()
    print(f"[routes] (c) bit-equal to (a): {same}")
