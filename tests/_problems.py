"""Inputs and models of the GPU tests: every seeded problem recipe once, and the constructors that turn an oracle
configuration into a model on the device.  Needs numpy, scipy, torch and the oracle at import; spmf_amd is imported
inside the model builders.  A recipe's RNG call order is part of it: the tests' inputs depend on it bit for bit."""
import math

import numpy as np
import scipy.sparse as sp
import torch

from oracle import spmf_oracle as O

T = torch.as_tensor


# ---- Poisson / linear ------------------------------------------------------------------------------------------
def make_problem(B, D, K, S, seed, density, scale_rows=True, empty=True, xmax=2.0):
    rng = np.random.default_rng(seed)
    mask = rng.random((B, D)) < density
    x = (mask * (1 + rng.poisson(xmax, size=(B, D)))).astype(np.float64)
    if empty and B > 4 and D > 4:
        x[1, :] = 0.0
        x[:, 2] = 0.0
        x[B - 1, :] = 0.0
    cfg = O.OracleConfig(latent_dim=K, feature_dim=D, scale_rows=scale_rows,
                         u_tau_scale=1.0 / math.sqrt(B * D))
    cfg.eta_i = torch.as_tensor(rng.uniform(0.5, 3.0, size=(1, D)))
    cfg.xi_u_global = float(rng.uniform(2.0, 6.0))
    params = O.random_params(cfg, S, seed + 1, fp32_exact=True)
    return cfg, x, params


def _csr(lengths, D, rng):
    """Rows of the given numbers of stored entries (integer counts 1 + Poisson(1.5)), columns drawn without
    replacement."""
    lengths = np.asarray(lengths, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    idx = [np.sort(rng.choice(D, size=int(n), replace=False)) for n in lengths]
    indices = np.concatenate(idx) if len(idx) else np.zeros(0, dtype=np.int64)
    data = (1 + rng.poisson(1.5, size=int(indptr[-1]))).astype(np.float64)
    return sp.csr_matrix((data, indices, indptr), shape=(len(lengths), D))


def _counts(X, panel_rows):
    from spmf_amd import SparseCounts
    return SparseCounts.from_any(X, "cuda", panel_rows)


def _config(X, K, seed, S=1, scale_rows=True, log_transform=False, xi=(2.0, 6.0), rng=None, params_seed=None):
    """Configuration and fp32-exact parameters for a given batch (dense or CSR).  ``rng``: the generator of ``seed``
    after the caller's own draws of X, where X and the configuration come from one stream; ``params_seed``: where
    the parameters' seed is not seed + 1."""
    B, D = X.shape
    rng = np.random.default_rng(seed) if rng is None else rng
    cfg = O.OracleConfig(latent_dim=K, feature_dim=D, scale_rows=scale_rows, log_transform=log_transform,
                         u_tau_scale=1.0 / math.sqrt(B * D))
    cfg.eta_i = T(rng.uniform(0.5, 3.0, size=(1, D)))
    cfg.xi_u_global = float(rng.uniform(*xi))
    return cfg, O.random_params(cfg, S, seed + 1 if params_seed is None else params_seed, fp32_exact=True)


# ---- the other likelihoods -------------------------------------------------------------------------------------
# Each recipe takes ``x``: a dense batch, or (B, D, density) to draw one from the recipe's own stream first.
def cap_exponents(cfg, x, params, top, both_signs=False):
    """Rescale v in place so that the largest exponent <z, eta v> of a log_transform decoder is ``top`` (both_signs:
    the largest magnitude, for logits of either sign)."""
    y = torch.matmul(O.encode(cfg, T(x), T(params["u"]), T(params["s"])), T(params["v"])) * cfg.eta_i
    params["v"] *= top / (max(float(y.abs().max()), 1e-30) if both_signs else float(y.max()))


def _drawn(x, rng, counts):
    """(x, drawn): the given batch, or one of (B, D, density) = x: a pattern, times 1 + Poisson(2) for counts."""
    if not isinstance(x, tuple):
        return x, False
    B, D, density = x
    x = rng.random((B, D)) < density
    if counts:
        x = x * (1 + rng.poisson(2.0, size=(B, D)))
    return x.astype(np.float64), True


def _plant_empty(x):
    if x.shape[0] > 4 and x.shape[1] > 4:
        x[1, :] = 0
        x[:, 2] = 0


def poisson_log_problem(x, K, S, seed, scale_rows=True, xi=(4.0, 8.0), params_seed=None):
    """Poisson + log_transform (poisson.py:41-42,52-53); v rescaled so that the largest exponent is 8.  A drawn
    batch gets an empty row and an empty column."""
    rng = np.random.default_rng(seed)
    x, drawn = _drawn(x, rng, counts=True)
    if drawn:
        _plant_empty(x)
    cfg, params = _config(x, K, seed, S, scale_rows, True, xi, rng, params_seed)
    cap_exponents(cfg, x, params, 8.0)
    return cfg, x, params


def bernoulli_problem(x, K, S, seed, log_transform=False, params_seed=None):
    """Bernoulli (bernoulli.py), logits of both signs: v with random signs (Identity bijector), w *= -3.
    log_transform (bernoulli.py:49-50,60-61): g(x) = log(x/eta + 1), logit = exp(<z, eta v>) - 1 + phi, exponents
    within [-3, 3].  A drawn batch gets an empty row and an empty column."""
    rng = np.random.default_rng(seed)
    x, drawn = _drawn(x, rng, counts=False)
    if drawn:
        _plant_empty(x)
    B, D = x.shape
    cfg = O.OracleConfig(latent_dim=K, feature_dim=D, scale_rows=False, likelihood="bernoulli",
                         u_tau_scale=1.0 / math.sqrt(B * D))
    cfg.eta_i = T(rng.uniform(0.5, 2.0, size=(1, D)))
    params = O.random_params(cfg, S, seed + 1 if params_seed is None else params_seed, fp32_exact=True)
    params["v"] = params["v"] * rng.choice([-1.0, 1.0], size=params["v"].shape)
    params["w"] = -3.0 * params["w"]
    if log_transform:
        cfg.log_transform = True
        cap_exponents(cfg, x, params, 3.0, both_signs=True)
    return cfg, x, params


def mixed_problem(x, K, S, seed, scale_rows=True, params_seed=None):
    """The build-defined mixed likelihood, every other column Bernoulli (as config 5): those columns of ``x`` become
    its pattern (a given x: in place), their v gets random signs and their w *= -3.  -> cfg, x, params, mask."""
    rng = np.random.default_rng(seed)
    x, _ = _drawn(x, rng, counts=True)
    B, D = x.shape
    mask = np.arange(D) % 2 == 1
    x[:, mask] = x[:, mask] > 0
    cfg = O.OracleConfig(latent_dim=K, feature_dim=D, scale_rows=scale_rows, likelihood="mixed",
                         u_tau_scale=1.0 / math.sqrt(B * D), extra={"bernoulli_columns": mask})
    cfg.eta_i = T(rng.uniform(0.5, 2.0, size=(1, D)))
    cfg.xi_u_global = float(rng.uniform(2.0, 6.0))
    params = O.random_params(cfg, S, seed + 1 if params_seed is None else params_seed, fp32_exact=True)
    sign = np.where(mask, rng.choice([-1.0, 1.0], size=D), 1.0)
    params["v"] = params["v"] * sign[None, None, :]
    params["w"] = params["w"] * np.where(mask, -3.0, 1.0)[None, None, :]
    return cfg, x, params, mask


# ---- the per-cell (dense) problems of all five likelihood codes -------------------------------------------------
LIKELIHOODS = ("poisson", "poisson_log", "bernoulli", "bernoulli_log", "mixed")


def _dense_problem(lik, B, D, K, S, seed, density=0.3, xmax=2.0, x=None):
    """One batch, its oracle configuration and fp32-exact parameters for a likelihood code of
    dense_ll.hip: 0 Poisson/linear, 1 Poisson + log_transform, 2 Bernoulli, 4 Bernoulli +
    log_transform, 3 mixed (every third column Bernoulli, so both 64-column blocks of a
    D > 64 batch hold some).  With log_transform v is scaled so that the largest exponent is 8."""
    rng = np.random.default_rng(seed)
    if x is None:
        x = ((rng.random((B, D)) < density) * (1 + rng.poisson(xmax, size=(B, D)))).astype(np.float64)
    logt = lik.endswith("_log")
    mask = None
    if lik.startswith("bernoulli"):
        x = (x > 0).astype(np.float64)
        cfg = O.OracleConfig(latent_dim=K, feature_dim=D, likelihood="bernoulli", scale_rows=False,
                             log_transform=logt)
    elif lik == "mixed":
        mask = np.arange(D) % 3 == 1
        x[:, mask] = x[:, mask] > 0
        cfg = O.OracleConfig(latent_dim=K, feature_dim=D, likelihood="mixed",
                             extra={"bernoulli_columns": mask})
    else:
        cfg = O.OracleConfig(latent_dim=K, feature_dim=D, log_transform=logt,
                             u_tau_scale=1.0 / math.sqrt(B * D))
    cfg.eta_i = T(rng.uniform(0.5, 3.0, size=(1, D)))
    cfg.xi_u_global = float(rng.uniform(2.0, 6.0))
    params = O.random_params(cfg, S, seed + 1, fp32_exact=True)
    if mask is not None or lik.startswith("bernoulli"):
        # logits of both signs; the Poisson columns of a mixed model keep their positive intercept
        cols = mask if mask is not None else np.ones(D, dtype=bool)
        params["w"][..., cols] -= 1.0
    if logt:
        z = O.encode(cfg, T(x), T(params["u"]), T(params["s"]))
        top = float((torch.matmul(z, T(params["v"])) * cfg.eta_i).max())
        if top > 0:
            params["v"] = params["v"] * (7.99 / top)
    for k in ("v", "w"):
        params[k] = params[k].astype(np.float32).astype(np.float64)
    return cfg, x, params, mask


def _dense_model(lik, cfg, mask, panel_rows):
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    K, D = cfg.latent_dim, cfg.feature_dim
    if lik.startswith("bernoulli"):
        m = BernoulliFactorization(latent_dim=K, feature_dim=D, log_transform=cfg.log_transform,
                                   column_norms=cfg.eta_i, device="cuda", panel_rows=panel_rows)
    elif lik == "mixed":
        m = MixedFactorization(mask, latent_dim=K, column_norms=cfg.eta_i, initialize_distributions=False,
                               device="cuda", panel_rows=panel_rows)
    else:
        m = PoissonFactorization(latent_dim=K, feature_dim=D, u_tau_scale=cfg.u_tau_scale,
                                 log_transform=cfg.log_transform, column_norms=cfg.eta_i,
                                 initialize_distributions=False, device="cuda", panel_rows=panel_rows)
    m.xi_u_global = cfg.xi_u_global
    return m


# ---- the non-finite rule ----------------------------------------------------------------------------------------
def _bad_cell_problem(logt=False):
    cfg, x, params = make_problem(24, 15, 2, 2, 3, 0.3, empty=False)
    cfg.log_transform = logt
    if logt:
        params["v"] *= 0.3
    params["w"][0, 0, 0] = 0.0          # phi = 0 for draw 0, column 0
    params["u"][0, 0, :] = 0.0          # column 0 feeds nothing into z
    x[:, 0] = 0
    x[0, :] = 0
    x[0, 0] = 3.0                       # row 0: only column 0 -> z_0 = 0 -> rate 0 under x = 3
    x[5, 0] = 2.0                       # a second stored cell in column 0 (finite: z_5 > 0)
    return cfg, x, params


def _rule_energy(cfg, x, params):
    """The energy of poisson.py:582-621 with the replacement rule written so that
    autograd carries what the rule MEANS: finite cells pass through clip with
    gradient one, replaced cells are worth min_val = (min over finite cells) - 10,
    whose derivative is that of the minimum's cell.  (Differentiating the
    reference's own graph literally -- TF or torch alike -- multiplies the zero
    cotangent of the unselected where() branch by d log(r)/dr = inf at a rate-0
    cell and yields NaN; see test_literal_autograd_through_the_rule_is_nan.)"""
    p = {k: T(np.asarray(v, dtype=np.float64)).clone().requires_grad_(True) for k, v in params.items()}
    xt = T(np.asarray(x, dtype=np.float64))
    parts = O.prior_log_prob_parts(cfg, p)
    theta = O.encode(cfg, xt, p["u"], p["s"])
    rate = O.decoder_function(cfg, torch.matmul(theta, p["v"])) + O.intercept_matrix(cfg, p["w"], p["s"])
    bad = (xt > 0) & ~(rate > 0)
    safe = torch.where(bad, torch.ones_like(rate), rate)
    ll = O.poisson_log_prob(xt, safe)
    good = ~bad
    mval = torch.minimum(ll[good.expand_as(ll)].min(), torch.zeros((), dtype=ll.dtype)) - 10.0
    parts["x"] = torch.where(good, ll, torch.zeros_like(ll)).sum((-1, -2)) + bad.sum((-1, -2)) * mval
    parts["z"] = (O.HALF_LOG_2_OVER_PI - 0.5 * theta ** 2).sum((-1, -2))
    tot = sum(v.sum() for v in parts.values())
    g = torch.autograd.grad(tot, [p[k] for k in O.VAR_ORDER])
    return ({k: v.detach() for k, v in parts.items()},
            {k: gk.numpy() for k, gk in zip(O.VAR_ORDER, g)})


# ---- models -----------------------------------------------------------------------------------------------------
def build_model(cfg, panel_rows=64):
    from spmf_amd import PoissonFactorization
    m = PoissonFactorization(
        latent_dim=cfg.latent_dim, feature_dim=cfg.feature_dim,
        u_tau_scale=cfg.u_tau_scale, s_tau_scale=cfg.s_tau_scale,
        symmetry_breaking_decay=cfg.symmetry_breaking_decay,
        scale_rows=cfg.scale_rows, log_transform=cfg.log_transform, column_norms=cfg.eta_i,
        initialize_distributions=False, device="cuda", panel_rows=panel_rows)
    m.xi_u_global = cfg.xi_u_global
    return m


def likelihood_model(cfg, panel_rows=64):
    """The model of a recipe's configuration, by its likelihood: build_model for Poisson, the Bernoulli and mixed
    classes with their surrogate (they are built as a user builds them)."""
    from spmf_amd import BernoulliFactorization, MixedFactorization
    K, D = cfg.latent_dim, cfg.feature_dim
    if cfg.likelihood == "bernoulli":
        return BernoulliFactorization(latent_dim=K, feature_dim=D, u_tau_scale=cfg.u_tau_scale,
                                      column_norms=cfg.eta_i, log_transform=cfg.log_transform, device="cuda",
                                      panel_rows=panel_rows)
    if cfg.likelihood == "mixed":
        m = MixedFactorization(cfg.extra["bernoulli_columns"], latent_dim=K, u_tau_scale=cfg.u_tau_scale,
                               scale_rows=cfg.scale_rows, column_norms=cfg.eta_i, device="cuda",
                               panel_rows=panel_rows)
        m.xi_u_global = cfg.xi_u_global
        return m
    return build_model(cfg, panel_rows)
