"""GPU: the row pass's dispatch of a short row's LAST chunk on its gather count (row_pass.hip sweep1_last /
sweep2_last, K <= 32).

A row of n <= 128 stored entries is one full chunk of 64 (if n > 64) and a last chunk of 1 ... 64; the kernel picks,
once per sweep, the straight-line arm for the T = ceil(last / NPI) gather instructions that carry entries (NPI = 256 / K
entries per instruction, T = 1 ... K / 4).  What can go wrong with that is an arm that gathers, folds or
back-substitutes one instruction too few or too many, a partly filled last instruction, the boundaries at 64 and 128
entries, an empty row, and the state one row's arm leaves for the next row -- so the matrix below holds EVERY row
length 0 ... 136 once, in a seeded order, between two empty rows, and every case runs it (or its lengths tiled to the
batch sizes that select the other launch shapes).  K = 64 keeps the guarded per-group code and runs the same matrix.

Reference and bars are those of tests/test_gpu_stream_issue.py: the fp64 sparse-exact port (oracle/sparse_exact.py) for
'x', 'z' and the gradients, parts at 1e-5 (rtol and atol), gradients entry by entry through
tests/_gradcheck.assert_grads_entrywise at 1e-5 of the summed absolute contributions.  The other likelihoods have no
sparse-exact form and use the dense fp64 oracle at the bars of their own test files (1e-5 on every part, gradients
entry-wise at 1e-5); the non-finite rule case uses the literal oracle and the checks of tests/test_gpu_rule_shapes.py."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _rule_cases as RC
from oracle import spmf_oracle as O
from oracle import sparse_exact as SE
from _chunked_oracle import data_term as dense_data_term, prior_scales
from _gradcheck import assert_grads_entrywise
from test_gpu_parity import build_model
from test_gpu_stream_issue import _csr, _counts

pytestmark = pytest.mark.gpu

RTOL = 1e-5
D = 512
T = torch.as_tensor


def _lengths():
    """0, then 1 ... 136 in a seeded order (neighbouring rows take different arms), then 0."""
    return [0] + [int(n) for n in np.random.default_rng(7001).permutation(np.arange(1, 137))] + [0]


@functools.lru_cache(maxsize=1)
def _matrix():
    return _csr(_lengths(), D, np.random.default_rng(7002))


def _config(X, K, seed, S=1):
    B, Dc = X.shape
    rng = np.random.default_rng(seed)
    cfg = O.OracleConfig(latent_dim=K, feature_dim=Dc, scale_rows=True, u_tau_scale=1.0 / math.sqrt(B * Dc))
    cfg.eta_i = T(rng.uniform(0.5, 3.0, size=(1, Dc)))
    cfg.xi_u_global = float(rng.uniform(2.0, 6.0))
    return cfg, O.random_params(cfg, S, seed + 1, fp32_exact=True)


def _reference(cfg, X, params, s=0, chunk=8192):
    """(sparse-exact data term, total gradients of the 12 variables, their entry-wise yardsticks) of draw s."""
    one = {k: np.asarray(v[s], dtype=np.float64) for k, v in params.items()}
    eta = cfg.eta_i.numpy().reshape(-1)
    ref = SE.data_term(X, eta, float(cfg.xi_u_global), cfg.scale_rows, one["u"], one["v"], one["w"], one["s"])
    assert ref["n_nonfinite"] == 0
    _, pg = SE.prior_term(one, cfg.u_tau_scale, cfg.s_tau_scale,
                          cfg.symmetry_breaking_decay ** np.arange(cfg.latent_dim))
    grads = {k: pg[k] + ref["grads"].get(k, 0.0) for k in pg}
    p64 = {k: np.asarray(v[s:s + 1], dtype=np.float64) for k, v in params.items()}
    dense = dense_data_term(cfg, X, p64, chunk=chunk, scales=True)
    psc = prior_scales(cfg, p64)
    scales = {k: psc[k][0] + (dense["scales"][k][0] if k in dense["scales"] else 0.0) for k in pg}
    return ref, grads, scales


def _check(cfg, X, params, batch, model, tag, chunk=8192):
    parts, grads, nnf = model.energy_and_grads(batch, params)
    assert float(nnf.sum()) == 0, tag
    S = next(iter(params.values())).shape[0]
    for s in range(S):
        data, grads_ref, scales = _reference(cfg, X, params, s, chunk)
        for k in ("x", "z"):
            got = float(parts[k][s])
            print(tag, "draw", s, k, got, data[k])
            np.testing.assert_allclose(got, data[k], rtol=RTOL, atol=RTOL, err_msg=f"{tag} draw {s} part {k}")
        assert_grads_entrywise({k: v[s] for k, v in grads.items()}, grads_ref, scales, RTOL, f"{tag} draw {s}")


def test_the_matrix_holds_every_length_once_between_two_empty_rows():
    n = np.diff(_matrix().indptr)
    assert n[0] == 0 and n[-1] == 0 and sorted(n[1:-1]) == list(range(1, 137))


@pytest.mark.parametrize("K", [4, 8, 16, 32, 64])
def test_every_row_length_at_every_k(K):
    """Every T in both chunk positions (a single chunk, and the chunk behind a full one), a partly filled last
    instruction, 64 / 65 and 128 / 129 entries, the first long rows (129 ... 136: the streamed path), empty rows.
    256-thread launch (138 rows)."""
    X = _matrix()
    cfg, params = _config(X, K, 7010 + K)
    _check(cfg, X, params, {"counts": _counts(X, 64)}, build_model(cfg, 64), f"lengths K={K}")


def _tiled(B, fmt):
    lengths = _lengths()[:-1]                                    # period 137: 0 ... 136
    X = _csr([lengths[b % len(lengths)] for b in range(B)], D, np.random.default_rng(7020))
    if fmt == "fractional":
        X.data[5] = 2.5
    return X


@pytest.mark.parametrize("fmt", ["packed", "fractional"])
@pytest.mark.parametrize("K", [32, 16])
def test_the_resident_set_launch_in_both_entry_formats(K, fmt):
    """B = 4096 + 137 rows: the 512-thread resident-set launch with phi in LDS (K >= 16, B >= 4096); integer counts
    travel as packed words, one fractional value selects the canonical col / val arrays."""
    X = _tiled(4096 + 137, fmt)
    sc = _counts(X, 1024)
    assert (sc.ent is not None) == (fmt == "packed")
    cfg, params = _config(X, K, 7030 + K)
    _check(cfg, X, params, {"counts": sc}, build_model(cfg, 1024), f"resident set K={K} {fmt}")


def test_the_1024_thread_form():
    """D = 20 481 is the first width whose phi (4 D bytes) no longer fits two workgroups' LDS per CU: one 1024-thread
    workgroup per CU.  B = 4096, rows of at most 24 entries (T = 1 ... 3 at K = 32, and empty rows)."""
    Dw = 20481
    assert 4 * (Dw - 1) <= 80 * 1024 < 4 * Dw
    rng = np.random.default_rng(7040)
    X = _csr(rng.integers(0, 25, size=4096), Dw, rng)
    cfg, params = _config(X, 32, 7041)
    _check(cfg, X, params, {"counts": _counts(X, 1024)}, build_model(cfg, 1024), "1024 threads", chunk=512)


def test_two_draws_in_one_launch():
    """S = 2 on 138 rows: both draws in one launch (gridDim.y = 2), each with its own tables, outputs and sums."""
    X = _matrix()
    cfg, params = _config(X, 32, 7050, S=2)
    _check(cfg, X, params, {"counts": _counts(X, 64)}, build_model(cfg, 64), "S=2")


# ---- the other likelihood codes of the kernel, K = 32, on the same matrix ------------------------------------------
def _likelihood_problem(kind):
    """The recipes of tests/test_gpu_logtransform.py, test_gpu_bernoulli.py and test_gpu_mixed.py on the 0 ... 136
    matrix (Bernoulli cells are its pattern)."""
    X = _matrix()
    B, K = X.shape[0], 32
    rng = np.random.default_rng({"log_transform": 7060, "bernoulli": 7061, "mixed": 7062, "bernoulli_exp": 7063}[kind])
    x = np.asarray(X.todense(), dtype=np.float64)
    mask = None
    if kind == "log_transform":
        cfg = O.OracleConfig(latent_dim=K, feature_dim=D, scale_rows=True, log_transform=True,
                             u_tau_scale=1.0 / math.sqrt(B * D))
        cfg.eta_i = T(rng.uniform(0.5, 3.0, size=(1, D)))
        cfg.xi_u_global = float(rng.uniform(4.0, 8.0))
        params = O.random_params(cfg, 1, 7070, fp32_exact=True)
        z = O.encode(cfg, T(x), T(params["u"]), T(params["s"]))
        params["v"] *= 8.0 / float((torch.matmul(z, T(params["v"])) * cfg.eta_i).max())     # largest exponent: 8
    elif kind in ("bernoulli", "bernoulli_exp"):
        x = (x > 0).astype(np.float64)
        cfg = O.OracleConfig(latent_dim=K, feature_dim=D, scale_rows=False, likelihood="bernoulli",
                             u_tau_scale=1.0 / math.sqrt(B * D))
        cfg.eta_i = T(rng.uniform(0.5, 2.0, size=(1, D)))
        params = O.random_params(cfg, 1, 7071, fp32_exact=True)
        params["v"] = params["v"] * rng.choice([-1.0, 1.0], size=params["v"].shape)
        params["w"] = -3.0 * params["w"]
        if kind == "bernoulli_exp":
            cfg.log_transform = True
            z = O.encode(cfg, T(x), T(params["u"]), T(params["s"]))
            ymax = float((torch.matmul(z, T(params["v"])) * cfg.eta_i).abs().max())
            params["v"] *= 3.0 / max(ymax, 1e-30)                                           # exponents within [-3, 3]
    else:
        mask = np.arange(D) % 2 == 1
        x[:, mask] = x[:, mask] > 0
        cfg = O.OracleConfig(latent_dim=K, feature_dim=D, scale_rows=True, likelihood="mixed",
                             u_tau_scale=1.0 / math.sqrt(B * D), extra={"bernoulli_columns": mask})
        cfg.eta_i = T(rng.uniform(0.5, 2.0, size=(1, D)))
        cfg.xi_u_global = float(rng.uniform(2.0, 6.0))
        params = O.random_params(cfg, 1, 7072, fp32_exact=True)
        sign = np.where(mask, rng.choice([-1.0, 1.0], size=D), 1.0)
        params["v"] = params["v"] * sign[None, None, :]
        params["w"] = params["w"] * np.where(mask, -3.0, 1.0)[None, None, :]
    return cfg, x, params, mask


def _likelihood_model(kind, cfg, mask):
    from spmf_amd import BernoulliFactorization, MixedFactorization
    if kind == "log_transform":
        return build_model(cfg, 64)
    if kind == "mixed":
        m = MixedFactorization(mask, latent_dim=32, u_tau_scale=cfg.u_tau_scale, scale_rows=True,
                               column_norms=cfg.eta_i, device="cuda", panel_rows=64)
        m.xi_u_global = cfg.xi_u_global
        return m
    return BernoulliFactorization(latent_dim=32, feature_dim=D, u_tau_scale=cfg.u_tau_scale, column_norms=cfg.eta_i,
                                  log_transform=kind == "bernoulli_exp", device="cuda", panel_rows=64)


@pytest.mark.parametrize("kind", ["log_transform", "bernoulli", "mixed", "bernoulli_exp"])
def test_the_other_likelihood_codes(kind):
    """Likelihood codes 1 ... 4 of the kernel, and with them its modes 1, 2 and 3 (sweep 1 alone, sweep 2 alone on the
    stored z_b, both sweeps with the dense row term subtracted later) through their three-launch flows.  Dense fp64
    oracle, 1e-5 on every part, gradients entry-wise at 1e-5: the bars of each likelihood's own test file."""
    cfg, x, params, mask = _likelihood_problem(kind)
    pref, gref, _ = O.energy_and_grads(cfg, x, params)
    parts, grads, nnf = _likelihood_model(kind, cfg, mask).energy_and_grads({"counts": x}, params)
    assert float(nnf.sum()) == 0
    for k, r in pref.items():
        np.testing.assert_allclose(parts[k].cpu().numpy(), r.numpy(), rtol=1e-5, atol=1e-5, err_msg=f"{kind} {k}")
    assert_grads_entrywise(grads, gref, O.energy_grad_scales(cfg, x, params), 1e-5, kind)


# ---- the non-finite rule with the offending cells in a partly filled last chunk ------------------------------------
# draw 1: rows of exactly 83 stored entries (a full chunk, then 19 entries = 3 of 8 gather instructions, the third
# holding 3 of 8); draw 2: rows of exactly 19.  EVERY stored cell of a planted row has rate 0, the one in the last
# occupied slot of the last chunk included.  The minimum over the finite cells is placed in draw 0 (deep cell).
RULE = RC.RuleCase("k32_last_slot_of_a_partly_filled_chunk", 300, 150, 32, 3, 7080, 0.25,
                   {1: ([3, 64, -1], list(range(20, 103))), 2: ([10, 200], list(range(110, 129)))},
                   deep=(0, 120, 140, 3), expect={"draw": 0})


def test_non_finite_cells_in_the_last_slot_of_a_partly_filled_last_chunk():
    from test_gpu_rule_and_surface import _rule_energy
    from test_gpu_rule_shapes import _check as rule_check, MIN_GAP
    c = RULE
    cfg, x, params = RC.build(c)
    for s, (rows, cols) in c.plants.items():
        n = (x[[r % c.B for r in rows]] > 0).sum(1)
        last = int(n[0]) - 64 * ((int(n[0]) - 1) // 64)
        assert (n == len(cols)).all() and 0 < -(-last // 8) < 8 and last % 8 != 0
    ll, rate, bad, (s, b, d), gap = RC.minimum_of(cfg, x, params)
    assert (bad == ((rate <= 0) & (x > 0)[None])).all() and bad.sum((1, 2)).tolist() == RC.planted_counts(c)
    assert gap >= MIN_GAP and (s, b, d) == c.deep[:3]
    ref_v = O.unormalized_log_prob_parts(cfg, x, params)
    rparts, rgrads = _rule_energy(cfg, x, params)
    rule_check(c, build_model(cfg, c.panel_rows), {"counts": x}, params, ref_v, rgrads)
