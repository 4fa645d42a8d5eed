"""GPU: the column pass's list fetch (col_pass.hip): eight packed words per lane at K <= 32, no second fetch
for a wave of short lists.

A lane group fetches FE = EPL * KP/4 entries of its list at a time -- EPL = 8 words per lane for the packed lists
at KP <= 32 (FE = 8, 16, 32, 64 at KP = 4, 8, 16, 32), four at KP = 64 (FE = 64), for the canonical arrays and
for a caller whose padding is too short for eight -- and the loop fetches again only while some group of the
wave has entries left.  What can go wrong with that: a list whose length sits on a fetch, gather-group or segment
boundary, a lane that now loads where it used to be masked off (the last list of the shard: the padding), a wave
whose groups disagree about being done, lane groups without an item, and the launch shapes that deal items out
differently.  Reference: the fp64 sparse-exact port (oracle/sparse_exact.py) through the helpers of
tests/test_gpu_stream_issue.py for the Poisson / linear cases -- parts 1e-5, gradients entry by entry through
tests/_gradcheck.assert_grads_entrywise at 1e-5 of the summed absolute contributions -- and the dense fp64
oracle with the same two bars for S = 2 and for the likelihoods the port does not cover."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import spmf_oracle as O
from _gradcheck import assert_grads_entrywise
from test_gpu_parity import build_model
from test_gpu_stream_issue import _check, _config, _counts, _reference

pytestmark = pytest.mark.gpu

RTOL = 1e-5
R, D = 320, 24                                        # rows of a panel, columns of the list problems


def _fe(K):
    """Entries per fetch and lane group of the packed lists at latent dimension K."""
    kp = 4 * -(-K // 4)
    return (8 if kp <= 32 else 4) * (kp // 4)


def _lengths(K):
    fe = _fe(K)
    return sorted({0, 1, fe - 1, fe, fe + 1, 2 * fe - 1, 2 * fe, 2 * fe + 1, 255, 256, 257})


def _list_matrix(K, seed):
    """Two panels of R rows.  Panel 0 is ordinary; panel 1 holds nothing but the lists of _lengths(K) in the LAST
    columns, ascending: the list of 257 entries (two segments of SEGMENT_ENTRIES = 256: 256 + 1) is the last list
    of the panel-CSC arrays, so its fetches run into the padding.  Panel 1 has 10 non-empty lists = 11 work items:
    no multiple of the 64, 32, 16, 8 or 4 items of a wave, so its last wave has lane groups without an item."""
    rng = np.random.default_rng(seed)
    x = np.zeros((2 * R, D))
    x[:R] = (rng.random((R, D)) < 0.05) * (1 + rng.poisson(1.5, size=(R, D)))
    L = _lengths(K)
    for j, n in enumerate(L):
        rows = R + np.sort(rng.choice(R, size=n, replace=False))
        x[rows, D - len(L) + j] = 1 + rng.poisson(1.5, size=n)
    return x


@functools.lru_cache(maxsize=None)
def _list_case(K):
    X = sp.csr_matrix(_list_matrix(K, 800 + K))
    cfg, params = _config(X, K, 810 + K)
    return cfg, X, params, _reference(cfg, X, params)


def _whole_lists(sc):
    """The work items of a production shape: a batch as small as these is cut into segments of 16 entries, so
    that it offers a few thousand items; the shapes the pass is built for (C3: 1M x 20k) reach SEGMENT_ENTRIES =
    256, where a list of up to 256 entries is ONE item and runs the fetch loop over its whole length.  Cut this
    batch's lists the same way."""
    from spmf_amd.sparse import SEGMENT_ENTRIES
    ptr = sc.pc_ptr.view(sc.n_panels, sc.n_cols + 1).to(torch.int64)
    sc._build_items((ptr[:, 1:] - ptr[:, :-1]).reshape(-1), ptr[:, :-1].reshape(-1), seg=SEGMENT_ENTRIES)
    sc.__dict__.pop("_hp", None)
    assert not sc._struct_cache
    return sc


def _packed(X, panel_rows=R):
    sc = _whole_lists(_counts(X, panel_rows))
    assert sc.pc_ent is not None and sc.pc_pad >= 7
    return sc


# ---- the packed path, Poisson / linear -----------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 4, 8, 16, 32, 64])
def test_packed_lists_around_the_fetch_and_segment_boundaries(K):
    """Lists of 0, 1, FE - 1 ... 2 FE + 1 and 255, 256, 257 entries in one panel, the longest last in the shard;
    two panels (the flat block -> panel mapping); a last wave with idle lane groups."""
    cfg, X, params, ref = _list_case(K)
    sc = _packed(X)
    ip = sc.item_ptr.cpu().numpy()
    ng = 64 // (4 * -(-K // 4) // 4)
    assert sc.n_panels == 2 and ip[2] - ip[1] == 11 and (ip[2] - ip[1]) % ng != 0
    lens = sc.items.cpu().numpy()[ip[1]:ip[2], 1]
    assert sorted(lens) == sorted([n for n in _lengths(K) if 0 < n <= 256] + [256, 1])
    _check(cfg, X, params, {"counts": sc}, build_model(cfg, R), f"lists K={K}", ref)


@pytest.mark.parametrize("K", [8, 32])
def test_one_long_list_among_short_ones_in_a_wave(K):
    """One panel whose items fill exactly one wave: one list of FE + 5 entries (a second fetch) and NG - 1 of at
    most FE.  The loop's exit is the wave's, not a group's: the short groups run the second step empty."""
    fe, ng = _fe(K), 64 // (K // 4)
    rng = np.random.default_rng(820 + K)
    rows = 2 * fe + 8
    x = np.zeros((rows, ng))
    for j in range(ng):
        n = fe + 5 if j == 3 else int(rng.integers(1, fe + 1))
        x[np.sort(rng.choice(rows, size=n, replace=False)), j] = 1 + rng.poisson(1.5, size=n)
    X = sp.csr_matrix(x)
    cfg, params = _config(X, K, 830 + K)
    sc = _packed(X, rows)
    assert sc.n_panels == 1 and int(sc.item_ptr[1] - sc.item_ptr[0]) == ng
    _check(cfg, X, params, {"counts": sc}, build_model(cfg, rows), f"one long list K={K}")


def test_eight_or_more_panels_with_a_ragged_last_one():
    """373 rows in panels of 40: ten panels (the residue block -> panel mapping), the last of 13 rows; K = 16, lists
    of about 34 entries on both sides of FE = 32."""
    rng = np.random.default_rng(840)
    x = (rng.random((373, 30)) < 0.85) * (1 + rng.poisson(1.5, size=(373, 30)))
    X = sp.csr_matrix(x.astype(np.float64))
    cfg, params = _config(X, 16, 841)
    sc = _packed(X, 40)
    assert sc.n_panels == 10
    _check(cfg, X, params, {"counts": sc}, build_model(cfg, 40), "ten panels")


def test_panel_range_minibatch_without_the_first_and_last_panel():
    """Four panels of 96 rows, lists of about 48 entries (FE = 64 at K = 32: some lists take a second fetch); the
    step runs panels 1 and 2."""
    rng = np.random.default_rng(850)
    x = (rng.random((4 * 96, 20)) < 0.5) * (1 + rng.poisson(1.5, size=(4 * 96, 20)))
    x[100:190, 7] = 1.0                                # (and one list past FE for certain: 90 entries in panel 1)
    X = sp.csr_matrix(x.astype(np.float64))
    cfg, params = _config(X, 32, 851)
    sc = _packed(X, 96)
    assert sc.n_panels == 4
    _check(cfg, X[96:288], params, {"counts": sc, "panels": (1, 3)}, build_model(cfg, 96), "panels 1:3")


def _dense_check(model, cfg, x, params, tag):
    pref, gref, _ = O.energy_and_grads(cfg, x, params)
    parts, grads, nnf = model.energy_and_grads({"counts": _packed(x)}, params)
    assert float(nnf.sum()) == 0, tag
    for k, r in pref.items():
        np.testing.assert_allclose(parts[k].cpu().numpy(), r.numpy(), rtol=RTOL, atol=RTOL, err_msg=f"{tag} part {k}")
    assert_grads_entrywise(grads, gref, O.energy_grad_scales(cfg, x, params), RTOL, tag)


def test_two_draws_per_launch():
    """S = 2: the draws are gridDim.y of one launch.  Dense fp64 oracle."""
    x = _list_matrix(32, 860)
    cfg, _ = _config(sp.csr_matrix(x), 32, 861)
    params = O.random_params(cfg, 2, 862, fp32_exact=True)
    _dense_check(build_model(cfg, R), cfg, x, params, "S=2")


# ---- the other likelihood codes ------------------------------------------------------------------------------
def _bernoulli(x, K, seed, log_transform=False):
    from spmf_amd import BernoulliFactorization
    rng = np.random.default_rng(seed)
    B, Dx = x.shape
    cfg = O.OracleConfig(latent_dim=K, feature_dim=Dx, scale_rows=False, likelihood="bernoulli",
                         u_tau_scale=1.0 / math.sqrt(B * Dx))
    cfg.eta_i = torch.as_tensor(rng.uniform(0.5, 2.0, size=(1, Dx)))
    params = O.random_params(cfg, 1, seed + 1, fp32_exact=True)
    params["v"] = params["v"] * rng.choice([-1.0, 1.0], size=params["v"].shape)
    params["w"] = -3.0 * params["w"]
    if log_transform:
        cfg.log_transform = True
        T = torch.as_tensor
        z = O.encode(cfg, T(x), T(params["u"]), T(params["s"]))
        ymax = float((torch.matmul(z, T(params["v"])) * cfg.eta_i).abs().max())
        params["v"] *= 3.0 / max(ymax, 1e-30)          # exponents within [-3, 3]
    m = BernoulliFactorization(latent_dim=K, feature_dim=Dx, u_tau_scale=cfg.u_tau_scale, column_norms=cfg.eta_i,
                               log_transform=log_transform, device="cuda", panel_rows=R)
    return m, cfg, params


def _mixed(x, K, seed):
    from spmf_amd import MixedFactorization
    rng = np.random.default_rng(seed)
    B, Dx = x.shape
    mask = np.arange(Dx) % 2 == 1
    x[:, mask] = x[:, mask] > 0
    cfg = O.OracleConfig(latent_dim=K, feature_dim=Dx, scale_rows=True, likelihood="mixed",
                         u_tau_scale=1.0 / math.sqrt(B * Dx), extra={"bernoulli_columns": mask})
    cfg.eta_i = torch.as_tensor(rng.uniform(0.5, 2.0, size=(1, Dx)))
    cfg.xi_u_global = float(rng.uniform(2.0, 6.0))
    params = O.random_params(cfg, 1, seed + 1, fp32_exact=True)
    params["v"] = params["v"] * np.where(mask, rng.choice([-1.0, 1.0], size=Dx), 1.0)[None, None, :]
    params["w"] = params["w"] * np.where(mask, -3.0, 1.0)[None, None, :]
    m = MixedFactorization(mask, latent_dim=K, u_tau_scale=cfg.u_tau_scale, scale_rows=True, column_norms=cfg.eta_i,
                           device="cuda", panel_rows=R)
    m.xi_u_global = cfg.xi_u_global
    return m, cfg, params


def _poisson_log_transform(x, K, seed):
    rng = np.random.default_rng(seed)
    B, Dx = x.shape
    cfg = O.OracleConfig(latent_dim=K, feature_dim=Dx, scale_rows=True, log_transform=True,
                         u_tau_scale=1.0 / math.sqrt(B * Dx))
    cfg.eta_i = torch.as_tensor(rng.uniform(0.5, 3.0, size=(1, Dx)))
    cfg.xi_u_global = float(rng.uniform(2.0, 6.0))
    params = O.random_params(cfg, 1, seed + 1, fp32_exact=True)
    T = torch.as_tensor
    z = O.encode(cfg, T(x), T(params["u"]), T(params["s"]))
    params["v"] *= 8.0 / float((torch.matmul(z, T(params["v"])) * cfg.eta_i).max())   # largest exponent: 8
    return build_model(cfg, R), cfg, params


@pytest.mark.parametrize("lik,K", [("bernoulli", 32), ("mixed", 32), ("poisson_log_transform", 16),
                                   ("bernoulli_log_transform", 8)])
def test_the_other_likelihood_codes_on_the_list_problem(lik, K):
    """Every likelihood code takes the eight-word fetch at K <= 32 (the log_transform codes fetch pc_gval at the
    same width): the list problem of the given K with the data each of them stores."""
    x = _list_matrix(K, 870 + K)
    if lik.startswith("bernoulli"):
        x = (x > 0).astype(np.float64)
        m, cfg, params = _bernoulli(x, K, 871 + K, lik.endswith("log_transform"))
    elif lik == "mixed":
        m, cfg, params = _mixed(x, K, 872 + K)
    else:
        m, cfg, params = _poisson_log_transform(x, K, 873 + K)
    _dense_check(m, cfg, x, params, f"{lik} K={K}")


# ---- the launches that keep another form ---------------------------------------------------------------------
def test_a_real_valued_batch_runs_the_canonical_form():
    """One non-integer value: no packed stream, pc_row / pc_val through the four-entry fetch."""
    cfg, X, params, _ = _list_case(32)
    X = X.copy()
    X.data[5] = 2.5
    sc = _whole_lists(_counts(X, R))
    assert sc.pc_ent is None
    _check(cfg, X, params, {"counts": sc}, build_model(cfg, R), "canonical")


@pytest.mark.parametrize("K", [2, 4])
def test_padding_short_of_eight_words_runs_the_four_word_form(K):
    """pc_pad = 6 satisfies the documented rule at KP = 4 (pc_pad >= 4 ceil(K/4) - 1 = 3) and is one short of the
    seven entries the eight-word fetch may read behind a list: the packed four-word instance runs."""
    cfg, X, params, ref = _list_case(K)
    sc = _packed(X)
    sc.pc_pad = 6
    _check(cfg, X, params, {"counts": sc}, build_model(cfg, R), f"pc_pad=6 K={K}", ref)


def test_deterministic_mode_repeats_bit_for_bit():
    cfg, X, params, ref = _list_case(32)
    m = build_model(cfg, R)
    m.deterministic = True
    sc = _packed(X)
    pa, ga = _check(cfg, X, params, {"counts": sc}, m, "deterministic step 1", ref)
    pb, gb = _check(cfg, X, params, {"counts": sc}, m, "deterministic step 2", ref)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
