"""GPU: the column pass's list fetch (col_pass.hip): eight packed words per lane at K <= 32, no second fetch
for a wave of short lists.

A lane group fetches FE = EPL * KP/4 entries of its list at a time -- EPL = 8 words per lane for the packed lists
at KP <= 32 (FE = 8, 16, 32, 64 at KP = 4, 8, 16, 32), four at KP = 64 (FE = 64), for the canonical arrays and
for a caller whose padding is too short for eight -- and the loop fetches again only while some group of the
wave has entries left.  What can go wrong with that: a list whose length sits on a fetch, gather-group or segment
boundary, a lane that now loads where it used to be masked off (the last list of the shard: the padding), a wave
whose groups disagree about being done, lane groups without an item, and the launch shapes that deal items out
differently.  Reference: the fp64 sparse-exact port (oracle/sparse_exact.py) through
tests/_energy_check.py for the Poisson / linear cases -- parts 1e-5, gradients entry by entry through
tests/_gradcheck.assert_grads_entrywise at 1e-5 of the summed absolute contributions -- and the dense fp64
oracle with the same two bars for S = 2 and for the likelihoods the port does not cover."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import spmf_oracle as O
from _energy_check import assert_same_bits, check_dense_oracle, check_sparse
from _pass_cases import R, _fe, _list_case, _list_lengths, _list_matrix, _packed, _whole_lists
from _problems import (_config, _counts, bernoulli_problem, build_model, likelihood_model, mixed_problem,
                       poisson_log_problem)

pytestmark = pytest.mark.gpu


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
    assert sorted(lens) == sorted([n for n in _list_lengths(K) if 0 < n <= 256] + [256, 1])
    check_sparse(cfg, X, params, {"counts": sc}, build_model(cfg, R), f"lists K={K}", ref)


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
    check_sparse(cfg, X, params, {"counts": sc}, build_model(cfg, rows), f"one long list K={K}")


def test_eight_or_more_panels_with_a_ragged_last_one():
    """373 rows in panels of 40: ten panels (the residue block -> panel mapping), the last of 13 rows; K = 16, lists
    of about 34 entries on both sides of FE = 32."""
    rng = np.random.default_rng(840)
    x = (rng.random((373, 30)) < 0.85) * (1 + rng.poisson(1.5, size=(373, 30)))
    X = sp.csr_matrix(x.astype(np.float64))
    cfg, params = _config(X, 16, 841)
    sc = _packed(X, 40)
    assert sc.n_panels == 10
    check_sparse(cfg, X, params, {"counts": sc}, build_model(cfg, 40), "ten panels")


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
    check_sparse(cfg, X[96:288], params, {"counts": sc, "panels": (1, 3)}, build_model(cfg, 96), "panels 1:3")


def test_two_draws_per_launch():
    """S = 2: the draws are gridDim.y of one launch.  Dense fp64 oracle."""
    x = _list_matrix(32, 860)
    cfg, _ = _config(sp.csr_matrix(x), 32, 861)
    params = O.random_params(cfg, 2, 862, fp32_exact=True)
    check_dense_oracle(build_model(cfg, R), cfg, x, params, batch={"counts": _packed(x)}, tag="S=2")


# ---- the other likelihood codes ------------------------------------------------------------------------------
@pytest.mark.parametrize("lik,K", [("bernoulli", 32), ("mixed", 32), ("poisson_log_transform", 16),
                                   ("bernoulli_log_transform", 8)])
def test_the_other_likelihood_codes_on_the_list_problem(lik, K):
    """Every likelihood code takes the eight-word fetch at K <= 32 (the log_transform codes fetch pc_gval at the
    same width): the list problem of the given K with the data each of them stores."""
    x = _list_matrix(K, 870 + K)
    if lik.startswith("bernoulli"):
        x = (x > 0).astype(np.float64)
        cfg, x, params = bernoulli_problem(x, K, 1, 871 + K, lik.endswith("log_transform"))
    elif lik == "mixed":
        cfg, x, params, _ = mixed_problem(x, K, 1, 872 + K)
    else:
        cfg, x, params = poisson_log_problem(x, K, 1, 873 + K, xi=(2.0, 6.0))
    check_dense_oracle(likelihood_model(cfg, R), cfg, x, params, batch={"counts": _packed(x)}, tag=f"{lik} K={K}")


# ---- the launches that keep another form ---------------------------------------------------------------------
def test_a_real_valued_batch_runs_the_canonical_form():
    """One non-integer value: no packed stream, pc_row / pc_val through the four-entry fetch."""
    cfg, X, params, _ = _list_case(32)
    X = X.copy()
    X.data[5] = 2.5
    sc = _whole_lists(_counts(X, R))
    assert sc.pc_ent is None
    check_sparse(cfg, X, params, {"counts": sc}, build_model(cfg, R), "canonical")


@pytest.mark.parametrize("K", [2, 4])
def test_padding_short_of_eight_words_runs_the_four_word_form(K):
    """pc_pad = 6 satisfies the documented rule at KP = 4 (pc_pad >= 4 ceil(K/4) - 1 = 3) and is one short of the
    seven entries the eight-word fetch may read behind a list: the packed four-word instance runs."""
    cfg, X, params, ref = _list_case(K)
    sc = _packed(X)
    sc.pc_pad = 6
    check_sparse(cfg, X, params, {"counts": sc}, build_model(cfg, R), f"pc_pad=6 K={K}", ref)


def test_deterministic_mode_repeats_bit_for_bit():
    cfg, X, params, ref = _list_case(32)
    m = build_model(cfg, R)
    m.deterministic = True
    sc = _packed(X)
    pa, ga = check_sparse(cfg, X, params, {"counts": sc}, m, "deterministic step 1", ref)
    pb, gb = check_sparse(cfg, X, params, {"counts": sc}, m, "deterministic step 2", ref)
    assert_same_bits((pa, ga), (pb, gb))
