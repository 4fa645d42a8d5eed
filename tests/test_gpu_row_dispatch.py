"""GPU: the row pass's dispatch of a short row's LAST chunk on its gather count (row_pass.hip sweep1_last /
sweep2_last, K <= 32).

A row of n <= 128 stored entries is one full chunk of 64 (if n > 64) and a last chunk of 1 ... 64; the kernel picks,
once per sweep, the straight-line arm for the T = ceil(last / NPI) gather instructions that carry entries (NPI = 256 / K
entries per instruction, T = 1 ... K / 4).  What can go wrong with that is an arm that gathers, folds or
back-substitutes one instruction too few or too many, a partly filled last instruction, the boundaries at 64 and 128
entries, an empty row, and the state one row's arm leaves for the next row -- so the matrix below holds EVERY row
length 0 ... 136 once, in a seeded order, between two empty rows, and every case runs it (or its lengths tiled to the
batch sizes that select the other launch shapes).  K = 64 keeps the guarded per-group code and runs the same matrix.

Reference and bars are those of tests/_energy_check.py: the fp64 sparse-exact port (oracle/sparse_exact.py) for
'x', 'z' and the gradients, parts at 1e-5 (rtol and atol), gradients entry by entry through
tests/_gradcheck.assert_grads_entrywise at 1e-5 of the summed absolute contributions.  The other likelihoods have no
sparse-exact form and use the dense fp64 oracle at the bars of their own test files (1e-5 on every part, gradients
entry-wise at 1e-5); the non-finite rule case uses the literal oracle and check_rule, the check of tests/test_gpu_rule_shapes.py."""
import functools

import numpy as np
import pytest

import _rule_cases as RC
from oracle import spmf_oracle as O
from _energy_check import MIN_GAP, check_dense_oracle, check_rule, check_sparse
from _problems import (_config, _counts, _csr, _rule_energy, bernoulli_problem, build_model, likelihood_model,
                       mixed_problem, poisson_log_problem)

pytestmark = pytest.mark.gpu

D = 512


def _lengths():
    """0, then 1 ... 136 in a seeded order (neighbouring rows take different arms), then 0."""
    return [0] + [int(n) for n in np.random.default_rng(7001).permutation(np.arange(1, 137))] + [0]


@functools.lru_cache(maxsize=1)
def _matrix():
    return _csr(_lengths(), D, np.random.default_rng(7002))


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
    check_sparse(cfg, X, params, {"counts": _counts(X, 64)}, build_model(cfg, 64), f"lengths K={K}")


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
    check_sparse(cfg, X, params, {"counts": sc}, build_model(cfg, 1024), f"resident set K={K} {fmt}")


def test_the_1024_thread_form():
    """D = 20 481 is the first width whose phi (4 D bytes) no longer fits two workgroups' LDS per CU: one 1024-thread
    workgroup per CU.  B = 4096, rows of at most 24 entries (T = 1 ... 3 at K = 32, and empty rows)."""
    Dw = 20481
    assert 4 * (Dw - 1) <= 80 * 1024 < 4 * Dw
    rng = np.random.default_rng(7040)
    X = _csr(rng.integers(0, 25, size=4096), Dw, rng)
    cfg, params = _config(X, 32, 7041)
    check_sparse(cfg, X, params, {"counts": _counts(X, 1024)}, build_model(cfg, 1024), "1024 threads", chunk=512)


def test_two_draws_in_one_launch():
    """S = 2 on 138 rows: both draws in one launch (gridDim.y = 2), each with its own tables, outputs and sums."""
    X = _matrix()
    cfg, params = _config(X, 32, 7050, S=2)
    check_sparse(cfg, X, params, {"counts": _counts(X, 64)}, build_model(cfg, 64), "S=2")


# ---- the other likelihood codes of the kernel, K = 32, on the same matrix ------------------------------------------
def _likelihood_problem(kind):
    """The recipes of tests/_problems.py on the 0 ... 136 matrix (Bernoulli cells are its pattern)."""
    x = np.asarray(_matrix().todense(), dtype=np.float64)
    if kind == "log_transform":
        return poisson_log_problem(x, 32, 1, 7060, params_seed=7070)
    if kind == "mixed":
        return mixed_problem(x, 32, 1, 7062, params_seed=7072)[:3]
    x = (x > 0).astype(np.float64)
    return bernoulli_problem(x, 32, 1, {"bernoulli": 7061, "bernoulli_exp": 7063}[kind], kind == "bernoulli_exp", 7071)


@pytest.mark.parametrize("kind", ["log_transform", "bernoulli", "mixed", "bernoulli_exp"])
def test_the_other_likelihood_codes(kind):
    """Likelihood codes 1 ... 4 of the kernel, and with them its modes 1, 2 and 3 (sweep 1 alone, sweep 2 alone on the
    stored z_b, both sweeps with the dense row term subtracted later) through their three-launch flows.  Dense fp64
    oracle, 1e-5 on every part, gradients entry-wise at 1e-5: the bars of each likelihood's own test file."""
    cfg, x, params = _likelihood_problem(kind)
    check_dense_oracle(likelihood_model(cfg, 64), cfg, x, params, tag=kind)


# ---- the non-finite rule with the offending cells in a partly filled last chunk ------------------------------------
# draw 1: rows of exactly 83 stored entries (a full chunk, then 19 entries = 3 of 8 gather instructions, the third
# holding 3 of 8); draw 2: rows of exactly 19.  EVERY stored cell of a planted row has rate 0, the one in the last
# occupied slot of the last chunk included.  The minimum over the finite cells is placed in draw 0 (deep cell).
RULE = RC.RuleCase("k32_last_slot_of_a_partly_filled_chunk", 300, 150, 32, 3, 7080, 0.25,
                   {1: ([3, 64, -1], list(range(20, 103))), 2: ([10, 200], list(range(110, 129)))},
                   deep=(0, 120, 140, 3), expect={"draw": 0})


def test_non_finite_cells_in_the_last_slot_of_a_partly_filled_last_chunk():
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
    check_rule(c, build_model(cfg, c.panel_rows), {"counts": x}, params, ref_v, rgrads)
