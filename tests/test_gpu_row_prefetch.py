"""GPU: the row pass's warm-up of coming rows' entry lines (row_pass.hip: issue_next, warm_issue / warm_retire,
K <= 32; row_prefetch.h).

At a row's issue point the kernel now also asks for the row pointers of the row three ahead in the wave's sequence
and, with the pair it asked for one row earlier, reads one entry word of every 64-byte half line of the row two
ahead by scalar loads; the entry loads of such rows drop their non-temporal hint.  The words read are dead, so what
can go wrong is an ADDRESS (a word outside the row: an empty row, a row of one word, the window's end at 128 of a longer row, the last row of the arrays), the extra pipeline stage at
a wave's first and last rows (waves with 1, 2, 3, 4 rows: the stage fills only from the fourth), the hand-over
between rows that have the warm-up and rows that a counter hands out (they have none), and a long row (> 128
entries) next to short ones.  Those shapes are below, in both entry formats (the canonical one carries the warm-up
at K <= 16) and at K = 64, which keeps the parent's loop.

Reference and bars are those of tests/_energy_check.py (check_sparse): the fp64 sparse-exact port
(oracle/sparse_exact.py) for 'x', 'z' and the gradients, parts at 1e-5 (rtol and atol), gradients entry by entry
through tests/_gradcheck.assert_grads_entrywise at 1e-5 of the summed absolute contributions; the encode-only call
against the port's z rows as in tests/test_gpu_stream_issue.py."""
import numpy as np
import pytest
import torch

from oracle import sparse_exact as SE
from _energy_check import assert_same_bits, check_sparse, sparse_reference
from _pass_cases import _fractional, _mixed_lengths
from _problems import _config, _counts, _csr, build_model

pytestmark = pytest.mark.gpu

RTOL = 1e-5


def test_the_lengths_cover_the_issue():
    n = np.diff(_mixed_lengths().indptr).tolist()
    assert set(n) == {0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300}
    assert n[0] == 0 and n[1] == 0 and n[-1] == 0 and n[17:20] == [0, 0, 0]
    pairs = set(zip(n, n[1:]))
    assert {(65, 129), (129, 127), (127, 300), (300, 128), (1, 129), (129, 300), (300, 0), (33, 300), (129, 64)} <= pairs


# ---- row lengths, every K, both formats ----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["packed", "canonical"])
@pytest.mark.parametrize("K", [4, 16, 32, 64])
def test_mixed_row_lengths(K, fmt):
    """33 rows, one per wave of the 256-thread form: the issue point of every length with nothing to warm."""
    X = _mixed_lengths() if fmt == "packed" else _fractional(_mixed_lengths())
    sc = _counts(X, 16)
    assert (sc.ent is not None) == (fmt == "packed")
    cfg, params = _config(X, K, 9010 + K)
    check_sparse(cfg, X, params, {"counts": sc}, build_model(cfg, 16), f"lengths K={K} {fmt}")


@pytest.mark.parametrize("K,fmt", [(32, "packed"), (16, "canonical"), (16, "packed")])
def test_mixed_row_lengths_several_rows_per_wave(K, fmt):
    """6 x 4096 + 33 rows on the 4096 waves of the resident-set launch: six or seven rows per wave (under eight: no
    dynamic tail), so a wave's fourth row onward is warmed, and the waves' stride of 4096 rows is 4 modulo the 33
    lengths -- a wave's consecutive rows run through different ones, the long ones and the empty ones included, as
    the row that warms, the row that is warmed and the row whose pointers are asked for."""
    B = 6 * 4096 + 33
    X = _mixed_lengths(B) if fmt == "packed" else _fractional(_mixed_lengths(B))
    sc = _counts(X, 4096)
    assert (sc.ent is not None) == (fmt == "packed")
    cfg, params = _config(X, K, 9020 + K)
    check_sparse(cfg, X, params, {"counts": sc}, build_model(cfg, 4096), f"tiled lengths K={K} {fmt}")


# ---- pipeline fill and drain ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 3])
def test_fewer_rows_than_a_workgroup_has_waves(B):
    rng = np.random.default_rng(9030 + B)
    X = _csr(rng.integers(1, 40, size=B), 64, rng)
    cfg, params = _config(X, 32, 9035 + B)
    check_sparse(cfg, X, params, {"counts": _counts(X, 16)}, build_model(cfg, 16), f"B={B}")


@pytest.mark.parametrize("B,rows", [(16384, (1, 1)), (16384 + 8192, (1, 2)), (2 * 16384 + 8192, (2, 3)),
                                    (3 * 16384 + 8192, (3, 4))])
def test_the_256_thread_form_with_one_to_four_rows_per_wave(B, rows):
    """K = 8 stays on the 256-thread form, whose grid stops at 4096 workgroups = 16 384 waves: B rows give a wave
    B // 16384 or one more.  A wave's fourth row is the first whose lines are warmed; with one, two or three rows the
    extra stage only fills and drains."""
    assert (B // 16384, -(-B // 16384)) == rows
    rng = np.random.default_rng(9040 + B % 97)
    X = _csr(np.minimum(rng.poisson(5, size=B), 40), 40, rng)
    cfg, params = _config(X, 8, 9045)
    check_sparse(cfg, X, params, {"counts": _counts(X, 4096)}, build_model(cfg, 4096), f"256-thread form B={B}")


def test_the_smallest_resident_set_launch():
    """B = 4096: the LDS form, one row per wave, no dynamic tail."""
    rng = np.random.default_rng(9050)
    X = _csr(rng.integers(0, 40, size=4096), 96, rng)
    cfg, params = _config(X, 32, 9051)
    check_sparse(cfg, X, params, {"counts": _counts(X, 1024)}, build_model(cfg, 1024), "B=4096")


def test_rows_with_the_warm_up_meet_rows_dealt_out_by_the_counters():
    """B = 40 000, D = 256, about ten entries per row, K = 32: nine rows per wave of the LDS form, of which the last
    come from the counters -- no number, so no pointers, that early: the pair stays (0, 0) and nothing is read."""
    rng = np.random.default_rng(9060)
    X = _csr(np.minimum(rng.poisson(10, size=40_000), 256), 256, rng)
    cfg, params = _config(X, 32, 9061)
    check_sparse(cfg, X, params, {"counts": _counts(X, 4096)}, build_model(cfg, 4096), "dynamic tail")


# ---- draws, modes ---------------------------------------------------------------------------------------------------
def test_two_draws_in_one_launch():
    """S = 2 on 3 x 4096 + 33 rows: gridDim.y = 2, each draw with its own tables; the entry arrays are shared."""
    B = 3 * 4096 + 33
    X = _mixed_lengths(B)
    cfg, params = _config(X, 32, 9070, S=2)
    check_sparse(cfg, X, params, {"counts": _counts(X, 4096)}, build_model(cfg, 4096), "S=2")


@pytest.mark.parametrize("B", [33, 5 * 4096 + 33])
def test_encode_alone_gives_the_oracles_z(B):
    """The encode-only call: its issue point, warm-up included, stands behind the last sweep-1 group.  The 256-thread
    grid and the resident-set launch (five or six rows per wave)."""
    X = _mixed_lengths(B)
    cfg, params = _config(X, 32, 9080)
    one = {k: np.asarray(v[0], dtype=np.float64) for k, v in params.items()}
    ref = SE.data_term(X, cfg.eta_i.numpy().reshape(-1), float(cfg.xi_u_global), True, one["u"], one["v"], one["w"],
                       one["s"])["z_rows"]
    m = build_model(cfg, 4096)
    T = torch.as_tensor
    z = m.encode(_counts(X, 4096), u=T(params["u"]), s=T(params["s"])).cpu().numpy().reshape(ref.shape)
    np.testing.assert_allclose(z, ref, rtol=RTOL, atol=RTOL * np.abs(ref).max())


def test_deterministic_mode_repeats_bit_for_bit():
    """Five or six rows per wave of the LDS form, all dealt out with the fixed stride (the mode has no dynamic tail)."""
    B = 5 * 4096 + 33
    X = _mixed_lengths(B)
    cfg, params = _config(X, 32, 9090)
    m = build_model(cfg, 4096)
    m.deterministic = True
    sc = _counts(X, 4096)
    steps = []
    for i in (1, 2):
        parts, grads, nnf = m.energy_and_grads({"counts": sc}, params)
        assert float(nnf.sum()) == 0
        steps.append(({k: v.clone() for k, v in parts.items()}, {k: v.clone() for k, v in grads.items()}))
    data, grads_ref, scales = sparse_reference(cfg, X, params)
    from _gradcheck import assert_grads_entrywise
    for k in ("x", "z"):
        np.testing.assert_allclose(float(steps[0][0][k][0]), data[k], rtol=RTOL, atol=RTOL, err_msg=k)
    assert_grads_entrywise({k: v[0] for k, v in steps[0][1].items()}, grads_ref, scales, RTOL, "deterministic")
    assert_same_bits(steps[0], steps[1])
