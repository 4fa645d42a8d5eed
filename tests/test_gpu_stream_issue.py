"""GPU: the issue point of the stream loads in the row pass (row_pass.hip issue_next), and the column lists.

The row pass issues the loads for the next rows (entry words through a per-row buffer, row pointers and scale as
scalar loads, the dynamic tail's counter as a range-checked atomic) at one point of a row, behind its LAST gathers
(K <= 32; at the top of the row at K = 64), unconditionally on every path; z_b is still stored between the sweeps.
What can go wrong with that is a row whose last chunk / group is not where the code expects it, a lane that now
loads where it used to be masked off, and the launch shapes that deal rows out differently -- those shapes are
below.  The column pass's code is unchanged (the forms that moved its list fetch measured slower and were not
merged); the column-list cases below cover that unchanged code at the list lengths around its fetch, gather-group
and segment boundaries.  Reference: the fp64 sparse-exact port (oracle/sparse_exact.py) for 'x', 'z' and the
gradients, held to the bars of tests/test_gpu_parity.py: parts 1e-5 (rtol and atol), gradients entry by entry
through tests/_gradcheck.assert_grads_entrywise at 1e-5 of the summed absolute contributions (yardstick: the dense
oracle in row chunks, tests/_chunked_oracle.py).  The log_transform case has no sparse-exact form (the port is the
linear decoder's) and uses the dense fp64 oracle it is pinned to."""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import spmf_oracle as O
from oracle import sparse_exact as SE
from _energy_check import RTOL, assert_same_bits, check_sparse, sparse_reference
from _gradcheck import assert_grads_entrywise
from _problems import _config, _counts, _csr, build_model, cap_exponents

pytestmark = pytest.mark.gpu

ROW_LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300]


# ---- row lengths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 32, 64])
@pytest.mark.parametrize("shape", ["boundaries", "only_last_row"])
def test_row_lengths_around_the_chunks_and_empty_rows_at_both_ends(shape, K):
    """Lengths around every chunk (64) and gather-group boundary, short rows (<= 128: both chunks in registers)
    and long ones, in one matrix whose first and last rows are empty; and a matrix whose only stored row is the
    last (every wave but one runs the prologue alone)."""
    rng = np.random.default_rng(600 + K)
    lengths = ROW_LENGTHS + [0] if shape == "boundaries" else [0, 0, 0, 0, 0, 70]
    X = _csr(lengths, 512, rng)
    cfg, params = _config(X, K, 610 + K)
    check_sparse(cfg, X, params, {"counts": _counts(X, 64)}, build_model(cfg, 64), f"{shape} K={K}")


# ---- row counts and launch shapes -------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 5])
def test_fewer_rows_than_waves(B):
    """Waves with no row or one row: the prologue's loads and nothing else."""
    rng = np.random.default_rng(620 + B)
    X = _csr(rng.integers(0, 30, size=B), 40, rng)
    cfg, params = _config(X, 32, 630 + B)
    check_sparse(cfg, X, params, {"counts": _counts(X, 16)}, build_model(cfg, 16), f"B={B}")


@pytest.mark.parametrize("B,fmt", [(4096, "packed"), (4097, "packed"), (4097, "large_count"), (4097, "fractional")])
def test_the_switch_to_the_resident_set_launch_in_both_entry_formats(B, fmt):
    """B = 4096 is the first batch the 512-thread resident-set launch takes (K >= 16), 4097 leaves one wave a
    second row.  Integer counts travel as packed words; one count of 70 000 or one non-integer value selects the
    canonical col / val arrays (and pc_row / pc_val in the column pass)."""
    rng = np.random.default_rng(640 + B)
    X = _csr(rng.integers(0, 24, size=B), 96, rng)
    if fmt == "large_count":
        X.data[5] = 70000.0
    elif fmt == "fractional":
        X.data[5] = 2.5
    sc = _counts(X, 512)
    assert (sc.ent is not None and sc.pc_ent is not None) == (fmt == "packed")
    cfg, params = _config(X, 32, 650 + B)
    check_sparse(cfg, X, params, {"counts": sc}, build_model(cfg, 512), f"B={B} {fmt}")


@pytest.mark.parametrize("B,D,K,mean", [(40_000, 64, 32, 10), (140_000, 48, 8, 6)])
def test_rows_dealt_out_by_the_counters(B, D, K, mean):
    """More than 8 rows per wave -- 40 000 rows on the 4096 waves of the 512-thread launch at K = 32, 140 000 on
    the 16 384 waves of the 256-thread form at K = 8 -- so the last eighth of a wave's rows comes from the
    counters: their atomic is asked at the new issue point, on every row, and answered only where a row is due."""
    rng = np.random.default_rng(660 + K)
    X = _csr(np.minimum(rng.poisson(mean, size=B), D), D, rng)
    cfg, params = _config(X, K, 670 + K)
    check_sparse(cfg, X, params, {"counts": _counts(X, 4096)}, build_model(cfg, 4096), f"B={B} K={K}")


# ---- modes ------------------------------------------------------------------------------------------------------
def _mode_problem(K=32, B=4200, D=300, seed=680, scale_rows=True):
    rng = np.random.default_rng(seed)
    X = _csr([ROW_LENGTHS[b % len(ROW_LENGTHS)] for b in range(B)], D, rng)
    cfg, params = _config(X, K, seed + 1, scale_rows=scale_rows)
    return cfg, X, params


@pytest.mark.parametrize("scale_rows", [True, False])
def test_row_scaling_on_and_off(scale_rows):
    cfg, X, params = _mode_problem(scale_rows=scale_rows)
    check_sparse(cfg, X, params, {"counts": _counts(X, 1024)}, build_model(cfg, 1024), f"scale_rows={scale_rows}")


@pytest.mark.parametrize("B", [37, 4200])
def test_encode_alone_gives_the_oracles_z(B):
    """spmf_encode: sweep 1 alone (its issue point is behind the last sweep-1 group), the 256-thread grid and the
    resident-set launch."""
    cfg, X, params = _mode_problem(B=B)
    one = {k: np.asarray(v[0], dtype=np.float64) for k, v in params.items()}
    ref = SE.data_term(X, cfg.eta_i.numpy().reshape(-1), float(cfg.xi_u_global), True, one["u"], one["v"], one["w"],
                       one["s"])["z_rows"]
    m = build_model(cfg, 1024)
    T = torch.as_tensor
    z = m.encode(_counts(X, 1024), u=T(params["u"]), s=T(params["s"])).cpu().numpy().reshape(ref.shape)
    np.testing.assert_allclose(z, ref, rtol=RTOL, atol=RTOL * np.abs(ref).max())


def test_log_transform_launches_at_K64():
    """The exp decoder runs the row pass as sweep 1 / dense / sweep 2 launches (modes 3 and 2: z_b is gathered back,
    not recomputed).  64 x 48, K = 64, against the dense fp64 oracle."""
    rng = np.random.default_rng(690)
    x = ((rng.random((64, 48)) < 0.3) * (1 + rng.poisson(2.0, size=(64, 48)))).astype(np.float64)
    x[0, :] = 0.0
    x[63, :] = 0.0
    cfg, params = _config(x, 64, 690, log_transform=True, rng=rng)
    cap_exponents(cfg, x, params, 8.0)                                                 # largest exponent: 8
    pref, gref, _ = O.energy_and_grads(cfg, x, params)
    parts, grads, nnf = build_model(cfg, 32).energy_and_grads({"counts": x}, params)
    assert float(nnf.sum()) == 0
    for k in ("x", "z"):
        np.testing.assert_allclose(parts[k].cpu().numpy(), pref[k].numpy(), rtol=RTOL, atol=RTOL, err_msg=k)
    assert_grads_entrywise(grads, gref, O.energy_grad_scales(cfg, x, params), RTOL, "log_transform K=64")


def test_panel_range_minibatch():
    cfg, X, params = _mode_problem(B=1024, seed=700)
    sc = _counts(X, 256)
    m = build_model(cfg, 256)
    for p0, p1 in [(0, 1), (1, 4), (3, 4)]:
        check_sparse(cfg, X[p0 * 256:p1 * 256], params, {"counts": sc, "panels": (p0, p1)}, m, f"panels {p0}:{p1}")


def test_deterministic_mode_repeats_bit_for_bit():
    cfg, X, params = _mode_problem(seed=710)
    m = build_model(cfg, 1024)
    m.deterministic = True
    sc = _counts(X, 1024)
    ref = sparse_reference(cfg, X, params)
    pa, ga = check_sparse(cfg, X, params, {"counts": sc}, m, "deterministic step 1", ref)
    pb, gb = check_sparse(cfg, X, params, {"counts": sc}, m, "deterministic step 2", ref)
    assert_same_bits((pa, ga), (pb, gb))


# ---- column lists -----------------------------------------------------------------------------------------------
LIST_LENGTHS = [1, 31, 32, 33, 63, 64, 65, 600]


def _list_problem(K):
    """Two panels of 640 rows.  Panel 0 is ordinary; in panel 1 the LAST columns hold lists of the given lengths,
    the longest (600: three segments of SEGMENT_ENTRIES = 256) in the last column -- it is the last list of the
    panel-CSC arrays, so what the fetch reads behind it is the padding."""
    rng = np.random.default_rng(720 + K)
    R, D = 640, 40
    x = np.zeros((2 * R, D))
    x[:R] = (rng.random((R, D)) < 0.05) * (1 + rng.poisson(1.5, size=(R, D)))
    for j, n in enumerate(LIST_LENGTHS):
        rows = R + np.sort(rng.choice(R, size=n, replace=False))
        x[rows, D - len(LIST_LENGTHS) + j] = 1 + rng.poisson(1.5, size=n)
    X = sp.csr_matrix(x)
    cfg, params = _config(X, K, 730 + K)
    return cfg, X, params


@pytest.fixture(scope="module", params=[8, 32])
def list_case(request):
    cfg, X, params = _list_problem(request.param)
    return cfg, X, params, sparse_reference(cfg, X, params)


@pytest.mark.parametrize("fetch", ["wide", "narrow"])
def test_column_lists_around_the_fetch_and_segment_boundaries(list_case, fetch):
    """Column-pass code this change leaves as it was: lists of 1 ... 65 entries (a wide fetch holds 4 * K/4 of them, a
    gather group four) and of 600 (several work items), the longest last.  narrow: pc_pad = 0, the entry-at-a-time
    fetch of a caller without padding."""
    cfg, X, params, ref = list_case
    sc = _counts(X, 640)
    assert sc.n_panels == 2
    if fetch == "narrow":
        sc.pc_pad = 0
    check_sparse(cfg, X, params, {"counts": sc}, build_model(cfg, 640), f"lists K={cfg.latent_dim} {fetch}", ref)
