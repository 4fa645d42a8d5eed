"""GPU: waic_streaming(col_scores=True) (spmf_waic_accumulate_cols, csrc/waic.hip): the per-column sums of the
per-cell lppd_i / pwaic_i against the fp64 oracle's per-cell log-likelihood, reduced on the CPU along the rows.

The oracle, the shapes, the seeds and the bounds are those of tests/test_gpu_waic_streaming.py for the row scores:
lppd 1e-5 and pwaic 1e-3 relative, each plus that fraction of the largest column value; the totals 1e-5 / 1e-3 / 1e-5
(lppd / pwaic / waic).  The column sum of elpd_i^2 is held to those two bounds carried to each cell and through the
square: |d(e^2)| <= 2 |e| |de|, |de| <= 1e-5 |lppd_i| + 1e-3 |pwaic_i|, summed over the column's counted cells.
'col_se' is held to ``combine``'s formula of the column's own five sums only.

The method returns six derived keys per column; the five raw sums of a call (and the six totals) are read where the
method hands them to spmf_amd.waic.combine_columns / combine, which the helper here watches."""
import functools
import importlib.util
import math
import os
from unittest import mock

import numpy as np
import pytest
import torch

from oracle import spmf_oracle as O
from _problems import LIKELIHOODS, _dense_model, _dense_problem, build_model, make_problem
from _stream_cases import assert_shared_errors, gpu_good_call, host_ctx

pytestmark = pytest.mark.gpu
T = torch.as_tensor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL_KEYS = {"col_n", "col_n_excluded", "col_lppd", "col_pwaic", "col_waic", "col_se"}


# ---- the oracle -------------------------------------------------------------------------------------------------
def _cells(cfg, x, params):
    """Oracle: per-cell (lppd_i, pwaic_i) [B,D] fp64 and the mask of cells finite in every draw."""
    ll = O.log_likelihood_components(cfg, T(x), T(params["s"]), T(params["u"]), T(params["v"]),
                                     T(params["w"]))["log_likelihood"]
    S = ll.shape[0]
    ok = torch.isfinite(ll).all(0)
    lp = torch.logsumexp(ll, 0) - math.log(S)
    pw = ll.var(0, unbiased=True)
    return lp, pw, ok


def _reference(cfg, x, params):
    """The column sums of the oracle's cells, the bound of the elpd^2 sums, and the totals."""
    lp, pw, ok = _cells(cfg, x, params)
    zero = torch.zeros_like(lp)
    e = lp - pw

    def cols(v):
        return torch.where(ok, v, zero).sum(0).numpy()
    tol_e2 = cols(2.0 * e.abs() * (1e-5 * lp.abs() + 1e-3 * pw.abs()))
    return {"n": ok.sum(0).numpy(), "x": (~ok).sum(0).numpy(), "lppd": cols(lp), "pwaic": cols(pw),
            "e2": cols(e * e), "tol_e2": tol_e2,
            "total": {"lppd": float(lp[ok].sum()), "pwaic": float(pw[ok].sum()), "waic": float(-2.0 * e[ok].sum()),
                      "n": int(ok.sum()), "n_excluded": int((~ok).sum())}}


@functools.lru_cache(maxsize=None)
def _dense_case(lik, B, D, K, S, seed):
    """A _dense_problem and its reference, computed once and shared (read-only)."""
    cfg, x, params, mask = _dense_problem(lik, B, D, K, S, seed)
    return cfg, x, params, mask, _reference(cfg, x, params)


# ---- the call and its checks ------------------------------------------------------------------------------------
def _stream_cols(m, data, **kw):
    """waic_streaming(col_scores=True) -> (result, [D,5] column sums, [6] totals): the sums are copied where the
    method hands them to combine_columns / combine."""
    from spmf_amd import waic as W
    seen = {}
    combine, combine_columns = W.combine, getattr(W, "combine_columns", None)

    def watch_totals(s):
        seen["totals"] = s.detach().cpu().numpy().copy()
        return combine(s)

    def watch_cols(s):
        seen["cols"] = s.detach().cpu().numpy().copy()
        return combine_columns(s)
    # (create: without the feature the call below fails on its keyword, not here)
    with mock.patch.object(W, "combine", watch_totals), mock.patch.object(W, "combine_columns", watch_cols,
                                                                          create=True):
        out = m.waic_streaming(data, col_scores=True, **kw)
    assert seen["cols"].dtype == np.float64 and seen["cols"].shape == (m.feature_dim, 5)
    return out, seen["cols"], seen["totals"]


def _assert_se(out, sums, tag):
    """col_se is ``combine``'s formula of the column's own five sums: NaN where n <= 1, finite elsewhere, and equal
    up to the rounding of the formula's own cancellation, 2^-52 (sum e^2) / (sum e^2 - (sum e)^2 / n) per step."""
    from spmf_amd import waic as W
    se = out["col_se"].cpu().numpy()
    for d in range(sums.shape[0]):
        n, e, e2 = sums[d, 0], sums[d, 1] - sums[d, 2], sums[d, 3]
        want = W.combine(np.concatenate([sums[d], [0.0]]))["se"]
        if n <= 1:
            assert math.isnan(se[d]) and math.isnan(want), (tag, d)
            continue
        assert math.isfinite(se[d]) and math.isfinite(want), (tag, d, se[d], want)
        cond = e2 / max(e2 - e * e / n, 1e-300)
        assert abs(se[d] - want) <= 16.0 * 2.0 ** -52 * cond * abs(want) + 1e-300, (tag, d, se[d], want, cond)


def _assert_cols(out, sums, ref, tag):
    """The result and the raw column sums against the reference; -> the largest err / tol of the elpd^2 sums."""
    assert COL_KEYS <= set(out), tag
    D = ref["n"].shape[0]
    for k in COL_KEYS:
        assert out[k].is_cuda and tuple(out[k].shape) == (D,), (tag, k)
        assert out[k].dtype == (torch.int64 if k in ("col_n", "col_n_excluded") else torch.float64), (tag, k)
    got = {k: out[k].cpu().numpy() for k in COL_KEYS}
    np.testing.assert_array_equal(got["col_n"], ref["n"], err_msg=tag)
    np.testing.assert_array_equal(got["col_n_excluded"], ref["x"], err_msg=tag)
    np.testing.assert_array_equal(sums[:, 0], ref["n"].astype(np.float64), err_msg=tag)
    np.testing.assert_array_equal(sums[:, 4], ref["x"].astype(np.float64), err_msg=tag)
    np.testing.assert_array_equal(got["col_lppd"], sums[:, 1], err_msg=tag)
    np.testing.assert_array_equal(got["col_pwaic"], sums[:, 2], err_msg=tag)
    np.testing.assert_array_equal(got["col_waic"], -2.0 * (sums[:, 1] - sums[:, 2]), err_msg=tag)
    np.testing.assert_allclose(got["col_lppd"], ref["lppd"], rtol=1e-5, atol=1e-5 * np.abs(ref["lppd"]).max(),
                               err_msg=tag)
    np.testing.assert_allclose(got["col_pwaic"], ref["pwaic"], rtol=1e-3, atol=1e-3 * np.abs(ref["pwaic"]).max(),
                               err_msg=tag)
    err, tol = np.abs(sums[:, 3] - ref["e2"]), ref["tol_e2"]
    ratio = float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
    print(f"{tag}: largest err / tol of the column sums of elpd^2 = {ratio:.3g}")
    assert (err <= tol).all(), (tag, ratio)
    _assert_se(out, sums, tag)
    return ratio


def _assert_totals(out, ref, tag):
    """The lppd / pwaic / waic bounds of test_gpu_waic_streaming._assert_totals."""
    assert out["n"] == ref["n"] and out["n_excluded"] == ref["n_excluded"], tag
    assert math.isfinite(out["lppd"]) and math.isfinite(ref["lppd"]), tag
    assert abs(out["lppd"] - ref["lppd"]) <= 1e-5 * abs(ref["lppd"]), tag
    assert abs(out["pwaic"] - ref["pwaic"]) <= 1e-3 * max(abs(ref["pwaic"]), 1e-9) + 1e-9, tag
    assert abs(out["waic"] - ref["waic"]) <= 1e-5 * abs(ref["waic"]), tag


def _run(m, x, params, ref, tag):
    out, sums, totals = _stream_cols(m, {"counts": x}, draws=params)
    _assert_totals(out, ref["total"], tag)
    _assert_cols(out, sums, ref, tag)
    return out, sums, totals


# ---- the tests --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D,K,S", [(70, 45, 3, 2), (131, 97, 16, 7)])
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_every_likelihood_at_ragged_tiles(lik, B, D, K, S):
    """70 x 45: D < 64, so the second wave column of the block is partly beyond D, and K is padded 3 -> 4.
    131 x 97: three row blocks and two column blocks add into the same columns."""
    cfg, x, params, mask, ref = _dense_case(lik, B, D, K, S, 4100 + B + K)
    out, _, _ = _run(_dense_model(lik, cfg, mask, 32), x, params, ref, f"{lik} {B}x{D} K={K} S={S}")
    assert (out["col_n"] == B).all() and (out["col_n_excluded"] == 0).all()


def test_wide_k_runs_two_chunks_per_draw():
    cfg, x, params, mask, ref = _dense_case("poisson", 70, 45, 64, 5, 4364)
    out, _, _ = _run(_dense_model("poisson", cfg, mask, 32), x, params, ref, "K=64")
    assert (out["col_n"] == 70).all() and (out["col_n_excluded"] == 0).all()


def test_empty_column_and_a_full_row():
    """make_problem leaves column 2 empty: the dense kernel alone serves it.  Row 5 is stored in every other
    column: the fix kernel adds into 44 columns from one row at once."""
    cfg, x, params = make_problem(70, 45, 5, 4, 77, 0.25)
    x[5, :] = 1 + (np.arange(45) % 4)
    x[5, 2] = 0
    assert (x[:, 2] == 0).all() and (x[5] != 0).sum() == 44
    ref = _reference(cfg, x, params)
    out, sums, _ = _run(_dense_model("poisson", cfg, None, 32), x, params, ref, "edges")
    assert (out["col_n"] == 70).all() and (out["col_n_excluded"] == 0).all()
    assert sums[2, 0] == 70 and sums[2, 1] < 0 and sums[2, 2] > 0      # (scored, within _run's bounds)


def test_nan_count_takes_one_cell_out_of_every_column():
    cfg, x, params = make_problem(37, 23, 3, 3, 913, 0.3)
    x[6, 11] = float("nan")
    ref = _reference(cfg, x, params)
    assert (ref["x"] == 1).all() and (ref["n"] == 36).all()
    out, _, _ = _run(build_model(cfg, 16), x, params, ref, "NaN row")
    assert (out["col_n_excluded"] == 1).all() and (out["col_n"] == 36).all()
    assert ((out["col_n"] + out["col_n_excluded"]) == 37).all()


def test_rate_zero_under_a_positive_count_excludes_one_cell_of_column_0():
    cfg, x, params = make_problem(24, 15, 2, 3, 3, 0.3, empty=False)
    params["w"][0, 0, 0] = 0.0
    params["u"][0, 0, :] = 0.0
    x[:, 0] = 0
    x[0, :] = 0
    x[0, 0] = 3.0
    ref = _reference(cfg, x, params)
    assert ref["x"].tolist() == [1] + [0] * 14
    out, _, _ = _run(build_model(cfg, 8), x, params, ref, "rate 0")
    assert out["col_n_excluded"].tolist() == [1] + [0] * 14 and out["col_n"].tolist() == [23] + [24] * 14
    assert ((out["col_n"] + out["col_n_excluded"]) == 24).all()


def test_columns_sum_to_the_totals():
    """Counts exactly; the fp64 sums to the order-of-addition bound of test_row_chunks_and_several_batches_add_up."""
    cfg, x, params, mask, ref = _dense_case("poisson", 131, 97, 16, 7, 4100 + 131 + 16)
    out, sums, totals = _stream_cols(_dense_model("poisson", cfg, mask, 32), {"counts": x}, draws=params)
    assert int(out["col_n"].sum()) == out["n"] == 131 * 97 and sums[:, 0].sum() == totals[0]
    assert int(out["col_n_excluded"].sum()) == out["n_excluded"] == 0 and sums[:, 4].sum() == totals[4]
    assert abs(float(out["col_lppd"].sum()) - out["lppd"]) <= 1e-12 * abs(out["lppd"])
    assert abs(float(out["col_pwaic"].sum()) - out["pwaic"]) <= 1e-12 * abs(out["pwaic"])
    for j in (1, 2, 3):
        assert abs(sums[:, j].sum() - totals[j]) <= 1e-12 * abs(totals[j]), (j, sums[:, j].sum(), totals[j])


def test_row_chunks_and_several_batches_add_up():
    """max_rows below B, an iterable of two batches and a data factory against the same rows as one batch: the
    columns add where the row scores concatenate, and only the fp64 addition order differs."""
    cfg, x, params, mask = _dense_problem("poisson", 131, 97, 16, 4, 4700)
    m = _dense_model("poisson", cfg, mask, 32)
    one, s_one, _ = _stream_cols(m, {"counts": x}, draws=params, row_scores=True)
    parts = [{"counts": x[:64].copy()}, {"counts": x[64:].copy()}]
    forms = {"chunked": _stream_cols(m, {"counts": x}, draws=params, row_scores=True, max_rows=32),
             "two batches": _stream_cols(m, parts, draws=params, row_scores=True),
             "factory": _stream_cols(m, lambda: iter(parts), draws=params, row_scores=True)}
    assert (one["col_n"] == 131).all() and tuple(one["row_lppd"].shape) == (131,)
    for tag, (o, s, _) in forms.items():
        assert torch.equal(o["col_n"], one["col_n"]) and torch.equal(o["col_n_excluded"], one["col_n_excluded"]), tag
        np.testing.assert_array_equal(s[:, [0, 4]], s_one[:, [0, 4]], err_msg=tag)
        for j in (1, 2, 3):
            np.testing.assert_allclose(s[:, j], s_one[:, j], rtol=1e-12, atol=1e-12 * np.abs(s_one[:, j]).max(),
                                       err_msg=f"{tag} slot {j}")
        np.testing.assert_allclose(o["row_lppd"].cpu().numpy(), one["row_lppd"].cpu().numpy(), rtol=1e-12, err_msg=tag)


def test_raw_call_equals_the_method_and_keeps_the_error_contract():
    """spmf_waic_accumulate_cols through ctypes: refused calls (the draw stage's shared cases,
    _stream_cases.assert_shared_errors, then the entry's own) write nothing; with row_out and col_out set the
    method's numbers; with col_out NULL the plain entry, a poisoned [D,5] buffer untouched."""
    from spmf_amd import _lib
    B, D = 70, 45
    cfg, x, params, mask, _ = _dense_case("poisson", B, D, 3, 2, 4100 + 70 + 3)
    m = _dense_model("poisson", cfg, mask, 32)
    out, s_method, t_method = _stream_cols(m, {"counts": x}, draws=params, row_scores=True)
    lib, h = _lib.load(), m._handle()
    good, need, outs, scratch, no_u = gpu_good_call("waic_cols", m, x, params)
    sums, rows, cols = outs["sums"], outs["rows"], outs["colsum"]
    assert tuple(cols.shape) == (D, 5) and tuple(rows.shape) == (B, 2)
    raw = host_ctx(lib, 3, _lib.FLAG_MIXED)        # a mixed context nobody gave column types

    def untouched():
        torch.cuda.synchronize()
        assert all(bool((t == -7.0).all()) for t in outs.values()) and not bool(scratch.any())
    try:
        call = assert_shared_errors(lib, "waic_cols", good, need, no_u, raw, after=untouched)
    finally:
        lib.spmf_ctx_destroy(raw)
    assert call(sums=None) == -1                                # SPMF_E_ARG
    assert lib.spmf_last_error(h).decode() == "waic_accumulate_cols: null argument"
    untouched()
    assert call(S=1) == -1                                      # SPMF_E_ARG
    assert lib.spmf_last_error(h).decode().startswith("waic_accumulate_cols: S must be in 2..65535")
    untouched()
    assert call(nbytes=need - 1) == -3                          # SPMF_E_WORKSPACE
    msg = lib.spmf_last_error(h).decode()
    assert msg.startswith("waic_accumulate_cols: scratch too small") and str(need) in msg, msg
    untouched()

    def close(a, b, tag):
        a, b = a.cpu().numpy(), np.asarray(b)
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * np.abs(b).max(), err_msg=tag)
    for t in outs.values():         # the call adds into its outputs
        t.zero_()
    assert call() == 0
    torch.cuda.synchronize()
    close(sums, t_method, "sums6")
    close(cols, s_method, "col_out")
    close(rows[:, 0], out["row_lppd"].cpu().numpy(), "row lppd")
    close(rows[:, 1], out["row_pwaic"].cpu().numpy(), "row pwaic")
    np.testing.assert_array_equal(cols[:, [0, 4]].cpu().numpy(), s_method[:, [0, 4]])

    first = rows.cpu().numpy()
    poison = cols.fill_(-7.0)
    sums.zero_()
    rows.zero_()
    assert call(colsum=None) == 0
    torch.cuda.synchronize()
    close(sums, t_method, "sums6 without col_out")
    close(rows, first, "row_out without col_out")
    assert bool((poison == -7.0).all())


def test_cli_writes_the_gene_table(tmp_path, capsys):
    """bin/factorize_scrnaseq_counts.py --gene-waic on the toy matrix of tests/test_gpu_sets_cli.py: the file, and
    its values replayed from the watched model and generator state (to 1e-12: the sums are atomics)."""
    spec = importlib.util.spec_from_file_location(
        "factorize_scrnaseq_counts", os.path.join(ROOT, "bin", "factorize_scrnaseq_counts.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    rng = np.random.default_rng(4)
    N, D, P, G = 130, 30, 2, 3
    types = rng.integers(0, G, size=N)
    prog = rng.gamma(0.3, 1.0, size=(G, D)) * (rng.random((G, D)) < 0.3) * 6.0 + 0.2
    X = rng.poisson(prog[types] * rng.lognormal(0.0, 0.4, size=(N, 1))).astype(np.int64)
    np.save(tmp_path / "toy_counts.npy", X)
    seen = {}
    scoring = cli.gene_waic

    def watched(factor, data, *rest):
        seen["factor"], seen["data"] = factor, data
        seen["cpu"], seen["cuda"] = torch.get_rng_state(), torch.cuda.get_rng_state(factor.device)
        return scoring(factor, data, *rest)
    cli.gene_waic = watched
    cli.main(["--counts", str(tmp_path / "toy_counts.npy"), "-d", str(P), "-b", "64", "-e", "3", "--seed", "3",
              "--top", "4", "--gene-waic", "--waic-draws", "5"])
    printed = capsys.readouterr().out
    assert "gene waic: " in printed and "worst per cell: " in printed, printed
    table = np.load(tmp_path / f"toy_genewaic_{P}.npy")
    assert table.shape == (D, 6) and table.dtype == np.float64 and np.isfinite(table).all()
    np.testing.assert_array_equal(table[:, 0] + table[:, 1], np.full(D, float(N)))
    assert not (tmp_path / f"toy_setscore_{P}.npy").exists()
    factor = seen["factor"]
    torch.set_rng_state(seen["cpu"])
    torch.cuda.set_rng_state(seen["cuda"], factor.device)
    ref = factor.waic_streaming({factor.count_key: seen["data"]}, nsamples=5, col_scores=True)
    for j, k in enumerate(("col_n", "col_n_excluded", "col_lppd", "col_pwaic", "col_waic", "col_se")):
        want = ref[k].cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(table[:, j], want, rtol=1e-12, atol=1e-12 * np.abs(want).max(), err_msg=k)
