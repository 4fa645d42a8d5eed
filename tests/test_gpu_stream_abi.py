"""GPU: the C-ABI error contract the draw-stage entry points share (the table of tests/_stream_cases.py:
spmf_waic_accumulate, spmf_topk_rows, spmf_score_cells, spmf_rank_cells, spmf_predict_columns, spmf_group_sums,
spmf_embed_rows, spmf_waic_accumulate_cols, spmf_toprows_columns, spmf_set_scores: include/spmf_hip.h), through
ctypes at B = 70, D = 45, K = 3, S = 2, Poisson, panel_rows = 32: a ragged 64-row block, K padded 3 -> 4, two
draws so that sd and the WAIC variance are defined.  Every error returns before a launch:
outputs and scratch keep their sentinels.  Then the valid call returns what the Python method returns: the same
bits for every entry but the WAIC sums, which go through fp64 atomics and are held to the tolerances of
test_gpu_waic_streaming.py (lppd and waic 1e-5 relative, pwaic 1e-3, row scores the same with an atol of that
fraction of the largest row value).  The entry-specific cases (k, flags, the lists' own arguments) stay with
each entry's own test file."""
import numpy as np
import pytest
import torch

from _stream_cases import (B, D, K, S, ENTRIES, PANEL_COLS, PANEL_SETS, PANEL_WEIGHTS, _problem,
                           assert_shared_errors, gpu_good_call)
from _problems import _dense_model

pytestmark = pytest.mark.gpu
ACCUMULATED = ("waic", "groups", "waic_cols")          # entries that add into their outputs


def _bits(t):
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.dtype.is_floating_point else t


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_shared_errors_launch_nothing_and_the_valid_call_is_the_methods(entry):
    from spmf_amd import _lib
    from spmf_amd import waic as _waic
    cfg, x, params, mask, _ = _problem("poisson", B, D, K, S)
    m = _dense_model("poisson", cfg, mask, 32)
    lib = _lib.load()
    good, need, out, scratch, no_u = gpu_good_call(entry, m, x, params)
    raw = _dense_model("mixed", cfg, np.arange(D) % 3 == 1, 32)._new_ctx()   # a mixed context nobody gave column types

    def untouched():
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in out.values()) and not bool(scratch.any())
    try:
        call = assert_shared_errors(lib, entry, good, need, no_u, raw)
    finally:
        lib.spmf_ctx_destroy(raw)
    untouched()
    if entry in ACCUMULATED:
        for t in out.values():
            t.zero_()
    assert call() == 0
    torch.cuda.synchronize()
    batch, lists = {"counts": x}, good["keep"][-1]
    if entry == "topk":
        want = m.top_k(batch, k=good["k"], draws=params)
        assert _same(out["cols"], want["columns"]) and _same(out["scores"], want["scores"])
    elif entry == "cells":
        want = m.score_cells(batch, lists["row"], lists["col"], values=lists["val"], draws=params)
        assert _same(out["mean"], want["mean"]) and _same(out["lppd"], want["lppd"])
    elif entry == "rank":
        want = m.rank_cells(batch, lists["row"], lists["col"], draws=params)
        assert _same(out["rank"], want["rank"]) and _same(out["cand"], want["candidates"])
        assert _same(out["score"], want["score"])
    elif entry == "predict":
        want = m.predict(batch, cols=list(PANEL_COLS), draws=params, sd=True, p_nonzero=True)
        assert _same(out["mean"], want["mean"]) and _same(out["sd"], want["sd"])
        assert _same(out["pnz"], want["p_nonzero"])
    elif entry == "groups":
        want = m.group_means(batch, lists["labels"], n_groups=good["G"], cols=list(PANEL_COLS), draws=params,
                             p_nonzero=True)
        assert _same(out["sum"], want["sum"]) and _same(out["nz"], want["sum_nonzero"])
        assert want["count"].tolist() == [18, 17, 17], "the labels -1, 0, 1, 2, -1, ... of 70 rows"
    elif entry == "embed":
        want = m.embed(batch, draws=params, sd=True)
        assert _same(out["mean"], want["mean"]) and _same(out["sd"], want["sd"])
    elif entry == "toprows":
        want = m.top_rows(batch, cols=list(PANEL_COLS), k=good["k"], draws=params)
        assert torch.equal(out["rows"].long(), want["rows"]) and _same(out["scores"], want["scores"])
    elif entry == "sets":
        want = m.set_scores(batch, PANEL_SETS, PANEL_WEIGHTS, draws=params, sd=True)
        assert _same(out["mean"], want["mean"]) and _same(out["sd"], want["sd"])
    else:       # waic and waic_cols (the column sums against the method's: tests/test_gpu_waic_cols.py)
        got = _waic.combine(out["sums"])
        want = m.waic_streaming(batch, draws=params, row_scores=True)
        print("ctypes", got, "method", {k: v for k, v in want.items() if not k.startswith("row_")})
        assert got["n"] == want["n"] == B * D and got["n_excluded"] == want["n_excluded"] == 0
        assert abs(got["lppd"] - want["lppd"]) <= 1e-5 * abs(want["lppd"])
        assert abs(got["pwaic"] - want["pwaic"]) <= 1e-3 * max(abs(want["pwaic"]), 1e-9) + 1e-9
        assert abs(got["waic"] - want["waic"]) <= 1e-5 * abs(want["waic"])
        for i, (key, tol) in enumerate((("row_lppd", 1e-5), ("row_pwaic", 1e-3))):
            r = want[key].cpu().numpy()
            np.testing.assert_allclose(out["rows"][:, i].cpu().numpy(), r, rtol=tol, atol=tol * np.abs(r).max())
