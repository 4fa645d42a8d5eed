"""GPU: the C-ABI error contract the three streaming entry points share (spmf_waic_accumulate,
spmf_topk_rows, spmf_score_cells: include/spmf_hip.h), through ctypes at B = 70, D = 45, K = 3,
S = 2, Poisson, panel_rows = 32.  Every error returns before a launch: outputs and scratch keep
their sentinels.  Then the valid call returns what the Python method returns: the same bits for
top-k and the cell list; the WAIC sums go through fp64 atomics, so they are held to the
tolerances of test_gpu_waic_streaming.py (lppd and waic 1e-5 relative, pwaic 1e-3, row scores
the same with an atol of that fraction of the largest row value).  The entry-specific cases (k,
flags, the cell list's own arguments) stay with test_gpu_topk.py / test_gpu_score_cells.py."""
import numpy as np
import pytest
import torch

from _stream_cases import ENTRIES, _problem, assert_shared_errors, gpu_good_call
from test_gpu_dense import _dense_model

pytestmark = pytest.mark.gpu
B, D, K, S = 70, 45, 3, 2


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_shared_errors_launch_nothing_and_the_valid_call_is_the_methods(entry):
    from spmf_amd import _lib
    from spmf_amd import waic as _waic
    cfg, x, params, mask, _ = _problem("poisson", B, D, K, S)
    m = _dense_model("poisson", cfg, mask, 32)
    lib = _lib.load()
    good, need, out, scratch, no_u = gpu_good_call(entry, m, x, params)
    raw = _dense_model("mixed", cfg, np.arange(D) % 3 == 1, 32)._new_ctx()   # a mixed context nobody gave column types
    try:
        call = assert_shared_errors(lib, entry, good, need, no_u, raw)
    finally:
        lib.spmf_ctx_destroy(raw)
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out.values()) and not bool(scratch.any())
    if entry == "waic":                                   # sums and row scores are accumulated
        for t in out.values():
            t.zero_()
    assert call() == 0
    torch.cuda.synchronize()
    if entry == "topk":
        want = m.top_k({"counts": x}, k=good["k"], draws=params)
        assert torch.equal(out["cols"], want["columns"]) and torch.equal(_bits(out["scores"]), _bits(want["scores"]))
    elif entry == "cells":
        lists = good["keep"][-1]
        want = m.score_cells({"counts": x}, lists["row"], lists["col"], values=lists["val"], draws=params)
        assert torch.equal(_bits(out["mean"]), _bits(want["mean"]))
        assert torch.equal(_bits(out["lppd"]), _bits(want["lppd"]))
    else:
        got = _waic.combine(out["sums"])
        want = m.waic_streaming({"counts": x}, draws=params, row_scores=True)
        print("ctypes", got, "method", {k: v for k, v in want.items() if not k.startswith("row_")})
        assert got["n"] == want["n"] == B * D and got["n_excluded"] == want["n_excluded"] == 0
        assert abs(got["lppd"] - want["lppd"]) <= 1e-5 * abs(want["lppd"])
        assert abs(got["pwaic"] - want["pwaic"]) <= 1e-3 * max(abs(want["pwaic"]), 1e-9) + 1e-9
        assert abs(got["waic"] - want["waic"]) <= 1e-5 * abs(want["waic"])
        for i, (key, tol) in enumerate((("row_lppd", 1e-5), ("row_pwaic", 1e-3))):
            r = want[key].cpu().numpy()
            np.testing.assert_allclose(out["rows"][:, i].cpu().numpy(), r, rtol=tol, atol=tol * np.abs(r).max())
