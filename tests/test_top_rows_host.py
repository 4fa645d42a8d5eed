"""CPU-side tests of top_rows (PoissonFactorization.top_rows, spmf_toprows_columns, csrc/toprows.hip): the method's
argument checks on a CPU-only model, the error contract of the entry through raw ctypes (the draw stage's shared
cases, _stream_cases.assert_shared_errors, then the entry's own) -- all refused before anything touches a
device --, the scratch size, and the driver's stable fold of the row chunks against a brute-force fp64 reference.
(The method on the classes: the "toprows" row of tests/test_stream_host.py; the valid call:
tests/test_gpu_top_rows.py.)"""
import numpy as np
import pytest
import torch

from _stream_cases import (B, D, ENTRIES, S, assert_declared_exported_bound, assert_shared_errors, cpu_model, host_ctx,
                           host_good_call, library, no_library)


def test_entry_points_are_declared_exported_and_bound():
    lib = library()
    assert_declared_exported_bound("spmf_toprows_scratch_bytes", 4)
    assert_declared_exported_bound("spmf_toprows_columns", len(ENTRIES["toprows"].own) + 8)
    assert len(ENTRIES["toprows"].own) + 8 == 14
    assert callable(lib.spmf_toprows_columns) and callable(lib.spmf_toprows_scratch_bytes)
    assert lib.spmf_version() == 6


def test_shared_and_own_errors_return_before_any_device_call():
    """The dummy-address call of _stream_cases.host_good_call (K = 3, D = 45, 70 empty rows, a list of four
    columns): only refused calls and the call with an empty list may be made with it."""
    lib = library()
    good, need, no_u, raw, cleanup = host_good_call(lib, "toprows")
    h, cs = good["h"], good["ct"]

    def error():
        return lib.spmf_last_error(h).decode()
    try:
        call = assert_shared_errors(lib, "toprows", good, need, no_u, raw)
        # the entry's own
        for k in (0, 65, -1):
            assert call(k=k) == -1, k
            assert "k must be in 1..64" in error()
        assert call(flags=2) == -1 and call(flags=3) == -1, "flag bit 1"
        assert "flag" in error()
        assert call(n=-1) == -1 and call(n=D + 1) == -1
        assert "n_cols" in error()
        assert call(cols=None) == -1, "cols == NULL with n_cols != D"
        assert "n_cols must be D" in error()
        assert call(rows=None) == -1 and call(scores=None) == -1
        assert "rows_out" in error()
        # errors come before the empty returns
        empty = type(cs).from_buffer_copy(cs)
        empty.n_rows = 0
        need_b0 = int(lib.spmf_toprows_scratch_bytes(h, 0, S, 4))
        need_c0 = int(lib.spmf_toprows_scratch_bytes(h, B, S, 0))
        assert 0 < need_c0 <= need and 0 < need_b0 <= need
        assert call(ct=empty, nbytes=need_b0 - 256) == -3 and call(n=0, nbytes=need_c0 - 256) == -3
        assert call(ct=empty, k=0) == -1 and call(ct=empty, flags=2) == -1 and call(ct=empty, rows=None) == -1
        assert call(n=0, S=0) == -1 and call(n=0, k=65) == -1 and call(n=0, flags=2) == -1
        # an empty list is served without a launch or a write: no pointer here could be dereferenced
        # (cols == NULL stays "all D columns": with n_cols = 0 it is refused like any other count but D)
        assert call(n=0) == 0 and call(n=0, rows=None, scores=None) == 0
        assert call(n=0, cols=None) == -1
        assert call(ct=empty, n=0) == 0
    finally:
        cleanup()


@pytest.mark.parametrize("k", [3, 16, 64, 128])
def test_scratch_size(k):
    """0 for bad arguments; a multiple of 256; with no column exactly the rank_cells size (the draw tables and the
    bitmap), which is the top_k size where top_k takes one slice (this context: one column block); non-decreasing
    in the rows, in S and in the listed columns (D = 45 is one column block, so the row slices do not depend on
    n_cols and every region grows with it); at D columns above the predict size (the same tables, the bitmap
    more)."""
    lib = library()
    h = host_ctx(lib, k)
    try:
        def size(rows, s, n):
            return int(lib.spmf_toprows_scratch_bytes(h, rows, s, n))
        for rows in (0, 1, 63, 64, 65, B, 1000, 100000):
            prev_s = 0
            for s in (1, 2, 7, 8, 9, 64):
                prev_n = 0
                for n in (0, 1, 4, 31, 32, 33, D):
                    v = size(rows, s, n)
                    assert v > 0 and v % 256 == 0, (rows, s, n, v)
                    assert v >= prev_n, ("n_cols", rows, s, n)
                    prev_n = v
                assert size(rows, s, 0) == int(lib.spmf_rank_scratch_bytes(h, rows, s)), (rows, s)
                assert size(rows, s, 0) >= int(lib.spmf_topk_scratch_bytes(h, rows, s)), (rows, s)
                assert size(rows, s, D) > int(lib.spmf_predict_scratch_bytes(h, rows, s)) or rows == 0, (rows, s)
                assert size(rows, s, D) >= prev_s, ("S", rows, s)
                prev_s = size(rows, s, D)
        prev_rows = 0
        for rows in (0, 1, 63, 64, 65, B, 1000, 100000):
            v = size(rows, 2, 4)
            assert v >= prev_rows, ("rows", rows)
            prev_rows = v
        # one column block, 16 row slices at most: their results are [slices][n_cols][64] int32 and float
        assert size(100000, 2, 4) - size(100000, 2, 0) >= 16 * 4 * 64 * 8
        for bad in ((-1, 2, 4), (B, 0, 4), (B, 2, -1), (B, 2, D + 1)):
            assert size(*bad) == 0, bad
        assert int(lib.spmf_toprows_scratch_bytes(None, B, 2, 4)) == 0
    finally:
        lib.spmf_ctx_destroy(h)


# ---- the method's argument checks ---------------------------------------------------------------

def test_bad_k_and_cols_raise_value_error_without_a_library_call(monkeypatch):
    m, x, draws = cpu_model()
    no_library(monkeypatch)
    data = {"counts": x}
    for k in (True, False, 0, 65, -1, 2.0, None, "3"):
        with pytest.raises(ValueError, match="top_rows"):
            m.top_rows(data, k=k, draws=draws)
    with pytest.raises(ValueError, match="integers"):
        m.top_rows(data, cols=np.array([0.0, 2.0]), draws=draws)
    with pytest.raises(ValueError, match="integers"):
        m.top_rows(data, cols=torch.tensor([True, False]), draws=draws)
    with pytest.raises(ValueError, match="1-D"):
        m.top_rows(data, cols=np.arange(4).reshape(2, 2), draws=draws)
    with pytest.raises(ValueError, match=r"cols must lie in \[0, 6\), got 0 .. 6"):
        m.top_rows(data, cols=[0, 6], draws=draws)
    with pytest.raises(ValueError, match=r"cols must lie in \[0, 6\), got -1 .. 2"):
        m.top_rows(data, cols=torch.tensor([2, -1]), draws=draws)
    with pytest.raises(ValueError, match="more than the 6 there are"):
        m.top_rows(data, cols=[0, 1, 2, 3, 4, 5, 0], draws=draws)


def test_custom_codec_raises_after_the_argument_checks(monkeypatch):
    m, x, draws = cpu_model(encoder_function=lambda t: t, decoder_function=lambda t: t)
    no_library(monkeypatch)
    with pytest.raises(ValueError, match="must lie in"):
        m.top_rows({"counts": x}, cols=[0, 6], draws=draws)
    with pytest.raises(ValueError, match="1 <= k <= 64"):
        m.top_rows({"counts": x}, k=0, draws=draws)
    with pytest.raises(NotImplementedError, match=r"top_rows.*predict"):
        m.top_rows({"counts": x}, cols=[0, 1], draws=draws)


def test_a_valid_call_on_a_cpu_model_fails_like_top_k():
    m, x, draws = cpu_model()
    with pytest.raises(Exception) as e_topk:
        m.top_k({"counts": x}, k=3, draws=draws)
    with pytest.raises(Exception) as e_rows:
        m.top_rows({"counts": x}, cols=[0, 5, 5], k=3, draws=draws)
    assert type(e_rows.value) is type(e_topk.value), (e_rows.value, e_topk.value)
    assert not isinstance(e_rows.value, ValueError)


# ---- the driver's fold --------------------------------------------------------------------------

def _chunk_result(scores, k):
    """What one library call returns for a chunk with the fp32 scores [rows, C] (NaN: no candidate): per column
    the best k by (score descending, row ascending), rows relative to the chunk, padded with -1 / -inf."""
    n, ncol = scores.shape
    rows = np.full((ncol, k), -1, dtype=np.int32)
    out = np.full((ncol, k), -np.inf, dtype=np.float32)
    for j in range(ncol):
        cand = [b for b in range(n) if np.isfinite(scores[b, j])]
        cand.sort(key=lambda b: (-float(scores[b, j]), b))
        for i, b in enumerate(cand[:k]):
            rows[j, i], out[j, i] = b, scores[b, j]
    return rows, out


@pytest.mark.parametrize("k", [1, 4, 64])
def test_fold_keeps_the_best_k_with_ties_in_ascending_row_order(k):
    """Random chunk results with planted ties (scores drawn from five values), columns without a candidate in some
    or all chunks, chunks of 1 .. 90 rows and an empty running state: the fold over the chunks equals the
    brute-force selection over all rows, taken in fp64 with the order (score descending, row ascending)."""
    from spmf_amd.streaming import fold_top_rows
    rng = np.random.default_rng(40 + k)
    ncol = 9
    lengths = [1, 90, 7, 64, 3]
    total = sum(lengths)
    scores = rng.choice(np.array([0.25, 0.5, 1.0, 1.5, 3.0], dtype=np.float32), size=(total, ncol))
    scores[:, 1] = rng.random(total).astype(np.float32)          # no ties
    scores[:, 2] = np.nan                                        # no candidate at all
    scores[rng.random(total) < 0.9, 3] = np.nan                  # fewer than k (for k = 64), missing in whole chunks
    scores[:, 4] = 2.0                                           # one tie: rows 0 .. k-1
    scores[lengths[0]:lengths[0] + lengths[1], 5] = np.nan       # the largest chunk has none
    rows = torch.full((ncol, k), -1, dtype=torch.int64)
    best = torch.full((ncol, k), float("-inf"), dtype=torch.float32)
    off = 0
    for n in lengths:
        r, s = _chunk_result(scores[off:off + n], k)
        rows, best = fold_top_rows(rows, best, torch.as_tensor(r), torch.as_tensor(s), off)
        assert rows.dtype == torch.int64 and best.dtype == torch.float32
        assert tuple(rows.shape) == (ncol, k) and tuple(best.shape) == (ncol, k)
        off += n
    ref = scores.astype(np.float64)
    for j in range(ncol):
        cand = [b for b in range(total) if np.isfinite(ref[b, j])]
        cand.sort(key=lambda b: (-ref[b, j], b))
        want_r = cand[:k] + [-1] * (k - len(cand[:k]))
        want_s = [ref[b, j] for b in cand[:k]] + [-np.inf] * (k - len(cand[:k]))
        assert rows[j].tolist() == want_r, j
        assert best[j].double().tolist() == want_s, j
    assert rows[4].tolist() == list(range(k)) and (rows[2] == -1).all()
