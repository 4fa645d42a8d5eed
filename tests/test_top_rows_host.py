"""CPU-side tests of top_rows (PoissonFactorization.top_rows, spmf_toprows_columns, csrc/toprows.hip): the entry
points in the header, the export list and the binding, the method on the classes, the method's argument checks on
a CPU-only model, the error contract of the entry through a raw ctypes call of this file's own (the draw stage's
shared cases as tests/_stream_cases.assert_shared_errors lists them, then the entry's own) -- all refused before
anything touches a device --, the scratch size, and the driver's stable fold of the row chunks against a
brute-force fp64 reference.  The valid call is tests/test_gpu_top_rows.py's.

The call takes 14 arguments: ctx, counts, S, params, eta | n_cols, cols, k, flags, rows, scores | scratch,
scratch_bytes, stream -- the declaration of include/spmf_hip.h counted the way tests/test_stream_host.py counts
the other entries (five in front, the entry's own six, three behind); the size function takes four."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from _stream_cases import B, D, K, S, assert_declared_exported_bound

OWN = (("n_cols", C.c_int32), ("cols", C.c_void_p), ("k", C.c_int), ("flags", C.c_uint), ("rows", C.c_void_p),
       ("scores", C.c_void_p))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from spmf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    assert_declared_exported_bound("spmf_toprows_scratch_bytes", 4)
    assert_declared_exported_bound("spmf_toprows_columns", len(OWN) + 8)
    assert len(OWN) + 8 == 14
    assert callable(lib.spmf_toprows_columns) and callable(lib.spmf_toprows_scratch_bytes)
    assert lib.spmf_version() == 6


def test_method_is_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        assert callable(getattr(cls, "top_rows", None)), cls.__name__


def _host_good_call(lib):
    """A valid-looking call that needs no device, as _stream_cases.host_good_call builds them: K = 3, D = 45, a
    hand-filled descriptor of 70 empty rows, dummy aligned addresses, a list of four columns.  Only refused calls
    and the call with an empty list may be made with it."""
    from spmf_amd import _lib
    from spmf_amd._lib import VAR_ORDER
    h, raw = C.c_void_p(), C.c_void_p()
    assert lib.spmf_ctx_create(0, K, D, 0, C.byref(h)) == 0
    assert lib.spmf_ctx_create(0, K, D, _lib.FLAG_MIXED, C.byref(raw)) == 0
    cs = _lib.CountsStruct()
    cs.struct_size = C.sizeof(_lib.CountsStruct)
    cs.n_cols, cs.n_rows, cs.nnz, cs.row_ptr = D, B, 0, 0x10000
    slots = {n: 0x100000 * (i + 1) for i, n in enumerate(VAR_ORDER) if n in ("s", "u", "v", "w")}
    need = int(lib.spmf_toprows_scratch_bytes(h, B, S, 4))
    assert need > 0 and need % 256 == 0
    good = dict(h=h, ct=cs, S=S, pin=_lib.PtrArray(*[slots.get(n) for n in VAR_ORDER]), eta=0x7000000,
                n_cols=4, cols=0x2000000, k=5, flags=1, rows=0x3000000, scores=0x4000000,
                ptr=0x8000000, nbytes=need, stream=None)
    no_u = _lib.PtrArray(*[slots.get(n) if n != "u" else None for n in VAR_ORDER])
    fn = C.CDLL(_lib.LIB_PATH).spmf_toprows_columns
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [t for _, t in OWN] + [
        C.c_void_p, C.c_size_t, C.c_void_p]

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], C.byref(a["ct"]) if a["ct"] is not None else None, a["S"], a["pin"], a["eta"],
                  *[a[n] for n, _ in OWN], a["ptr"], a["nbytes"], a["stream"])

    def cleanup():
        lib.spmf_ctx_destroy(h)
        lib.spmf_ctx_destroy(raw)
    return good, need, no_u, raw, call, cleanup


def test_shared_and_own_errors_return_before_any_device_call(lib):
    good, need, no_u, raw, call, cleanup = _host_good_call(lib)
    h, cs = good["h"], good["ct"]

    def error():
        return lib.spmf_last_error(h).decode()
    try:
        # the draw stage's (tests/_stream_cases.assert_shared_errors, spelled for this entry)
        assert call(S=0) == -1 and call(S=65536) == -1
        assert error().startswith("toprows_columns: "), error()
        for name in ("pin", "eta", "ptr", "ct"):
            assert call(**{name: None}) == -1, name
        assert call(pin=no_u) == -1, "slot u missing"
        assert error().startswith("toprows_columns: "), error()
        assert call(ptr=good["ptr"] + 4) == -1, "scratch off by 4 bytes"
        assert "aligned" in error()
        bad = type(cs).from_buffer_copy(cs)
        bad.struct_size += 8
        assert call(ct=bad) == -1
        assert call(h=raw) == -1
        assert "column_types" in lib.spmf_last_error(raw).decode()
        assert call(nbytes=need - 256) == -3
        assert str(need) in error() and error().startswith("toprows_columns: "), error()
        # the entry's own
        for k in (0, 65, -1):
            assert call(k=k) == -1, k
            assert "k must be in 1..64" in error()
        assert call(flags=2) == -1 and call(flags=3) == -1, "flag bit 1"
        assert "flag" in error()
        assert call(n_cols=-1) == -1 and call(n_cols=D + 1) == -1
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
        assert call(ct=empty, nbytes=need_b0 - 256) == -3 and call(n_cols=0, nbytes=need_c0 - 256) == -3
        assert call(ct=empty, k=0) == -1 and call(ct=empty, flags=2) == -1 and call(ct=empty, rows=None) == -1
        assert call(n_cols=0, S=0) == -1 and call(n_cols=0, k=65) == -1 and call(n_cols=0, flags=2) == -1
        # an empty list is served without a launch or a write: no pointer here could be dereferenced
        # (cols == NULL stays "all D columns": with n_cols = 0 it is refused like any other count but D)
        assert call(n_cols=0) == 0 and call(n_cols=0, rows=None, scores=None) == 0
        assert call(n_cols=0, cols=None) == -1
        assert call(ct=empty, n_cols=0) == 0
    finally:
        cleanup()


@pytest.mark.parametrize("k", [3, 16, 64, 128])
def test_scratch_size(lib, k):
    """0 for bad arguments; a multiple of 256; with no column exactly the rank_cells size (the draw tables and the
    bitmap), which is the top_k size where top_k takes one slice (this context: one column block); non-decreasing
    in the rows, in S and in the listed columns (D = 45 is one column block, so the row slices do not depend on
    n_cols and every region grows with it); at D columns above the predict size (the same tables, the bitmap
    more)."""
    h = C.c_void_p()
    assert lib.spmf_ctx_create(0, k, D, 0, C.byref(h)) == 0
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

def _cpu_model(**kw):
    from spmf_amd import PoissonFactorization
    m = PoissonFactorization(latent_dim=2, feature_dim=6, initialize_distributions=False, device="cpu", **kw)
    rng = np.random.default_rng(0)
    x = rng.poisson(1.0, size=(8, 6)).astype(np.float64)
    draws = {"u": rng.random((2, 6, 2)), "v": rng.random((2, 2, 6)), "w": rng.random((2, 1, 6)),
             "s": rng.random((2, 2, 6))}
    return m, x, draws


def _no_library(monkeypatch):
    """Any load of the library from here on fails the test."""
    from spmf_amd import _lib

    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def test_bad_k_and_cols_raise_value_error_without_a_library_call(monkeypatch):
    m, x, draws = _cpu_model()
    _no_library(monkeypatch)
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
    m, x, draws = _cpu_model(encoder_function=lambda t: t, decoder_function=lambda t: t)
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match="must lie in"):
        m.top_rows({"counts": x}, cols=[0, 6], draws=draws)
    with pytest.raises(ValueError, match="1 <= k <= 64"):
        m.top_rows({"counts": x}, k=0, draws=draws)
    with pytest.raises(NotImplementedError, match=r"top_rows.*predict"):
        m.top_rows({"counts": x}, cols=[0, 1], draws=draws)


def test_a_valid_call_on_a_cpu_model_fails_like_top_k():
    m, x, draws = _cpu_model()
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
