"""CPU-side tests of predict (PoissonFactorization.predict, spmf_predict_columns, csrc/panel.hip): the error
contract of the draw stage and the entry's own argument errors -- all refused before anything touches a
device -- the empty cases, the scratch size, and the argument checks of the method that need no device.
(Declared / exported / bound and the method on the classes: the "predict" row of tests/test_stream_host.py; the
valid call: tests/test_gpu_predict.py.)"""
import numpy as np
import pytest

from _stream_cases import B, D, ENTRIES, S, assert_shared_errors, cpu_model, host_ctx, host_good_call, library

CALL, SIZE = ENTRIES["predict"].call, ENTRIES["predict"].size


def test_symbols_are_in_the_built_library():
    lib = library()
    assert callable(getattr(lib, CALL)) and callable(getattr(lib, SIZE))
    assert lib.spmf_version() == 6


def test_shared_and_own_errors_return_before_any_device_call():
    """The dummy-address call of _stream_cases.host_good_call (K = 3, D = 45, 70 empty rows): the error cases of
    the draw stage (_stream_cases.assert_shared_errors) and the entry's own are refused with their codes, before
    the empty returns; nothing here is a valid call with work to do, so nothing may be launched or dereferenced."""
    lib = library()
    good, need, no_u, raw, cleanup = host_good_call(lib, "predict")
    h, cs = good["h"], good["ct"]
    try:
        call = assert_shared_errors(lib, "predict", good, need, no_u, raw)
        # the entry's own
        assert call(mean=None) == -1, "no mean_out with work to do"
        assert "mean_out" in lib.spmf_last_error(h).decode()
        need1 = int(lib.spmf_predict_scratch_bytes(h, B, 1))
        assert call(S=1, nbytes=need1) == -1, "sd_out with one draw"
        assert "sd_out" in lib.spmf_last_error(h).decode()
        assert call(n=-1) == -1 and call(n=D + 1) == -1
        assert "n_cols" in lib.spmf_last_error(h).decode()
        assert call(cols=None) == -1 and call(cols=None, n=D - 1) == -1 and call(cols=None, n=0) == -1, \
            "no list: n_cols must be D"
        # errors come before the empty returns
        empty = type(cs).from_buffer_copy(cs)
        empty.n_rows = 0
        need0 = int(lib.spmf_predict_scratch_bytes(h, 0, S))
        assert call(n=0, nbytes=need - 256) == -3 and call(ct=empty, nbytes=need0 - 256) == -3
        assert call(n=0, S=1, nbytes=need1) == -1 and call(ct=empty, S=1) == -1, "sd_out with one draw, no work"
        assert call(ct=empty, n=D + 1) == -1 and call(ct=empty, cols=None) == -1
        assert call(n=0, S=0) == -1 and call(n=0, ptr=good["ptr"] + 4) == -1
        # the empty cases are served without a launch: no pointer here could be dereferenced
        assert call(n=0) == 0 and call(n=0, mean=None, sd=None, pnz=None) == 0
        assert call(ct=empty) == 0 and call(ct=empty, cols=None, n=D) == 0 and call(ct=empty, mean=None) == 0, \
            "an empty batch"
        assert call(n=0, S=1, sd=None, nbytes=need1) == 0
    finally:
        cleanup()


@pytest.mark.parametrize("k", [3, 16, 64, 128])
def test_scratch_size(k):
    """A multiple of 256: the draw stage's scratch plus the compacted tables of a listed panel sized for
    n_cols = D (V' rows, phi and the column types, three regions of their own); 0 for S < 1, for negative
    rows and without a context; a function of (rows, S) alone."""
    lib = library()
    h, h2 = host_ctx(lib, k), host_ctx(lib, k)
    try:
        kp = int(lib.spmf_padded_k(h))
        for rows in (0, 1, B, 1000):
            for s in (1, 2, 7):
                size, cells = (int(getattr(lib, f)(h, rows, s)) for f in (SIZE, "spmf_cells_scratch_bytes"))
                tables = s * D * kp * 4 + s * D * 4 + D
                assert size % 256 == 0 and cells + tables <= size <= cells + tables + 3 * 255, (rows, s, size)
                assert int(lib.spmf_predict_scratch_bytes(h, rows, s)) == size
                assert int(lib.spmf_predict_scratch_bytes(h2, rows, s)) == size
        assert int(lib.spmf_predict_scratch_bytes(h, B, 0)) == 0
        assert int(lib.spmf_predict_scratch_bytes(h, -1, 2)) == 0
        assert int(lib.spmf_predict_scratch_bytes(None, B, 2)) == 0
    finally:
        lib.spmf_ctx_destroy(h)
        lib.spmf_ctx_destroy(h2)


# ---- the method's argument checks ---------------------------------------------------------------

def test_bad_column_lists_raise_value_error_without_a_device():
    import torch
    m, x, draws = cpu_model()
    data = {"counts": x}
    with pytest.raises(ValueError, match=r"^predict: cols must be 1-D, got shape \(2, 1\)$"):
        m.predict(data, np.zeros((2, 1), dtype=np.int64), draws=draws)
    with pytest.raises(ValueError, match="1-D"):
        m.predict(data, torch.tensor(3), draws=draws)
    with pytest.raises(ValueError, match="integers"):
        m.predict(data, [1.0, 5.0], draws=draws)
    for cols in ([0, 6], [-1, 0], torch.tensor([5, 2, 7]), np.array([3, -2], dtype=np.int32)):
        with pytest.raises(ValueError, match=r"must lie in \[0, 6\)"):
            m.predict(data, cols, draws=draws)
    with pytest.raises(ValueError, match="more than the 6"):
        m.predict(data, [0, 1, 2, 3, 4, 5, 0], draws=draws)


def test_sd_needs_two_draws():
    m, x, draws = cpu_model()
    one = {n: v[:1] for n, v in draws.items()}
    with pytest.raises(ValueError, match="at least 2 draws"):
        m.predict({"counts": x}, [0, 1], draws=one, sd=True)
    with pytest.raises(ValueError, match="nsamples >= 2"):
        m.predict({"counts": x}, [0, 1], nsamples=1, sd=True)


def test_custom_codec_raises_after_the_argument_checks():
    m, x, draws = cpu_model(encoder_function=lambda t: t, decoder_function=lambda t: t)
    with pytest.raises(ValueError, match="must lie in"):
        m.predict({"counts": x}, [0, 6], draws=draws)
    with pytest.raises(NotImplementedError, match="predict"):
        m.predict({"counts": x}, [0, 5], draws=draws)


def test_a_valid_list_on_a_cpu_model_fails_like_top_k():
    """Past the argument checks the call needs the library's context, as top_k does: the same failure, and not a
    ValueError."""
    m, x, draws = cpu_model()
    with pytest.raises(Exception) as e_topk:
        m.top_k({"counts": x}, k=3, draws=draws)
    for cols in (None, [5, 0, 0]):
        with pytest.raises(Exception) as e_pred:
            m.predict({"counts": x}, cols, draws=draws, sd=True, p_nonzero=True)
        assert type(e_pred.value) is type(e_topk.value), (e_pred.value, e_topk.value)
        assert not isinstance(e_pred.value, ValueError)
