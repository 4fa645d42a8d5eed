"""CPU-side tests of set_scores (PoissonFactorization.set_scores, spmf_set_scores, csrc/sets.hip) and of
spmf_amd.sets: the method's argument checks on a CPU-only model, pack / read_gmt, the error contract of the entry
through raw ctypes (the draw stage's shared cases, _stream_cases.assert_shared_errors, then the entry's own) -- all
refused before anything touches a device -- and the scratch size.  (The method on the classes: the "sets" row of
tests/test_stream_host.py; the valid call: tests/test_gpu_sets.py.)"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from _stream_cases import (B, ENTRIES, S, assert_declared_exported_bound, assert_shared_errors, cpu_model, host_ctx,
                           host_good_call, library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_exported_and_bound():
    lib = library()
    assert_declared_exported_bound("spmf_sets_scratch_bytes", 5)
    assert_declared_exported_bound("spmf_set_scores", len(ENTRIES["sets"].own) + 8)
    assert callable(lib.spmf_set_scores) and callable(lib.spmf_sets_scratch_bytes)
    assert lib.spmf_version() == 6


def _i64(*v):
    return (C.c_int64 * len(v))(*v)


def test_shared_and_own_errors_return_before_any_device_call():
    """The dummy-address call of _stream_cases.host_good_call (K = 3, D = 45, 70 empty rows, two sets of 4 and 5
    listed columns behind a real host set_ptr): only refused and empty calls may be made with it."""
    lib = library()
    good, need, no_u, raw, cleanup = host_good_call(lib, "sets")
    h, cs = good["h"], good["ct"]
    try:
        call = assert_shared_errors(lib, "sets", good, need, no_u, raw)
        # the entry's own
        assert call(set_ptr=_i64(0, 5, 4)) == -1, "decreasing"
        assert "set_ptr" in lib.spmf_last_error(h).decode()
        assert call(set_ptr=_i64(1, 4, 9)) == -1, "set_ptr[0] != 0"
        assert call(set_ptr=None) == -1
        assert call(n_sets=-1) == -1
        assert "n_sets" in lib.spmf_last_error(h).decode()
        assert call(ld=1) == -1
        assert "ld" in lib.spmf_last_error(h).decode()
        assert call(mean=None) == -1
        assert "mean_out" in lib.spmf_last_error(h).decode()
        assert call(cols=None) == -1, "NULL set_cols with listed columns"
        assert "set_cols" in lib.spmf_last_error(h).decode()
        assert call(S=1) == -1, "sd with one draw"
        assert "S >= 2" in lib.spmf_last_error(h).decode()
        assert call(set_ptr=_i64(0, 0, 0), mean=None) == -1, "all sets empty: the zero fill needs mean too"
        # errors come before the empty returns
        empty = type(cs).from_buffer_copy(cs)
        empty.n_rows = 0
        need_b0 = int(lib.spmf_sets_scratch_bytes(h, 0, S, 2, good["set_ptr"]))
        need_g0 = int(lib.spmf_sets_scratch_bytes(h, B, S, 0, None))
        assert 0 < need_g0 <= need and 0 < need_b0 <= need
        assert call(ct=empty, nbytes=need_b0 - 256) == -3 and call(n_sets=0, nbytes=need_g0 - 256) == -3
        assert call(ct=empty, ld=1) == -1 and call(ct=empty, set_ptr=_i64(0, 5, 4)) == -1
        assert call(n_sets=0, S=0) == -1 and call(n_sets=0, ld=-1) == -1
        assert call(ct=empty, S=1) == -1, "sd with one draw, empty batch"
        # the empty cases are served without a launch: no pointer here could be dereferenced
        assert call(n_sets=0) == 0 and call(n_sets=0, set_ptr=None, cols=None, weights=None, mean=None, sd=None) == 0
        assert call(ct=empty) == 0 and call(ct=empty, mean=None, cols=None, sd=None) == 0, "an empty batch"
    finally:
        cleanup()


@pytest.mark.parametrize("k", [3, 16, 64, 128])
def test_scratch_size(k):
    """0 for bad arguments; a multiple of 256; non-decreasing in the rows, in S and in the listed columns of a
    set; at least the draw carve (spmf_embed_scratch_bytes); a pure function of the padded sizes."""
    lib = library()
    h = host_ctx(lib, k)
    try:
        def size(rows, s, ptr):
            return int(lib.spmf_sets_scratch_bytes(h, rows, s, len(ptr) - 1, _i64(*ptr)))
        prev_n = 0
        for n in (0, 1, 63, 64, 65, 128, 129, 1000, 5000):
            ptr = (0, 3, 3, 3 + n)
            prev_rows = 0
            for rows in (0, 1, 63, 64, 65, B, 1000, 100000):
                prev_s = 0
                for s in (1, 2, 7, 8, 9, 64):
                    v = size(rows, s, ptr)
                    assert v > 0 and v % 256 == 0, (n, rows, s, v)
                    assert v >= int(lib.spmf_embed_scratch_bytes(h, rows, s)), (n, rows, s)
                    assert v >= prev_s, ("S", n, rows, s)
                    prev_s = v
                v2 = size(rows, 2, ptr)
                assert v2 >= prev_rows, ("rows", n, rows)
                prev_rows = v2
            vn = size(B, 2, ptr)
            assert vn >= prev_n, ("listed", n)
            prev_n = vn
        assert size(B, 2, (0, 1, 2)) == size(B, 2, (0, 64, 128)), "whole 64-column blocks per set"
        assert size(B, 2, (0, 65)) == size(B, 2, (0, 64, 128))
        assert size(B, 2, (0, 1, 2)) > size(B, 2, (0, 2)), "two sets of one column are two blocks"
        for bad in ((-1, 2, (0, 4)), (B, 0, (0, 4)), (B, 2, (1, 4)), (B, 2, (0, 4, 3)), (B, 2, (0, 1 << 40))):
            assert size(*bad) == 0, bad
        assert int(lib.spmf_sets_scratch_bytes(h, B, 2, -1, _i64(0))) == 0
        assert int(lib.spmf_sets_scratch_bytes(h, B, 2, 1, None)) == 0
        assert int(lib.spmf_sets_scratch_bytes(None, B, 2, 1, _i64(0, 4))) == 0
        assert int(lib.spmf_sets_scratch_bytes(h, B, 2, 0, None)) == int(lib.spmf_embed_scratch_bytes(h, B, 2))
    finally:
        lib.spmf_ctx_destroy(h)


# ---- the method's argument checks ---------------------------------------------------------------

def test_bad_sets_and_weights_raise_value_error_without_a_device():
    m, x, draws = cpu_model()
    data = {"counts": x}
    with pytest.raises(ValueError, match="1-D"):
        m.set_scores(data, [np.arange(4).reshape(2, 2)], draws=draws)
    with pytest.raises(ValueError, match="sequence of 1-D"):
        m.set_scores(data, np.arange(4).reshape(2, 2), draws=draws)
    with pytest.raises(ValueError, match="integers"):
        m.set_scores(data, [[0, 1], np.array([0.0, 2.0])], draws=draws)
    with pytest.raises(ValueError, match="integers"):
        m.set_scores(data, [torch.tensor([True, False])], draws=draws)
    with pytest.raises(ValueError, match=r"set 1 must lie in \[0, 6\), got 0 .. 6"):
        m.set_scores(data, [[0, 5], [0, 6]], draws=draws)
    with pytest.raises(ValueError, match=r"set 0 must lie in \[0, 6\), got -1 .. 2"):
        m.set_scores(data, [torch.tensor([2, -1])], draws=draws)
    with pytest.raises(ValueError, match="as long as the set, got 1 for 2"):
        m.set_scores(data, [[0, 1], [2]], weights=[[1.0], [1.0]], draws=draws)
    with pytest.raises(ValueError, match="one array per set, got 1 for 2"):
        m.set_scores(data, [[0, 1], [2]], weights=[[1.0, 1.0]], draws=draws)
    with pytest.raises(ValueError, match="finite"):
        m.set_scores(data, [[0, 1], [2]], weights=[[1.0, float("nan")], [1.0]], draws=draws)
    with pytest.raises(ValueError, match="finite"):
        m.set_scores(data, [[0]], weights=[[float("inf")]], draws=draws)
    with pytest.raises(ValueError, match="1-D"):
        m.set_scores(data, [[0, 1]], weights=[[[1.0, 1.0]]], draws=draws)


def test_sd_needs_two_draws():
    m, x, draws = cpu_model()
    one = {n: v[:1] for n, v in draws.items()}
    with pytest.raises(ValueError, match="at least 2 draws"):
        m.set_scores({"counts": x}, [[0, 1]], draws=one, sd=True)
    with pytest.raises(ValueError, match="nsamples >= 2"):
        m.set_scores({"counts": x}, [[0, 1]], nsamples=1, sd=True)


def test_custom_codec_raises_after_the_argument_checks():
    m, x, draws = cpu_model(encoder_function=lambda t: t, decoder_function=lambda t: t)
    with pytest.raises(ValueError, match="must lie in"):
        m.set_scores({"counts": x}, [[0, 6]], draws=draws)
    with pytest.raises(NotImplementedError, match="set_scores"):
        m.set_scores({"counts": x}, [[0, 1]], draws=draws)


def test_a_valid_call_on_a_cpu_model_fails_like_top_k():
    m, x, draws = cpu_model()
    with pytest.raises(Exception) as e_topk:
        m.top_k({"counts": x}, k=3, draws=draws)
    with pytest.raises(Exception) as e_set:
        m.set_scores({"counts": x}, [[0, 1], []], weights=[[1.0, -1.0], []], draws=draws, sd=True)
    assert type(e_set.value) is type(e_topk.value), (e_set.value, e_topk.value)
    assert not isinstance(e_set.value, ValueError)


# ---- spmf_amd.sets --------------------------------------------------------------------------------

def test_pack_lays_the_lists_one_behind_the_other():
    from spmf_amd import sets
    ptr, cols, w = sets.pack([[5, 0, 0], [], torch.tensor([3]), np.array([1, 2], dtype=np.int32)], None, 6)
    assert ptr.dtype == np.int64 and ptr.tolist() == [0, 3, 3, 4, 6] and w is None
    assert cols.dtype == torch.int32 and cols.tolist() == [5, 0, 0, 3, 1, 2]
    ptr, cols, w = sets.pack([[5, 0], []], [np.array([0.5, -2.0]), []], 6)
    assert ptr.tolist() == [0, 2, 2] and w.dtype == torch.float32 and w.tolist() == [0.5, -2.0]
    ptr, cols, w = sets.pack([], None, 6)
    assert ptr.tolist() == [0] and cols.numel() == 0
    ptr, cols, w = sets.pack([[]], [[]], 6)
    assert ptr.tolist() == [0, 0] and cols.numel() == 0 and w.numel() == 0


def test_read_gmt_maps_names_and_drops_unknown_members(tmp_path):
    from spmf_amd import sets
    path = tmp_path / "toy.gmt"
    path.write_text("CYCLE\tcell cycle\tg3\tg0\tnope\tg3\n"
                    "\n"
                    "NONE\tno known member\tabc\txyz\n"
                    "BARE\tno member at all\n"
                    "TAIL\thttp://example.invalid/set\tg5\t\t\r\n")
    names = np.array([f"g{j}" for j in range(6)], dtype=object)
    set_names, lists, dropped = sets.read_gmt(str(path), names)
    assert set_names == ["CYCLE", "NONE", "BARE", "TAIL"] and dropped == 3
    assert [s.tolist() for s in lists] == [[3, 0, 3], [], [], [5]], "a duplicate member stays, unknown ones go"
    assert all(s.dtype == np.int64 for s in lists)
    ptr, cols, _ = sets.pack(lists, None, 6)
    assert ptr.tolist() == [0, 3, 3, 3, 4] and cols.tolist() == [3, 0, 3, 5]


def test_scrnaseq_cli_has_the_gene_sets_flag_off_by_default():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "factorize_scrnaseq_counts", os.path.join(ROOT, "bin", "factorize_scrnaseq_counts.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    args = cli.build_parser().parse_args(["--counts", "x_counts.npy"])
    assert args.gene_sets is None and args.set_draws == 32 and args.labels is None
    assert cli.build_parser().parse_args(["--counts", "x", "--gene-sets", "s.gmt"]).gene_sets == "s.gmt"
