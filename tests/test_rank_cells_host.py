"""CPU-side tests of rank_cells (PoissonFactorization.rank_cells, spmf_rank_cells, csrc/rank.hip): the error
contract of the draw stage and the entry's own argument errors -- all refused before anything touches a
device -- the scratch size, the summary of spmf_amd.heldout.rank_summary on hand cases, and the argument checks
of the method that need no device.  (Declared / exported / bound and the method on the classes: the "rank" row
of tests/test_stream_host.py; the valid call: tests/test_gpu_rank_cells.py.)"""
import math

import numpy as np
import pytest
import torch

from _stream_cases import B, D, ENTRIES, assert_shared_errors, cpu_model, host_ctx, host_good_call, library

CALL, SIZE = ENTRIES["rank"].call, ENTRIES["rank"].size


def test_symbols_are_in_the_built_library():
    lib = library()
    assert callable(getattr(lib, CALL)) and callable(getattr(lib, SIZE))


def test_shared_and_own_errors_return_before_any_device_call():
    """The dummy-address call of _stream_cases.host_good_call: the error cases of the draw stage
    (_stream_cases.assert_shared_errors) and the entry's own are refused with their codes; nothing here is a
    valid call, so nothing may be launched or dereferenced."""
    lib = library()
    good, need, no_u, raw, cleanup = host_good_call(lib, "rank")
    h, cs = good["h"], good["ct"]
    try:
        call = assert_shared_errors(lib, "rank", good, need, no_u, raw)
        # the entry's own
        assert call(n=-1) == -1
        assert "n_cells" in lib.spmf_last_error(h).decode()
        for name in ("row", "col", "rank", "cand", "score"):
            assert call(**{name: None}) == -1, name
        assert call(flags=2) == -1 and call(flags=3) == -1
        assert "flag" in lib.spmf_last_error(h).decode()
        assert call(n=0, flags=4) == -1, "an unknown flag is refused for an empty list too"
        assert call(n=0, nbytes=need - 256) == -3, "errors come before the empty-list return"
        # an empty list is served without a launch: no pointer here could be dereferenced
        assert call(n=0) == 0 and call(n=0, row=None, col=None, rank=None, cand=None, score=None) == 0
        empty = type(cs).from_buffer_copy(cs)
        empty.n_rows = 0
        assert call(ct=empty) == 0, "an empty batch"
    finally:
        cleanup()


@pytest.mark.parametrize("k", [3, 16, 64, 128])
def test_scratch_size(k):
    """A multiple of 256: the draw stage's scratch and the bitmap of the stored cells (at most the top-k call's,
    which adds its slices' partial results); 0 for S < 1, for negative rows and without a context."""
    lib = library()
    h = host_ctx(lib, k)
    try:
        for s in (1, 2, 7):
            rank, cells, topk = (int(getattr(lib, f)(h, B, s)) for f in
                                 (SIZE, "spmf_cells_scratch_bytes", "spmf_topk_scratch_bytes"))
            bitmap = B * ((D + 31) // 32) * 4
            assert rank % 256 == 0 and cells + bitmap <= rank <= cells + bitmap + 255 and rank <= topk
        assert int(lib.spmf_rank_scratch_bytes(h, B, 0)) == 0
        assert int(lib.spmf_rank_scratch_bytes(h, -1, 2)) == 0
        assert int(lib.spmf_rank_scratch_bytes(None, B, 2)) == 0
    finally:
        lib.spmf_ctx_destroy(h)


# ---- heldout.rank_summary ----------------------------------------------------------------------

def test_rank_summary_hand_case():
    from spmf_amd.heldout import rank_summary
    rank = torch.tensor([0, 3, -1, 9], dtype=torch.int32)
    cand = torch.tensor([10, 10, 0, 10], dtype=torch.int32)
    out = rank_summary(rank, cand, (1, 5))
    assert set(out) == {"n", "n_excluded", "hit_rate", "mrr", "auc"}
    assert out["n"] == 3 and out["n_excluded"] == 1
    assert set(out["hit_rate"]) == {1, 5}
    assert out["hit_rate"][1] == 1 / 3 and out["hit_rate"][5] == 2 / 3
    assert abs(out["mrr"] - (1 + 1 / 4 + 1 / 10) / 3) <= 1e-15
    assert abs(out["auc"] - (1 + 0.7 + 0.1) / 3) <= 1e-15
    assert rank_summary(rank.numpy(), cand.numpy(), (1, 5)) == out               # numpy in
    assert rank_summary(rank, cand, 5)["hit_rate"] == {5: 2 / 3}                 # a single cut-off


def test_rank_summary_auc_leaves_out_cells_without_other_candidates():
    from spmf_amd.heldout import rank_summary
    out = rank_summary([0, 0, 2], [0, 4, 4], (1,))
    assert out["n"] == 3 and out["n_excluded"] == 0 and out["hit_rate"][1] == 2 / 3
    assert out["auc"] == (1.0 + 0.5) / 2
    assert abs(out["mrr"] - (1 + 1 + 1 / 3) / 3) <= 1e-15


def test_rank_summary_does_not_depend_on_the_order_of_the_list():
    from spmf_amd.heldout import rank_summary
    rng = np.random.default_rng(5)
    cand = rng.integers(0, 20_000, size=26_000)
    rank = np.where(cand > 0, rng.integers(0, np.maximum(cand, 1) + 1), 0)
    rank[::13] = -1
    one = rank_summary(torch.as_tensor(rank), torch.as_tensor(cand))
    assert one["n"] == 24_000 and one["n_excluded"] == 2_000 and 0.0 < one["auc"] < 1.0 and 0.0 < one["mrr"] < 1.0
    assert sorted(one["hit_rate"]) == [1, 5, 10, 20, 50]
    for seed in (1, 2, 3):
        p = np.random.default_rng(seed).permutation(rank.size)
        assert rank_summary(torch.as_tensor(rank[p]), torch.as_tensor(cand[p])) == one


def test_rank_summary_of_an_empty_list_and_of_unranked_cells():
    from spmf_amd.heldout import rank_summary
    for rank, cand, excl in (([], [], 0), ([-1, -1], [0, 0], 2)):
        out = rank_summary(torch.tensor(rank, dtype=torch.int32), torch.tensor(cand, dtype=torch.int32), (1, 5))
        assert out["n"] == 0 and out["n_excluded"] == excl
        assert math.isnan(out["mrr"]) and math.isnan(out["auc"])
        assert set(out["hit_rate"]) == {1, 5} and all(math.isnan(v) for v in out["hit_rate"].values())
    with pytest.raises(ValueError):
        rank_summary([0, 1], [3])


# ---- the method's argument checks ---------------------------------------------------------------

def test_bad_lists_raise_value_error_without_a_device():
    m, x, draws = cpu_model()
    data = {"counts": x}
    with pytest.raises(ValueError, match="1-D"):
        m.rank_cells(data, np.zeros((2, 1), dtype=np.int64), [1, 5], draws=draws)
    with pytest.raises(ValueError, match="integers"):
        m.rank_cells(data, [0, 3], [1.0, 5.0], draws=draws)
    with pytest.raises(ValueError, match="equal length"):
        m.rank_cells(data, [0, 3], [1], draws=draws)
    for rows, cols in (([0, 8], [0, 1]), ([0, -1], [0, 1]), ([0, 1], [6, 1]), ([0, 1], [3, -1])):
        with pytest.raises(ValueError, match="must lie in"):
            m.rank_cells(data, rows, cols, draws=draws)
    with pytest.raises(ValueError, match="ONE batch"):
        m.rank_cells([data], [0], [1], draws=draws)
    with pytest.raises(ValueError, match="ONE batch"):
        m.rank_cells(lambda: iter([data]), [0], [1], draws=draws)
    with pytest.raises(ValueError, match="cut-offs"):
        m.rank_cells(data, [0], [1], k=(1, 0), draws=draws)


def test_a_valid_list_on_a_cpu_model_fails_like_top_k():
    """Past the argument checks the call needs the library's context, as top_k does: the same failure, and not a
    ValueError."""
    m, x, draws = cpu_model()
    with pytest.raises(Exception) as e_topk:
        m.top_k({"counts": x}, k=3, draws=draws)
    with pytest.raises(Exception) as e_rank:
        m.rank_cells({"counts": x}, [0, 3], [1, 5], draws=draws)
    assert type(e_rank.value) is type(e_topk.value), (e_rank.value, e_topk.value)
    assert not isinstance(e_rank.value, ValueError)


def test_score_cells_keeps_its_error_messages():
    """The two methods share their list handling; each names itself."""
    m, x, draws = cpu_model()
    with pytest.raises(ValueError, match=r"^score_cells: rows must be 1-D, got shape \(2, 1\)$"):
        m.score_cells({"counts": x}, np.zeros((2, 1), dtype=np.int64), [1, 5], draws=draws)
    with pytest.raises(ValueError, match=r"^score_cells: rows, cols and values must have equal length, got 2, 2, 1$"):
        m.score_cells({"counts": x}, [0, 3], [1, 5], values=[1.0], draws=draws)
    with pytest.raises(ValueError, match=r"^score_cells: cols must lie in \[0, 6\), got 1 \.\. 6$"):
        m.score_cells({"counts": x}, [0, 3], [1, 6], draws=draws)
    with pytest.raises(ValueError, match=r"^score_cells takes ONE batch"):
        m.score_cells([{"counts": x}], [0], [1], draws=draws)
    with pytest.raises(ValueError, match=r"^rank_cells: cols must lie in \[0, 6\), got 1 \.\. 6$"):
        m.rank_cells({"counts": x}, [0, 3], [1, 6], draws=draws)
