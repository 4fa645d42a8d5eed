"""CPU-side tests of the streaming calls of tests/_stream_cases.py's contract table (waic_streaming with and
without column sums, top_k, score_cells, rank_cells, predict, group_means, embed, top_rows, set_scores): their
entry points in the header, the export list and
the binding, the methods on the class surface, and the part of the C-ABI error contract they share, which is
checked before anything touches a device -- every library call made here fails by contract (the valid call
is tests/test_gpu_stream_abi.py's).  An entry's own argument errors are with its own *_host.py file."""
import pytest

from _stream_cases import (B, ENTRIES, assert_declared_exported_bound, assert_shared_errors, host_ctx, host_good_call,
                           library)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_entry_points_are_declared_exported_and_bound(entry):
    e = ENTRIES[entry]
    for name, nargs in zip((e.size, e.call), e.header_args):
        assert_declared_exported_bound(name, nargs)
    # the table's own arguments are the header's: ctx, counts, S, params, eta | own | scratch, bytes, stream
    assert len(e.own) + 8 == e.header_args[1] and len(e.size_args) + 3 == e.header_args[0], entry


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_method_is_on_all_three_classes(entry):
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        assert callable(getattr(cls, ENTRIES[entry].method, None)), cls.__name__


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_shared_errors_return_before_any_device_call(entry):
    """The dummy-address call of _stream_cases.host_good_call: every shared error case is refused with its
    code; nothing here is a valid call."""
    lib = library()
    good, need, no_u, raw, cleanup = host_good_call(lib, entry)
    try:
        assert_shared_errors(lib, entry, good, need, no_u, raw)
    finally:
        cleanup()


@pytest.mark.parametrize("k", [3, 16, 64, 128])
def test_scratch_sizes_of_the_three_calls(k):
    """waic, topk and cells (the size of every later entry is with its own *_host.py file).  Multiples of 256; the
    cell call's scratch is the draw stage's alone (= the WAIC call's from two draws on), the top-k call adds its
    own buffers; 0 below the smallest S of each."""
    lib = library()
    h = host_ctx(lib, k)
    try:
        for s in (2, 7):
            waic, topk, cells = (int(getattr(lib, ENTRIES[e].size)(h, B, s)) for e in ("waic", "topk", "cells"))
            assert waic > 0 and waic % 256 == 0 and topk % 256 == 0 and cells % 256 == 0
            assert cells == waic and topk >= waic
        assert int(lib.spmf_waic_scratch_bytes(h, B, 1)) == 0 and int(lib.spmf_waic_scratch_bytes(h, B, 0)) == 0
        for name in ("spmf_topk_scratch_bytes", "spmf_cells_scratch_bytes"):
            assert int(getattr(lib, name)(h, B, 0)) == 0
            assert int(getattr(lib, name)(h, B, 1)) > 0 and int(getattr(lib, name)(h, B, 1)) % 256 == 0
    finally:
        lib.spmf_ctx_destroy(h)
