"""CPU-side tests of the three streaming calls (waic_streaming, top_k, score_cells): their entry points
in the header, the export list and the binding, the methods on the class surface, and the part of
the C-ABI error contract they share, which is checked before anything touches a device -- every
library call made here fails by contract (the valid call is tests/test_gpu_stream_abi.py's)."""
import ctypes as C
import fnmatch
import os
import re

import pytest

from _stream_cases import ENTRIES, assert_shared_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# arguments of (scratch size, call) in include/spmf_hip.h
HEADER_ARGS = {"waic": (3, 10), "topk": (3, 12), "cells": (3, 14)}
B, D, K, S = 70, 45, 3, 2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from spmf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def _header_args(hdr, name):
    """Number of arguments of the declaration of `name` in the header."""
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/spmf_hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_entry_points_are_declared_exported_and_bound(entry):
    from spmf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spmf_hip.h")).read(), flags=re.S)
    exports = open(os.path.join(ROOT, "spmf_amd", "csrc", "exports.map")).read()
    exports = re.sub(r"/\*.*?\*/", "", exports, flags=re.S)
    globs = re.search(r"global:\s*([^}]*?)local:", exports, re.S).group(1)
    patterns = [p.strip() for p in globs.split(";") if p.strip()]
    call, size = ENTRIES[entry][:2]
    for name, nargs in zip((size, call), HEADER_ARGS[entry]):
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == _header_args(hdr, name) == nargs, name
    assert "define SPMF_ABI_VERSION 6" in hdr and _lib.ABI_VERSION == 6


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_method_is_on_all_three_classes(entry):
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        assert callable(getattr(cls, ENTRIES[entry][3], None)), cls.__name__


def _ctx(lib, k, flags=0):
    h = C.c_void_p()
    assert lib.spmf_ctx_create(0, k, D, flags, C.byref(h)) == 0
    return h


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_shared_errors_return_before_any_device_call(lib, entry):
    """A context of spmf_ctx_create, a hand-filled descriptor of 70 empty rows and dummy aligned addresses:
    every shared error case is refused with its code; nothing here is a valid call."""
    from spmf_amd import _lib
    from spmf_amd._lib import VAR_ORDER
    h, raw = _ctx(lib, K), _ctx(lib, K, _lib.FLAG_MIXED)
    try:
        cs = _lib.CountsStruct()
        cs.struct_size = C.sizeof(_lib.CountsStruct)
        cs.n_cols, cs.n_rows, cs.nnz, cs.row_ptr = D, B, 0, 0x10000
        slots = {n: 0x100000 * (i + 1) for i, n in enumerate(VAR_ORDER) if n in ("s", "u", "v", "w")}
        need = int(getattr(lib, ENTRIES[entry][1])(h, B, S))
        assert need > 0
        own = {"waic": dict(sums=0x2000000, rows=None),
               "topk": dict(k=5, flags=1, cols=0x2000000, scores=0x3000000),
               "cells": dict(n=4, row=0x2000000, col=0x3000000, val=0x4000000, mean=0x5000000,
                             lppd=0x6000000)}[entry]
        good = dict(h=h, ct=cs, S=S, pin=_lib.PtrArray(*[slots.get(n) for n in VAR_ORDER]), eta=0x7000000,
                    ptr=0x8000000, nbytes=need, stream=None, **own)
        no_u = _lib.PtrArray(*[slots.get(n) if n != "u" else None for n in VAR_ORDER])
        assert_shared_errors(lib, entry, good, need, no_u, raw)
    finally:
        lib.spmf_ctx_destroy(h)
        lib.spmf_ctx_destroy(raw)


@pytest.mark.parametrize("k", [3, 16, 64, 128])
def test_scratch_sizes_of_the_three_calls(lib, k):
    """Multiples of 256; the cell call's scratch is the draw stage's alone (= the WAIC call's from two draws
    on), the top-k call adds its own buffers; 0 below the smallest S of each."""
    h = _ctx(lib, k)
    try:
        for s in (2, 7):
            waic, topk, cells = (int(getattr(lib, ENTRIES[e][1])(h, B, s)) for e in ("waic", "topk", "cells"))
            assert waic > 0 and waic % 256 == 0 and topk % 256 == 0 and cells % 256 == 0
            assert cells == waic and topk >= waic
        assert int(lib.spmf_waic_scratch_bytes(h, B, 1)) == 0 and int(lib.spmf_waic_scratch_bytes(h, B, 0)) == 0
        for name in ("spmf_topk_scratch_bytes", "spmf_cells_scratch_bytes"):
            assert int(getattr(lib, name)(h, B, 0)) == 0
            assert int(getattr(lib, name)(h, B, 1)) > 0 and int(getattr(lib, name)(h, B, 1)) % 256 == 0
    finally:
        lib.spmf_ctx_destroy(h)
