"""CPU-side tests of the silhouette (PoissonFactorization.silhouette, spmf_silhouette,
csrc/silhouette.hip): the two entry points in the header, the export list and the binding, the methods on the class
surface, every argument check of the methods before a library call, the raw entry's refusals through a ctypes call
with dummy aligned addresses, and the scratch size.  (The valid calls: tests/test_gpu_silhouette.py.)"""
import inspect

import numpy as np
import pytest
import torch

from _silhouette_cases import assert_silhouette_errors
from _stream_cases import K, assert_declared_exported_bound, cpu_model, host_ctx, library, no_library

HEADER_ARGS = {"spmf_silhouette_scratch_bytes": 4, "spmf_silhouette": 16}


def test_entry_points_are_declared_exported_and_bound():
    lib = library()
    for name, nargs in HEADER_ARGS.items():
        assert_declared_exported_bound(name, nargs)
        assert callable(getattr(lib, name)), name
    assert lib.spmf_version() == 6


def test_methods_and_signatures_on_all_three_classes():
    from spmf_amd import BernoulliFactorization, MixedFactorization, PoissonFactorization
    E = inspect.Parameter.empty
    want = {"silhouette": [("points", E), ("labels", E), ("n_clusters", None), ("metric", "euclidean")]}
    for cls in (PoissonFactorization, BernoulliFactorization, MixedFactorization):
        for name, params in want.items():
            fn = getattr(cls, name, None)
            assert callable(fn), (cls.__name__, name)
            got = [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]
            assert got == params, (cls.__name__, name, got)
        doc = cls.silhouette.__doc__
        assert "N^2" in doc and "2^-24" in doc and "coarse" in doc, "the docstring states the cost and the accuracy"


def test_every_argument_check_raises_before_a_library_call(monkeypatch):
    m = cpu_model()[0]
    no_library(monkeypatch)
    pts = torch.zeros(9, 3)
    lab = np.zeros(9, dtype=np.int64)
    # the labels: length, dtype, shape, range
    for bad in (np.zeros(8, dtype=np.int64), np.zeros(10, dtype=np.int32), torch.zeros(0, dtype=torch.int64)):
        with pytest.raises(ValueError, match="one entry per row"):
            m.silhouette(pts, bad)
    for bad in (np.zeros(9), torch.zeros(9), np.zeros(9, dtype=bool)):
        with pytest.raises(ValueError, match="integers"):
            m.silhouette(pts, bad)
    with pytest.raises(ValueError, match="1-D"):
        m.silhouette(pts, np.zeros((9, 1), dtype=np.int64))
    for bad, g in ((np.array([-2] + [0] * 8), None), (np.full(9, 3), 3), (np.arange(9), 8), (np.full(9, -5), 4)):
        with pytest.raises(ValueError, match="labels must lie in"):
            m.silhouette(pts, bad, g)
    with pytest.raises(ValueError, match="n_clusters must be at least 1"):
        m.silhouette(pts, np.full(9, -1))                 # max + 1 = 0
    for g in (0, -1):
        with pytest.raises(ValueError, match="n_clusters must be at least 1"):
            m.silhouette(pts, np.full(9, -1), g)
    for g in (True, 2.0, "3"):
        with pytest.raises(ValueError, match="n_clusters must be an integer"):
            m.silhouette(pts, lab, g)
    with pytest.raises(ValueError, match="at most 65536"):
        m.silhouette(pts, lab, 65537)
    with pytest.raises(ValueError, match="at most 65536"):
        m.silhouette(pts, np.full(9, 65536))
    # the metric
    for metric in ("l2", "Euclidean", None, 0):
        with pytest.raises(ValueError, match="metric"):
            m.silhouette(pts, lab, metric=metric)
    # the points
    with pytest.raises(ValueError, match="torch tensor"):
        m.silhouette(np.zeros((9, 3), dtype=np.float32), lab)
    with pytest.raises(ValueError, match="2-D"):
        m.silhouette(torch.zeros(9), lab)
    with pytest.raises(ValueError, match="float32"):
        m.silhouette(pts.double(), lab)
    with pytest.raises(ValueError, match="width"):
        m.silhouette(torch.zeros(9, 257), lab)
    with pytest.raises(ValueError, match="width"):
        m.silhouette(torch.zeros(9, 0), lab)
    with pytest.raises(ValueError, match="device"):
        m.silhouette(pts, lab)                            # host memory is never handed to the library
    with pytest.raises(ValueError, match="device"):
        m.silhouette(pts, lab, 2, metric="cosine")


def test_raw_errors_return_before_any_device_call():
    """A context of spmf_ctx_create and dummy aligned addresses: no call here is valid, so nothing may be
    launched or dereferenced."""
    lib = library()
    h = host_ctx(lib, K)
    try:
        n, G, row_len = 70, 5, 33
        need = int(lib.spmf_silhouette_scratch_bytes(h, n, G, row_len))
        assert need > 0 and need % 256 == 0
        good = dict(h=h, x=0x1000000, n=n, row_len=row_len, labels=0x2000000, G=G, flags=0, sil=0x3000000,
                    a=0x4000000, b=0x5000000, nearest=0x6000000, sums=0x7000000, counts=0x9000000, ptr=0x8000000,
                    nbytes=need, stream=None)
        assert_silhouette_errors(lib, good, need)
    finally:
        lib.spmf_ctx_destroy(h)


def test_scratch_size():
    """0 for arguments the call refuses, else a positive multiple of 256 that holds the padded working rows, their
    biases and the ordering, and does not shrink as the rows grow."""
    lib = library()
    h = host_ctx(lib, K)
    try:
        for bad in ((-1, 5, 8), (2 ** 31 - 63, 5, 8), (5, 0, 8), (5, 65537, 8), (5, 5, 0), (5, 5, 257)):
            assert int(lib.spmf_silhouette_scratch_bytes(h, *bad)) == 0, bad
        assert int(lib.spmf_silhouette_scratch_bytes(None, 5, 5, 8)) == 0
        assert int(lib.spmf_silhouette_scratch_bytes(h, 0, 1, 1)) > 0
        for G, row_len, kp in ((1, 1, 4), (5, 33, 64), (64, 8, 8), (1000, 256, 256), (65536, 16, 16)):
            last = 0
            for n in (0, 1, 63, 64, 65, 1000, 4096, 32704, 32768, 32769, 65536, 10 ** 6, 10 ** 6 + 1, 2 ** 31 - 64):
                need = int(lib.spmf_silhouette_scratch_bytes(h, n, G, row_len))
                slots = (n + 63) // 64 * 64 + 64 * G          # every cluster in whole 64-row blocks
                assert need % 256 == 0 and need >= slots * (kp + 2) * 4 + n * 8, (n, G, row_len)
                assert need >= last, (n, G, row_len, need, last)
                last = need
    finally:
        lib.spmf_ctx_destroy(h)
