"""What the two test files of the silhouette share (test_silhouette_host.py, test_gpu_silhouette.py): the argument
list of spmf_silhouette, its raw call and its error contract, asserted without a device on dummy addresses and with
one on real buffers."""
import ctypes as C

SIL_ARGS = (("x", C.c_void_p), ("n", C.c_int64), ("row_len", C.c_int), ("labels", C.c_void_p), ("G", C.c_int32),
            ("flags", C.c_uint), ("sil", C.c_void_p), ("a", C.c_void_p), ("b", C.c_void_p), ("nearest", C.c_void_p),
            ("sums", C.c_void_p), ("counts", C.c_void_p), ("ptr", C.c_void_p), ("nbytes", C.c_size_t),
            ("stream", C.c_void_p))


def silhouette_raw_call(good):
    """-> call(**overrides): spmf_silhouette through a binding of its own with the arguments of ``good``."""
    from spmf_amd import _lib
    fn = C.CDLL(_lib.LIB_PATH).spmf_silhouette
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [t for _, t in SIL_ARGS]

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], *[a[n] for n, _ in SIL_ARGS])
    return call


def assert_silhouette_errors(lib, good, need, after=lambda: None):
    """The error contract of spmf_silhouette; every call here returns before a launch or a memset, and ``after``
    is run behind each (the GPU file checks its sentinels there)."""
    call, h = silhouette_raw_call(good), good["h"]

    def refused(code, **kw):
        assert call(**kw) == code, kw
        msg = lib.spmf_last_error(h).decode()
        assert msg.startswith("silhouette: "), msg
        after()
        return msg
    for g in (0, -1, 65537):
        assert "n_clusters" in refused(-1, G=g)
    for w in (0, 257, -1):
        assert "row_len" in refused(-1, row_len=w)
    for rows in (-1, 2 ** 31 - 63, 2 ** 40):
        assert "n_rows" in refused(-1, n=rows)
    for flags in (2, 3, 1 << 31):
        assert "flag" in refused(-1, flags=flags)
    for name in ("x", "labels", "sil", "sums", "counts", "ptr"):
        assert "null" in refused(-1, **{name: None})
    for name in ("sums", "counts", "ptr"):
        refused(-1, n=0, **{name: None})
    assert "aligned" in refused(-1, ptr=good["ptr"] + 4)
    assert str(need) in refused(-3, nbytes=need - 256)
    refused(-3, n=0, nbytes=0)               # errors come before the empty return
    assert call(h=None) == -1
