"""CPU-side tests of group_means (PoissonFactorization.group_means, spmf_group_sums, csrc/groups.hip) and of
spmf_amd.groups: the method's argument checks on a CPU-only model, the error contract of the entry through raw ctypes --
all refused before anything touches a device -- the scratch size, and contrast / observed against numpy
restatements written here.  (Declared / exported / bound and the method on the classes: the "groups" row of
tests/test_stream_host.py; the valid call: tests/test_gpu_groups.py.)"""
import os

import numpy as np
import pytest
import torch

from _stream_cases import B, D, ENTRIES, S, assert_shared_errors, cpu_model, host_ctx, host_good_call, library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL, SIZE = ENTRIES["groups"].call, ENTRIES["groups"].size
G = 4


def test_symbols_are_in_the_built_library():
    lib = library()
    assert callable(getattr(lib, CALL)) and callable(getattr(lib, SIZE))
    assert lib.spmf_version() == 6


def test_shared_and_own_errors_return_before_any_device_call():
    """The dummy-address call of _stream_cases.host_good_call (K = 3, D = 45, 70 empty rows, G = 4, four
    columns): the draw stage's error cases (_stream_cases.assert_shared_errors) and the entry's own are refused
    with their codes before the empty returns; nothing here is a valid call with work to do, so nothing may be
    launched or dereferenced."""
    lib = library()
    good, need, no_u, raw, cleanup = host_good_call(lib, "groups")
    h, cs = good["h"], good["ct"]
    assert good["G"] == G and need == int(lib.spmf_groups_scratch_bytes(h, B, S, G, 4))
    try:
        call = assert_shared_errors(lib, "groups", good, need, no_u, raw)
        # the entry's own
        assert call(G=0) == -1 and call(G=-3) == -1
        assert "n_groups" in lib.spmf_last_error(h).decode()
        assert call(n=-1) == -1 and call(n=D + 1) == -1
        assert "n_cols" in lib.spmf_last_error(h).decode()
        assert call(cols=None) == -1 and call(cols=None, n=D - 1) == -1 and call(cols=None, n=0) == -1, \
            "no list: n_cols must be D"
        assert call(labels=None) == -1 and call(sum=None) == -1, "no labels / sum_out with work to do"
        assert "sum_out" in lib.spmf_last_error(h).decode()
        # errors come before the empty returns
        empty = type(cs).from_buffer_copy(cs)
        empty.n_rows = 0
        need_n0 = int(lib.spmf_groups_scratch_bytes(h, B, S, G, 0))
        need_b0 = int(lib.spmf_groups_scratch_bytes(h, 0, S, G, 4))
        assert call(n=0, nbytes=need_n0 - 256) == -3 and call(ct=empty, nbytes=need_b0 - 256) == -3
        assert call(ct=empty, G=0) == -1 and call(n=0, G=0) == -1
        assert call(ct=empty, n=D + 1) == -1 and call(ct=empty, cols=None) == -1
        assert call(n=0, S=0) == -1 and call(n=0, ptr=good["ptr"] + 4) == -1
        # the empty cases are served without a launch: no pointer here could be dereferenced
        assert call(n=0) == 0 and call(n=0, labels=None, sum=None, nz=None) == 0
        needD = int(lib.spmf_groups_scratch_bytes(h, 0, S, G, D))
        assert call(ct=empty) == 0 and call(ct=empty, cols=None, n=D, nbytes=needD) == 0
        assert call(ct=empty, sum=None, labels=None) == 0, "an empty batch"
    finally:
        cleanup()


@pytest.mark.parametrize("k", [3, 16, 64, 128])
def test_scratch_size(k):
    """0 for bad arguments; a multiple of 256; non-decreasing in the rows and in S; at least the draw carve
    (spmf_embed_scratch_bytes); the same on a second context."""
    lib = library()
    h, h2 = host_ctx(lib, k), host_ctx(lib, k)
    try:
        size = lambda hh, rows, s, g=G, n=D: int(lib.spmf_groups_scratch_bytes(hh, rows, s, g, n))   # noqa: E731
        for g, n in ((1, D), (G, D), (G, 7), (300, 1), (G, 0)):
            prev_rows = 0
            for rows in (0, 1, 63, 64, 65, B, 1000, 1025, 5000, 100000):
                prev_s = 0
                for s in (1, 2, 7, 8, 9, 64):
                    v = size(h, rows, s, g, n)
                    assert v > 0 and v % 256 == 0, (rows, s, g, n, v)
                    assert v >= int(lib.spmf_embed_scratch_bytes(h, rows, s)), (rows, s, g, n)
                    assert v >= prev_s, ("S", rows, s, g, n)
                    assert v == size(h2, rows, s, g, n)
                    prev_s = v
                v2 = size(h, rows, 2, g, n)
                assert v2 >= prev_rows, ("rows", rows, g, n)
                prev_rows = v2
        # the partial sums are bounded: a million rows x all columns x 64 draws stays below z twice over + 1 GiB
        kp = int(lib.spmf_padded_k(h))
        big = size(h, 1 << 20, 64, 12, D)
        assert big <= int(lib.spmf_embed_scratch_bytes(h, 1 << 20, 64)) + 64 * ((1 << 20) + 64 * 13) * kp * 4 \
            + (1 << 30), big
        for bad in ((-1, 2, G, D), (B, 0, G, D), (B, 2, 0, D), (B, 2, -1, D), (B, 2, G, -1), (B, 2, G, D + 1)):
            assert size(h, *bad) == 0, bad
        assert int(lib.spmf_groups_scratch_bytes(None, B, 2, G, D)) == 0
    finally:
        lib.spmf_ctx_destroy(h)
        lib.spmf_ctx_destroy(h2)


@pytest.mark.parametrize("k,d,g,n,s,lo,hi", [
    (16, 45, 4, 45, 2, 261_000, 263_000),        # one column block: 4096 runs, RB 1 -> 2 at 4097 row blocks
    (64, 4096, 12, 4096, 1, 3_000, 4_000),       # 64 column blocks: 64 runs, RB 1 -> 2 at 65 row blocks
    (64, 4096, 12, 64, 8, 261_000, 263_000),     # a listed panel of 64 columns of D = 4096
    (3, 45, 300, 45, 3, 0, 2_000),               # more groups than row blocks
])
def test_scratch_size_never_drops_as_the_rows_grow(k, d, g, n, s, lo, hi):
    """Every row count of a range that crosses a step of the run length RB (where the number of runs, ceil(NB /
    RB), falls to about half): the size must not fall with it; and every row count up to three run lengths."""
    lib = library()
    h = host_ctx(lib, k, d=d)
    try:
        for a, b in ((lo, hi), (0, 300)):
            prev = 0
            for rows in range(a, b + 1):
                v = int(lib.spmf_groups_scratch_bytes(h, rows, s, g, n))
                assert v >= prev, (rows, v, prev)
                prev = v
    finally:
        lib.spmf_ctx_destroy(h)


# ---- the method's argument checks ---------------------------------------------------------------

def test_bad_labels_raise_value_error_without_a_device():
    m, x, draws = cpu_model()
    data = {"counts": x}
    lab = np.array([0, 1, 2, -1, 0, 1, 2, 2])
    with pytest.raises(ValueError, match="one entry per row, got 7 for 8"):
        m.group_means(data, lab[:7], draws=draws)
    with pytest.raises(ValueError, match="one entry per row, got 8 for 16"):
        m.group_means([data, {"counts": x.copy()}], lab, draws=draws)
    with pytest.raises(ValueError, match="one entry per row, got 8 for 16"):
        m.group_means(lambda: iter([data, {"counts": x.copy()}]), lab, draws=draws)      # a factory: counted first
    with pytest.raises(ValueError, match="1-D"):
        m.group_means(data, lab.reshape(4, 2), draws=draws)
    with pytest.raises(ValueError, match="integers"):
        m.group_means(data, lab.astype(np.float32), draws=draws)
    with pytest.raises(ValueError, match="integers"):
        m.group_means(data, torch.as_tensor(lab > 0), draws=draws)
    bad = lab.copy()
    bad[3] = -2
    with pytest.raises(ValueError, match=r"must lie in \[-1, 3\)"):
        m.group_means(data, bad, draws=draws)
    with pytest.raises(ValueError, match=r"must lie in \[-1, 2\)"):
        m.group_means(data, lab, n_groups=2, draws=draws)
    with pytest.raises(ValueError, match="n_groups must be at least 1"):
        m.group_means(data, lab, n_groups=0, draws=draws)
    with pytest.raises(ValueError, match="n_groups must be at least 1"):
        m.group_means(data, np.full(8, -1), draws=draws)          # max(labels) + 1 == 0
    with pytest.raises(ValueError, match=r"cols must lie in \[0, 6\)"):
        m.group_means(data, lab, cols=[0, 6], draws=draws)


def test_output_cap_points_at_cols():
    m, x, draws = cpu_model()
    lab = np.zeros(8, dtype=np.int64)
    cap = m._GROUP_OUT_CAP
    g = cap // (2 * 6 * 8) + 1                 # S * G * C * 8 just above the cap
    with pytest.raises(ValueError, match="cols"):
        m.group_means({"counts": x}, lab, n_groups=g, draws=draws)
    with pytest.raises(ValueError, match="cols"):
        m.group_means({"counts": x}, lab, n_groups=cap // (32 * 6 * 8) + 1, nsamples=32)


def test_custom_codec_raises_after_the_argument_checks():
    m, x, draws = cpu_model(encoder_function=lambda t: t, decoder_function=lambda t: t)
    lab = np.zeros(8, dtype=np.int64)
    with pytest.raises(ValueError, match="one entry per row"):
        m.group_means({"counts": x}, lab[:3], draws=draws)
    with pytest.raises(NotImplementedError, match="group_means"):
        m.group_means({"counts": x}, lab, draws=draws)


def test_a_valid_call_on_a_cpu_model_fails_like_top_k():
    m, x, draws = cpu_model()
    with pytest.raises(Exception) as e_topk:
        m.top_k({"counts": x}, k=3, draws=draws)
    with pytest.raises(Exception) as e_grp:
        m.group_means({"counts": x}, np.zeros(8, dtype=np.int64), draws=draws, p_nonzero=True)
    assert type(e_grp.value) is type(e_topk.value), (e_grp.value, e_topk.value)
    assert not isinstance(e_grp.value, ValueError)


def test_scrnaseq_cli_has_the_labels_flag_off_by_default():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "factorize_scrnaseq_counts", os.path.join(ROOT, "bin", "factorize_scrnaseq_counts.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    args = cli.build_parser().parse_args(["--counts", "x_counts.npy"])
    assert args.labels is None and args.group_draws == 32
    assert cli.build_parser().parse_args(["--counts", "x", "--labels", "l.npy"]).labels == "l.npy"


# ---- spmf_amd.groups ------------------------------------------------------------------------------

def _fake_result(rng, S=5, G=4, Cn=6):
    count = np.array([3, 0, 5, 2])[:G]
    sums = rng.gamma(2.0, 1.0, size=(S, G, Cn)) * count[None, :, None]
    return {"sum": torch.as_tensor(sums), "count": torch.as_tensor(count)}, sums, count


def test_contrast_agrees_with_numpy():
    from spmf_amd import groups
    rng = np.random.default_rng(5)
    res, sums, count = _fake_result(rng)
    for a, b, pc, delta in ((0, 2, 1e-3, 1.0), ((0, 3), 2, 0.5, 0.25), (2, (0, 1, 3), 1e-3, 0.1)):
        ia = list(a) if isinstance(a, tuple) else [a]
        ib = list(b) if isinstance(b, tuple) else [b]
        ma = sums[:, ia].sum(1) / count[ia].sum()
        mb = sums[:, ib].sum(1) / count[ib].sum()
        ref = np.log2((ma + pc) / (mb + pc))
        out = groups.contrast(res, a, b, pseudocount=pc, delta=delta)
        np.testing.assert_allclose(out["lfc_draws"].numpy(), ref, rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(out["lfc"].numpy(), ref.mean(0), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(out["sd"].numpy(), ref.std(0, ddof=1), rtol=1e-12, atol=1e-15)
        np.testing.assert_array_equal(out["p_abs_gt"].numpy(), (np.abs(ref) > delta).mean(0))
    # the empty group: NaN fold changes, share 0
    out = groups.contrast(res, 1, 0)
    assert bool(torch.isnan(out["lfc_draws"]).all()) and bool((out["p_abs_gt"] == 0).all())
    one = {"sum": res["sum"][:1], "count": res["count"]}
    assert "sd" not in groups.contrast(one, 0, 2)
    with pytest.raises(ValueError):
        groups.contrast(res, 4, 0)
    with pytest.raises(ValueError):
        groups.contrast(res, (), 0)


def test_observed_agrees_with_numpy():
    import scipy.sparse as sp
    from spmf_amd import groups
    rng = np.random.default_rng(6)
    Bn, Dn, Gn = 23, 9, 4
    x = ((rng.random((Bn, Dn)) < 0.4) * (1 + rng.poisson(3.0, size=(Bn, Dn)))).astype(np.float64)
    lab = rng.integers(-1, Gn, size=Bn)
    lab[lab == 2] = 0                         # group 2 is empty
    lab[:2] = (-1, 3)
    cols = np.array([8, 0, 0, 5])             # a duplicate
    ref_sum, ref_nz = np.zeros((Gn, Dn)), np.zeros((Gn, Dn))
    for b in range(Bn):
        if lab[b] >= 0:
            ref_sum[lab[b]] += x[b]
            ref_nz[lab[b]] += x[b] != 0
    for data in (x, torch.as_tensor(x), sp.csr_matrix(x)):
        for c in (None, cols, torch.as_tensor(cols)):
            out = groups.observed(data, lab, Gn, cols=c)
            sel = slice(None) if c is None else cols
            assert out["sum"].dtype == torch.float64 and out["nonzero"].dtype == torch.float64
            np.testing.assert_array_equal(out["sum"].numpy(), ref_sum[:, sel])
            np.testing.assert_array_equal(out["nonzero"].numpy(), ref_nz[:, sel])
            np.testing.assert_array_equal(out["count"].numpy(), np.bincount(lab[lab >= 0], minlength=Gn))
            assert int(out["count"][2]) == 0 and not bool(out["sum"][2].any())
    with pytest.raises(ValueError):
        groups.observed(x, lab[:5], Gn)
    with pytest.raises(ValueError):
        groups.observed(x, lab, 3)
    with pytest.raises(ValueError):
        groups.observed(x, lab, 0)
