"""GPU: group_means (spmf_group_sums, csrc/groups.hip).

Two references.  (1) The fp64 oracle: O.log_likelihood_components(...)["rate"] [S,B,D], per draw m_s = rate |
sigmoid(rate) (test_gpu_predict._per_draw), summed by group in numpy.  Every sum[s,g,j] lies within the sum over
the group's rows of the per-cell bar of test_gpu_predict._bar, bar(v) = 1e-5 |v| + 1e-5 max|m| with the maximum
over all per-draw cells of the problem -- on a mixed problem over the cells of the column's own type, which is
the same bar on the Poisson columns and a narrower one on the Bernoulli columns: with the maximum over all cells
(279 .. 1.1e5 on these problems, beside Bernoulli cells <= 1) the oracle's own sums on the Bernoulli columns are
only 0.9 .. 5.9 times their bar and the comparison would say nothing there; sum_nonzero within the summed per-cell bound of
test_gpu_predict._pnz_view, exp(-r) (1e-5 |r| + 1e-5 max|r|) + 2^-22, on that file's damped problems.  That every
non-empty group's sum exceeds ten times its bar is asserted on the oracle first.  (2) The cells of predict:
predict(draws = draw s alone)["mean"] has the bits of m_s (S = 1: 0 + m_s, times 1), summed by group in numpy
fp64.  sum[s] equals it within 1e-12 * sum |m|: an fp64 reordering of at most 131 addends moves a sum by at most
131 * 2^-53 = 1.5e-14 relative, any fp32 accumulation by about 1e-7 -- the bound leaves room for the first and
catches the second.  The large case of the peak-memory test has up to 2048 addends: 2048 * 2^-53 = 2.3e-13, still
inside 1e-12."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from _problems import LIKELIHOODS, _dense_model, _dense_problem, build_model, make_problem
from _stream_cases import SHAPES, _bar, _case, _damped_case, _lists

pytestmark = pytest.mark.gpu
T = torch.as_tensor
REL = 1e-12


def _patterns(B):
    """name -> (labels [B] int64, G): the rows of a group are scattered over the batch, so the sort has work."""
    rng = np.random.default_rng(500 + B)
    out = {"one": (np.zeros(B, dtype=np.int64), 1)}
    lab = rng.integers(-1, 5, size=B)
    lab[lab == 3] = 1                                    # group 3 stays empty
    lab[0] = 4                                           # (the largest label is in use: G = 5 by default too)
    out["draw"] = (lab, 5)
    if B == 131:    # a full block, a block edge crossed, a single row, one unlabelled row
        lab = np.concatenate([np.full(64, 0), np.full(65, 1), [2], [-1]])
        out["edges"] = (rng.permutation(lab), 3)
    return out


def _by_group(vals, lab, G):
    """vals [S,B,C] fp64 -> [S,G,C]: the sums over the rows of every group."""
    out = np.zeros((vals.shape[0], G, vals.shape[2]))
    for g in range(G):
        out[:, g] = vals[:, lab == g].sum(axis=1)
    return out


def _route(m, x, params, cols=None):
    """The route of the parent commit: predict one draw at a time.  -> (m_s, -expm1(-r_s) | m_s) as fp64
    [S,B,C] with the bits of the fp32 cells."""
    S = int(params["u"].shape[0])
    ms, pz = [], []
    for s in range(S):
        one = {n: params[n][s:s + 1] for n in ("s", "u", "v", "w")}
        out = m.predict({"counts": x}, cols, draws=one, p_nonzero=True)
        ms.append(out["mean"].cpu().double().numpy())
        pz.append(out["p_nonzero"].cpu().double().numpy())
    return np.stack(ms), np.stack(pz)


@functools.lru_cache(maxsize=None)
def _gcase(lik, B, D, K, S):
    """test_gpu_predict._case plus predict's per-draw cells and the full group_means of every label pattern;
    computed once and shared (read-only)."""
    c = dict(_case(lik, B, D, K, S))
    c["cells"], c["cells_nz"] = _route(c["m"], c["x"], c["params"])
    c["res"] = {name: c["m"].group_means({"counts": c["x"]}, lab, n_groups=G, draws=c["params"], p_nonzero=True)
                for name, (lab, G) in _patterns(B).items()}
    return c


def _i64(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_i64(a), _i64(b))


def _assert_is_sum_of_cells(got, cells, lab, G, what):
    """check 2: got [S,G,C] (device, fp64) against the fp64 sums of predict's cells."""
    ref, mag = _by_group(cells, lab, G), _by_group(np.abs(cells), lab, G)
    got = got.cpu().numpy()
    err = np.abs(got - ref)
    print(f"{what}: max |sum - sum of predict's cells| / sum |m| = "
          f"{float((err / np.maximum(mag, 1e-300)).max()):.3e}")
    assert np.isfinite(got).all() and (err <= REL * mag).all(), (what, float(err.max()))
    return ref


def _check_oracle_and_cells(c, B, S):
    ms, bern = c["ms"], c["bern"]
    # max|m| over the cells of the column's own type: the maximum over all cells unless the problem is mixed
    mmax = np.full(ms.shape[2], float(np.abs(ms).max()))
    if bern.any() and not bern.all():
        mmax = np.where(bern, np.abs(ms[:, :, bern]).max(), np.abs(ms[:, :, ~bern]).max())
        assert mmax.max() == np.abs(ms).max()
    for name, (lab, G) in _patterns(B).items():
        res = c["res"][name]
        assert res["sum"].dtype == torch.float64 and tuple(res["sum"].shape) == (S, G, ms.shape[2])
        ref, bar = _by_group(ms, lab, G), _by_group(_bar(ms, mmax), lab, G)
        filled = np.bincount(lab[lab >= 0], minlength=G) > 0
        assert (ref[:, filled] > 10.0 * bar[:, filled]).all(), name           # on the oracle alone
        got = res["sum"].cpu().numpy()
        err = np.abs(got - ref)
        print(f"{name}: max |sum - oracle| {err.max():.3e}, worst err/bar "
              f"{float((err[:, filled] / bar[:, filled]).max()):.3f}")
        assert (err <= bar).all(), (name, float(err.max()))
        assert (got[:, ~filled] == 0).all(), name
        _assert_is_sum_of_cells(res["sum"], c["cells"], lab, G, name + " sum")
        _assert_is_sum_of_cells(res["sum_nonzero"], c["cells_nz"], lab, G, name + " sum_nonzero")


@pytest.mark.parametrize("B,D,K,S", SHAPES)
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_sums_against_the_oracle_and_predicts_cells(lik, B, D, K, S):
    c = _gcase(lik, B, D, K, S)
    _check_oracle_and_cells(c, B, S)
    bern = c["bern"]
    if bern.any():     # on a Bernoulli column sum_nonzero is the sum itself
        sel = T(np.flatnonzero(bern), device="cuda")
        for res in c["res"].values():
            assert _same(res["sum_nonzero"][:, :, sel], res["sum"][:, :, sel])


@pytest.mark.parametrize("B,D,K,S", SHAPES)
@pytest.mark.parametrize("lik", ["poisson", "mixed", "poisson_log"])
def test_sum_nonzero_against_the_oracle(lik, B, D, K, S):
    """The Poisson columns of the damped problems of test_gpu_predict (poisson_log: its undamped problem)."""
    dc = _case(lik, B, D, K, S) if lik == "poisson_log" else _damped_case(lik, B, D, K, S)
    pois = ~dc["bern"]
    r = dc["rate"][:, :, pois]
    rmax = float(np.abs(r).max())
    cell = -np.expm1(-r)
    bound = np.exp(-r) * (1e-5 * np.abs(r) + 1e-5 * rmax) + 2.0 ** -22
    if lik != "poisson_log":       # the condition on the inputs, on the oracle alone (as test_p_nonzero)
        assert 0.010 <= r.min() and r.max() <= 2.8, (float(r.min()), float(r.max()))
    m = _dense_model(lik, dc["cfg"], dc["mask"], 32)
    for name, (lab, G) in _patterns(B).items():
        res = m.group_means({"counts": dc["x"]}, lab, n_groups=G, draws=dc["params"], p_nonzero=True)
        got = res["sum_nonzero"].cpu().numpy()[:, :, pois]
        ref, bnd = _by_group(cell, lab, G), _by_group(bound, lab, G)
        err = np.abs(got - ref)
        filled = np.bincount(lab[lab >= 0], minlength=G) > 0
        print(f"{lik} {name}: max |sum_nonzero - oracle| {err.max():.3e}, worst err/bound "
              f"{float((err[:, filled] / bnd[:, filled]).max()):.3f}")
        assert (err <= bnd).all(), (name, float(err.max()))
        # the fraction of the group: sum_nonzero / count
        n = np.bincount(lab[lab >= 0], minlength=G).astype(np.float64)
        frac = res["p_nonzero_draws"].cpu().numpy()[:, filled][:, :, pois]
        np.testing.assert_allclose(frac, got[:, filled] / n[filled][None, :, None], rtol=1e-15, atol=0)


@pytest.mark.parametrize("B,D,K,S", SHAPES)
@pytest.mark.parametrize("lik", LIKELIHOODS)
def test_repeats_give_the_same_bits_and_variants_agree(lik, B, D, K, S):
    c = _gcase(lik, B, D, K, S)
    m, x, params = c["m"], c["x"], c["params"]
    data = {"counts": x}
    lists = _lists(D)
    assert len(lists["dup"]) == min(D, 65) and lists["dup"][:3].tolist() == [D - 1, 0, 0]
    if lik == "mixed":   # Bernoulli and Poisson columns side by side inside one 32-lane tile
        for name in ("perm", "dup"):
            b = c["bern"][lists[name]]
            j = np.flatnonzero(b[1:] != b[:-1])
            assert (j // 32 == (j + 1) // 32).any(), name
    for pname, (lab, G) in _patterns(B).items():
        full = c["res"][pname]
        again = m.group_means(data, lab, n_groups=G, draws=params, p_nonzero=True)
        for n in ("sum", "sum_nonzero"):
            assert _same(again[n], full[n]), (pname, n)
        mag = T(_by_group(np.abs(c["cells"]), lab, G), device="cuda")
        mag_nz = T(_by_group(np.abs(c["cells_nz"]), lab, G), device="cuda")

        def close(out, sel, what):
            assert bool(((out["sum"] - full["sum"][:, :, sel]).abs() <= REL * mag[:, :, sel]).all()), (pname, what)
            if "sum_nonzero" in out:
                assert bool(((out["sum_nonzero"] - full["sum_nonzero"][:, :, sel]).abs()
                             <= REL * mag_nz[:, :, sel]).all()), (pname, what)
        for name in ("one", "perm", "dup"):
            cols = lists[name]
            out = m.group_means(data, lab, n_groups=G, cols=cols, draws=params, p_nonzero=True)
            assert out["columns"].dtype == torch.int32 and out["columns"].cpu().tolist() == cols.tolist(), name
            close(out, T(cols, device="cuda"), name)
        plain = m.group_means(data, T(lab, device="cuda"), draws=params)        # torch labels, the default G
        assert "sum_nonzero" not in plain and "p_nonzero" not in plain and "columns" not in plain
        assert int(plain["sum"].shape[1]) == G
        close(plain, slice(None), "no p_nonzero")
        if B > 32:
            close(m.group_means(data, lab, n_groups=G, draws=params, p_nonzero=True, max_rows=32), slice(None),
                  "max_rows")
            h = B // 2 + 3
            two = [{"counts": x[:h].copy()}, {"counts": x[h:].copy()}]
            close(m.group_means(two, lab, n_groups=G, draws=params, p_nonzero=True), slice(None), "two batches")


def test_a_nan_row_makes_its_own_group_nan_and_no_other():
    cfg, x, params = make_problem(37, 23, 3, 3, 913, 0.3)
    m = build_model(cfg, 16)
    lab = np.random.default_rng(4).integers(0, 4, size=37)
    lab[6], G = 2, 4
    assert (lab == 2).sum() > 1 and all((lab == g).any() for g in range(G))
    cols = np.array([22, 11, 0, 11, 5])
    xn = x.copy()
    xn[6, 11] = float("nan")
    others = T([0, 1, 3], device="cuda")
    for cl in (None, cols):
        clean = m.group_means({"counts": x}, lab, n_groups=G, cols=cl, draws=params, p_nonzero=True)
        dirty = m.group_means({"counts": xn}, lab, n_groups=G, cols=cl, draws=params, p_nonzero=True)
        for n in ("sum", "sum_nonzero", "draws", "p_nonzero_draws"):
            assert bool(torch.isfinite(clean[n]).all()), n
            assert bool(torch.isnan(dirty[n][:, 2]).all()), n
            assert _same(dirty[n][:, others], clean[n][:, others]), n
        off = lab.copy()
        off[6] = -1
        clean = m.group_means({"counts": x}, off, n_groups=G, cols=cl, draws=params, p_nonzero=True)
        dirty = m.group_means({"counts": xn}, off, n_groups=G, cols=cl, draws=params, p_nonzero=True)
        for n in ("sum", "sum_nonzero"):
            assert bool(torch.isfinite(dirty[n]).all()) and _same(dirty[n], clean[n]), n


def test_c_abi_margins_no_group_labels_an_outside_column_and_errors():
    """Through ctypes with an exactly sized scratch and outputs pre-filled with 0.5, a margin of -7 behind them:
    body = 0.5 + the sums, the margin and the scratch beyond the need untouched; labels n_groups and -5 are no
    group; the listed column D gives a NaN output column; a scratch 256 bytes short is -3 and writes nothing."""
    from spmf_amd import _lib
    from spmf_amd._lib import VAR_ORDER
    B, D, K, S = 70, 45, 3, 2
    c = _gcase("mixed", B, D, K, S)
    m, x, params = c["m"], c["x"], c["params"]
    lib, h = _lib.load(), m._handle()
    _, cs = m._batch({"counts": x})
    S_, P = m._pack_params(params, names=("s", "u", "v", "w"))
    assert S_ == S
    pin = _lib.PtrArray(*[P[n].data_ptr() if n in P else None for n in VAR_ORDER])
    eta = m._eta_device()
    G = 4                                   # group 3 has no rows
    lab = np.random.default_rng(8).integers(0, 3, size=B)
    lab[5], lab[17], lab[40] = G, -5, -1
    eff = np.where((lab >= 0) & (lab < G), lab, -1)
    labels = T(lab, dtype=torch.int32, device="cuda")
    listed = [3, D, 7, 0, 44, 4, 4]
    Cn = len(listed)
    cols = torch.tensor(listed, dtype=torch.int32, device="cuda")
    need = int(lib.spmf_groups_scratch_bytes(h, int(cs.n_rows), S, G, Cn))
    assert need > 0 and need % 256 == 0
    scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    off = (-scratch.data_ptr()) % 256
    base = scratch.data_ptr() + off
    n_body = S * G * Cn

    def fresh():
        t = torch.full((n_body + 64,), -7.0, dtype=torch.float64, device="cuda")
        t[:n_body] = 0.5
        return t
    outs = {"sum": fresh(), "nz": fresh()}
    stream = torch.cuda.current_stream().cuda_stream

    def call(nbytes=need, n=Cn, lst=cols.data_ptr(), g=G, o=outs):
        return lib.spmf_group_sums(h, C.byref(cs), S, pin, eta.data_ptr(), labels.data_ptr(), g, n, lst,
                                   o["sum"].data_ptr(), o["nz"].data_ptr(), base, nbytes, stream)
    assert call(nbytes=need - 256) == -3
    msg = lib.spmf_last_error(h).decode()
    assert str(need) in msg, msg
    assert call(g=0) == -1 and call(n=D + 1) == -1 and call(n=-1) == -1 and call(lst=None) == -1
    torch.cuda.synchronize()
    for t in outs.values():
        assert bool((t[:n_body] == 0.5).all()) and bool((t[n_body:] == -7.0).all())
    assert not bool(scratch.any())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool(scratch[off + need:].any()) and not bool(scratch[:off].any())
    good = [j for j, d in enumerate(listed) if d < D]
    sel = [listed[j] for j in good]
    for n, cells in (("sum", c["cells"]), ("nz", c["cells_nz"])):
        body, margin = outs[n][:n_body].view(S, G, Cn).cpu().numpy(), outs[n][n_body:]
        assert bool((margin == -7.0).all()), n
        assert np.isnan(body[:, :3, 1]).all() and (body[:, 3] == 0.5).all(), n
        ref, mag = _by_group(cells[:, :, sel], eff, G), _by_group(np.abs(cells[:, :, sel]), eff, G)
        # (the addition onto 0.5 rounds once more: half an ulp of the result)
        err = np.abs(body[:, :, good] - (0.5 + ref))
        assert (err <= REL * mag + 2.0 ** -53 * (0.5 + mag)).all(), (n, float(err.max()))
    # all columns, no list, no nonzero_out: the second output is not touched; a second call accumulates
    wide = {"sum": torch.zeros(S * G * D + 64, dtype=torch.float64, device="cuda"), "nz": fresh()}
    needD = int(lib.spmf_groups_scratch_bytes(h, int(cs.n_rows), S, G, D))
    big = torch.zeros(needD + 256, dtype=torch.uint8, device="cuda")
    bbase = big.data_ptr() + (-big.data_ptr()) % 256
    for _ in range(2):
        assert lib.spmf_group_sums(h, C.byref(cs), S, pin, eta.data_ptr(), labels.data_ptr(), G, D, None,
                                   wide["sum"].data_ptr(), None, bbase, needD, stream) == 0
    torch.cuda.synchronize()
    ref, mag = _by_group(c["cells"], eff, G), _by_group(np.abs(c["cells"]), eff, G)
    body = wide["sum"][:S * G * D].view(S, G, D).cpu().numpy()
    assert (np.abs(body - 2.0 * ref) <= 4.0 * REL * mag).all() and bool((wide["sum"][S * G * D:] == 0).all())
    assert bool((wide["nz"][:n_body] == 0.5).all()) and bool((wide["nz"][n_body:] == -7.0).all())


def test_many_groups_walk_two_column_ranges():
    """600 groups over 1500 rows (two or three rows each, some empty), 400 columns, S = 3, mixed: 624 row blocks in
    312 runs of two, 912 segments, partial sums of 43 776 bytes per column -- all 448 padded columns would need
    19.6 MB, above the 16 MiB budget, so the entry walks the ranges [0, 320) and [320, 400); the offsets scan takes
    three strips of 256 groups.  Against the sums of predict's cells, twice for the bits, and with a list that
    straddles the range edge."""
    from spmf_amd import _lib
    B, D, K, S, G = 1500, 400, 3, 3, 600
    cfg, x, params, mask = _dense_problem("mixed", B, D, K, S, 9900)
    m = _dense_model("mixed", cfg, mask, 256)
    lib, h = _lib.load(), m._handle()
    need_all = int(lib.spmf_groups_scratch_bytes(h, B, S, G, D))
    need_320 = int(lib.spmf_groups_scratch_bytes(h, B, S, G, 320))
    kp = int(lib.spmf_padded_k(h))
    assert need_all - need_320 < 80 * S * (kp + 1) * 4 + 80 + 2 * 256 + (1 << 20), "the partials are capped"
    lab = np.random.default_rng(21).integers(-1, G, size=B)
    cells, cells_nz = _route(m, x, params)
    out = m.group_means({"counts": x}, lab, n_groups=G, draws=params, p_nonzero=True)
    again = m.group_means({"counts": x}, lab, n_groups=G, draws=params, p_nonzero=True)
    for n, c in (("sum", cells), ("sum_nonzero", cells_nz)):
        _assert_is_sum_of_cells(out[n], c, lab, G, n)
        assert _same(out[n], again[n]), n
    cols = np.arange(300, 340)
    part = m.group_means({"counts": x}, lab, n_groups=G, cols=cols, draws=params)
    _assert_is_sum_of_cells(part["sum"], cells[:, :, cols], lab, G, "listed")


def test_wide_k_runs_four_chunks_per_draw():
    """Poisson K = 65 (KP = 128): the wide-K encode sweep and four 32-float K chunks per draw."""
    B, D, K, S = 40, 70, 65, 2
    _check_oracle_and_cells(_gcase("poisson", B, D, K, S), B, S)


def test_peak_memory_stays_below_the_materialised_rates():
    """B = 2048, D = 1024, K = 16, S = 8, six groups, all columns: the peak over the call stays below S*B*D*4
    bytes (64 MiB), the [S,B,D] fp32 rates alone; 64 sampled columns agree with the sums of predict's cells."""
    from spmf_amd.sparse import SparseCounts
    B, D, K, S, G = 2048, 1024, 16, 8, 6
    cfg, x, params, mask = _dense_problem("poisson", B, D, K, S, 9800, density=0.05)
    m = _dense_model("poisson", cfg, mask, 256)
    batch = {"counts": SparseCounts.from_any(x, m.device, 256, latent_dim=K)}
    draws = {n: T(params[n]).to("cuda", torch.float32) for n in ("s", "u", "v", "w")}
    lab = np.random.default_rng(12).integers(-1, G, size=B)
    labels = T(lab, device="cuda")
    m.group_means({"counts": x[:64].copy()}, lab[:64], n_groups=G, draws=draws, p_nonzero=True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = m.group_means(batch, labels, n_groups=G, draws=draws, p_nonzero=True)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"peak above the allocation before the call: {extra / 2**20:.1f} MiB; "
          f"S*B*D*4 = {S * B * D * 4 / 2**20:.1f} MiB")
    assert extra < S * B * D * 4, extra
    cols = np.random.default_rng(3).permutation(D)[:64].copy()
    cells, cells_nz = _route(m, x, draws, cols)
    sel = T(cols, device="cuda")
    _assert_is_sum_of_cells(out["sum"][:, :, sel], cells, lab, G, "sum")
    _assert_is_sum_of_cells(out["sum_nonzero"][:, :, sel], cells_nz, lab, G, "sum_nonzero")


def test_draws_mean_sd_and_count_are_the_moments_of_sum_over_count():
    B, D, K, S = SHAPES[1]
    c = _gcase("poisson_log", B, D, K, S)
    lab, G = _patterns(B)["draw"]
    res = c["res"]["draw"]
    count = torch.bincount(T(lab[lab >= 0]), minlength=G).cuda()
    assert res["count"].dtype == torch.int64 and torch.equal(res["count"], count) and int(count[3]) == 0
    filled = count > 0
    per = res["sum"][:, filled] / count[filled].double()[None, :, None]
    pnz = res["sum_nonzero"][:, filled] / count[filled].double()[None, :, None]
    assert torch.equal(res["draws"][:, filled], per) and torch.equal(res["p_nonzero_draws"][:, filled], pnz)
    torch.testing.assert_close(res["mean"][filled], per.mean(0), rtol=1e-14, atol=0)
    torch.testing.assert_close(res["sd"][filled], per.std(0, unbiased=True), rtol=1e-12, atol=0)
    torch.testing.assert_close(res["p_nonzero"][filled], pnz.mean(0), rtol=1e-14, atol=0)
    for n in ("draws", "mean", "sd", "p_nonzero_draws", "p_nonzero"):
        assert res[n].dtype == torch.float64 and res[n].is_cuda
        assert bool(torch.isnan(res[n][..., 3, :]).all()), n
    assert bool((res["sum"][:, 3] == 0).all())
    # a factory is called twice (count, run); a one-shot iterator is checked as its batches arrive
    x, h = c["x"], B // 2
    for data in (lambda: iter([{"counts": x[:h].copy()}, {"counts": x[h:].copy()}]),
                 iter([{"counts": x[:h].copy()}, {"counts": x[h:].copy()}])):
        two = c["m"].group_means(data, lab, n_groups=G, draws=c["params"])
        mag = T(_by_group(np.abs(c["cells"]), lab, G), device="cuda")
        assert bool(((two["sum"] - res["sum"]).abs() <= REL * mag).all())
    for short, msg in ((lab[:-1], "for at least"), (np.append(lab, 0), f"for {B} rows")):
        with pytest.raises(ValueError, match="one entry per row.*" + msg):
            c["m"].group_means(iter([{"counts": x[:h].copy()}, {"counts": x[h:].copy()}]), short, n_groups=G,
                               draws=c["params"])
    one = {n: c["params"][n][:1] for n in ("s", "u", "v", "w")}
    single = c["m"].group_means({"counts": c["x"]}, lab, n_groups=G, draws=one)
    assert "sd" not in single and tuple(single["draws"].shape) == (1, G, D)
    mag = T(_by_group(np.abs(c["cells"]), lab, G), device="cuda")
    assert bool(((single["sum"][0] - res["sum"][0]).abs() <= REL * mag[0]).all())
