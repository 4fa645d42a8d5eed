"""GPU: spmf_graph_transform (csrc/graph_transform.hip) and the methods on top (graph_transform, umap_transform).

One epoch against the fp64 restatement ``spmf_amd.graph.transform_reference`` through raw library calls with
sentinels around y_out, both sides from the same fp32 y_in, per row in the units of
``_graph_layout_cases.error_units``:
    |y_gpu - y_ref|_inf <= T 2^-24 (|y_i|_inf + alpha A_i / max(1, W_i)),
A_i the sum of the absolute values of the row's clipped contributions.  T = 8 x the error of a float32 numpy
restatement of the same formulas (tests/_graph_transform_cases.py restate32) against the fp64 reference, measured on
the CPU over the cases of this file: 11.63 units as the largest (Q = 65, k = 17, M = 64, n_ref = 1, min_dist 0.5,
lr 1; 11.62 at Q = 257), so T = 93.0.  The restatement adds a row's terms one after the other, and its largest errors
are the 64 equal repulsive terms of a reference of one or two rows, whose sequential fp32 sum is off by a share of
64 / 2 roundings (at M <= 17 it stays below 5); the factor 8 is, as for the layout, for the hardware's exp2 / log2 at
exponents up to |b log2 d^2| of about 20 and for another order of the additions.
The kernel measured 3.61 units as the largest over the same cases on an MI355X (Q = 257, k = 16, M = 17, n_ref = 2,
min_dist 0.1, lr 1: its sums are trees) and 1.25 on the skip-rule case; the start at most 0.24 of its bar.

The start (y_in = NULL, no epoch) per row: |y0 - ref|_inf <= 2 (k + 2) 2^-24 max_j |y_j|_inf -- a sum of k products of
one sign pattern in the weights, each rounded, and the division by a sum of k weights.

Then bits: the in-register epoch loop against chained one-epoch calls and a split through epoch0, row chunks through
row0 and the independence of a row from the other rows' entries; the skip rules; the error contract with sentinels;
umap_transform against the calls by hand; and the quality on the split blobs, independent of the layout kernel."""
import numpy as np
import pytest
import torch

from _graph_layout_cases import error_units
from _graph_transform_cases import (EPOCH, LRS, N_HEADER_ARGS, QS, TOTAL, assert_graph_transform_errors, blob_split,
                                    curve, graph_transform_raw_call, one_epoch_cases, one_epoch_reference, restate32,
                                    transform_case, transform_quality)
from _problems import _dense_model
from _stream_cases import _problem, assert_declared_exported_bound
from spmf_amd import graph, neighbors

pytestmark = pytest.mark.gpu

T_UNITS = 8 * 11.63
SENTINEL = -7.0


def _model():
    from spmf_amd import PoissonFactorization
    return PoissonFactorization(latent_dim=3, feature_dim=8, initialize_distributions=False, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class _Call:
    """Raw calls on one set of query entries: device copies of the arrays, y_out inside a buffer of sentinels."""

    def __init__(self, m, idx, w, y_ref):
        from spmf_amd import _lib
        self.lib, self.h = _lib.load(), m._handle()
        self.n, self.k = idx.shape
        self.n_ref = len(y_ref)
        self.idx = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int32)).cuda()
        self.w = torch.as_tensor(np.ascontiguousarray(w, dtype=np.float32)).cuda()
        # (one spare row: an empty reference still has an address)
        self.y_ref = torch.zeros(self.n_ref + 1, 2, dtype=torch.float32, device="cuda")
        self.y_ref[:self.n_ref] = torch.as_tensor(np.ascontiguousarray(y_ref, dtype=np.float32).reshape(-1, 2)).cuda()
        self.buf = torch.full((self.n + 16, 2), SENTINEL, dtype=torch.float32, device="cuda")

    def good(self, y, **kw):
        y_in = None
        if y is not None:
            y_in = y if torch.is_tensor(y) else torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32)).cuda()
        a, b = curve(0.1)
        args = dict(h=self.h, n=self.n, k=self.k, idx=self.idx.data_ptr(), w=self.w.data_ptr(),
                    y_ref=self.y_ref.data_ptr(), n_ref=self.n_ref, y_in=y_in.data_ptr() if y_in is not None else None,
                    y_out=self.buf[8:].data_ptr(), row0=0, epoch0=EPOCH, n_epochs=1, total=TOTAL, lr=1.0, a=a, b=b,
                    gamma=1.0, rate=5.0, M=8, seed=0, stream=torch.cuda.current_stream().cuda_stream, keep=y_in)
        args.update(kw)
        return args

    def untouched(self):
        return bool((self.buf[:8] == SENTINEL).all()) and bool((self.buf[8 + self.n:] == SENTINEL).all())

    def run(self, y, alias=False, **kw):
        """-> y_out float32 [n, 2] (a copy).  ``alias``: y_in is y_out."""
        self.buf.fill_(SENTINEL)
        if alias:
            self.buf[8:8 + self.n] = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32)).cuda()
            args = self.good(self.buf[8:8 + self.n], **kw)
            args["y_in"] = args["y_out"]
        else:
            args = self.good(y, **kw)
        rc = graph_transform_raw_call(args)()
        assert rc == 0, self.lib.spmf_last_error(self.h).decode()
        torch.cuda.synchronize()
        assert self.untouched(), "a write outside y_out"
        return self.buf[8:8 + self.n].clone()


@pytest.mark.parametrize("Q", QS)
def test_one_epoch_against_the_reference(Q):
    m = _model()
    worst, soft_worst = (-1.0, None), (-1.0, None)
    for k, M, n_ref, md in one_epoch_cases(Q):
        a, b = curve(md)
        c = transform_case(Q, k, M, n_ref, md)
        call = _Call(m, c["idx"], c["w"], c["y_ref"])
        for lr in LRS:
            ref, A, W, alpha = one_epoch_reference(c, M, md, lr)
            got = call.run(c["y_in"], lr=lr, a=a, b=b, M=M).cpu().numpy()
            assert np.isfinite(got).all()
            units = error_units(got, ref, c["y_in"], alpha, A, W)
            soft = error_units(restate32(c["idx"], c["w"], c["y_ref"], c["y_in"], 0, EPOCH, TOTAL, lr, a, b, 1.0, 5.0,
                                         M, 0), ref, c["y_in"], alpha, A, W)
            if units > worst[0]:
                worst = (units, (k, M, n_ref, md, lr))
            if soft > soft_worst[0]:
                soft_worst = (soft, (k, M, n_ref, md, lr))
    print(f"graph_transform Q={Q}: kernel {worst[0]:.2f} units at (k, M, n_ref, min_dist, lr) = {worst[1]}, float32 "
          f"restatement {soft_worst[0]:.2f} at {soft_worst[1]}, bar {T_UNITS:.1f}")
    assert worst[0] <= T_UNITS, worst


@pytest.mark.parametrize("Q", [1, 17, 257])
def test_start_is_the_weighted_mean(Q):
    m = _model()
    for k, n_ref in ((1, 1), (15, 300), (16, 2), (17, 300), (48, 300), (64, 300)):
        c = transform_case(Q, k, 8, n_ref)
        w = c["w"].copy()
        if Q > 2:
            w[Q // 2] = 0.0                                    # a row without a valid entry
        call = _Call(m, c["idx"], w, c["y_ref"])
        got = call.run(None, epoch0=0, n_epochs=0).cpu().numpy()
        ref = graph.transform_reference(c["idx"], w, c["y_ref"], None, 0, 0, 0, TOTAL, 1.0, *curve(0.1))
        has = np.ones(Q, dtype=bool)
        if Q > 2:
            has[Q // 2] = False
            assert np.isnan(got[Q // 2]).all() and np.isnan(ref[Q // 2]).all()
        bar = 2 * (k + 2) * 2.0 ** -24 * np.abs(c["y_ref"][c["idx"]]).max((1, 2))
        err = np.abs(got.astype(np.float64) - ref).max(1)
        print(f"graph_transform start Q={Q} k={k} n_ref={n_ref}: {float((err[has] / bar[has]).max()):.3f} of the bar")
        assert (err[has] <= bar[has]).all(), (k, n_ref, float((err[has] / bar[has]).max()))
        # the start followed by epochs is the epochs from that start
        e3 = call.run(None, epoch0=0, n_epochs=3, M=5)
        assert torch.equal(_bits(e3), _bits(call.run(got, epoch0=0, n_epochs=3, M=5)))


def test_epoch_loop_bits():
    """7 epochs in one launch, 7 one-epoch calls chained through y_out, and the split 3 + 4 by epoch0."""
    m = _model()
    for Q, k, M, n_ref in ((257, 15, 5, 300), (65, 64, 64, 300), (17, 17, 17, 2)):
        c = transform_case(Q, k, M, n_ref, seed=3, epoch=0)
        call = _Call(m, c["idx"], c["w"], c["y_ref"])
        kw = dict(total=7, M=M, seed=3 + (9 << 32), lr=0.7)
        whole = call.run(c["y_in"], epoch0=0, n_epochs=7, **kw)
        assert bool(torch.isfinite(whole).all())
        assert torch.equal(_bits(whole), _bits(call.run(c["y_in"], epoch0=0, n_epochs=7, **kw))), "two calls, one result"
        y = torch.as_tensor(c["y_in"]).cuda()
        for e in range(7):
            y = call.run(y, epoch0=e, n_epochs=1, **kw)
        assert torch.equal(_bits(whole), _bits(y)), "7 one-epoch calls are the 7 epochs of one launch"
        part = call.run(c["y_in"], epoch0=0, n_epochs=3, **kw)
        assert not torch.equal(_bits(part), _bits(whole))
        assert torch.equal(_bits(whole), _bits(call.run(part, epoch0=3, n_epochs=4, **kw))), "3 + 4 epochs"
        assert torch.equal(_bits(whole), _bits(call.run(c["y_in"], alias=True, epoch0=0, n_epochs=7, **kw))), "y_out = y_in"
        assert not torch.equal(_bits(whole), _bits(call.run(c["y_in"], epoch0=0, n_epochs=7, **dict(kw, seed=4))))
        # no epoch: y_in is copied, and left alone in place
        y_in = torch.as_tensor(c["y_in"]).cuda()
        assert torch.equal(_bits(call.run(c["y_in"], epoch0=4, n_epochs=0, **kw)), _bits(y_in))
        assert torch.equal(_bits(call.run(c["y_in"], alias=True, epoch0=7, n_epochs=0, **kw)), _bits(y_in))
        # the whole schedule against fp64: the error of 7 epochs stays a small multiple of one epoch's
        a, b = curve(0.1)
        ref = graph.transform_reference(c["idx"], c["w"], c["y_ref"], c["y_in"], 0, 0, 7, 7, 0.7, a, b, 1.0, 5.0, M,
                                        3 + (9 << 32))
        assert np.abs(whole.cpu().numpy() - ref).max() <= 1e-3 * max(1.0, np.abs(ref).max())


def test_rows_are_independent_and_chunks_keep_the_bits():
    m = _model()
    Q, k, M, n_ref = 100, 15, 8, 300
    c = transform_case(Q, k, M, n_ref)
    kw = dict(epoch0=0, n_epochs=5, total=5, M=M, seed=21)
    for start in (c["y_in"], None):
        def part(lo, hi, row0):
            sub = None if start is None else start[lo:hi]
            return _Call(m, c["idx"][lo:hi], c["w"][lo:hi], c["y_ref"]).run(sub, row0=row0, **kw)
        whole = part(0, Q, 0)
        assert torch.equal(_bits(whole), _bits(torch.cat([part(0, 37, 0), part(37, Q, 37)]))), "chunks through row0"
        assert not torch.equal(_bits(whole[37:]), _bits(part(37, Q, 0))), "row0 numbers the draws"
        # the other rows' entries replaced by garbage: rows g keep their bits
        keep = np.array([0, 15, 16, 17, 50, 99])
        rng = np.random.default_rng(6)
        idx = rng.integers(-5, n_ref + 5, size=(Q, k)).astype(np.int32)
        w = rng.standard_normal((Q, k)).astype(np.float32) * 1e3
        idx[keep], w[keep] = c["idx"][keep], c["w"][keep]
        y = None
        if start is not None:
            y = (rng.standard_normal((Q, 2)) * 50).astype(np.float32)
            y[keep] = start[keep]
        other = _Call(m, idx, w, c["y_ref"]).run(y, **kw)
        assert torch.equal(_bits(whole[keep]), _bits(other[keep]))
        assert not torch.equal(_bits(whole), _bits(other))


def test_skip_rules():
    """Entries with index -1 / n_ref / INT32_MIN, with weight NaN / inf / 0 / negative and a neighbour at a
    non-finite reference position: the result is the reference's under the same rules; a row whose every entry is
    skipped and a NaN row keep their bits; an empty reference is read nowhere."""
    m = _model()
    Q, k, M, n_ref = 65, 17, 5, 300
    c = transform_case(Q, k, M, n_ref, seed=1)
    rng = np.random.default_rng(8)
    idx, w, y_ref, y_in = c["idx"].copy(), c["w"].copy(), c["y_ref"].copy(), c["y_in"].copy()
    flat = rng.choice(Q * k, size=14, replace=False)
    rows, cols = flat // k, flat % k
    idx[rows[0], cols[0]], idx[rows[1], cols[1]], idx[rows[2], cols[2]] = -1, n_ref, -2 ** 31
    idx[rows[3], cols[3]] = 2 ** 31 - 1
    for t, v in zip(range(4, 9), (np.nan, np.inf, 0.0, -1.0, -0.0)):
        w[rows[t], cols[t]] = v
    y_ref[idx[rows[9], cols[9]]] = (np.nan, 1.0)
    y_ref[idx[rows[10], cols[10]]] = (np.inf, -np.inf)
    nan_row, dead = 7, 11
    y_in[nan_row] = (np.nan, 1.0)
    w[dead] = -0.0                                             # every entry of the row is skipped: W = 0
    a, b = curve(0.1)
    call = _Call(m, idx, w, y_ref)
    got = call.run(y_in, M=M, seed=1).cpu().numpy()
    ref, A, W = graph.transform_reference(idx, w, y_ref, y_in, 0, EPOCH, 1, TOTAL, 1.0, a, b, 1.0, 5.0, M, 1,
                                          details=True)
    keep = np.array([nan_row, dead])
    assert np.array_equal(_np_bits(got[keep]), _np_bits(y_in[keep])), "a NaN row and a W = 0 row keep their bits"
    assert W[dead] == 0 and np.isnan(ref[nan_row]).any()
    moving = np.setdiff1d(np.arange(Q), keep)
    assert np.isfinite(got[moving]).all()
    alpha = float(np.float32(1.0 - EPOCH / TOTAL))
    units = error_units(got[moving], ref[moving], y_in[moving], alpha, A[moving], W[moving])
    print(f"graph_transform skip rules: kernel {units:.2f} units, bar {T_UNITS:.1f}")
    assert units <= T_UNITS
    # from no start: the dead row is NaN, the others within the start's bar of the reference
    y0 = call.run(None, epoch0=0, n_epochs=0).cpu().numpy()
    r0 = graph.transform_reference(idx, w, y_ref, None, 0, 0, 0, TOTAL, 1.0, a, b)
    assert np.isnan(y0[dead]).all() and np.isnan(r0[dead]).all()
    alive = np.setdiff1d(np.arange(Q), [dead])
    ok = (idx >= 0) & (idx < n_ref) & np.isfinite(w) & (w > 0)
    yj = y_ref[np.where(ok, idx, 0)]
    ok &= np.isfinite(yj).all(2)
    largest = np.where(ok, np.abs(np.where(np.isfinite(yj), yj, 0.0)).max(2), 0.0).max(1)
    assert (np.abs(y0[alive] - r0[alive]).max(1) <= (2 * (k + 2) * 2.0 ** -24 * largest)[alive]).all()
    two = call.run(None, epoch0=0, n_epochs=2, M=M).cpu().numpy()
    assert np.isnan(two[dead]).all() and np.isfinite(two[alive]).all()
    # a row of only invalid entries of every kind
    bad_i = np.tile(np.array([-1, n_ref, -2 ** 31, 0, 1, 2, 3, idx[rows[9], cols[9]]], dtype=np.int32), (3, 1))
    bad_w = np.tile(np.array([1, 1, 1, np.nan, np.inf, 0, -1, 1], dtype=np.float32), (3, 1))
    y3 = y_in[:3].copy()
    out = _Call(m, bad_i, bad_w, y_ref).run(y3, M=M).cpu().numpy()
    assert np.array_equal(_np_bits(out), _np_bits(y3))
    # no reference row: OK, every row keeps its bits (NaN from no start), and y_ref may be NULL
    empty = _Call(m, c["idx"], c["w"], np.zeros((0, 2), dtype=np.float32))
    assert np.array_equal(_np_bits(empty.run(y_in, M=M).cpu().numpy()), _np_bits(y_in))
    assert np.array_equal(_np_bits(empty.run(y_in, M=M, y_ref=None, n_epochs=3, epoch0=0).cpu().numpy()), _np_bits(y_in))
    assert np.isnan(empty.run(None, M=M, y_ref=None, epoch0=0).cpu().numpy()).all()


def test_errors_leave_everything_untouched():
    m = _model()
    c = transform_case(65, 15, 8, 300)
    call = _Call(m, c["idx"], c["w"], c["y_ref"])
    good = call.good(c["y_in"], epoch0=0, n_epochs=3)
    assert_declared_exported_bound("spmf_graph_transform", N_HEADER_ARGS)

    def after():
        torch.cuda.synchronize()
        assert bool((call.buf == SENTINEL).all())
    call.buf.fill_(SENTINEL)
    assert_graph_transform_errors(call.lib, good, after)
    assert graph_transform_raw_call(good)(n=0) == 0
    after()
    assert graph_transform_raw_call(good)() == 0               # and the good call is one
    torch.cuda.synchronize()
    assert call.untouched() and bool(torch.isfinite(call.buf[8:8 + call.n]).all())


def test_umap_transform_is_the_calls_by_hand():
    case = ("poisson", 70, 45, 3, 2)
    lik, B, D, K, S = case
    cfg, x, params, mask, _ = _problem(*case)
    m = _dense_model(lik, cfg, mask, 32)
    old, new = {"counts": np.ascontiguousarray(x[:50])}, {"counts": np.ascontiguousarray(x[50:])}
    reference = m.umap(old, k=7, draws=params, n_epochs=30, n_negatives=5, min_dist=0.3, seed=11)
    labels = torch.arange(50) % 4
    labels[3] = -1
    kw = dict(n_epochs=12, n_negatives=5, seed=13, learning_rate=0.3)
    emb = m.embed(new, draws=params)["mean"]
    nn = m.knn(reference["latent"], k=6, queries=emb)
    want = m.graph_transform(nn["indices"], nn["distances"], reference["embedding"], a=reference["a"],
                             b=reference["b"], **kw)
    assert set(want) == {"embedding", "weights", "sigma", "a", "b", "n_epochs"}
    qw = graph.query_weights(nn["indices"], nn["distances"])
    assert torch.equal(_bits(want["weights"]), _bits(qw["weights"])) and torch.equal(want["sigma"], qw["sigma"])
    split = [{"counts": np.ascontiguousarray(x[50:58])}, {"counts": np.ascontiguousarray(x[58:])}]
    for data in (new, split):
        for run in range(2):
            got = m.umap_transform(data, reference, k=6, draws=params, labels=labels, **kw)
            assert set(got) == {"embedding", "weights", "sigma", "a", "b", "n_epochs", "latent", "indices",
                                "distances", "labels", "label_share"}
            assert torch.equal(_bits(got["embedding"]), _bits(want["embedding"]))
            assert torch.equal(_bits(got["latent"]), _bits(emb)) and torch.equal(got["indices"], nn["indices"])
            assert torch.equal(_bits(got["distances"]), _bits(nn["distances"]))
            assert torch.equal(_bits(got["weights"]), _bits(want["weights"]))
            assert (got["a"], got["b"], got["n_epochs"]) == (reference["a"], reference["b"], 12)
            lab, share = neighbors.vote(nn["indices"].cpu(), want["weights"].cpu(), labels, None)
            assert got["labels"].is_cuda and torch.equal(got["labels"].cpu(), lab)
            torch.testing.assert_close(got["label_share"].cpu(), share, rtol=1e-12, atol=0, equal_nan=True)
    y = want["embedding"]
    assert tuple(y.shape) == (20, 2) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    assert "labels" not in m.umap_transform(new, reference, k=6, draws=params, **kw)
    # the pieces: given weights and a given start are taken as they are; chunks through row_offset keep the bits
    given = m.graph_transform(nn["indices"], nn["distances"], reference["embedding"], weights=want["weights"],
                              a=reference["a"], b=reference["b"], **kw)
    assert given["sigma"] is None and torch.equal(_bits(given["embedding"]), _bits(y))
    start = m.graph_transform(nn["indices"], nn["distances"], reference["embedding"], a=reference["a"],
                              b=reference["b"], **dict(kw, n_epochs=0))["embedding"]
    again = m.graph_transform(nn["indices"], nn["distances"], reference["embedding"], init=start, a=reference["a"],
                              b=reference["b"], **kw)["embedding"]
    assert torch.equal(_bits(again), _bits(y))
    parts = [m.graph_transform(nn["indices"][lo:hi], nn["distances"][lo:hi], reference["embedding"],
                               weights=want["weights"][lo:hi], a=reference["a"], b=reference["b"], row_offset=lo,
                               **kw)["embedding"] for lo, hi in ((0, 7), (7, 20))]
    assert torch.equal(_bits(torch.cat(parts)), _bits(y))
    assert m.graph_transform(nn["indices"], nn["distances"], reference["embedding"])["n_epochs"] == 100
    # the reference map has not moved
    assert torch.equal(_bits(reference["embedding"]),
                       _bits(m.umap(old, k=7, draws=params, n_epochs=30, n_negatives=5, min_dist=0.3, seed=11)["embedding"]))


def test_quality_on_the_split_blobs():
    """80 of the 480 blob rows mapped onto the fp64 layout of the other 400 (k = 10, 100 epochs, lr 0.25, M = 8):
    purity >= 0.99 (8 of 800 votes for fp32 drift over 100 epochs; the fp64 restatement has 1.0000, and fp32 against
    fp64 positions differed by at most 3e-3), spacing ratio in [0.5, 2] (fp64: 0.980), all positions finite, and the
    rows move from the start.  Measured on an MI355X: purity 1.0000 (start 1.0000), spacing ratio 0.980, mean
    displacement 0.304, at most 2.8e-5 from the fp64 positions."""
    m = _model()
    s = blob_split()
    call = _Call(m, s["idx"], s["w"], s["y_ref"])
    kw = dict(total=100, lr=0.25, a=s["a"], b=s["b"], M=8, seed=0)
    y0 = call.run(None, epoch0=0, n_epochs=0, **kw).cpu().numpy()
    y = call.run(None, epoch0=0, n_epochs=100, **kw).cpu().numpy()
    assert np.isfinite(y0).all() and np.isfinite(y).all()
    pure, ratio = transform_quality(y, s)
    moved = float(np.abs(y.astype(np.float64) - y0).max(1).mean())
    ref = graph.transform_reference(s["idx"], s["w"], s["y_ref"], None, 0, 0, 100, 100, 0.25, s["a"], s["b"], 1.0, 5.0,
                                    8, 0)
    print(f"graph_transform blobs: purity {pure:.4f} (start {transform_quality(y0, s)[0]:.4f}), spacing ratio "
          f"{ratio:.3f}, mean displacement {moved:.3f}, largest distance from the fp64 positions "
          f"{float(np.abs(y - ref).max()):.2e}")
    assert pure >= 0.99
    assert 0.5 <= ratio <= 2.0
    assert moved > 0
    # the method on the device arrays, with the memberships it forms there
    idx, dist = torch.as_tensor(s["idx"]).cuda(), torch.as_tensor(s["dist"]).cuda()
    res = m.graph_transform(idx, dist, torch.as_tensor(s["y_ref"]).cuda(), n_epochs=100, a=s["a"], b=s["b"])
    np.testing.assert_allclose(res["weights"].cpu().numpy(), s["w"], rtol=1e-6, atol=0)
    assert transform_quality(res["embedding"].cpu().numpy(), s)[0] >= 0.99
