"""GPU: spmf_graph_scale / spmf_graph_spmm / spmf_block_gram / spmf_block_rotate (csrc/spectral.hip) and the methods
on top (spectral, spectral_cluster, with spmf_amd.spectral's helpers).

The product against the fp64 restatement of its definition (tests/_spectral_cases.py spmm_reference) through raw
library calls with sentinels around the output, per entry:
    |y_gpu - y_ref| <= T 2^-24 (|c_s| s_i sum_j w_ij s_j |x_j| + |c_x x_i| + |c_z z_i|).
T = 8 x the largest error of the float32 numpy backend (spmf_amd.spectral.NumpyOps) against the same reference, in
the bar's units, over the same cases: measured 5.59 units (the 700-entry hub of N = 1000, a sequential float32 sum),
so T = 44.7.  The kernel measured 4.68 units as the largest over the same cases on an MI355X (the same
hub, the filter step; 3.51 on the skip-rule graph).

Then the skip rules, NaN propagation, aliasing, the scale to one ulp, the Gram matrix and the rotation against fp64
with the bars of their definitions, the error contracts with sentinels, and end to end: ``spectral`` on the three
graphs of the host tests under the same fp64 criteria at tol = 1e-5.  The residual a float32 block can reach on the
library's product -- the residual of the reference's fp64 eigenvectors rounded to float32 and pushed through
spmf_graph_spmm -- measured 6.9e-8 (cycle), 1.0e-7 (blobs) and 7.4e-8 (rings) on an MI355X (the numpy backend:
8.1e-8, 9.5e-8, 8.0e-8), so
tol = 1e-5 is more than 4 x the floor and stands."""
import numpy as np
import pytest
import torch

from _graph_layout_cases import blobs, layout_case, purity
from _spectral_cases import (BLOCK, CHUNK, SPMM_SHAPES, agreement, assert_criteria, assert_errors, assert_sign_rule,
                             coefficient_sets, end_to_end_graphs, host_array, many_components, raw_call, reference_of,
                             rings,
                             spmm_case, spmm_reference, spmm_units)
from spmf_amd import spectral

pytestmark = pytest.mark.gpu

T_UNITS = 8 * 5.59
TOL = 1e-5
SENTINEL = -7.0


def _model():
    from spmf_amd import PoissonFactorization
    return PoissonFactorization(latent_dim=3, feature_dim=8, initialize_distributions=False, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _cuda_graph(g):
    return {n: g[n].cuda() for n in ("indptr", "indices", "weights")}


class _Call:
    """Raw calls on one graph: device copies of the arrays, every output inside a buffer of sentinels (8 rows in
    front, 8 behind), block_gram's scratch exactly as large as the size function says with zeros behind it."""

    def __init__(self, m, indptr, indices, weights):
        from spmf_amd import _lib
        self.lib, self.h = _lib.load(), m._handle()
        self.n = len(indptr) - 1
        self.g = [_dev(v) for v in (indptr, indices, weights)]
        self.stream = torch.cuda.current_stream().cuda_stream
        self.out = torch.full((self.n + 16, BLOCK), SENTINEL, dtype=torch.float32, device="cuda")
        self.sc = torch.full((self.n + 16,), SENTINEL, dtype=torch.float32, device="cuda")
        self.gram = torch.full((BLOCK * BLOCK + 32,), SENTINEL, dtype=torch.float64, device="cuda")
        self.need = int(self.lib.spmf_block_gram_scratch_bytes(self.h, self.n))
        assert self.need > 0 and self.need % 256 == 0
        self.scratch = torch.zeros(self.need + 512, dtype=torch.uint8, device="cuda")
        self.ptr = self.scratch.data_ptr() + (-self.scratch.data_ptr()) % 256
        self.guard = self.ptr - self.scratch.data_ptr() + self.need

    def graph_args(self):
        return dict(h=self.h, n=self.n, nnz=int(self.g[1].numel()), indptr=self.g[0].data_ptr(),
                    indices=self.g[1].data_ptr(), weights=self.g[2].data_ptr(), stream=self.stream)

    def rows(self, buf):
        return buf[8:8 + self.n]

    def untouched(self):
        ok = all(bool((b[:8] == SENTINEL).all()) and bool((b[8 + self.n:] == SENTINEL).all())
                 for b in (self.out, self.sc))
        ok = ok and bool((self.gram[:16] == SENTINEL).all()) and bool((self.gram[16 + BLOCK * BLOCK:] == SENTINEL).all())
        return ok and not bool(self.scratch[self.guard:].any())

    def finish(self, rc):
        assert rc == 0, self.lib.spmf_last_error(self.h).decode()
        torch.cuda.synchronize()
        assert self.untouched(), "a write outside an output or the scratch"

    def scale(self):
        self.sc.fill_(SENTINEL)
        self.finish(raw_call("graph_scale", dict(self.graph_args(), scale=self.rows(self.sc).data_ptr()))())
        return self.rows(self.sc).clone()

    def spmm(self, x, scale=None, z=None, cs=1.0, cx=None, cz=0.0, alias_z=False):
        """-> y float32 [n, 16] (a copy).  ``alias_z``: y is z."""
        self.out.fill_(SENTINEL)
        c = host_array(np.zeros(BLOCK) if cx is None else cx)
        y = self.rows(self.out)
        if alias_z:
            y.copy_(z)
            z = y
        args = dict(self.graph_args(), scale=scale.data_ptr() if scale is not None else None, x=x.data_ptr(),
                    z=z.data_ptr() if z is not None else None, y=y.data_ptr(), cs=cs, cx=c, cz=cz)
        self.finish(raw_call("graph_spmm", args)())
        return y.clone()

    def gram_args(self, x, y):
        return dict(h=self.h, n=self.n, x=x.data_ptr(), y=y.data_ptr(), g=self.gram[16:].data_ptr(), ptr=self.ptr,
                    nbytes=self.need, stream=self.stream)

    def block_gram(self, x, y):
        self.gram.fill_(SENTINEL)
        self.finish(raw_call("block_gram", self.gram_args(x, y))())
        return self.gram[16:16 + BLOCK * BLOCK].clone().cpu().numpy().reshape(BLOCK, BLOCK)

    def rotate(self, x, r, alias=False):
        self.out.fill_(SENTINEL)
        y = self.rows(self.out)
        if alias:
            y.copy_(x)
            x = y
        keep = host_array(np.asarray(r, dtype=np.float64).reshape(-1))
        self.finish(raw_call("block_rotate", dict(h=self.h, n=self.n, x=x.data_ptr(), r=keep, y=y.data_ptr(),
                                                  stream=self.stream))())
        return y.clone()


def _empty_graph_call(m, n):
    return _Call(m, np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))


def _assert_scale(got, graph):
    """Within one float32 ulp of 1 / sqrt(the fp64 degree), exactly 0 on rows without a valid entry."""
    d = spectral.degrees(graph)
    want = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    got = got.cpu().numpy()
    assert (got[d == 0] == 0).all() and (d == 0).any() == (got == 0).any()
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - want) <= ulp).all()


@pytest.mark.parametrize("N,hub", SPMM_SHAPES)
def test_product_against_the_reference(N, hub):
    m = _model()
    c = spmm_case(N, hub)
    call = _Call(m, c["indptr"], c["indices"], c["weights"])
    s = call.scale()
    _assert_scale(s, c)
    if N >= 8:
        assert float(s[N // 2]) == 0.0, "the case has a row without an edge"
    s_host = s.cpu().numpy()
    x, z = _dev(c["x"]), _dev(c["z"])
    worst = (-1.0, None)
    for name, cs, cx, cz, with_z in coefficient_sets():
        for scaled in (True, False):
            zz = z if with_z else None
            got = call.spmm(x, scale=s if scaled else None, z=zz, cs=cs, cx=cx, cz=cz)
            ref, bar = spmm_reference(c, s_host if scaled else None, c["x"], c["z"] if with_z else None, cs, cx, cz)
            units = spmm_units(got.cpu().numpy(), ref, bar)
            print(f"graph_spmm N={N} hub={hub} {name} scaled={scaled}: kernel {units:.2f} units, bar {T_UNITS:.1f}")
            if units > worst[0]:
                worst = (units, (name, scaled))
            if with_z:
                same = call.spmm(x, scale=s if scaled else None, z=z, cs=cs, cx=cx, cz=cz, alias_z=True)
                assert torch.equal(_bits(same), _bits(got)), "y = z gives the bits of the call that does not alias"
            assert torch.equal(_bits(got), _bits(call.spmm(x, scale=s if scaled else None, z=zz, cs=cs, cx=cx, cz=cz)))
    assert worst[0] <= T_UNITS, worst


def test_skip_rules():
    """test_gpu_graph_layout.py test_skip_rules' list: indices -1 / N / +-2^31, weights 0 / -1 / NaN / inf, an
    indptr beyond [0, nnz], a falling indptr.  The result is the reference's under the same rules, and the graph
    cleaned of the skipped entries gives the same bits on rows that lost none."""
    m = _model()
    N = 65
    c = spmm_case(N, 0)
    rng = np.random.default_rng(8)
    indices, w = c["indices"].copy(), c["weights"].copy()
    spots = rng.choice(len(indices), size=12, replace=False)
    indices[spots[0]], indices[spots[1]] = -1, N
    indices[spots[2]], indices[spots[3]] = -2 ** 31, 2 ** 31 - 1
    w[spots[4]], w[spots[5]], w[spots[6]], w[spots[7]] = 0.0, -1.0, np.nan, np.inf
    dead = 11
    w[c["indptr"][dead]:c["indptr"][dead + 1]] = -0.0          # every entry of the row is skipped
    indptr = c["indptr"].copy()
    indptr[0], indptr[-1] = -5, len(indices) + 100            # clamped to 0 and nnz: the same lists
    dirty = dict(indptr=indptr, indices=indices, weights=w)
    call = _Call(m, indptr, indices, w)
    s = call.scale()
    _assert_scale(s, dirty)
    assert float(s[dead]) == 0.0
    x, z = _dev(c["x"]), _dev(c["z"])
    _, cs, cx, cz, _ = coefficient_sets()[2]
    got = call.spmm(x, scale=s, z=z, cs=cs, cx=cx, cz=cz)
    ref, bar = spmm_reference(dirty, s.cpu().numpy(), c["x"], c["z"], cs, cx, cz)
    assert bool(torch.isfinite(got).all())
    units = spmm_units(got.cpu().numpy(), ref, bar)
    print(f"graph_spmm skip rules: kernel {units:.2f} units, bar {T_UNITS:.1f}")
    assert units <= T_UNITS
    # the skipped entries are no part of the result: the clean graph without them gives the same bits
    with np.errstate(invalid="ignore"):
        ok = (indices >= 0) & (indices < N) & np.isfinite(w) & (w > 0)
    row = np.repeat(np.arange(N), np.diff(c["indptr"]))
    ptr = np.searchsorted(row[ok], np.arange(N + 1)).astype(np.int64)
    clean = _Call(m, ptr, indices[ok], w[ok]).spmm(x, scale=s, z=z, cs=cs, cx=cx, cz=cz)
    assert torch.equal(_bits(got), _bits(clean)), "list order without the skipped entries: every row's bits"
    # a falling indptr is an empty row, not a read before the list
    fall = c["indptr"].copy()
    fall[20] = fall[22]
    fallen = dict(indptr=fall, indices=c["indices"], weights=c["weights"])
    fc = _Call(m, fall, c["indices"], c["weights"])
    fs = fc.scale()
    _assert_scale(fs, fallen)
    assert float(fs[20]) == 0.0
    out = fc.spmm(x, scale=fs, z=z, cs=cs, cx=cx, cz=cz)
    want, bar = spmm_reference(fallen, fs.cpu().numpy(), c["x"], c["z"], cs, cx, cz)
    assert bool(torch.isfinite(out).all()) and spmm_units(out.cpu().numpy(), want, bar) <= T_UNITS


def test_a_nan_reaches_the_rows_that_list_it_and_no_further():
    m = _model()
    c = spmm_case(257, 0)
    call = _Call(m, c["indptr"], c["indices"], c["weights"])
    s = call.scale()
    xs = c["x"].copy()
    src, col = 3, 5
    xs[src, col] = np.nan
    got = call.spmm(_dev(xs), scale=s, cs=1.0, cx=np.full(BLOCK, 0.5)).cpu().numpy()
    lists = np.repeat(np.arange(257), np.diff(c["indptr"]))[c["indices"] == src]
    want = np.zeros(257, dtype=bool)
    want[lists] = True
    want[src] = True
    assert len(lists) > 0 and np.array_equal(np.isnan(got[:, col]), want)
    assert np.isfinite(np.delete(got, col, axis=1)).all()


@pytest.mark.parametrize("N", [1, CHUNK - 1, CHUNK, CHUNK + 1, 5000])
def test_gram_against_fp64(N):
    """|G - ref| <= N 2^-52 sum_r |x_ra y_rb|: the float32 products are exact in fp64, only the additions round."""
    m = _model()
    rng = np.random.default_rng(6100 + N)
    x = (rng.standard_normal((N, BLOCK)) * np.exp(rng.uniform(-2, 2, size=(N, 1)))).astype(np.float32)
    y = rng.standard_normal((N, BLOCK)).astype(np.float32)
    call = _empty_graph_call(m, N)
    assert call.need >= 8 * BLOCK * BLOCK * -(-N // CHUNK)
    xd, yd = _dev(x), _dev(y)
    got = call.block_gram(xd, yd)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    ref, mag = x64.T @ y64, np.abs(x64).T @ np.abs(y64)
    off = np.abs(got - ref) / (N * 2.0 ** -52 * mag)
    print(f"block_gram N={N}: largest error {off.max():.3f} of the bar")
    assert (np.abs(got - ref) <= N * 2.0 ** -52 * mag).all()
    assert np.array_equal(got.view(np.int64), call.block_gram(xd, yd).view(np.int64)), "the same bits twice"
    sym = call.block_gram(xd, xd)
    assert np.array_equal(sym, sym.T), "x^T x: a and b add the same products in the same order"


@pytest.mark.parametrize("N", [1, 17, 1000])
def test_rotate_against_fp64(N):
    """|got - ref| <= 2^-24 |ref| + 16 2^-52 sum_k |x_k r_kb|; y = x gives the same bits."""
    m = _model()
    rng = np.random.default_rng(6200 + N)
    x = (rng.standard_normal((N, BLOCK)) * np.exp(rng.uniform(-2, 2, size=(N, 1)))).astype(np.float32)
    r = rng.standard_normal((BLOCK, BLOCK)) * np.exp(rng.uniform(-2, 2, size=(1, BLOCK)))
    call = _empty_graph_call(m, N)
    xd = _dev(x)
    got = call.rotate(xd, r)
    x64 = x.astype(np.float64)
    ref, mag = x64 @ r, np.abs(x64) @ np.abs(r)
    assert (np.abs(got.cpu().numpy().astype(np.float64) - ref) <= 2.0 ** -24 * np.abs(ref) + 16 * 2.0 ** -52 * mag).all()
    assert torch.equal(_bits(got), _bits(call.rotate(xd, r, alias=True))), "y = x"
    eye = call.rotate(xd, np.eye(BLOCK))
    assert torch.equal(_bits(eye), _bits(xd)), "the identity returns the block"


def test_errors_leave_everything_untouched():
    m = _model()
    c = spmm_case(65, 0)
    call = _Call(m, c["indptr"], c["indices"], c["weights"])
    x, z = _dev(c["x"]), _dev(c["z"])
    s = call.scale()
    call.out.fill_(SENTINEL)
    call.sc.fill_(SENTINEL)
    call.gram.fill_(SENTINEL)
    x0 = x.clone()

    def after():
        torch.cuda.synchronize()
        assert bool((call.out == SENTINEL).all()) and bool((call.sc == SENTINEL).all())
        assert bool((call.gram == SENTINEL).all()) and not bool(call.scratch.any())
        assert torch.equal(_bits(x), _bits(x0)), "y = x is refused with nothing written"
    goods = {
        "graph_scale": dict(call.graph_args(), scale=call.rows(call.sc).data_ptr()),
        "graph_spmm": dict(call.graph_args(), scale=s.data_ptr(), x=x.data_ptr(), z=z.data_ptr(),
                           y=call.rows(call.out).data_ptr(), cs=1.0, cx=host_array([0.5] * BLOCK), cz=-1.0),
        "block_gram": call.gram_args(x, z),
        "block_rotate": dict(h=call.h, n=call.n, x=x.data_ptr(), r=host_array(np.eye(BLOCK).reshape(-1)),
                             y=call.rows(call.out).data_ptr(), stream=call.stream),
    }
    for entry, good in goods.items():
        assert_errors(call.lib, entry, good, call.need, after)
    # the empty calls touch nothing but block_gram's g, which is zero-filled
    for entry, good in goods.items():
        assert raw_call(entry, good)(n=0) == 0
    torch.cuda.synchronize()
    assert bool((call.out == SENTINEL).all()) and bool((call.sc == SENTINEL).all()) and not bool(call.scratch.any())
    assert bool((call.gram[16:16 + BLOCK * BLOCK] == 0).all()) and call.untouched()
    for entry, good in goods.items():
        assert raw_call(entry, good)() == 0                    # and the good calls are good
    torch.cuda.synchronize()
    assert call.untouched()


# ---- end to end -------------------------------------------------------------------------------------------------------
def _floor(m, name, g, n_components):
    """The residual of the reference's fp64 eigenvectors rounded to float32 on the library's product."""
    from spmf_amd import _lib
    _, val, vec = reference_of(name)
    ops = spectral.LibraryOps(_lib.load(), m._handle(), g["indptr"], g["indices"], g["weights"])
    v = np.zeros((ops.n, BLOCK), dtype=np.float32)
    v[:, :n_components + 1] = vec[:, :n_components + 1]
    cx = np.zeros(BLOCK)
    cx[:n_components + 1] = -val[:n_components + 1]
    r = ops.spmm(ops.block(v), cs=1.0, cx=cx).cpu().numpy().astype(np.float64)
    return float(np.linalg.norm(r, axis=0)[:n_components + 1].max())


@pytest.mark.parametrize("name", ["cycle", "blobs", "rings"])
def test_spectral_against_the_reference(name):
    m = _model()
    cpu, k = {n: (gr, mm) for n, gr, mm in end_to_end_graphs()}[name]
    g = _cuda_graph(cpu)
    floor = _floor(m, name, g, k)
    print(f"spectral {name}: residual floor of a float32 block on the library's product {floor:.2e}")
    assert TOL >= 4.0 * floor, "tol = 1e-5 is at least four times the floor"
    res = m.spectral(g, n_components=k, tol=TOL)
    assert res["vectors"].is_cuda and res["vectors"].dtype == torch.float32 and res["scale"].is_cuda
    assert tuple(res["embedding"].shape) == (int(g["indptr"].numel()) - 1, k)
    assert_criteria(name, res, k, TOL)
    assert_sign_rule(res["vectors"])
    again = m.spectral(g, n_components=k, tol=TOL)
    assert torch.equal(_bits(res["vectors"]), _bits(again["vectors"])), "the same bits twice"
    assert np.array_equal(res["values"], again["values"]) and np.array_equal(res["residuals"], again["residuals"])
    assert res["n_unit"] == {"cycle": 1, "blobs": 7, "rings": 2}[name]
    other = m.spectral(g, n_components=k, tol=TOL, seed=1)
    assert not torch.equal(_bits(res["vectors"]), _bits(other["vectors"])), "another seed: other bits"
    assert_criteria(name, other, k, TOL)                       # ... of the same subspace


def test_more_components_than_columns_do_not_stall():
    """20 components against a block of 16 columns (tests/test_spectral_host.py has the case): converged at
    tol = 1e-5 within 10 outer iterations."""
    m = _model()
    cpu = many_components()
    res = m.spectral(_cuda_graph(cpu), n_components=2, tol=TOL, max_iter=30)
    print(f"spectral, 20 components: {res['n_iter']} iterations, {res['n_products']} products, largest residual "
          f"{res['residuals'].max():.2e}")
    assert res["converged"] and res["n_iter"] <= 10 and res["n_unit"] == 3
    S = spectral.normalized_dense(cpu)
    V = res["vectors"].cpu().double().numpy()
    assert np.abs(np.linalg.norm(S @ V - V * res["values"][None, :], axis=0) - res["residuals"]).max() <= 1e-6


def test_spectral_cluster_separates_the_rings_and_kmeans_does_not():
    m = _model()
    cpu, x, truth = rings()
    g = _cuda_graph(cpu)
    out = m.spectral_cluster(g, 2, tol=TOL)
    assert out["labels"].dtype == torch.int32 and tuple(out["features"].shape) == (400, 2)
    assert out["spectral"]["n_unit"] == 2 and out["spectral"]["converged"]
    ours = agreement(out["labels"].cpu().numpy(), truth.numpy())
    raw = agreement(m.kmeans(x.cuda(), 2)["labels"].cpu().numpy(), truth.numpy())
    print(f"rings: spectral_cluster agrees with the truth on {ours:.3f} of the rows, kmeans of the points on {raw:.3f}")
    assert ours >= 0.99
    assert raw <= 0.60
    again = m.spectral_cluster(g, 2, tol=TOL)
    assert torch.equal(out["labels"], again["labels"])


def test_the_spectral_start_of_a_layout_on_the_blobs():
    """The purity bar of test_gpu_graph_layout.py test_quality_on_the_blobs: at least 0.95 (k = 10, 200 epochs,
    M = 8), from ``layout_init`` of the spectral embedding passed as a tensor."""
    m = _model()
    x, labels = blobs()
    xd = x.cuda()
    nn = m.knn(xd, k=10)
    g = m.fuzzy_graph(nn["indices"], nn["distances"])
    res = m.spectral(g, n_components=2)
    assert res["converged"]
    start = spectral.layout_init(res["embedding"], seed=0)
    assert start.is_cuda and abs(float(start.abs().max()) - 10.0) <= 1e-3
    y = m.graph_layout(g, start, n_epochs=200, n_negatives=8)["embedding"]
    end = purity(y, labels)
    print(f"blobs: purity of the spectral start {purity(start, labels):.3f}, of the layout from it {end:.3f}")
    assert bool(torch.isfinite(y).all()) and end >= 0.95
