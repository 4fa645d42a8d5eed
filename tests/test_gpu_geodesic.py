"""GPU: spmf_graph_relax (csrc/graph_paths.hip) and ``geodesic`` / ``pseudotime`` on top of it.

Raw library calls with 8 sentinel words on both sides of x_out, pred_out and changed_out and an exactly sized scratch:
on the hand-made edge graph (tests/_geodesic_cases.py edge_graph) for 0, 1, 2 and 17 sweeps from a block of 16
different sources, in place, without the optional outputs, twice; at the block edges of the launch; the error contract
and the empty call.  Distances and predecessors equal ``NumpyOps.relax`` exactly -- there is no tolerance anywhere: the
sweep is one float32 addition and comparisons.  Then end to end: ``model.geodesic`` returns the arrays of
``solve(NumpyOps)``, ``n_sweeps`` included, twice; ``model.pseudotime`` is the composition of its parts; and on the
chain of blobs pseudotime orders the blobs."""
import numpy as np
import pytest
import torch

from _geodesic_cases import (BLOCK, EDGE_N, assert_errors, chain_lengths, edge_graph, edge_sources, graph_numpy,
                             raw_call, scratch_bytes, spiral)
from spmf_amd import geodesic

pytestmark = pytest.mark.gpu

SENTINEL = -77
PAD = 8
INF = float("inf")


def _model():
    from spmf_amd import PoissonFactorization
    return PoissonFactorization(latent_dim=3, feature_dim=8, initialize_distributions=False, device="cuda")


def _dev(a):
    return torch.as_tensor(np.array(a)).cuda()                # (a copy: the cases' arrays are read-only)


class _Call:
    """Raw calls on a graph of numpy arrays (indptr, indices, weights): device copies, the three outputs inside
    buffers of sentinels (8 words in front, 8 behind), an exactly sized scratch."""

    def __init__(self, m, g):
        from spmf_amd import _lib
        self.m = m                         # the model owns the context: it lives as long as the handle is used
        self.lib, self.h = _lib.load(), m._handle()
        self.n = len(g["indptr"]) - 1
        self.t = {k: _dev(g[k]) for k in ("indptr", "indices", "weights")}
        self.keep = None

    def args(self, x, n_sweeps):
        need = scratch_bytes(self.lib, self.h, self.n)
        assert need > 0 and need % 256 == 0
        scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
        words = self.n * BLOCK
        self.out = {"x": torch.full((words + 2 * PAD,), float(SENTINEL), dtype=torch.float32, device="cuda"),
                    "pred": torch.full((words + 2 * PAD,), SENTINEL, dtype=torch.int32, device="cuda"),
                    "changed": torch.full((1 + 2 * PAD,), SENTINEL, dtype=torch.int32, device="cuda")}
        self.keep = (_dev(np.asarray(x, dtype=np.float32)), scratch)
        nnz = int(self.t["indices"].numel())
        return dict(h=self.h, n=self.n, nnz=nnz, indptr=self.t["indptr"].data_ptr(),
                    indices=self.t["indices"].data_ptr() if nnz else None,
                    lengths=self.t["weights"].data_ptr() if nnz else None, x_in=self.keep[0].data_ptr(),
                    x_out=self.out["x"][PAD:].data_ptr(), pred=self.out["pred"][PAD:].data_ptr(),
                    changed=self.out["changed"][PAD:].data_ptr(), n_sweeps=n_sweeps,
                    ptr=scratch.data_ptr() + (-scratch.data_ptr()) % 256, nbytes=need,
                    stream=torch.cuda.current_stream().cuda_stream)

    def untouched(self, whole=False, inner=()):
        """The sentinels around every output are whole; with ``whole`` (or for the outputs named in ``inner``) the
        output itself too."""
        for k, t in self.out.items():
            if not bool((t[:PAD] == SENTINEL).all()) or not bool((t[-PAD:] == SENTINEL).all()):
                return False
            if (whole or k in inner) and not bool((t[PAD:-PAD] == SENTINEL).all()):
                return False
        return True

    def run(self, x, n_sweeps, **kw):
        """-> (x_out [N, 16], pred_out [N, 16], changed) on the CPU after a checked call."""
        rc = raw_call(self.args(x, n_sweeps))(**kw)
        assert rc == 0, self.lib.spmf_last_error(self.h).decode()
        torch.cuda.synchronize()
        assert self.untouched(), "a write outside an output"
        return (self.out["x"][PAD:-PAD].cpu().reshape(self.n, BLOCK), self.out["pred"][PAD:-PAD].cpu().reshape(self.n, BLOCK),
                int(self.out["changed"][PAD]))


def _start(n, sources):
    x = np.full((n, BLOCK), np.inf, dtype=np.float32)
    for l, s in enumerate(sources):
        x[s, l] = 0.0
    return x


def _same(a, b):
    """Bit equality of two float32 tensors."""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_is_numpy(call, g, x, n_sweeps):
    y, p, changed = call.run(x, n_sweeps)
    wy, wp, wchanged = geodesic.NumpyOps(g).relax(torch.from_numpy(x), n_sweeps, True)
    assert _same(y, wy), ("distances", n_sweeps, torch.nonzero(y != wy)[:5].tolist())
    if n_sweeps:
        assert torch.equal(p, wp), ("predecessors", n_sweeps, torch.nonzero(p != wp)[:5].tolist())
    else:
        assert bool((p == SENTINEL).all()), "without a sweep no predecessor is written"
    assert changed == int(wchanged), (n_sweeps, changed, wchanged)
    return y, p, changed


@pytest.mark.parametrize("n_sweeps", [0, 1, 2, 17])
def test_the_edge_graph_is_the_numpy_sweep(n_sweeps):
    e = edge_graph()
    call = _Call(_model(), e)
    x = _start(EDGE_N, edge_sources())
    assert np.isfinite(x[:, 15]).sum() == 1, "column 15 is used"
    y, p, changed = _assert_is_numpy(call, e, x, n_sweeps)
    assert changed == (1 if n_sweeps in (1, 2) else 0), "1 before the fixed point, 0 at it"
    if n_sweeps == 17:
        fixed = geodesic.solve(geodesic.NumpyOps(e), torch.from_numpy(edge_sources()), predecessors=True)
        assert _same(y, fixed["distances"]) and torch.equal(p, fixed["predecessors"])
    again = call.run(x, n_sweeps)
    assert _same(again[0], y) and torch.equal(again[1], p) and again[2] == changed, "the same bits twice"
    # in place: x_out == x_in (the start sits in the output's buffer)
    good = call.args(x, n_sweeps)
    call.out["x"][PAD:-PAD] = call.keep[0].reshape(-1)
    rc = raw_call(good)(x_in=good["x_out"])
    assert rc == 0, call.lib.spmf_last_error(call.h).decode()
    torch.cuda.synchronize()
    assert call.untouched() and _same(call.out["x"][PAD:-PAD].cpu().reshape(EDGE_N, BLOCK), y)
    # without the optional outputs: nothing of them is written
    rc = raw_call(call.args(x, n_sweeps))(pred=None, changed=None)
    assert rc == 0, call.lib.spmf_last_error(call.h).decode()
    torch.cuda.synchronize()
    assert call.untouched(inner=("pred", "changed")) and _same(call.out["x"][PAD:-PAD].cpu().reshape(EDGE_N, BLOCK), y)


def _random_graph(n, per_row, seed):
    """Rows of 0 .. 2 ``per_row`` entries with random columns and random positive lengths -> dict numpy."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 2 * per_row + 1, size=n)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(indptr[-1])
    return dict(indptr=indptr, indices=rng.integers(0, n, size=nnz).astype(np.int32),
                weights=rng.uniform(0.01, 3.0, size=nnz).astype(np.float32))


@pytest.mark.parametrize("n", [15, 16, 17, 4097])
def test_block_edges_of_the_launch(n):
    """A workgroup takes 16 rows: one short of a workgroup, exactly one, one more, and 256 workgroups and a row."""
    m = _model()
    g = _random_graph(n, 8, n)
    rng = np.random.default_rng(n + 1)
    x = _start(n, rng.choice(n, size=BLOCK, replace=n < BLOCK))       # (15 rows: a source in two columns)
    call = _Call(m, g)
    for n_sweeps in (1, 3):
        y, p, changed = _assert_is_numpy(call, g, x, n_sweeps)
        assert changed == 1 and int(np.isfinite(y.numpy()).sum()) > BLOCK and int((p >= 0).sum()) > 0
    # the last row is reached and written: the sources' own rows include n - 1
    x = _start(n, [n - 1] * BLOCK)
    y, _, _ = _assert_is_numpy(call, g, x, 2)
    assert not y[n - 1].any()


def test_a_graph_without_entries_and_one_row():
    m = _model()
    empty = dict(indptr=np.zeros(71, dtype=np.int64), indices=np.zeros(0, dtype=np.int32),
                 weights=np.zeros(0, dtype=np.float32))
    x = _start(70, np.arange(BLOCK))
    y, p, changed = _assert_is_numpy(_Call(m, empty), empty, x, 2)
    assert changed == 0 and _same(y, torch.from_numpy(x)) and bool((p == -1).all())
    one = dict(indptr=np.array([0, 3], dtype=np.int64), indices=np.zeros(3, dtype=np.int32),
               weights=np.array([1.0, 0.5, 2.0], dtype=np.float32))
    x = np.full((1, BLOCK), 5.0, dtype=np.float32)
    x[0, 1] = INF
    y, p, changed = _assert_is_numpy(_Call(m, one), one, x, 1)
    assert changed == 0 and _same(y, torch.from_numpy(x)) and bool((p == -1).all()), "a self entry lowers nothing"


def test_errors_return_before_a_launch_and_the_empty_call_writes_nothing():
    e = edge_graph()
    call = _Call(_model(), e)
    good = call.args(_start(EDGE_N, edge_sources()), 3)

    def after():
        torch.cuda.synchronize()
        assert call.untouched(whole=True), "an output was written by a refused call"
    assert_errors(call.lib, good, after=after)
    # n_rows = 0: nothing is written
    rc = raw_call(good)(n=0, indptr=None, x_in=None, x_out=None)
    assert rc == 0, call.lib.spmf_last_error(call.h).decode()
    after()


def _on_device(g):
    return {k: _dev(g[k]) for k in ("indptr", "indices", "weights")}


@pytest.mark.parametrize("case", ["chain", "spiral"])
def test_geodesic_is_the_numpy_backends_arrays(case):
    if case == "chain":
        g = graph_numpy(chain_lengths()[0])
        sources = [torch.tensor([0]), torch.tensor([319]), torch.tensor([5, 170, 300])]
    else:
        g = graph_numpy(spiral()[0])
        sources = torch.tensor([0, 1500, 2999])
    want = geodesic.solve(geodesic.NumpyOps(g), sources, predecessors=True)
    assert want["converged"]
    m = _model()
    dev = _on_device(g)
    for _ in range(2):
        res = m.geodesic(dev, sources, predecessors=True)
        assert set(res) == {"distances", "predecessors", "n_sweeps", "converged"}
        assert res["distances"].is_cuda and res["predecessors"].is_cuda
        assert _same(res["distances"].cpu(), want["distances"])
        assert torch.equal(res["predecessors"].cpu(), want["predecessors"])
        assert res["n_sweeps"] == want["n_sweeps"] and res["converged"] is True
    plain = m.geodesic(dev, sources)
    assert plain["predecessors"] is None and _same(plain["distances"].cpu(), want["distances"])
    short = m.geodesic(dev, sources, max_sweeps=3)
    want_short = geodesic.solve(geodesic.NumpyOps(g), sources, max_sweeps=3)
    assert not short["converged"] and short["n_sweeps"] == 3 and _same(short["distances"].cpu(), want_short["distances"])
    with pytest.raises(ValueError, match="geodesic: .*device"):          # host memory is never handed to the library
        m.geodesic({k: torch.as_tensor(g[k]) for k in g}, sources)


def test_seventeen_sources_take_two_blocks():
    g = graph_numpy(chain_lengths()[0])
    m = _model()
    dev = _on_device(g)
    sources = torch.arange(0, 17 * 18, 18)
    res = m.geodesic(dev, sources, predecessors=True)
    want = geodesic.solve(geodesic.NumpyOps(g), sources, predecessors=True)
    assert tuple(res["distances"].shape) == (320, 17) and _same(res["distances"].cpu(), want["distances"])
    assert torch.equal(res["predecessors"].cpu(), want["predecessors"])
    one = m.geodesic(dev, sources[16:])
    assert _same(res["distances"][:, 16].cpu(), one["distances"][:, 0].cpu())


def test_pseudotime_is_the_composition_of_its_parts_and_orders_the_blob_chain():
    from spmf_amd import PoissonFactorization
    _, x, truth = chain_lengths()
    # counts whose encodings keep the blobs' order: a model as initialised, eight columns
    torch.manual_seed(0)
    m = PoissonFactorization(latent_dim=3, feature_dim=8, device="cuda")
    counts = torch.floor((x.double() + 4.0).clamp_min(0.0) * 3.0).numpy()
    draws = m.surrogate_distribution.sample(4)
    res = m.pseudotime({"counts": counts}, 0, k=10, draws=draws)
    assert set(res) == {"pseudotime", "geodesic", "n_sweeps", "converged", "graph", "latent", "indices", "distances"}
    emb = m.embed({"counts": counts}, draws=draws)["mean"]
    nn = m.knn(emb, k=10)
    g = geodesic.length_graph(nn["indices"], nn["distances"])
    geo = m.geodesic(g, torch.tensor([0]))
    assert torch.equal(res["latent"], emb) and torch.equal(res["indices"], nn["indices"])
    assert all(torch.equal(res["graph"][k], g[k]) for k in g)
    assert _same(res["geodesic"].cpu(), geo["distances"][:, 0].cpu()) and res["n_sweeps"] == geo["n_sweeps"]
    t = res["pseudotime"]
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (320,)
    assert torch.equal(t.cpu().view(torch.int32), geodesic.pseudotime(geo["distances"][:, 0]).cpu().view(torch.int32))
    # the graph made on the device is the graph made on the CPU, and both backends solve it alike
    host = geodesic.length_graph(nn["indices"].cpu(), nn["distances"].cpu())
    assert all(torch.equal(host[k], g[k].cpu()) for k in g)
    assert _same(geodesic.solve(geodesic.NumpyOps(host), torch.tensor([0]))["distances"], geo["distances"].cpu())
    # a tensor of roots gives a column each
    two = m.pseudotime({"counts": counts}, torch.tensor([0, 319]), k=10, draws=draws)
    assert tuple(two["pseudotime"].shape) == (320, 2) and _same(two["geodesic"][:, 0].cpu(), res["geodesic"].cpu())
    with pytest.raises(ValueError, match="pseudotime: sources must lie in"):
        m.pseudotime({"counts": counts}, 320, k=10, draws=draws)


def test_pseudotime_orders_the_blobs_of_the_chain():
    """On the chain's own graph of lengths, pseudotime from a row of the first blob orders the blobs' means along the
    chain."""
    g, _, truth = chain_lengths()
    m = _model()
    res = m.geodesic(_on_device(graph_numpy(g)), torch.tensor([0]))
    t = geodesic.pseudotime(res["distances"][:, 0]).cpu()
    assert res["converged"] and bool(torch.isfinite(t).all()) and float(t.max()) == 1.0 and float(t[0]) == 0.0
    means = [float(t[truth == b].mean()) for b in range(4)]
    assert means == sorted(means) and means[0] < 0.25 and means[3] > 0.6, means
