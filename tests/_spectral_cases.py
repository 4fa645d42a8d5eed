"""What the test files of the spectral calls share (test_spectral_host.py, test_gpu_spectral.py,
test_gpu_spectral_cli.py): the argument lists of spmf_graph_scale / spmf_graph_spmm / spmf_block_gram /
spmf_block_rotate, their raw calls and error contracts, asserted without a device on dummy addresses and with one on
real buffers; the three graphs of the end-to-end tests (a cycle, the blobs, two rings) and the fp64 criteria a
result is held to; the cases, coefficient sets, fp64 reference and error unit of the product's per-entry bar."""
import ctypes as C
import functools

import numpy as np
import torch

from _graph_layout_cases import blob_graph, layout_case

_P, _I64, _D = C.c_void_p, C.c_int64, C.c_double
_GRAPH = (("n", _I64), ("nnz", _I64), ("indptr", _P), ("indices", _P), ("weights", _P))
ARGS = {
    "graph_scale": _GRAPH + (("scale", _P), ("stream", _P)),
    "graph_spmm": _GRAPH + (("scale", _P), ("x", _P), ("z", _P), ("y", _P), ("cs", _D), ("cx", _P), ("cz", _D),
                            ("stream", _P)),
    "block_gram": (("n", _I64), ("x", _P), ("y", _P), ("g", _P), ("ptr", _P), ("nbytes", C.c_size_t), ("stream", _P)),
    "block_rotate": (("n", _I64), ("x", _P), ("r", _P), ("y", _P), ("stream", _P)),
}
# the argument counts of include/spmf_hip.h
HEADER_ARGS = {"spmf_graph_scale": 8, "spmf_graph_spmm": 14, "spmf_block_gram_scratch_bytes": 2,
               "spmf_block_gram": 8, "spmf_block_rotate": 6}
BLOCK = 16
CHUNK = 512                # include/spmf_hip.h SPMF_GRAM_CHUNK_ROWS


def raw_call(entry, good):
    """-> call(**overrides): spmf_<entry> through a binding of its own with the arguments of ``good``."""
    from spmf_amd import _lib
    fn = getattr(C.CDLL(_lib.LIB_PATH), "spmf_" + entry)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [t for _, t in ARGS[entry]]

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], *[a[n] for n, _ in ARGS[entry]])
    return call


def host_array(values):
    """A host array of doubles for c_x / r; the caller keeps it alive."""
    values = [float(v) for v in values]
    return (C.c_double * len(values))(*values)


def assert_errors(lib, entry, good, need=None, after=lambda: None):
    """The error contract of spmf_<entry>; every call here returns before a launch or a copy, and ``after`` is run
    behind each (the GPU file checks its sentinels there).  ``good``: the arguments of a valid call (for block_gram
    with a scratch of exactly ``need`` bytes)."""
    call, h = raw_call(entry, good), good["h"]
    nan, inf = float("nan"), float("inf")

    def refused(code, **kw):
        assert call(**kw) == code, (entry, kw)
        msg = lib.spmf_last_error(h).decode()
        assert msg.startswith(entry + ": "), msg
        after()
        return msg
    for rows in (-1, 2 ** 31 - 63, 2 ** 40):
        assert "n_rows" in refused(-1, n=rows)
    if entry in ("graph_scale", "graph_spmm"):
        assert "nnz" in refused(-1, nnz=-1)
        for name in ("indptr", "indices", "weights"):
            assert "null" in refused(-1, **{name: None})
    if entry == "graph_scale":
        assert "null" in refused(-1, scale=None)
    if entry == "graph_spmm":
        for name in ("x", "y", "cx"):
            assert "null" in refused(-1, **{name: None})
        refused(-1, n=0, cx=None)
        assert "z" in refused(-1, z=None, cz=-1.0)
        for v in (nan, inf, -inf, 1e39):
            assert "finite" in refused(-1, cs=v)
            assert "finite" in refused(-1, cz=v)
            bad = host_array([0.0] * 7 + [v] + [0.0] * 8)
            assert "finite" in refused(-1, cx=bad)
        assert "aliases" in refused(-1, y=good["x"])
    if entry == "block_gram":
        for name in ("x", "y", "g", "ptr"):
            assert "null" in refused(-1, **{name: None})
        refused(-1, n=0, g=None)
        refused(-1, n=0, ptr=None)
        assert "aligned" in refused(-1, ptr=good["ptr"] + 4)
        assert str(need) in refused(-3, nbytes=need - 256)
        refused(-3, n=0, nbytes=0)               # errors come before the empty return
    if entry == "block_rotate":
        for name in ("x", "y", "r"):
            assert "null" in refused(-1, **{name: None})
        refused(-1, n=0, r=None)
        for v in (nan, inf, -inf):
            bad = host_array([0.0] * 100 + [v] + [0.0] * 155)
            assert "finite" in refused(-1, r=bad)
    assert call(h=None) == -1


def host_good(entry, h, lib):
    """A valid-looking call of ``entry`` that needs no device: dummy aligned addresses (host arrays where the entry
    reads the host) -- only refused and empty calls may be made with it.  -> (good, need)."""
    good = dict(h=h, n=70, nnz=300, indptr=0x1000000, indices=0x2000000, weights=0x3000000, scale=0x4000000,
                x=0x5000000, z=0x6000000, y=0x7000000, cs=1.0, cx=host_array([0.5] * BLOCK), cz=-1.0,
                g=0x9000000, r=host_array([0.25] * (BLOCK * BLOCK)), ptr=0x8000000, nbytes=0, stream=None)
    need = None
    if entry == "block_gram":
        need = int(lib.spmf_block_gram_scratch_bytes(h, good["n"]))
        good["nbytes"] = need
    return good, need


# ---- the graphs of the end-to-end tests ------------------------------------------------------------------------------
def cycle_graph(n=64):
    """The cycle of ``n`` rows with unit weights: S = A / 2, eigenvalues cos(2 pi k / n), doubly degenerate."""
    idx = np.stack([(np.arange(n) - 1) % n, (np.arange(n) + 1) % n], 1)
    idx.sort(1)
    return {"indptr": torch.arange(0, 2 * n + 1, 2, dtype=torch.int64),
            "indices": torch.as_tensor(idx.reshape(-1), dtype=torch.int32), "weights": torch.ones(2 * n)}


@functools.lru_cache(maxsize=None)
def rings(per=200, k=10, seed=0):
    """Two concentric rings of ``per`` points (radii 1 and 3, radial noise 0.05) -> (the fuzzy graph of their exact
    kNN, the points float32 [2 per, 2], the truth int64 [2 per]); read-only.  The graph has two components."""
    from spmf_amd import graph, neighbors
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    theta = torch.rand(2 * per, generator=gen, dtype=torch.float64) * (2.0 * np.pi)
    truth = torch.arange(2).repeat_interleave(per)
    radius = torch.where(truth == 0, 1.0, 3.0).double() + 0.05 * torch.randn(2 * per, generator=gen,
                                                                             dtype=torch.float64)
    x = torch.stack([radius * torch.cos(theta), radius * torch.sin(theta)], 1).to(torch.float32)
    idx, dist = neighbors.brute_force(x, x, k, exclude_self=True)
    return graph.fuzzy_graph(idx, dist), x, truth


@functools.lru_cache(maxsize=None)
def many_components(n_blobs=20, per=40, dim=8, k=10, seed=3):
    """``n_blobs`` far-apart Gaussian blobs (centres 6 N(0, I), unit noise) -> the fuzzy graph of their exact kNN:
    one component per blob, so more eigenvalues at 1 than a block has columns, and the next at 0.78; read-only."""
    from spmf_amd import graph, neighbors
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    centres = 6.0 * torch.randn(n_blobs, dim, generator=gen, dtype=torch.float64)
    x = centres[torch.arange(n_blobs).repeat_interleave(per)] + torch.randn(n_blobs * per, dim, generator=gen,
                                                                            dtype=torch.float64)
    idx, dist = neighbors.brute_force(x.to(torch.float32), x.to(torch.float32), k, exclude_self=True)
    return graph.fuzzy_graph(idx, dist)


def end_to_end_graphs():
    """(name, graph on the CPU, n_components): the cycle of 64 rows at m = 2, the blobs' graph at m = 7 (7
    components; the first non-degenerate gap, 0.29, is behind them), the rings at m = 1."""
    return (("cycle", cycle_graph(64), 2), ("blobs", blob_graph(), 7), ("rings", rings()[0], 1))


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """The fp64 reference of an end-to-end graph, computed once: (S dense, values descending, vectors)."""
    from spmf_amd import spectral
    g = {n: gr for n, gr, _ in end_to_end_graphs()}[name]
    val, vec = spectral.reference(g, 0)
    return spectral.normalized_dense(g), val, vec


def agreement(labels, truth):
    """The share of rows on which a 2-clustering agrees with the truth, under the better of the two namings."""
    labels, truth = np.asarray(labels), np.asarray(truth)
    a = float((labels == truth).mean())
    return max(a, float((labels == 1 - truth).mean()))


def assert_criteria(name, res, m, tol):
    """The fp64 criteria of a ``solve`` result on the end-to-end graph ``name``:
      every returned residual is within 1e-6 of |S v - l v| recomputed in fp64, and <= tol;
      |l_c - l_c^ref| <= the residual of column c;
      |(I - V_ref V_ref^T) V|_2 <= 2 |R|_F / (l^ref_m - l^ref_{m+1})   (Davis-Kahan; the sine is a projection
      residual, not 1 - cos^2, which bottoms out at 3e-4 for float32 vectors).
    -> the figures, for printing."""
    S, val, vec = reference_of(name)
    V = torch.as_tensor(res["vectors"]).detach().cpu().double().numpy()
    lam, got = np.asarray(res["values"]), np.asarray(res["residuals"])
    assert V.shape == (S.shape[0], m + 1) and lam.shape == got.shape == (m + 1,)
    R = S @ V - V * lam[None, :]
    rn = np.linalg.norm(R, axis=0)
    Vr = vec[:, :m + 1]
    sine = float(np.linalg.norm(V - Vr @ (Vr.T @ V), 2))
    gap = float(val[m] - val[m + 1])
    bound = 2.0 * float(np.linalg.norm(R)) / gap
    fig = dict(residual=float(got.max()), recomputed_off=float(np.abs(rn - got).max()),
               value_off_over_residual=float((np.abs(lam - val[:m + 1]) / np.maximum(got, 1e-300)).max()),
               sine=sine, bound=bound, gap=gap, n_iter=res["n_iter"], n_products=res["n_products"])
    print(f"spectral {name} m={m}: {fig}")
    assert res["converged"] and (got <= tol).all(), fig
    assert (np.abs(rn - got) <= 1e-6).all(), fig
    assert (np.abs(lam - val[:m + 1]) <= got).all(), fig
    assert gap > 1e-4 and sine <= bound, fig
    assert (np.diff(lam) <= 0).all() and abs(lam[0] - 1.0) <= got[0]
    assert np.abs(np.linalg.norm(V, axis=0) - 1.0).max() <= 1e-6
    return fig


def assert_sign_rule(vectors):
    """Every column's entry of largest magnitude, the lowest row on a tie, is positive."""
    V = torch.as_tensor(vectors).detach().cpu().numpy()
    for c in range(V.shape[1]):
        first = int(np.flatnonzero(np.abs(V[:, c]) == np.abs(V[:, c]).max())[0])
        assert V[first, c] > 0, (c, first, V[first, c])


# ---- the product's cases ---------------------------------------------------------------------------------------------
SPMM_SHAPES = [(1, 0), (2, 0), (15, 0), (16, 0), (17, 0), (63, 0), (64, 0), (65, 0), (257, 0), (1000, 700)]


def coefficient_sets():
    """(name, c_s, c_x [16], c_z, with z): the plain product with a null z, the residual's per-column c_x, and a
    step of the filter on [-1, 0.3] (y = 2 (S x - c x) / e - z)."""
    c, e = 0.5 * (0.3 - 1.0), 0.5 * (0.3 + 1.0)
    return (("product", 1.0, np.zeros(BLOCK), 0.0, False),
            ("residual", 1.0, -np.linspace(1.0, -0.35, BLOCK), 0.0, False),
            ("filter", 2.0 / e, np.full(BLOCK, -2.0 * c / e), -1.0, True))


@functools.lru_cache(maxsize=None)
def spmm_case(N, hub):
    """A ``layout_case`` graph (an empty row, a one-edge row, with ``hub`` a 700-entry row) with seeded blocks x and
    z of mixed signs and magnitudes -> dict(indptr, indices, weights, x, z: numpy); read-only."""
    c = layout_case(N, hub)
    rng = np.random.default_rng(5200 + N + hub)
    x = (rng.standard_normal((N, BLOCK)) * np.exp(rng.uniform(-3, 3, size=(N, 1)))).astype(np.float32)
    z = rng.standard_normal((N, BLOCK)).astype(np.float32)
    return dict(indptr=c["indptr"], indices=c["indices"], weights=c["weights"], x=x, z=z)


def spmm_reference(graph, scale, x, z, cs, cx, cz):
    """The definition of spmf_graph_spmm in fp64 on the inputs as given (``scale`` float32 [N] or None, the
    coefficients rounded to float32 once) -> (Y fp64 [N, 16], the bar's scale B fp64 [N, 16]):
    B_i = |c_s| s_i sum_j w_ij s_j |x_j| + |c_x x_i| + |c_z z_i|."""
    from spmf_amd import spectral
    n, row, col, w = spectral.valid_edges(graph)
    s = np.ones(n) if scale is None else np.asarray(scale, dtype=np.float64)
    x64 = np.asarray(x, dtype=np.float64)
    z64 = np.zeros_like(x64) if z is None else np.asarray(z, dtype=np.float64)
    cs, cz = float(np.float32(cs)), float(np.float32(cz))
    cx = np.asarray(cx, dtype=np.float64).astype(np.float32).astype(np.float64)
    t = (w.astype(np.float64) * s[col])[:, None]
    acc, mag = np.zeros((n, BLOCK)), np.zeros((n, BLOCK))
    np.add.at(acc, row, t * x64[col])
    np.add.at(mag, row, t * np.abs(x64[col]))
    y = cs * s[:, None] * acc + cx[None, :] * x64 + cz * z64
    bar = abs(cs) * s[:, None] * mag + np.abs(cx[None, :] * x64) + np.abs(cz * z64)
    return y, bar


def spmm_units(got, ref, bar):
    """max over the entries of |got - ref| / (2^-24 B): the error in units of the per-entry bar."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    ok = bar > 0
    assert (err[~ok] == 0).all()
    return float((err[ok] / (2.0 ** -24 * bar[ok])).max()) if ok.any() else 0.0


def numpy_backend_units():
    """The largest error of the float32 numpy backend against ``spmm_reference`` over SPMM_SHAPES x
    coefficient_sets() x (scaled, unscaled), in the bar's units: what T is 8 times."""
    from spmf_amd import spectral
    worst = 0.0
    for N, hub in SPMM_SHAPES:
        c = spmm_case(N, hub)
        ops = spectral.NumpyOps(c)
        for _, cs, cx, cz, with_z in coefficient_sets():
            for scaled in (True, False):
                z = c["z"] if with_z else None
                got = ops.spmm(c["x"], cs=cs, cx=cx, cz=cz, z=z, scaled=scaled)
                ref, bar = spmm_reference(c, ops.scale() if scaled else None, c["x"], z, cs, cx, cz)
                worst = max(worst, spmm_units(got, ref, bar))
    return worst
