"""Host side of the spectral calls (PoissonFactorization.spectral / spectral_cluster, spmf_graph_scale,
spmf_graph_spmm, spmf_block_gram, spmf_block_rotate, csrc/spectral.hip): the leading eigenvectors of
S = D^-1/2 A D^-1/2 of the graph ``fuzzy_graph`` returns -- the spectral start of a layout (umap-learn's default
``init``), a spectral embedding / diffusion map of the rows (sklearn's ``SpectralEmbedding``, scanpy's
``tl.diffmap``) and the features of spectral clustering (Ng, Jordan, Weiss).  Importable without a GPU; numpy and
torch only.

The solver (``solve``) is written once over four operations on float32 [N, 16] blocks -- ``scale``, ``spmm``,
``gram``, ``rotate``, the definitions of include/spmf_hip.h -- and has two backends: ``LibraryOps``, the library's
calls on the device (the product), and ``NumpyOps``, a float32 numpy restatement of the same four definitions
(sequential sums in list order for ``spmm``, fp64 for ``gram`` and ``rotate``), which the host tests run on and
which the error bar of the GPU tests is measured with.  ``normalized_dense`` and ``reference`` are the fp64
restatement the results are held against.

Algorithm: Chebyshev-filtered subspace iteration on a block of 16 columns.
  1. start: ``torch.randn`` of a CPU generator seeded with ``seed``, fp64 rounded to float32; rows with scale 0 (no
     valid edge) are set to 0 and every later step keeps them 0;
  2. orthonormalise, twice: normalise the columns, G = X^T X (``gram``), ``eigh`` of G on the CPU in fp64,
     X <- X Q L^-1/2 (``rotate``) -- not Cholesky, which fails on a filtered block;
  3. Rayleigh-Ritz: W = S X, H = X^T W symmetrised, ``eigh``, X <- X Q with the values in descending order;
  4. residuals: R = S X - X L as ONE ``spmm`` with the per-column coefficient, then the diagonal of R^T R --
     formed explicitly: |S x|^2 - l^2 of a float32 block cancels at about 3e-4;
  5. stop when the residuals of the columns 0 .. m are <= tol, or after ``max_iter`` outer iterations;
  6. else filter on [-1, cut], cut the block's smallest Ritz value, c = (cut - 1) / 2, e = (cut + 1) / 2:
     Y_1 = (S X - c X) / e, Y_{t+1} = 2 (S Y_t - c Y_t) / e - Y_{t-1}, each step one ``spmm`` written over Y_{t-1};
  7. the degree is the largest d <= 20, at least 2, with cosh(d acosh((1 - c) / e)) <= 1e4: what the filter adds
     to the dominant vector then stays above float32's rounding of the others;
  8. back to 2.
Where more than 16 eigenvalues crowd the top of the spectrum -- more than 16 components, each a 1 -- the block's
smallest Ritz value rises into the crowd, and a filter cut there has no gain left for what is still to be damped
below it: the residuals stall.  So when an outer iteration has not halved the largest residual and the gain of the
wanted column m would be below 1.1, that iteration's cut is lowered to where degree 20 gives l_m the gain 1e4 (0.882
for l_m = 1): everything below is damped at once, and the crowd between is damped by its distance from l_m.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _args, _lib

BLOCK = 16                 # include/spmf_hip.h SPMF_BLOCK_COLS
MAX_COMPONENTS = 12
MIN_ROWS = 32              # rows with a valid edge below which dense eigh is the tool
MAX_DEGREE = 20
FILTER_GAIN = 1.0e4
MIN_GAIN = 1.1             # of the wanted column m per filter, below which a stalled iteration lowers the cut
_MIN_HALF_WIDTH = 0.05     # of the filter's interval: a cut at -1 would leave none


# ---- arguments ---------------------------------------------------------------------------------------------------
def check_args(name, n_components, tol, max_iter, seed):
    """The arguments of ``solve`` / ``spectral`` that need no graph -> (m, tol, max_iter, seed)."""
    m = _args.integer(name, "n_components", n_components, 1, MAX_COMPONENTS)
    max_iter = _args.integer(name, "max_iter", max_iter, 1, 2 ** 31 - 1)
    seed = _args.integer(name, "seed", seed, 0, 2 ** 63 - 1)
    return m, _args.number(name, "tol", tol, positive=True), max_iter, seed


def too_few_rows(name, n_live):
    return ValueError(f"{name}: {n_live} rows have a valid edge, fewer than the {MIN_ROWS} a block of {BLOCK} "
                      f"columns needs: use a dense eigh (spmf_amd.spectral.reference) on such a graph")


# ---- the fp64 restatement ------------------------------------------------------------------------------------------
def _arrays(graph):
    """(indptr, indices, weights) of a graph dict (tensors or arrays) as numpy."""
    def host(v):
        return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    return host(graph["indptr"]), host(graph["indices"]), host(graph["weights"])


def valid_edges(graph):
    """The entries that count under the library's rules -- indptr clamped to [0, nnz], a falling indptr an empty
    row, index in [0, N), weight finite and > 0 -- in list order -> (N, row int64, col int64, weight float32)."""
    from .graph import _edges
    indptr, indices, weights = _arrays(graph)
    n, nnz = len(indptr) - 1, len(indices)
    row, col, w = _edges(indptr, indices, weights, n, nnz)
    w = w.astype(np.float32)                              # exact: the fp64 copy of a float32
    with np.errstate(invalid="ignore"):
        keep = (col >= 0) & (col < n) & np.isfinite(w) & (w > 0)
    return n, row[keep], col[keep], w[keep]


def degrees(graph):
    """fp64 [N]: the sum of every row's valid weights."""
    n, row, _, w = valid_edges(graph)
    return np.bincount(row, weights=w.astype(np.float64), minlength=n).astype(np.float64)


def normalized_dense(graph):
    """S = D^-1/2 A D^-1/2 as a dense fp64 [N, N] array under the skip rules (a row without a valid entry has
    scale 0; an entry listed twice adds up)."""
    n, row, col, w = valid_edges(graph)
    d = np.bincount(row, weights=w.astype(np.float64), minlength=n)
    s = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    S = np.zeros((n, n))
    np.add.at(S, (row, col), s[row] * w.astype(np.float64) * s[col])
    return S


def reference(graph, m):
    """``numpy.linalg.eigh`` of ``normalized_dense`` -> (values fp64 [N] descending, vectors fp64 [N, N] in that
    order); the first ``m + 1`` are what ``solve(n_components=m)`` approximates."""
    val, vec = np.linalg.eigh(normalized_dense(graph))
    return val[::-1].copy(), vec[:, ::-1].copy()


# ---- the two backends ----------------------------------------------------------------------------------------------
class NumpyOps:
    """The four definitions of include/spmf_hip.h in float32 numpy on a graph dict: what ``restate32`` is to
    ``graph_layout``.  Blocks are numpy float32 [N, 16]."""

    def __init__(self, graph):
        self.n, self.row, self.col, self.w = valid_edges(graph)
        d = np.bincount(self.row, weights=self.w.astype(np.float64), minlength=self.n)
        self._scale = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0).astype(np.float32)
        # the entries by their position in their row: a product is one vectorised step per position, so a row's
        # additions run in list order
        lens = np.bincount(self.row, minlength=self.n)
        first = np.cumsum(lens) - lens
        self.pos = np.arange(len(self.row)) - first[self.row]
        self.steps = [np.flatnonzero(self.pos == t) for t in range(int(lens.max()) if len(lens) and len(self.row)
                                                                   else 0)]

    def block(self, x):
        return np.ascontiguousarray(x, dtype=np.float32)

    def host(self, x):
        return x

    def tensor(self, x):
        return torch.from_numpy(np.ascontiguousarray(x))

    def scale(self):
        return self._scale

    def spmm(self, x, cs=1.0, cx=None, cz=0.0, z=None, out=None, scaled=True):
        f = np.float32
        cx = np.zeros(BLOCK, dtype=f) if cx is None else np.asarray(cx, dtype=np.float64).astype(f)
        s = self._scale if scaled else np.ones(self.n, dtype=f)
        acc = np.zeros((self.n, BLOCK), dtype=f)
        t = (self.w * s[self.col]).astype(f)
        with np.errstate(invalid="ignore", over="ignore"):
            for e in self.steps:
                acc[self.row[e]] += t[e, None] * x[self.col[e]]
            y = cx[None, :] * x + (f(cs) * s)[:, None] * acc
            if z is not None and cz != 0.0:
                y = f(cz) * z + y
        y = y.astype(f)
        if out is not None:
            out[...] = y
            return out
        return y

    def gram(self, x, y):
        return x.astype(np.float64).T @ y.astype(np.float64)

    def rotate(self, x, r, out=None):
        y = (x.astype(np.float64) @ np.asarray(r, dtype=np.float64)).astype(np.float32)
        if out is not None:
            out[...] = y
            return out
        return y


class LibraryOps:
    """The library's four calls on the graph's device tensors.  Blocks are float32 [N, 16] device tensors;
    ``gram`` reads its 256 doubles back (the one synchronisation of a step)."""

    def __init__(self, lib, handle, indptr, indices, weights):
        self.lib, self.h = lib, handle
        self.g = (indptr.contiguous(), indices.contiguous(), weights.contiguous())
        self.n, self.nnz = int(indptr.numel()) - 1, int(indices.numel())
        self.device = indptr.device
        self._gram = torch.empty(BLOCK * BLOCK, dtype=torch.float64, device=self.device)
        self._scratch = _lib.Scratch(self.device)
        self._s = None

    def _call(self, fn, *args, scratch=None):
        _lib.call(self.h, fn, *args, device=self.device, scratch=scratch)

    def _graph(self):
        return (self.n, self.nnz, self.g[0].data_ptr(), self.g[1].data_ptr(), self.g[2].data_ptr())

    def block(self, x):
        return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)

    def host(self, x):
        return x.cpu().numpy()

    def tensor(self, x):
        return x

    def scale(self):
        if self._s is None:
            s = torch.empty(self.n, dtype=torch.float32, device=self.device)
            self._call("spmf_graph_scale", *self._graph(), s.data_ptr())
            self._s = s
        return self._s

    def spmm(self, x, cs=1.0, cx=None, cz=0.0, z=None, out=None, scaled=True):
        out = torch.empty_like(x) if out is None else out
        c = (C.c_double * BLOCK)(*([0.0] * BLOCK if cx is None else [float(v) for v in cx]))
        self._call("spmf_graph_spmm", *self._graph(), self.scale().data_ptr() if scaled else None, x.data_ptr(),
                   z.data_ptr() if z is not None else None, out.data_ptr(), float(cs), c, float(cz))
        return out

    def gram(self, x, y):
        self._call("spmf_block_gram", self.n, x.data_ptr(), y.data_ptr(), self._gram.data_ptr(),
                   scratch=(self._scratch, "spmf_block_gram_scratch_bytes", self.n))
        return self._gram.cpu().numpy().reshape(BLOCK, BLOCK).copy()

    def rotate(self, x, r, out=None):
        out = torch.empty_like(x) if out is None else out
        r = np.ascontiguousarray(r, dtype=np.float64)
        self._call("spmf_block_rotate", self.n, x.data_ptr(), r.ctypes.data, out.data_ptr())
        return out


# ---- the solver ----------------------------------------------------------------------------------------------------
def filter_degree(c, e):
    """The largest d in 2..MAX_DEGREE with cosh(d acosh((1 - c) / e)) <= FILTER_GAIN (at least 2)."""
    a = math.acosh(max((1.0 - c) / e, 1.0))
    d = MAX_DEGREE if a == 0.0 else int(math.acosh(FILTER_GAIN) / a)
    return max(2, min(MAX_DEGREE, d))


def _gain(x, c, e, d):
    """What a filter of degree ``d`` on [c - e, c + e] multiplies an eigenvalue ``x`` above the interval by."""
    return math.cosh(d * math.acosh(max((x - c) / e, 1.0)))


def filter_interval(lam, m, stalled=False):
    """The filter of an outer iteration from the block's Ritz values ``lam`` (descending) -> (c, e, d): the
    interval [-1, cut] as centre and half-width, and the degree.  cut is the smallest Ritz value, unless the
    iteration is ``stalled`` and the wanted column m would gain less than MIN_GAIN (the module's docstring has the
    reason)."""
    lo = 2.0 * _MIN_HALF_WIDTH - 1.0
    cut = max(float(lam[-1]), lo)
    c, e = 0.5 * (cut - 1.0), 0.5 * (cut + 1.0)
    d = filter_degree(c, e)
    if stalled and _gain(float(lam[m]), c, e, d) < MIN_GAIN:
        tau = math.cosh(math.acosh(FILTER_GAIN) / MAX_DEGREE)
        cut = max(min(cut, (2.0 * float(lam[m]) + 1.0 - tau) / (1.0 + tau)), lo)
        c, e = 0.5 * (cut - 1.0), 0.5 * (cut + 1.0)
        d = filter_degree(c, e)
    return c, e, d


def _orthonormalise(ops, x):
    """Step 2, once, in place: the columns normalised, then X <- X Q L^-1/2 of the eigh of X^T X."""
    g = ops.gram(x, x)
    d = np.diag(g)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(d > 0, 1.0 / np.sqrt(d), 0.0)
    ops.rotate(x, np.diag(inv), out=x)
    g = ops.gram(x, x)
    lam, q = np.linalg.eigh(0.5 * (g + g.T))
    keep = lam > 1e-10 * max(float(lam[-1]), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = q * np.where(keep, 1.0 / np.sqrt(np.where(keep, lam, 1.0)), 0.0)[None, :]
    ops.rotate(x, r, out=x)


def solve(ops, n_components=2, tol=1e-4, max_iter=100, seed=0, name="spectral"):
    """The ``n_components + 1`` leading eigenpairs of S = D^-1/2 A D^-1/2 of the graph behind ``ops`` (a
    ``LibraryOps`` or a ``NumpyOps``), by the iteration of this module's docstring.

    Returns a dict: 'values' fp64 [m + 1], descending, the first about 1; 'vectors' float32 [N, m + 1] (a tensor
    where the blocks live), unit norm, each with the sign that makes its entry of largest magnitude -- the lowest
    row on a tie -- positive; 'embedding', ``vectors[:, 1:]`` (umap-learn's convention); 'residuals' fp64 [m + 1],
    |S v - l v| of every column; 'converged', 'n_iter' (outer iterations), 'n_products' (calls of ``spmm``);
    'scale' float32 [N], 1 / sqrt(degree), 0 for a row without a valid edge (its row of 'vectors' is exactly 0);
    'n_unit', how many of the values are >= 1 - tol: the number of components of the graph seen so far.

    In a degenerate eigenspace (the 1's of several components among them) the basis returned is whatever the
    seeded start gives: reproducible, not canonical.  An asymmetric graph is not refused; it does not converge.
    Bit-reproducible for a given seed on one machine."""
    m, tol, max_iter, seed = check_args(name, n_components, tol, max_iter, seed)
    scale = ops.scale()
    s_host = ops.host(scale)
    live = s_host != 0
    if int(live.sum()) < MIN_ROWS:
        raise too_few_rows(name, int(live.sum()))
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    start = torch.randn(ops.n, BLOCK, generator=gen, dtype=torch.float64).to(torch.float32).numpy()
    start[~live] = 0.0
    x = ops.block(start)
    w = ops.block(np.zeros_like(start))
    y = ops.block(np.zeros_like(start))
    products, n_iter, converged = 0, 0, False
    values = residuals = last = None
    while True:
        _orthonormalise(ops, x)
        _orthonormalise(ops, x)
        ops.spmm(x, out=w)
        products += 1
        h = ops.gram(x, w)
        lam, q = np.linalg.eigh(0.5 * (h + h.T))
        lam, q = lam[::-1].copy(), q[:, ::-1].copy()
        ops.rotate(x, q, out=x)
        ops.spmm(x, cs=1.0, cx=-lam, out=w)
        products += 1
        res = np.sqrt(np.maximum(np.diag(ops.gram(w, w)), 0.0))
        n_iter += 1
        values, residuals = lam[:m + 1], res[:m + 1]
        converged = bool((residuals <= tol).all())
        if converged or n_iter >= max_iter:
            break
        worst = float(residuals.max())
        c, e, d = filter_interval(lam, m, stalled=last is not None and worst > 0.5 * last)
        last = worst
        ops.spmm(x, cs=1.0 / e, cx=np.full(BLOCK, -c / e), out=y)                     # Y_1, X is Y_0
        prev, cur = x, y
        for _ in range(d - 1):
            ops.spmm(cur, cs=2.0 / e, cx=np.full(BLOCK, -2.0 * c / e), cz=-1.0, z=prev, out=prev)
            prev, cur = cur, prev
        products += d
        x, y = cur, prev
    vec = ops.tensor(x)[:, :m + 1]
    mag = vec.abs()
    rows = torch.arange(ops.n, device=vec.device)[:, None].expand_as(mag)
    first = torch.where(mag == mag.amax(0, keepdim=True), rows, torch.full_like(rows, ops.n)).amin(0)
    sign = torch.where(vec.gather(0, first[None, :]) < 0, -1.0, 1.0).to(vec.dtype)
    vec = (vec * sign).contiguous()
    return {"values": values.copy(), "vectors": vec, "embedding": vec[:, 1:], "residuals": residuals.copy(),
            "converged": converged, "n_iter": n_iter, "n_products": products, "scale": ops.tensor(scale),
            "n_unit": int((values >= 1.0 - tol).sum())}


# ---- what the eigenvectors are for -----------------------------------------------------------------------------------
def layout_init(embedding, seed=0):
    """The spectral start of a layout as umap-learn forms it: the first two columns of ``embedding`` [N, >= 1]
    scaled so that the largest |coordinate| is 10, plus N(0, 1e-4^2) noise from a CPU generator seeded with
    ``seed`` -> float32 [N, 2] on the device of ``embedding``, to pass as ``graph_layout(init=...)``.  A single
    column leaves the second coordinate to the noise."""
    e = torch.as_tensor(embedding)
    if e.dim() != 2 or int(e.shape[1]) < 1:
        raise ValueError(f"layout_init: embedding must be [N, >= 1], got {tuple(e.shape)}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) <= 2 ** 63 - 1:
        raise ValueError(f"layout_init: seed must be an integer in 0..2^63 - 1, got {seed!r}")
    n = int(e.shape[0])
    two = torch.zeros(n, 2, dtype=torch.float64, device=e.device)
    k = min(2, int(e.shape[1]))
    two[:, :k] = e[:, :k].to(torch.float64)
    top = float(two.abs().max()) if n else 0.0
    if top > 0 and math.isfinite(top):
        two = two * (10.0 / top)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    noise = 1e-4 * torch.randn(n, 2, generator=gen, dtype=torch.float64)
    return (two + noise.to(e.device)).to(torch.float32).contiguous()


def diffusion_map(res, t=1):
    """The diffusion map of a ``solve`` result: psi_c = scale o v_c * l_c^t, fp64 [N, m + 1] -- the right
    eigenvectors of the random walk D^-1 A (D^-1 A psi = l psi), scaled by the eigenvalue's t-th power; the first
    column is constant on every component."""
    vec = res["vectors"].to(torch.float64)
    lam = torch.as_tensor(np.asarray(res["values"], dtype=np.float64), device=vec.device)
    return res["scale"].to(torch.float64)[:, None] * vec * lam[None, :] ** t


def cluster_features(res, n_clusters):
    """The rows of ``vectors[:, :n_clusters]`` scaled to unit length (Ng, Jordan, Weiss): float32 [N, n_clusters];
    a zero row (no valid edge) is NaN, which ``kmeans`` labels -1."""
    vec = res["vectors"]
    if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)) \
            or not 1 <= int(n_clusters) <= int(vec.shape[1]):
        raise ValueError(f"cluster_features: n_clusters must be an integer in 1..{int(vec.shape[1])} (the vectors "
                         f"of the result), got {n_clusters!r}")
    f = vec[:, :int(n_clusters)].to(torch.float64)
    norm = f.norm(dim=1, keepdim=True)
    return torch.where(norm > 0, f / norm, torch.full_like(f, float("nan"))).to(torch.float32).contiguous()
