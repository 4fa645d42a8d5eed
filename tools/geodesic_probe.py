"""spmf_graph_relax and geodesic (csrc/graph_paths.hip) at one C3 row shard: 122 880 rows, the symmetric graph of
knn(k = 15) on a trained-like embedding (32 centres N(0, I) with unit noise, K = 32: clusters that overlap), the points
of tools/paga_probe.py, the neighbours' distances as lengths (``geodesic.length_graph``); 16 sources, one block.

Timed with device events after a warm-up, `--calls` calls of `--repeat` sweeps (or products) each, the three alternated,
median and spread (min, max), from a block a few sweeps into the relaxation, where most rows are reached:
  relax   one library call of `--repeat` sweeps: the copy of the start into the scratch, the launches, the fill of
          the "changed" word; per sweep = / repeat;
  spmm    `--repeat` calls of spmf_graph_spmm (no scale, c_x = 0) on the same graph between two blocks: the same
          access pattern and traffic in the (+, x) semiring;
  torch   the same sweep in torch on the device: the gather x[col], one add, ``scatter_reduce_(.., "amin")`` over the
          rows and a minimum with x; whether it gives the same bits is recorded.
Beside the times: whether two calls give the same bits; ``model.geodesic`` end to end on the host clock (a call that
ends in read-backs: one per 16 sweeps) with its sweep count, with and without predecessors; and scipy's fp64
``dijkstra`` for the same 16 sources on the CPU, on the host clock, with the largest relative deviation of the float32
distances from it and the derived bound (n_sweeps + 1) 2^-23.  There is no time of an earlier commit to compare with:
the call is new.

usage: geodesic_probe.py [--rows N] [--calls N] [--out FILE]
       -> one JSON line, also written to FILE"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=122_880)
ap.add_argument("--latent", type=int, default=32)
ap.add_argument("--k", type=int, default=15)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeat", type=int, default=20, help="sweeps per timed call: one is too short a window")
ap.add_argument("--out", default=os.path.join("profiles", "geodesic_probe.json"))
a = ap.parse_args()

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spmf_amd import PoissonFactorization, _lib, geodesic, spectral  # noqa: E402

dev = torch.device("cuda", 0)
N, K = a.rows, a.latent
m = PoissonFactorization(latent_dim=K, feature_dim=64, initialize_distributions=False, device=dev)
gen = torch.Generator(device=dev).manual_seed(4)
centres = torch.randn(32, K, device=dev, generator=gen)
pts = (centres[torch.randint(0, 32, (N,), device=dev, generator=gen)]
       + torch.randn(N, K, device=dev, generator=gen)).contiguous()


def timed(fns, calls, warmup=2):
    """The functions alternated: -> one list of milliseconds per function."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(calls):
        for which, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[which].append(e0.elapsed_time(e1))
    return ms


def stats(ms, per=1):
    return {"median_us": round(statistics.median(ms) / per * 1e3, 2), "min_us": round(min(ms) / per * 1e3, 2),
            "max_us": round(max(ms) / per * 1e3, 2), "calls": len(ms), "sweeps_per_call": per}


nn = m.knn(pts, k=a.k)
g = geodesic.length_graph(nn["indices"], nn["distances"])
indptr, indices, lengths = g["indptr"], g["indices"], g["weights"]
nnz = int(indices.numel())
lib, h = _lib.load(), m._handle()
ops = geodesic.LibraryOps(lib, h, indptr, indices, lengths)
sources = torch.linspace(0, N - 1, geodesic.BLOCK).to(torch.int64)
start = torch.full((N, geodesic.BLOCK), float("inf"), device=dev)
start[sources.to(dev), torch.arange(geodesic.BLOCK, device=dev)] = 0.0
x, _, _ = ops.relax(start, 6)                              # a few sweeps in: most rows are reached
reached = float(torch.isfinite(x).double().mean())
y = torch.empty_like(x)
scratch = _lib.Scratch(dev)
graph_args = (N, nnz, indptr.data_ptr(), indices.data_ptr(), lengths.data_ptr())


def relax_call(n_sweeps, out):
    _lib.call(h, "spmf_graph_relax", *graph_args, x.data_ptr(), out.data_ptr(), None, ops._changed.data_ptr(),
              n_sweeps, device=dev, scratch=(scratch, "spmf_graph_relax_scratch_bytes", N))


zeros16 = (C.c_double * geodesic.BLOCK)()
z = torch.empty_like(x)


def spmm_calls():
    src, dst = x, z
    for _ in range(a.repeat):
        _lib.call(h, "spmf_graph_spmm", *graph_args, None, src.data_ptr(), None, dst.data_ptr(), 1.0, zeros16, 0.0,
                  device=dev)
        src, dst = (z, y) if dst is z else (y, z)


_, row, col, w = spectral.valid_edges({"indptr": indptr, "indices": indices, "weights": lengths})
row_d = torch.from_numpy(row).to(dev)[:, None].expand(-1, geodesic.BLOCK).contiguous()
col_d, w_d = torch.from_numpy(col).to(dev), torch.from_numpy(w).to(dev)[:, None]


def torch_sweep(v):
    t = v[col_d] + w_d
    best = torch.full_like(v, float("inf")).scatter_reduce_(0, row_d, t, "amin")
    return torch.minimum(best, v)


def torch_calls():
    v = x
    for _ in range(a.repeat):
        v = torch_sweep(v)


t_relax, t_spmm, t_torch = timed([lambda: relax_call(a.repeat, y), spmm_calls, torch_calls], a.calls)
one, two = torch.empty_like(x), torch.empty_like(x)
relax_call(1, one)
relax_call(1, two)
want = torch_sweep(x)
sweep = {"relax": stats(t_relax, a.repeat), "spmm": stats(t_spmm, a.repeat), "torch": stats(t_torch, a.repeat),
         "relax_over_spmm": round(statistics.median(t_relax) / statistics.median(t_spmm), 3),
         "speedup_over_torch": round(statistics.median(t_torch) / statistics.median(t_relax), 2),
         "share_of_block_reached": round(reached, 4),
         "equal_to_torch": bool(torch.equal(one.view(torch.int32), want.view(torch.int32))),
         "bit_equal_twice": bool(torch.equal(one.view(torch.int32), two.view(torch.int32)))}


def whole(fn):
    """A first call, then three timed on the host clock, each ending in a read-back."""
    walls = []
    for _ in range(1 + 3):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    return res, {"first_call_ms": round(walls[0], 2), "median_ms": round(statistics.median(walls[1:]), 2),
                 "min_ms": round(min(walls[1:]), 2), "max_ms": round(max(walls[1:]), 2), "calls": len(walls) - 1}


res, t_geo = whole(lambda: m.geodesic(g, sources))
t_geo.update(n_sweeps=res["n_sweeps"], converged=res["converged"], sources=int(sources.numel()),
             rows_unreached=int(torch.isinf(res["distances"][:, 0]).sum()))
with_pred, t_pred = whole(lambda: m.geodesic(g, sources, predecessors=True))
t_pred.update(n_sweeps=with_pred["n_sweeps"],
              same_distances=bool(torch.equal(with_pred["distances"], res["distances"])),
              rows_with_predecessor=int((with_pred["predecessors"][:, 0] >= 0).sum()))
one_by_one = geodesic.solve(ops, sources[:1], sweeps_per_call=1)

import scipy.sparse as sp  # noqa: E402
from scipy.sparse.csgraph import dijkstra  # noqa: E402

mat = sp.csr_matrix((w.astype(np.float64), (col, row)), shape=(N, N))      # entry (i, j) is the edge j -> i
t0 = time.perf_counter()
d64 = dijkstra(mat, directed=True, indices=sources.numpy())
t_scipy = (time.perf_counter() - t0) * 1e3
d32 = res["distances"].cpu().numpy().astype(np.float64)
ok = np.isfinite(d64.T) & (d64.T > 0)
dev_rel = float((np.abs(d32 - d64.T)[ok] / d64.T[ok]).max()) if ok.any() else 0.0

out = {"shape": {"rows": N, "K": K, "k": a.k, "nnz": nnz, "degree_mean": round(nnz / N, 2),
                 "degree_max": int(torch.diff(indptr).max()), "block_cols": geodesic.BLOCK,
                 "bytes_per_sweep_floor": 72 * nnz + 128 * N, "floor_note": "8 B of index and length and one 64 B row "
                 "of the block per entry, a row of the block read and written per row: an argument, not a measurement"},
       "sweep": sweep,
       "end_to_end": {"geodesic": t_geo, "geodesic_predecessors": t_pred,
                      "sweeps_to_converge_source_0_one_per_call": one_by_one["n_sweeps"],
                      "scipy_dijkstra_fp64_cpu": {"ms": round(t_scipy, 1), "sources": int(sources.numel()), "calls": 1},
                      "scipy_over_geodesic": round(t_scipy / t_geo["median_ms"], 1),
                      "largest_relative_deviation_from_fp64": dev_rel,
                      "derived_bound": (res["n_sweeps"] + 1) * 2.0 ** -23,
                      "same_rows_reached": bool(np.array_equal(np.isinf(d32), np.isinf(d64.T)))}}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
