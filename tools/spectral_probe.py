"""spmf_graph_spmm and spectral (csrc/spectral.hip) at one C3 row shard: 122 880 rows, the fuzzy graph of knn(k = 15)
on a trained-like embedding (32 centres 4 N(0, I) with unit noise, K = 32).

Timed with device events after a warm-up, `--calls` calls each, the two alternated, median and spread (min, max):
  graph_spmm   one call: Y = s o (A (s o X)) on a float32 [N, 16] block, one launch;
  torch        ``torch.sparse.mm`` of the same normalised matrix D^-1/2 A D^-1/2, built once as a sparse CSR tensor,
               with the same block.
Beside the times: the bytes a product must move (the index and weight streams, a 64-byte gather and a 4-byte scale
per entry, the block read and written) over the call's time, as a share of the HBM peak -- an end-to-end figure of
the call, launch included, not a kernel's share (the gathers are served by L2 / the Infinity Cache: the block is
7.9 MB); the largest difference between the two products; whether two runs of each agree bit for bit; a whole
``spectral(n_components=2)`` with its outer iterations and products, timed on the host clock around a call that ends
in a read-back -- on that graph (32 separated clusters: 32 eigenvalues at 1) and on the graph of the same rows with
the centres a quarter as far apart.

usage: spectral_probe.py [--rows N] [--calls N] [--out FILE]
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
ap.add_argument("--repeat", type=int, default=50, help="products per timed call: one is too short a window")
ap.add_argument("--out", default=os.path.join("profiles", "spectral_probe.json"))
a = ap.parse_args()

import torch  # noqa: E402

from spmf_amd import PoissonFactorization, _lib, spectral  # noqa: E402

HBM_PEAK = 8.0e12             # bytes / s (MI355X)
dev = torch.device("cuda", 0)
N, K = a.rows, a.latent
m = PoissonFactorization(latent_dim=K, feature_dim=64, initialize_distributions=False, device=dev)
gen = torch.Generator(device=dev).manual_seed(4)
centres = 4.0 * torch.randn(32, K, device=dev, generator=gen)
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
    return {"median_ms": round(statistics.median(ms) / per, 5), "min_ms": round(min(ms) / per, 5),
            "max_ms": round(max(ms) / per, 5), "calls": len(ms), "products_per_call": per}


nn = m.knn(pts, k=a.k)
g = m.fuzzy_graph(nn["indices"], nn["distances"])
nnz = int(g["indices"].numel())
deg = torch.diff(g["indptr"])
ops = spectral.LibraryOps(_lib.load(), m._handle(), g["indptr"], g["indices"], g["weights"])
s = ops.scale()
x = torch.randn(N, spectral.BLOCK, device=dev, generator=gen)
y = torch.empty_like(x)

row = torch.repeat_interleave(torch.arange(N, device=dev), deg)
vals = s[row] * g["weights"] * s[g["indices"].long()]
S = torch.sparse_csr_tensor(g["indptr"], g["indices"].long(), vals, size=(N, N))


def ours():
    for _ in range(a.repeat):
        ops.spmm(x, out=y)


def theirs():
    for _ in range(a.repeat):
        torch.sparse.mm(S, x)


t_ours, t_torch = timed([ours, theirs], a.calls)
y_a = ops.spmm(x).clone()
y_b = ops.spmm(x).clone()
z_a, z_b = torch.sparse.mm(S, x), torch.sparse.mm(S, x)
torch.cuda.synchronize()


def spectral_run(graph):
    """``spectral(n_components=2)`` on ``graph``: a first call, then three timed on the host clock."""
    walls, res = [], None
    for _ in range(1 + 3):
        t0 = time.perf_counter()
        res = m.spectral(graph, n_components=2)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    again = m.spectral(graph, n_components=2)
    return {"n_components": 2, "nnz": int(graph["indices"].numel()), "first_call_ms": round(walls[0], 2),
            "median_ms": round(statistics.median(walls[1:]), 2), "min_ms": round(min(walls[1:]), 2),
            "max_ms": round(max(walls[1:]), 2), "calls": len(walls) - 1, "n_iter": res["n_iter"],
            "n_products": res["n_products"], "converged": res["converged"],
            "values": [float(v) for v in res["values"]], "largest_residual": float(res["residuals"].max()),
            "n_unit": res["n_unit"],
            "bit_equal_twice": bool(torch.equal(res["vectors"].view(torch.int32), again["vectors"].view(torch.int32)))}


# the same rows with the centres a quarter as far apart: the clusters overlap and the graph is (nearly) connected,
# so the eigenvalues behind the first are no longer 1 and the filter has work to do
near = (0.25 * centres[torch.randint(0, 32, (N,), device=dev, generator=gen)]
        + torch.randn(N, K, device=dev, generator=gen)).contiguous()
nn_near = m.knn(near, k=a.k)
g_near = m.fuzzy_graph(nn_near["indices"], nn_near["distances"])

# what a product must move: per entry the index, the weight, the neighbour's scale and its 64-byte row; per row
# the list bounds, its scale, its row of X read and its row of Y written
product_bytes = nnz * (4 + 4 + 4 + 64) + N * (16 + 4 + 64 + 64)
per_product_us = statistics.median(t_ours) * 1e3 / a.repeat
out = {"shape": {"rows": N, "K": K, "k": a.k, "nnz": nnz, "degree_mean": round(nnz / N, 2), "degree_max": int(deg.max()),
                 "block_cols": spectral.BLOCK},
       "graph_spmm": stats(t_ours, a.repeat), "torch_sparse_mm": stats(t_torch, a.repeat),
       "speedup_over_torch": round(statistics.median(t_torch) / statistics.median(t_ours), 2),
       "graph_spmm_us_per_product": round(per_product_us, 2),
       "product_bytes": product_bytes,
       "bytes_per_s_end_to_end": round(product_bytes / (per_product_us * 1e-6), 0),
       "share_of_hbm_peak_end_to_end": round(product_bytes / (per_product_us * 1e-6) / HBM_PEAK, 4),
       "max_abs_difference_of_the_two_products": float((y_a - z_a).abs().max()),
       "graph_spmm_bit_equal_twice": bool(torch.equal(y_a.view(torch.int32), y_b.view(torch.int32))),
       "torch_bit_equal_twice": bool(torch.equal(z_a.view(torch.int32), z_b.view(torch.int32))),
       "spectral": spectral_run(g), "spectral_overlapping_clusters": spectral_run(g_near)}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
