"""graph_layout (csrc/graph_layout.hip) at one C3 row shard: 122 880 rows, the fuzzy graph of knn(k = 15) on a
trained-like embedding (32 centres 4 N(0, I) with unit noise, K = 32), 200 epochs, M = 8 negatives, 'pca' start.

Timed with device events after a warm-up, `--calls` calls each, the two alternated, median and spread (min, max):
  graph_layout   the call: 200 launches behind one copy;
  torch          the same epoch written in torch on the same card: the gather of both endpoints, the clipped terms,
                 ``index_add_`` over the rows (float atomics: not reproducible), the negatives from torch.randint,
                 about twenty launches an epoch.
Beside the times: the bytes an epoch must move (the index and weight streams, one 8-byte gather per entry and per
negative, the positions read and written) over the call's time per epoch, as a share of the HBM peak -- an
end-to-end figure of the call, launches included, not a kernel's share; whether two runs of each agree bit for
bit; the largest difference between the two layouts' first epoch (they draw different negatives, so later epochs
are not comparable); the time of fuzzy_graph and knn on the same points.

usage: umap_probe.py [--rows N] [--calls N] [--epochs N] [--out FILE]
       -> one JSON line, also written to FILE"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=122_880)
ap.add_argument("--latent", type=int, default=32)
ap.add_argument("--k", type=int, default=15)
ap.add_argument("--epochs", type=int, default=200)
ap.add_argument("--negatives", type=int, default=8)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--out", default=os.path.join("profiles", "umap_probe.json"))
a = ap.parse_args()

import torch  # noqa: E402

from spmf_amd import PoissonFactorization, graph  # noqa: E402

HBM_PEAK = 8.0e12             # bytes / s (MI355X)
dev = torch.device("cuda", 0)
N, K, E, M = a.rows, a.latent, a.epochs, a.negatives
m = PoissonFactorization(latent_dim=K, feature_dim=64, initialize_distributions=False, device=dev)
gen = torch.Generator(device=dev).manual_seed(4)
centres = 4.0 * torch.randn(32, K, device=dev, generator=gen)
pts = (centres[torch.randint(0, 32, (N,), device=dev, generator=gen)]
       + torch.randn(N, K, device=dev, generator=gen)).contiguous()


def timed(fns, calls, warmup=1):
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


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "calls": len(ms)}


nn = m.knn(pts, k=a.k)
g = m.fuzzy_graph(nn["indices"], nn["distances"])
y0 = graph.init_pca(pts)
ab = graph.find_ab(0.1, 1.0)
nnz = int(g["indices"].numel())
deg = torch.diff(g["indptr"])

row = torch.repeat_interleave(torch.arange(N, device=dev), deg)
col = g["indices"].long()
w = g["weights"]
W = torch.zeros(N, device=dev).index_add_(0, row, w)
A, B = (torch.tensor(v, dtype=torch.float32, device=dev) for v in ab)


def clipped(d, near):
    """The clipped step of each pair: ``d`` [.., 2] the differences, ``near``: attraction (else repulsion)."""
    d2 = (d * d).sum(-1)
    live = d2 > 0
    s = torch.where(live, d2, torch.ones_like(d2))
    q = A * s ** B
    c = -2.0 * B * q / (s * (1.0 + q)) if near else 2.0 * B / ((0.001 + s) * (1.0 + q))
    return (torch.where(live, c, torch.zeros_like(c)).unsqueeze(-1) * d).clamp(-4.0, 4.0)


def torch_layout(seed=0, epochs=None):
    tg = torch.Generator(device=dev).manual_seed(seed)
    y = y0.clone()
    scale = (5.0 / M * W).unsqueeze(1)
    inv = 1.0 / W.clamp_min(1.0).unsqueeze(1)
    for e in range(E if epochs is None else epochs):
        alpha = 1.0 - e / E
        F = torch.zeros(N, 2, device=dev).index_add_(0, row, w.unsqueeze(1) * clipped(y[row] - y[col], True))
        r = torch.randint(0, N, (N, M), device=dev, generator=tg)
        F += scale * clipped(y.unsqueeze(1) - y[r], False).sum(1)
        y = y + alpha * F * inv
    return y


def ours(epochs=None, **kw):
    return m.graph_layout(g, y0, n_epochs=E if epochs is None else epochs, a=ab[0], b=ab[1], n_negatives=M,
                          **kw)["embedding"]


t_ours, t_torch = timed([ours, torch_layout], a.calls)
t_graph, t_knn = timed([lambda: m.fuzzy_graph(nn["indices"], nn["distances"]), lambda: m.knn(pts, k=a.k)], a.calls)
y_a, y_b = ours(), ours()
z_a, z_b = torch_layout(), torch_layout()
torch.cuda.synchronize()
# one epoch without repulsion: the two differ by the order of the sums alone
first = ours(1, negative_rate=0.0)
tg_first = y0 + (1.0 / W.clamp_min(1.0).unsqueeze(1)) * torch.zeros(N, 2, device=dev).index_add_(
    0, row, w.unsqueeze(1) * clipped(y0[row] - y0[col], True))
# what an epoch must move: indices + weights + one position per entry, per row the list bounds, M positions,
# the row's own position and its new one
epoch_bytes = nnz * (4 + 4 + 8) + N * (16 + 8 * M + 8 + 8)
per_epoch_us = statistics.median(t_ours) * 1e3 / E
out = {"shape": {"rows": N, "K": K, "k": a.k, "nnz": nnz, "degree_mean": round(nnz / N, 2), "degree_max": int(deg.max()),
                 "epochs": E, "negatives": M, "a": ab[0], "b": ab[1]},
       "graph_layout": stats(t_ours), "torch": stats(t_torch),
       "speedup_over_torch": round(statistics.median(t_torch) / statistics.median(t_ours), 2),
       "graph_layout_us_per_epoch": round(per_epoch_us, 2),
       "torch_us_per_epoch": round(statistics.median(t_torch) * 1e3 / E, 2),
       "epoch_bytes": epoch_bytes,
       "bytes_per_s_end_to_end": round(epoch_bytes / (per_epoch_us * 1e-6), 0),
       "share_of_hbm_peak_end_to_end": round(epoch_bytes / (per_epoch_us * 1e-6) / HBM_PEAK, 4),
       "graph_layout_bit_equal_twice": bool(torch.equal(y_a.view(torch.int32), y_b.view(torch.int32))),
       "torch_bit_equal_twice": bool(torch.equal(z_a.view(torch.int32), z_b.view(torch.int32))),
       "first_epoch_attraction_max_abs_difference": float((first - tg_first).abs().max()),
       "extent": {"graph_layout": float(y_a.abs().max()), "torch": float(z_a.abs().max())},
       "fuzzy_graph": stats(t_graph), "knn": stats(t_knn)}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
