"""spmf_graph_group_edges and paga (csrc/graph_groups.hip) at one C3 row shard: 122 880 rows, the fuzzy graph of
knn(k = 15) on a trained-like embedding (32 centres N(0, I) with unit noise, K = 32: clusters that overlap), the graph
of tools/communities_probe.py, under two labellings: the labels ``communities`` finds there, and row // 120, which
gives 1 024 groups of consecutive rows.

Timed with device events after a warm-up, `--calls` calls of `--repeat` reductions each, the two alternated, median
and spread (min, max):
  group_edges  one call: the two zero fills, the launches of the ordering and the reduction;
  torch        the same integers in torch on the device: lab[row] G + lab[col] as the key of the counting entries, an
               int64 ``index_add_`` of the weights and of ones into G^2 zeros, and a ``bincount`` of the labels; it
               must give the same three arrays.
Beside the times: whether the two agree and two calls give the same bits; the share of the entries inside their own
group; ``model.paga`` and ``model.paga_init`` end to end on the host clock around a call that ends in a read-back.
There is no time of an earlier commit to compare with: the call is new.

usage: paga_probe.py [--rows N] [--calls N] [--out FILE]
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
ap.add_argument("--repeat", type=int, default=10, help="reductions per timed call: one is too short a window")
ap.add_argument("--out", default=os.path.join("profiles", "paga_probe.json"))
a = ap.parse_args()

import torch  # noqa: E402

from spmf_amd import PoissonFactorization, _lib, communities, paga  # noqa: E402

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
            "max_us": round(max(ms) / per * 1e3, 2), "calls": len(ms), "reductions_per_call": per}


def torch_group_edges(row, col, wq, lab, G):
    """The definition in torch on the device, (row, col, wq) being the counting entries' columns and weights."""
    a_, b_ = lab[row], lab[col]
    keep = (a_ >= 0) & (a_ < G) & (b_ >= 0) & (b_ < G)
    key = a_[keep] * G + b_[keep]
    weight = torch.zeros(G * G, dtype=torch.int64, device=key.device).index_add_(0, key, wq[keep])
    count = torch.zeros(G * G, dtype=torch.int64, device=key.device).index_add_(0, key, torch.ones_like(key))
    size = torch.bincount(lab[(lab >= 0) & (lab < G)], minlength=G)
    return count.reshape(G, G), weight.reshape(G, G), size


nn = m.knn(pts, k=a.k)
g = m.fuzzy_graph(nn["indices"], nn["distances"])
nnz = int(g["indices"].numel())
lib, h = _lib.load(), m._handle()
ops = paga.LibraryOps(lib, h, g["indptr"], g["indices"], g["weights"])
n, row, col, wq = communities._valid(*ops.g)
found = m.communities(g)
labellings = (("communities", found["labels"], found["n_communities"]),
              ("row_blocks", torch.arange(N, device=dev) // 120, (N + 119) // 120))
reduce = {}
for name, lab64, G in labellings:
    lab64 = lab64.to(torch.int64)
    lab32 = lab64.to(torch.int32).contiguous()

    def ours():
        for _ in range(a.repeat):
            ops.group_edges(lab32, G)

    def theirs():
        for _ in range(a.repeat):
            torch_group_edges(row, col, wq, lab64, G)
    t_ours, t_torch = timed([ours, theirs], a.calls)
    got, again, want = ops.group_edges(lab32, G), ops.group_edges(lab32, G), torch_group_edges(row, col, wq, lab64, G)
    inside = int(torch.diagonal(got[0]).sum())
    reduce[name] = {"n_groups": G, "group_edges": stats(t_ours, a.repeat), "torch": stats(t_torch, a.repeat),
                    "speedup_over_torch": round(statistics.median(t_torch) / statistics.median(t_ours), 2),
                    "entries_counted": int(got[0].sum()), "share_inside_own_group": round(inside / max(nnz, 1), 4),
                    "pairs_nonzero": int((got[0] > 0).sum()),
                    "equal_to_torch": all(bool(torch.equal(x, y)) for x, y in zip(got, want)),
                    "bit_equal_twice": all(bool(torch.equal(x, y)) for x, y in zip(got, again))}


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


end_to_end = {}
for name, lab64, G in labellings:
    res, t = whole(lambda: m.paga(g, lab64, n_groups=G))
    conn = res["connectivities"]
    t.update(n_groups=G, pairs_connected=int((conn > 0).sum()) // 2,
             tree_pairs=int((res["connectivities_tree"] > 0).sum()) // 2)
    end_to_end["paga_" + name] = t
    start, t = whole(lambda: m.paga_init(g, lab64, n_groups=G, seed=0))
    again = m.paga_init(g, lab64, n_groups=G, seed=0)
    t.update(n_groups=G, bit_equal_twice=bool(torch.equal(start["init"], again["init"])),
             finite=bool(torch.isfinite(start["init"]).all()))
    end_to_end["paga_init_" + name] = t

out = {"shape": {"rows": N, "K": K, "k": a.k, "nnz": nnz, "degree_mean": round(nnz / N, 2),
                 "degree_max": int(torch.diff(g["indptr"]).max()),
                 "bytes_streamed_floor": 16 * nnz, "floor_note": "12 B of index and weight and one 4 B label gather "
                 "per entry: an argument, not a measurement"},
       "group_edges": reduce, "end_to_end": end_to_end}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
