"""spmf_graph_move and communities (csrc/graph_move.hip) at one C3 row shard: 122 880 rows, the fuzzy graph of
knn(k = 15) on a trained-like embedding (32 centres N(0, I) with unit noise, K = 32: clusters that overlap).

Timed with device events after a warm-up, `--calls` calls of `--repeat` sweeps each, the two alternated, median and
spread (min, max), for an up sweep (from the identity labels) and a down sweep (from the labels the up sweep wrote):
  graph_move   one call: both launches of the sweep;
  torch        the same sweep in torch on the device: a sort of row N + label[col], ``unique_consecutive``, an int64
               ``index_add_``, the fp64 scores, an arg-max by two ``scatter_reduce``; it must write the same labels.
Beside the times: whether the two agree; a whole ``communities`` call on the host clock around a call that ends in a
read-back, split into the time of the sweeps (device events around every ``move``) and the rest (the integer sums,
the modularity, the coarse graphs, the launches' host side); sweeps per level and Q; whether two runs give the same
bits; and the wide path alone: a sweep over `--wide-rows` rows of `--wide-len` entries each, every row on the list.

usage: communities_probe.py [--rows N] [--calls N] [--out FILE]
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
ap.add_argument("--wide-rows", type=int, default=2048)
ap.add_argument("--wide-len", type=int, default=1024)
ap.add_argument("--out", default=os.path.join("profiles", "communities_probe.json"))
a = ap.parse_args()

import torch  # noqa: E402

from spmf_amd import PoissonFactorization, _lib, communities  # noqa: E402

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


def torch_sweep(n, row, col, wq, k, labels, tot, gamma, m2, direction):
    """The sweep's definition in torch on the device, the entries (row, col, wq) being the links (no self entry)."""
    lab = labels.to(torch.int64)
    key, order = torch.sort(row * n + lab[col])
    ukey, inv = torch.unique_consecutive(key, return_inverse=True)
    e = torch.zeros(int(ukey.numel()), dtype=torch.int64, device=key.device).index_add_(0, inv, wq[order])
    er = torch.div(ukey, n, rounding_mode="floor")
    ec = ukey - er * n
    own = lab[er]
    e_own = torch.zeros(n, dtype=torch.int64, device=key.device)
    mine = ec == own
    e_own[er[mine]] = e[mine]
    gk = gamma * k.to(torch.float64)
    stay = e_own.to(torch.float64) - (gk * (tot[lab] - k).to(torch.float64)) / float(m2)
    score = e.to(torch.float64) - (gk[er] * tot[ec].to(torch.float64)) / float(m2)
    cand = (ec > own) if direction == 0 else (ec < own)
    score = torch.where(cand, score, torch.full_like(score, float("-inf")))
    best = torch.full((n,), float("-inf"), dtype=torch.float64, device=key.device).scatter_reduce(0, er, score, "amax")
    top = cand & (score == best[er])
    to = torch.full((n,), n, dtype=torch.int64, device=key.device).scatter_reduce(0, er[top], ec[top], "amin")
    go = (to < n) & (best > stay) & (k > 0)
    return torch.where(go, to, lab).to(torch.int32)


nn = m.knn(pts, k=a.k)
g = m.fuzzy_graph(nn["indices"], nn["distances"])
nnz = int(g["indices"].numel())
deg = torch.diff(g["indptr"])
lib, h = _lib.load(), m._handle()
ops = communities.LibraryOps(lib, h, g["indptr"], g["indices"], g["weights"])
n, row, col, wq = ops.edges()
ops.set_level(n, *communities._csr(n, row, col, wq))
m2 = int(wq.sum())
k = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, row, wq)
link = row != col
lrow, lcol, lwq = row[link], col[link], wq[link]
labels0 = torch.arange(n, dtype=torch.int32, device=dev)
tot0 = k.clone()
labels1 = ops.move(labels0, tot0, 1.0, m2, 0)
tot1 = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, labels1.to(torch.int64), k)
sweeps = {}
for name, lab, tot, direction in (("up", labels0, tot0, 0), ("down", labels1, tot1, 1)):
    def ours():
        for _ in range(a.repeat):
            ops.move(lab, tot, 1.0, m2, direction)

    def theirs():
        for _ in range(a.repeat):
            torch_sweep(n, lrow, lcol, lwq, k, lab, tot, 1.0, m2, direction)
    t_ours, t_torch = timed([ours, theirs], a.calls)
    got, again = ops.move(lab, tot, 1.0, m2, direction), ops.move(lab, tot, 1.0, m2, direction)
    want = torch_sweep(n, lrow, lcol, lwq, k, lab, tot, 1.0, m2, direction)
    sweeps[name] = {"graph_move": stats(t_ours, a.repeat), "torch": stats(t_torch, a.repeat),
                    "speedup_over_torch": round(statistics.median(t_torch) / statistics.median(t_ours), 2),
                    "rows_moved": int((got != lab).sum()), "equal_to_torch": bool(torch.equal(got, want)),
                    "bit_equal_twice": bool(torch.equal(got, again))}


class TimedOps(communities.LibraryOps):
    """LibraryOps with device events around every sweep."""

    def __init__(self, *args):
        super().__init__(*args)
        self.events = []

    def move(self, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = super().move(*args)
        e1.record()
        self.events.append((e0, e1))
        return out


def whole():
    """``communities`` on the graph: a first call, then three timed on the host clock; then one through TimedOps."""
    walls, res = [], None
    for _ in range(1 + 3):
        t0 = time.perf_counter()
        res = m.communities(g)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    again = m.communities(g)
    timed_ops = TimedOps(lib, h, g["indptr"], g["indices"], g["weights"])
    t0 = time.perf_counter()
    split = communities.solve(timed_ops)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    kernel = sum(e0.elapsed_time(e1) for e0, e1 in timed_ops.events)
    return {"first_call_ms": round(walls[0], 2), "median_ms": round(statistics.median(walls[1:]), 2),
            "min_ms": round(min(walls[1:]), 2), "max_ms": round(max(walls[1:]), 2), "calls": len(walls) - 1,
            "split_call_ms": round(wall, 2), "split_sweeps_ms": round(kernel, 2),
            "split_host_and_torch_ms": round(wall - kernel, 2), "split_sweeps": len(timed_ops.events),
            "n_communities": res["n_communities"], "modularity": res["modularity"],
            "levels": res["levels"], "sizes_largest": res["sizes"][:8].tolist(),
            "bit_equal_twice": bool(torch.equal(res["labels"], again["labels"])
                                    and res["modularity"] == again["modularity"] and res["levels"] == again["levels"]
                                    and torch.equal(res["labels"], split["labels"]))}


def wide():
    """The wide path alone: ``wide_rows`` rows of ``wide_len`` random entries, random labels, every row listed."""
    R, d = a.wide_rows, a.wide_len
    cpu = torch.Generator().manual_seed(9)
    indptr = (torch.arange(R + 1, dtype=torch.int64) * d).to(dev)
    indices = torch.randint(0, R, (R * d,), generator=cpu, dtype=torch.int32).to(dev)
    w = torch.randint(1, 1 << 24, (R * d,), generator=cpu, dtype=torch.int64).to(dev)
    lab = torch.randint(0, max(R // 16, 1), (R,), generator=cpu, dtype=torch.int32).to(dev)
    wops = communities.LibraryOps(lib, h, indptr, indices, torch.ones(R * d, device=dev))
    wops.set_level(R, indptr, indices, w)
    kk = w.reshape(R, d).sum(1)
    tot = torch.zeros(R, dtype=torch.int64, device=dev).index_add_(0, lab.to(torch.int64), kk)
    mm2 = int(kk.sum())

    def ours():
        wops.move(lab, tot, 1.0, mm2, 0)
    (t,) = timed([ours], a.calls)
    rr = torch.arange(R, device=dev).repeat_interleave(d)
    keep = rr != indices.to(torch.int64)
    want = torch_sweep(R, rr[keep], indices.to(torch.int64)[keep], w[keep], kk, lab, tot, 1.0, mm2, 0)
    got = wops.move(lab, tot, 1.0, mm2, 0)
    med = statistics.median(t)
    return {"rows": R, "entries_per_row": d, "median_ms": round(med, 4), "min_ms": round(min(t), 4),
            "max_ms": round(max(t), 4), "us_per_row": round(med * 1e3 / R, 3),
            "ns_per_entry_pair_over_256": round(med * 1e6 / (R * d * d / 256.0), 4),
            "rows_moved": int((got != lab).sum()), "equal_to_torch": bool(torch.equal(got, want))}


out = {"shape": {"rows": N, "K": K, "k": a.k, "nnz": nnz, "degree_mean": round(nnz / N, 2), "degree_max": int(deg.max()),
                 "rows_longer_than_group": int((deg > communities.GROUP_LEN).sum())},
       "sweep": sweeps, "communities": whole(), "wide_path": wide()}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
