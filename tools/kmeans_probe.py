"""One Lloyd step (spmf_kmeans_step, csrc/kmeans.hip) against the route a user had before it, at 1 000 000 x 32
standard-normal points with G = 64 and G = 1 024 centroids (rows of the points).

  step   the library call: knn's selection and refinement of the nearest centroid, the ordering of the rows by
         label, the fp64 sums in a fixed order, the counts and the three statistics; outputs and scratch are
         allocated inside the timed call, as the route's are;
  route  knn(centroids, k=4, queries=points), its first column, index_add_ of points.double() into a zeroed
         [G, 32] fp64 array (float atomics: not reproducible) and bincount.
Both are timed with device events around the whole call, `--calls` calls per round, the two alternated for
`--rounds` rounds after a warm-up so that both see the same machine; median and spread (min, max) over all calls.
The expectation: the step's median is not above the route's median plus the route's own spread (max - min).  Also
reported: whether the labels agree, the largest relative difference of the sums, and whether two steps return the
same bits.

usage: kmeans_probe.py [--rows N] [--width K] [--calls N] [--rounds N] [--out FILE]
       -> one JSON line, also written to FILE
       kmeans_probe.py --once G: a single step, for a kernel trace"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--width", type=int, default=32)
ap.add_argument("--clusters", type=int, nargs="+", default=[64, 1024])
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--once", type=int, default=None, help="one step with this many centroids and nothing else: the "
                "command for `rocprofv3 --kernel-trace --stats`")
ap.add_argument("--out", default=os.path.join("profiles", "kmeans_probe.json"))
a = ap.parse_args()

import torch  # noqa: E402

from spmf_amd import PoissonFactorization, _lib  # noqa: E402

dev = torch.device("cuda", 0)
m = PoissonFactorization(latent_dim=3, feature_dim=8, initialize_distributions=False, device=dev)
lib, h = _lib.load(), m._handle()
N, W = a.rows, a.width
points = torch.randn(N, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))


def step(cent):
    G = cent.shape[0]
    out = {"labels": torch.empty(N, dtype=torch.int32, device=dev),
           "distances": torch.empty(N, dtype=torch.float32, device=dev),
           "sums": torch.empty(G, W, dtype=torch.float64, device=dev),
           "counts": torch.empty(G, dtype=torch.int64, device=dev),
           "stats": torch.empty(3, dtype=torch.float64, device=dev)}
    _lib.check(h, lib.spmf_kmeans_step(
        h, points.data_ptr(), N, W, cent.data_ptr(), G, None, out["labels"].data_ptr(), out["distances"].data_ptr(),
        out["sums"].data_ptr(), out["counts"].data_ptr(), out["stats"].data_ptr(),
        *_lib.Scratch(dev).fit(lib.spmf_kmeans_scratch_bytes(h, N, G, W)), torch.cuda.current_stream(dev).cuda_stream),
        "spmf_kmeans_step")
    return out


def route(cent):
    G = cent.shape[0]
    nn = m.knn(cent, k=min(4, G), queries=points)
    labels = nn["indices"][:, 0].to(torch.int64)
    sums = torch.zeros(G, W, dtype=torch.float64, device=dev).index_add_(0, labels, points.double())
    return {"labels": labels, "distances": nn["distances"][:, 0], "sums": sums,
            "counts": torch.bincount(labels, minlength=G)}


def timed(fn, calls):
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "calls": len(ms)}


if a.once is not None:
    out = step(points[:a.once].contiguous())
    torch.cuda.synchronize()
    print(json.dumps({"once": True, "labelled": int((out["labels"] >= 0).sum())}))
    sys.exit(0)

res = {"shape": {"rows": N, "width": W, "points": "standard normal", "centroids": "the first G points"}, "cases": {}}
for G in a.clusters:
    cent = points[:G].contiguous()
    for fn in (step, route):                     # warm-up: code objects, the allocator's blocks
        for _ in range(2):
            fn(cent)
    torch.cuda.synchronize()
    t_step, t_route = [], []
    for _ in range(a.rounds):
        t_step += timed(lambda: step(cent), a.calls)
        t_route += timed(lambda: route(cent), a.calls)
    s1, s2, r = step(cent), step(cent), route(cent)
    torch.cuda.synchronize()
    scale = r["sums"].abs().clamp_min(1e-300)
    st, rt = stats(t_step), stats(t_route)
    limit = rt["median_ms"] + (rt["max_ms"] - rt["min_ms"])
    res["cases"][f"G{G}"] = {
        "step": st, "route": rt, "limit_ms": round(limit, 3), "within_expectation": st["median_ms"] <= limit,
        "scratch_bytes": int(lib.spmf_kmeans_scratch_bytes(h, N, G, W)),
        "labels_equal": bool(torch.equal(s1["labels"].to(torch.int64), r["labels"])),
        "counts_equal": bool(torch.equal(s1["counts"], r["counts"])),
        "max_relative_sum_difference": float(((s1["sums"] - r["sums"]).abs() / scale).max()),
        "two_steps_same_bits": bool(torch.equal(s1["sums"].view(torch.int64), s2["sums"].view(torch.int64)) and
                                    torch.equal(s1["stats"].view(torch.int64), s2["stats"].view(torch.int64)))}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
