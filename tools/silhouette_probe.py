"""silhouette (csrc/silhouette.hip) at one C3 row shard: 122 880 rows, K = 32, the labels of ``cluster`` with
G = 16: every row's mean distance to every cluster over all N^2 pairs.

Two point sets of that shape: `embedding`, the untrained model's posterior mean encoding of
linear_structure(rows=122 880, D=20 000, density=0.005) over S = 8 draws with the labels ``cluster`` gives it (a
near-collinear cloud with large norms: DESIGN 7f), and `blobs`, a trained-like embedding -- 16 centres 4 N(0, I)
with unit noise -- with the labels of ``kmeans``.

Timed with device events after a warm-up, `--calls` calls each, median and spread (min, max):
  silhouette          the call, on both point sets (and under 'cosine' on the blobs);
  materialising       what a user had before: torch.cdist on `--chunk-rows` query rows against all rows (an
                      [chunk, N] block, about 2 GB) times a one-hot [N, G] matrix, chunks concatenated, then a / b / s
                      in torch;
  knn                 knn(k = 15) on the same points: the same MFMA work with a selection in place of the sums.
Agreement with fp64 on `--sample` rows (torch.cdist in fp64 without the matmul expansion against all rows, the
one-hot sums in fp64): the largest relative error of a and of b, the largest absolute error of s, the share of the
sample whose ``nearest`` is the fp64 argmin.

usage: silhouette_probe.py [--rows N] [--cols D] [--calls N] [--out FILE]
       -> one JSON line, also written to FILE
       silhouette_probe.py --once: a single call on the blobs, for a kernel trace"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=122_880)
ap.add_argument("--cols", type=int, default=20_000)
ap.add_argument("--latent", type=int, default=32)
ap.add_argument("--draws", type=int, default=8)
ap.add_argument("--clusters", type=int, default=16)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--chunk-rows", type=int, default=4096)
ap.add_argument("--sample", type=int, default=1024)
ap.add_argument("--once", action="store_true", help="one call on the blobs and nothing else: the command for "
                "`rocprofv3 --kernel-trace --stats`")
ap.add_argument("--out", default=os.path.join("profiles", "silhouette_probe.json"))
a = ap.parse_args()

import torch  # noqa: E402

from spmf_amd import PoissonFactorization, _lib, synth  # noqa: E402

dev = torch.device("cuda", 0)
N, D, K, S, G = a.rows, a.cols, a.latent, a.draws, a.clusters
m = PoissonFactorization(latent_dim=K, feature_dim=D, u_tau_scale=1.0 / (N * D) ** 0.5, device=dev,
                         panel_rows=a.chunk_rows)
gen = torch.Generator(device=dev).manual_seed(4)
centres = 4.0 * torch.randn(G, K, device=dev, generator=gen)
blobs = (centres[torch.randint(0, G, (N,), device=dev, generator=gen)]
         + torch.randn(N, K, device=dev, generator=gen)).contiguous()
blob_labels = m.kmeans(blobs, G, seed=0)["labels"]
if a.once:
    out = m.silhouette(blobs, blob_labels, G)
    torch.cuda.synchronize()
    print(json.dumps({"once": True, "score": out["score"]}))
    sys.exit(0)


def timed(fn, calls, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
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


def from_sums(sums, counts, lab, self_in=True):
    """a, b, nearest, s from the [rows, G] sums of distances (every row a member of cluster lab >= 0)."""
    rows = torch.arange(sums.shape[0], device=sums.device)
    n = counts.to(sums.dtype)
    ng = n[lab]
    aa = torch.where(ng > 1, sums[rows, lab] / (ng - 1).clamp_min(1), torch.zeros_like(ng))
    mean = sums / n.clamp_min(1)[None, :]
    mean = mean.masked_fill((counts == 0)[None, :], float("inf"))
    mean[rows, lab] = float("inf")
    bb, near = mean.min(1)
    mx = torch.maximum(aa, bb)
    ss = torch.where((ng > 1) & (mx > 0), (bb - aa) / mx, torch.zeros_like(mx))
    return aa, bb, near, ss


def materialising(pts, lab):
    keep = lab >= 0
    onehot = torch.zeros(pts.shape[0], G, device=dev)
    onehot[keep, lab[keep].long()] = 1.0
    counts = onehot.sum(0).long()
    sums = []
    for r0 in range(0, pts.shape[0], a.chunk_rows):
        d = torch.cdist(pts[r0:r0 + a.chunk_rows], pts)
        sums.append(d @ onehot)
        del d
    return from_sums(torch.cat(sums), counts, lab.long().clamp_min(0))


def agreement(pts, lab, out, metric="euclidean"):
    member = lab >= 0
    pool = torch.nonzero(member).flatten()
    pick = pool[torch.randperm(len(pool), generator=torch.Generator().manual_seed(3))[:a.sample].to(dev)].sort().values
    p64 = pts.double()
    if metric == "cosine":
        p64 = p64 / p64.norm(dim=1, keepdim=True)
    onehot = torch.zeros(N, G, device=dev, dtype=torch.float64)
    onehot[member, lab[member].long()] = 1.0
    counts = onehot.sum(0).long()
    sums = []
    for r0 in range(0, len(pick), 64):
        d = torch.cdist(p64[pick[r0:r0 + 64]], p64, compute_mode="donot_use_mm_for_euclid_dist")
        if metric == "cosine":
            d = 0.5 * d * d
        sums.append(d @ onehot)
        del d
    aa, bb, near, ss = from_sums(torch.cat(sums), counts, lab[pick].long())
    ga, gb, gs = (out[k][pick].double() for k in ("a", "b", "silhouette"))
    return {"sample": int(len(pick)),
            "a_max_relative_error": float(((ga - aa).abs() / aa.clamp_min(1e-300)).max()),
            "b_max_relative_error": float(((gb - bb).abs() / bb.clamp_min(1e-300)).max()),
            "s_max_absolute_error": float((gs - ss).abs().max()),
            "nearest_equal_share": float((out["nearest"][pick].long() == near).double().mean()),
            "score_fp64_sample_mean": float(ss.mean()), "score_sample_mean": float(gs.mean())}


sc = synth.linear_structure(N, D, 0.005, dev, panel_rows=a.chunk_rows)
torch.manual_seed(1)
draws = m.surrogate_distribution.sample(S)
res = m.cluster({"counts": sc}, G, draws=draws, seed=0)
emb, emb_labels = res["embedding"], res["labels"]
del sc, res
torch.cuda.empty_cache()

sets = {"embedding": (emb, emb_labels), "blobs": (blobs, blob_labels)}
out = {"shape": {"rows": N, "K": K, "G": G, "S": S, "D": D,
                 "silhouette_scratch_bytes": int(_lib.load().spmf_silhouette_scratch_bytes(m._handle(), N, G, K))},
       "flop_per_call": 2.0 * N * N * K}
for name, (pts, lab) in sets.items():
    t_sil = timed(lambda: m.silhouette(pts, lab, G), a.calls)
    t_knn = timed(lambda: m.knn(pts, k=15), a.calls)
    t_old = timed(lambda: materialising(pts, lab), a.calls, warmup=1)
    r = m.silhouette(pts, lab, G)
    norms = pts.double().norm(dim=1)
    out[name] = {"silhouette": stats(t_sil), "knn": stats(t_knn),
                 "materialising": dict(stats(t_old), chunk_rows=a.chunk_rows),
                 "tflops": round(2.0 * N * N * K / (statistics.median(t_sil) * 1e-3) / 1e12, 2),
                 "speedup_over_materialising": round(statistics.median(t_old) / statistics.median(t_sil), 2),
                 "time_over_knn": round(statistics.median(t_sil) / statistics.median(t_knn), 2),
                 "score": r["score"], "n_scored": r["n_scored"], "counts": r["counts"].tolist(),
                 "norm_min_max": [float(norms.min()), float(norms.max())],
                 "agreement": agreement(pts, lab, r)}
    torch.cuda.empty_cache()
t_cos = timed(lambda: m.silhouette(blobs, blob_labels, G, metric="cosine"), a.calls)
out["blobs"]["silhouette_cosine"] = stats(t_cos)
out["blobs"]["agreement_cosine"] = agreement(blobs, blob_labels, m.silhouette(blobs, blob_labels, G, metric="cosine"),
                                             "cosine")
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
