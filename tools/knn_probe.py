"""embed / knn (csrc/knn.hip) at one C3 row shard: linear_structure(rows=122 880, D=20 000, density=0.005),
K = 32, S = 8, k = 15: every row's 15 nearest other rows in the latent space.

Timed with device events after a warm-up, `--calls` calls each, median and spread (min, max):
  embed               the posterior mean encoding of the shard (prep + encode sweep of 8 draws + the reduction);
  knn_tile0 / _tile1  knn on that embedding with the select kernel's two tile functions (score_block as top_k
                      calls it | the query tile resident in LDS; SPMF_KNN_TILE), timed in alternating halves so
                      that both see the same machine, Euclidean; knn_cosine is the default tile under 'cosine';
  knn_gaussian        the same call on a standard normal cloud of the same shape (no structure, no near-ties);
  materialising       what a user had before: torch.cdist on `--chunk-rows` query rows against all rows (an
                      [chunk, N] block), torch.topk(k + 1), the row itself dropped, chunks concatenated;
  top_k / top_k_parent  top_k(k=10) of this build and of another build of the library (`--parent-lib FILE`), the
                      latter in a child process of its own: the selection moved into select_rows.h.
Agreement with the fp64 reference (spmf_amd.neighbors.brute_force) on `--sample` query rows: recall over all of
them and over the clear-cut ones (gap between the k-th and (k+1)-th squared distance above 2 bar, bar =
2e-5 (|q - c|^2 + |r - c|^2), the rule of tests/test_gpu_knn.py), the largest relative error of a returned
distance, and by how much the returned k-th distance exceeds the true k-th distance (median, max).

usage: knn_probe.py [--rows N] [--cols D] [--calls N] [--parent-lib FILE] [--out FILE]
       -> one JSON line, also written to FILE
       knn_probe.py --once: a single knn call on the embedding, for a kernel trace"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=122_880)
ap.add_argument("--cols", type=int, default=20_000)
ap.add_argument("--latent", type=int, default=32)
ap.add_argument("--draws", type=int, default=8)
ap.add_argument("--k", type=int, default=15)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--slow-calls", type=int, default=None, help="calls of the materialising route (default: --calls)")
ap.add_argument("--chunk-rows", type=int, default=4096)
ap.add_argument("--sample", type=int, default=1024)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--topk-only", action="store_true", help="(the child of --parent-lib) time top_k and print it")
ap.add_argument("--once", action="store_true", help="one knn call on the embedding and nothing else: the command "
                "for `rocprofv3 --kernel-trace --stats`")
ap.add_argument("--out", default=os.path.join("profiles", "knn_probe.json"))
a = ap.parse_args()

parent = None
if a.parent_lib and not a.topk_only:
    # before this process opens the device: a fresh process that loads the other build
    env = dict(os.environ, SPMF_LIB_PATH=os.path.abspath(a.parent_lib))
    cmd = [sys.executable, os.path.abspath(__file__), "--topk-only", "--rows", str(a.rows), "--cols", str(a.cols),
           "--latent", str(a.latent), "--draws", str(a.draws), "--calls", str(a.calls), "--chunk-rows",
           str(a.chunk_rows)]
    done = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=600, check=True)
    parent = json.loads(done.stdout.strip().splitlines()[-1])

import torch  # noqa: E402

from spmf_amd import _lib  # noqa: E402

if a.topk_only:
    # a build from before embed / knn has none of their entry points; nothing here calls them
    for name in ("spmf_embed_rows", "spmf_embed_scratch_bytes", "spmf_knn", "spmf_knn_scratch_bytes"):
        _lib.SIGNATURES.pop(name, None)
from spmf_amd import PoissonFactorization, synth  # noqa: E402
from spmf_amd.neighbors import brute_force, recall  # noqa: E402

dev = torch.device("cuda", 0)
B, D, K, S, k = a.rows, a.cols, a.latent, a.draws, a.k
sc = synth.linear_structure(B, D, 0.005, dev, panel_rows=a.chunk_rows)
m = PoissonFactorization(latent_dim=K, feature_dim=D, u_tau_scale=1.0 / (B * D) ** 0.5, device=dev,
                         panel_rows=a.chunk_rows)
torch.manual_seed(1)
draws = m.surrogate_distribution.sample(S)
batch = {"counts": sc}


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


if a.topk_only:
    print(json.dumps(dict(stats(timed(lambda: m.top_k(batch, k=10, draws=draws), a.calls)),
                          lib=os.path.relpath(_lib.LIB_PATH, ROOT))))
    sys.exit(0)

emb = m.embed(batch, draws=draws)["mean"]
if a.once:
    out = m.knn(emb, k=k)
    torch.cuda.synchronize()
    print(json.dumps({"once": True, "found": int((out["indices"] >= 0).sum())}))
    sys.exit(0)


def with_tile(tile, fn):
    def run():
        os.environ["SPMF_KNN_TILE"] = tile
        try:
            return fn()
        finally:
            del os.environ["SPMF_KNN_TILE"]
    return run


def materialising(pts):
    idx, dist = [], []
    rows = torch.arange(pts.shape[0], device=dev)
    for r0 in range(0, pts.shape[0], a.chunk_rows):
        d = torch.cdist(pts[r0:r0 + a.chunk_rows], pts)
        d[rows[:d.shape[0]], rows[r0:r0 + d.shape[0]]] = float("inf")      # a row is no neighbour of its own
        v, i = torch.topk(d, k, dim=1, largest=False)
        idx.append(i.to(torch.int32))
        dist.append(v)
        del d
    return torch.cat(idx), torch.cat(dist)


def agreement(pts, out, metric="euclidean"):
    """Against brute_force on a sample of the queries; clear-cut rows by the rule of tests/test_gpu_knn.py."""
    pick = torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(3))[:a.sample].to(dev).sort().values
    q = pts[pick]
    # brute_force excludes reference row `offset + i` for query i: one call per run of consecutive rows would be
    # slow, so self goes in as a candidate (k + 2 wanted) and is dropped here
    bi, bd = brute_force(q, pts, k + 2, metric, False)
    keep = bi != pick[:, None]
    first = keep.double().cumsum(1) <= k + 1
    bi = bi[keep & first].reshape(len(pick), k + 1)
    bd = bd[keep & first].reshape(len(pick), k + 1)
    p64 = pts.double()
    if metric == "cosine":
        w = p64 / p64.norm(dim=1, keepdim=True)
        d2 = 2.0 * bd
    else:
        w = p64 - p64[torch.isfinite(p64).all(1)].mean(0)
        d2 = bd ** 2
    n2 = (w * w).sum(1)
    bar = 2e-5 * (n2[pick][:, None] + n2[bi.clamp_min(0)])
    clear = (d2[:, k] - d2[:, k - 1]) > 2 * torch.maximum(bar[:, k], bar[:, k - 1])
    got_i, got_d = out["indices"][pick].long(), out["distances"][pick].double()
    eq = got_i[:, :, None] == bi[:, None, :k]
    hit = eq.any(-1)
    ref_d = torch.gather(bd, 1, eq.double().argmax(-1))
    rel = ((got_d - ref_d).abs() / ref_d.clamp_min(1e-300))[hit]
    # how much farther the returned k-th neighbour is than the true one (0: as near, whatever the indices)
    excess = got_d[:, k - 1] / bd[:, k - 1].clamp_min(1e-300) - 1.0
    return {"sample": int(len(pick)), "clear_cut_rows": int(clear.sum()),
            "recall": recall(got_i, bi[:, :k]),
            "recall_on_clear_cut_rows": recall(got_i[clear], bi[clear][:, :k]) if bool(clear.any()) else None,
            "max_relative_distance_error": float(rel.max()) if rel.numel() else 0.0,
            "kth_distance_excess_median": float(excess.median()), "kth_distance_excess_max": float(excess.max())}


half = max(1, a.calls // 2)
t_embed = timed(lambda: m.embed(batch, draws=draws), a.calls)
knn0, knn1 = with_tile("0", lambda: m.knn(emb, k=k)), with_tile("1", lambda: m.knn(emb, k=k))
t0 = timed(knn0, half)
t1 = timed(knn1, half)
t0 += timed(knn0, a.calls - half)
t1 += timed(knn1, a.calls - half)
o0, o1 = knn0(), knn1()
same = bool(torch.equal(o0["indices"], o1["indices"]) and
            torch.equal(o0["distances"].view(torch.int32), o1["distances"].view(torch.int32)))
del o0, o1
t_cos = timed(lambda: m.knn(emb, k=k, metric="cosine"), a.calls)
gauss = torch.randn(B, K, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
t_gauss = timed(lambda: m.knn(gauss, k=k), a.calls)
t_topk = timed(lambda: m.top_k(batch, k=10, draws=draws), a.calls)
agree = {"embedding": agreement(emb, m.knn(emb, k=k)),
         "embedding_cosine": agreement(emb, m.knn(emb, k=k, metric="cosine"), "cosine"),
         "gaussian": agreement(gauss, m.knn(gauss, k=k))}
mi, md = materialising(emb)
agree["materialising_route_recall_vs_knn"] = recall(mi, m.knn(emb, k=k)["indices"])
del mi, md
torch.cuda.empty_cache()
t_old = timed(lambda: materialising(emb), a.slow_calls or a.calls, warmup=1)
norms = emb.double().norm(dim=1)
res = {"shape": {"rows": B, "D": D, "K": K, "S": S, "k": k, "nnz": int(sc.nnz), "density": 0.005,
                 "generator": "synth.linear_structure",
                 "knn_scratch_bytes": int(_lib.load().spmf_knn_scratch_bytes(m._handle(), B, B, K)),
                 "embedding_norm_min_max": [float(norms.min()), float(norms.max())]},
       "embed": stats(t_embed), "knn_tile0": stats(t0), "knn_tile1": stats(t1), "tiles_bit_equal": same,
       "knn_cosine": stats(t_cos), "knn_gaussian": stats(t_gauss),
       "materialising": dict(stats(t_old), chunk_rows=a.chunk_rows),
       "top_k": stats(t_topk), "top_k_parent": parent,
       "flop_per_knn": 2.0 * B * B * K,
       "knn_tflops_tile0": round(2.0 * B * B * K / (statistics.median(t0) * 1e-3) / 1e12, 2),
       "knn_tflops_tile1": round(2.0 * B * B * K / (statistics.median(t1) * 1e-3) / 1e12, 2),
       "speedup_over_materialising": round(statistics.median(t_old) / min(statistics.median(t0), statistics.median(t1)), 2),
       "agreement": agree}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
