"""rank_cells (csrc/rank.hip) at one C3 row shard: linear_structure(rows=122 880, D=20 000, density=0.005),
K = 32, S = 8, against top_k at the same shape and against the materialising route.

Timed with device events after a warm-up, `--calls` calls each, median and spread (min, max):
  rank_cells          1.2 M listed cells drawn uniformly (with replacement): ~10 per row, every column block of a
                      row block holds some, so both phases sweep all blocks;
  rank_cells_one      one listed cell per row: phase 1 scores at most 64 of a row block's 313 column blocks;
  library_only        spmf_rank_cells through ctypes on the 1.2 M list already sorted, int32 and on the device:
                      prep + encode + mark + the rank kernel, nothing of torch;
  top_k               top_k(k=10) of this build;
  top_k_parent        top_k(k=10) of another build of the library (`--parent-lib FILE`, e.g. the parent commit's
                      built with tools/build_variant.sh), timed in a child process of its own that loads that file;
  materialising       what the library offered before: log_likelihood_components over 4096-row chunks
                      ([S,rows,D] rate and log-likelihood, 8 bytes per cell and draw), the mean over the draws,
                      the stored cells masked out, and per listed cell a comparison of its score with its row
                      (score descending, equal scores by ascending column), `--cmp-cells` cells at a time.  The
                      cells are sorted by row and cut into the chunks' segments before the clock starts, which
                      rank_cells does inside its timed call.
The two routes rank the same cells: the share of equal ranks and the largest rank difference are reported (the
materialising route forms its scores with another summation order, so near ties may fall the other way).

usage: rank_cells_probe.py [--rows N] [--cols D] [--cells N] [--calls N] [--parent-lib FILE] [--out FILE]
       -> one JSON line, also written to FILE
       rank_cells_probe.py --once: a single rank_cells call on the 1.2 M list, for a kernel trace"""
import argparse
import ctypes as C
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
ap.add_argument("--cells", type=int, default=1_200_000)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--slow-calls", type=int, default=None, help="calls of the materialising route (default: --calls)")
ap.add_argument("--chunk-rows", type=int, default=4096)
ap.add_argument("--cmp-cells", type=int, default=8192)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--topk-only", action="store_true", help="(the child of --parent-lib) time top_k and print it")
ap.add_argument("--once", action="store_true", help="one rank_cells call on the 1.2 M list and nothing else: the "
                "command for `rocprofv3 --kernel-trace --stats`")
ap.add_argument("--out", default=os.path.join("profiles", "rank_cells_probe.json"))
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
    # a build from before rank_cells has neither entry point; nothing here calls them
    for name in ("spmf_rank_cells", "spmf_rank_scratch_bytes"):
        _lib.SIGNATURES.pop(name, None)
from spmf_amd import PoissonFactorization, synth  # noqa: E402
from spmf_amd._lib import VAR_ORDER  # noqa: E402

dev = torch.device("cuda", 0)
B, D, K, S, N = a.rows, a.cols, a.latent, a.draws, a.cells
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
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "calls": calls}


if a.once:
    g = torch.Generator(device=dev).manual_seed(2)
    out = m.rank_cells(batch, torch.randint(0, B, (N,), generator=g, device=dev),
                       torch.randint(0, D, (N,), generator=g, device=dev), draws=draws)
    torch.cuda.synchronize()
    print(json.dumps({"once": True, "n": out["n"], "auc": out["auc"]}))
    sys.exit(0)
t_topk = timed(lambda: m.top_k(batch, k=10, draws=draws), a.calls)
if a.topk_only:
    print(json.dumps(dict(t_topk, lib=os.path.relpath(_lib.LIB_PATH, ROOT))))
    sys.exit(0)

g = torch.Generator(device=dev).manual_seed(2)
rows = torch.randint(0, B, (N,), generator=g, device=dev)
cols = torch.randint(0, D, (N,), generator=g, device=dev)
rows1 = torch.arange(B, device=dev)
cols1 = torch.randint(0, D, (B,), generator=g, device=dev)

# the list as the library takes it, and the segments of the materialising route's chunks
r_sorted, order = torch.sort(rows.to(torch.int32), stable=True)
c_sorted = cols.to(torch.int32)[order].contiguous()
edges = torch.searchsorted(r_sorted, torch.arange(0, sc.n_panels + 1, dtype=torch.int32, device=dev)
                           * a.chunk_rows).tolist()
lib, h = _lib.load(), m._handle()
Sp, P = m._pack_params(draws, names=("s", "u", "v", "w"))
pin = _lib.PtrArray(*[P[n].data_ptr() if n in P else None for n in VAR_ORDER])
_, cs = m._batch(batch)
need = int(lib.spmf_rank_scratch_bytes(h, int(cs.n_rows), S))
scratch = torch.empty(need + 256, dtype=torch.uint8, device=dev)
s_base = scratch.data_ptr() + (-scratch.data_ptr()) % 256
rank_o = torch.empty(N, dtype=torch.int32, device=dev)
cand_o = torch.empty(N, dtype=torch.int32, device=dev)
score_o = torch.empty(N, dtype=torch.float32, device=dev)
eta = m._eta_device()


def library_only():
    _lib.check(h, lib.spmf_rank_cells(h, C.byref(cs), S, pin, eta.data_ptr(), N, r_sorted.data_ptr(),
                                      c_sorted.data_ptr(), 1, rank_o.data_ptr(), cand_o.data_ptr(),
                                      score_o.data_ptr(), s_base, need,
                                      torch.cuda.current_stream(dev).cuda_stream), "spmf_rank_cells")


def materialising():
    ranks = []
    row_ptr = sc.row_ptr.long()
    for p in range(sc.n_panels):
        r0, r1 = p * a.chunk_rows, min((p + 1) * a.chunk_rows, B)
        rate = m.log_likelihood_components(s=draws["s"], u=draws["u"], v=draws["v"], w=draws["w"],
                                           data={"counts": sc, "panels": (p, p + 1)})["rate"]
        score = rate.mean(0)
        del rate
        lo, hi = edges[p], edges[p + 1]
        lr, lc = (r_sorted[lo:hi] - r0).long(), c_sorted[lo:hi].long()
        target = score[lr, lc]
        e0, e1 = int(row_ptr[r0]), int(row_ptr[r1])
        er = torch.repeat_interleave(torch.arange(r1 - r0, device=dev), row_ptr[r0 + 1:r1 + 1] - row_ptr[r0:r1])
        score[er, sc.col_idx[e0:e1].long()] = float("-inf")            # stored cells are no candidates
        score.masked_fill_(~torch.isfinite(score), float("-inf"))
        col = torch.arange(D, device=dev)
        for q in range(0, hi - lo, a.cmp_cells):
            s_rows = score[lr[q:q + a.cmp_cells]]
            t, c = target[q:q + a.cmp_cells, None], lc[q:q + a.cmp_cells, None]
            ahead = (s_rows > t) | ((s_rows == t) & (col[None, :] < c))
            ranks.append(ahead.sum(1).to(torch.int32))
        del score
    return torch.cat(ranks)


t_rank = timed(lambda: m.rank_cells(batch, rows, cols, draws=draws), a.calls)
t_one = timed(lambda: m.rank_cells(batch, rows1, cols1, draws=draws), a.calls)
t_lib = timed(library_only, a.calls)
out = m.rank_cells(batch, rows, cols, draws=draws)
ref = materialising()
mine = out["rank"][order]
diff = (mine - ref).abs()
agree = {"equal_share": float((diff == 0).double().mean()), "max_rank_difference": int(diff.max()),
         "n": out["n"], "n_excluded": out["n_excluded"], "hit_rate": out["hit_rate"], "mrr": out["mrr"],
         "auc": out["auc"]}
summary = {k: v for k, v in m.rank_cells(batch, rows1, cols1, draws=draws).items() if not torch.is_tensor(v)}
del out, ref, mine, diff
torch.cuda.empty_cache()
t_old = timed(materialising, a.slow_calls or a.calls, warmup=1)
res = {"shape": {"rows": B, "D": D, "K": K, "S": S, "cells": N, "nnz": int(sc.nnz), "density": 0.005,
                 "generator": "synth.linear_structure", "scratch_bytes": need},
       "rank_cells": t_rank, "rank_cells_one": dict(t_one, cells=B), "library_only": t_lib, "top_k": t_topk,
       "top_k_parent": parent,
       "materialising": dict(t_old, chunk_rows=a.chunk_rows, cmp_cells=a.cmp_cells, cells_presorted=True),
       "ratio_to_top_k": round(t_rank["median_ms"] / t_topk["median_ms"], 2),
       "ratio_to_top_k_parent": round(t_rank["median_ms"] / parent["median_ms"], 2) if parent else None,
       "one_cell_ratio_to_top_k": round(t_one["median_ms"] / t_topk["median_ms"], 2),
       "speedup_over_materialising": round(t_old["median_ms"] / t_rank["median_ms"], 2),
       "agreement": agree, "summary_one_cell_per_row": summary}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
