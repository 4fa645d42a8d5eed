"""score_cells (csrc/cells.hip) against the materialising path at one C3 row shard:
linear_structure(rows=122 880, D=20 000, density=0.005), K = 32, S = 8, 1.2 M cells drawn uniformly
(with replacement) with small held-out counts as values.

Timed with device events after a warm-up, 20 calls each, median and spread (min, max).  The
materialising path is what the library offered before: log_likelihood_components on 4096-row chunks
([S,rows,D] rate and log-likelihood, 8 bytes per cell and draw), the listed cells of the chunk indexed
out of `rate`, the mean over the draws, and the Poisson log-pmf of the held-out value with logsumexp over
the draws in torch (the chunk's `log_likelihood` is that of the STORED counts, so it cannot be indexed for
held-out values).  The cells are sorted by row and cut into the chunks' segments before the clock starts,
which score_cells does inside its timed call.

Where the time of score_cells goes is read from four more timings on the same batch and draws:
  library_only      spmf_score_cells through ctypes on the list already sorted, int32 and on the device:
                    prep + encode + the cell kernel, nothing of torch;
  library_one_cell  the same ctypes call on the same scratch with n_cells = 1: prep + encode + a cell
                    kernel of one wave, i.e. the library's cost that does not depend on the list;
  one_cell          score_cells (the Python method) with a single cell: library_one_cell plus the
                    method's fixed torch work (read-back of the index check, sort, scatter, summary);
  summary           heldout.summarize on the call's lppd alone;
  so  cell kernel ~ library_only - library_one_cell  (two ctypes calls, like for like),
      torch (sort, gather, scatter, summary) ~ score_cells - library_only.

usage: score_cells_probe.py [--rows N] [--cols D] [--cells N] [--calls N] [--out FILE]
       -> one JSON line, also written to FILE"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spmf_amd import PoissonFactorization, _lib, heldout, synth  # noqa: E402
from spmf_amd._lib import VAR_ORDER  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=122_880)
ap.add_argument("--cols", type=int, default=20_000)
ap.add_argument("--latent", type=int, default=32)
ap.add_argument("--draws", type=int, default=8)
ap.add_argument("--cells", type=int, default=1_200_000)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--chunk-rows", type=int, default=4096)
ap.add_argument("--out", default=os.path.join("profiles", "score_cells_probe.json"))
a = ap.parse_args()

dev = torch.device("cuda", 0)
B, D, K, S, N = a.rows, a.cols, a.latent, a.draws, a.cells
sc = synth.linear_structure(B, D, 0.005, dev, panel_rows=a.chunk_rows)
m = PoissonFactorization(latent_dim=K, feature_dim=D, u_tau_scale=1.0 / (B * D) ** 0.5, device=dev,
                         panel_rows=a.chunk_rows)
torch.manual_seed(1)
draws = m.surrogate_distribution.sample(S)
g = torch.Generator(device=dev).manual_seed(2)
rows = torch.randint(0, B, (N,), generator=g, device=dev)
cols = torch.randint(0, D, (N,), generator=g, device=dev)
vals = torch.poisson(torch.full((N,), 0.3, device=dev), generator=g)
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


def streaming():
    return m.score_cells(batch, rows, cols, values=vals, draws=draws)


def one_cell():
    return m.score_cells(batch, rows[:1], cols[:1], values=vals[:1], draws=draws)


# the list as the library takes it, and the segments of the materialising path's chunks
r_sorted, order = torch.sort(rows.to(torch.int32), stable=True)
c_sorted, v_sorted = cols.to(torch.int32)[order].contiguous(), vals[order].contiguous()
edges = torch.searchsorted(r_sorted, torch.arange(0, sc.n_panels + 1, dtype=torch.int32, device=dev)
                           * a.chunk_rows).tolist()
lib, h = _lib.load(), m._handle()
Sp, P = m._pack_params(draws, names=("s", "u", "v", "w"))
pin = _lib.PtrArray(*[P[n].data_ptr() if n in P else None for n in VAR_ORDER])
_, cs = m._batch(batch)
need = int(lib.spmf_cells_scratch_bytes(h, int(cs.n_rows), S))
scratch = torch.empty(need + 256, dtype=torch.uint8, device=dev)
s_base = scratch.data_ptr() + (-scratch.data_ptr()) % 256
mean_o = torch.empty(N, dtype=torch.float32, device=dev)
lppd_o = torch.empty(N, dtype=torch.float32, device=dev)
eta = m._eta_device()


def library_only():
    _lib.check(h, lib.spmf_score_cells(h, C.byref(cs), S, pin, eta.data_ptr(), N, r_sorted.data_ptr(),
                                       c_sorted.data_ptr(), v_sorted.data_ptr(), mean_o.data_ptr(),
                                       lppd_o.data_ptr(), s_base, need,
                                       torch.cuda.current_stream(dev).cuda_stream), "spmf_score_cells")


def library_one_cell():
    _lib.check(h, lib.spmf_score_cells(h, C.byref(cs), S, pin, eta.data_ptr(), 1, r_sorted.data_ptr(),
                                       c_sorted.data_ptr(), v_sorted.data_ptr(), mean_o.data_ptr(),
                                       lppd_o.data_ptr(), s_base, need,
                                       torch.cuda.current_stream(dev).cuda_stream), "spmf_score_cells")


def materialising():
    means, lppds = [], []
    for p in range(sc.n_panels):
        rate = m.log_likelihood_components(s=draws["s"], u=draws["u"], v=draws["v"], w=draws["w"],
                                           data={"counts": sc, "panels": (p, p + 1)})["rate"]
        lo, hi = edges[p], edges[p + 1]
        r = rate[:, (r_sorted[lo:hi] - p * a.chunk_rows).long(), c_sorted[lo:hi].long()]
        del rate
        v = v_sorted[lo:hi]
        means.append(r.mean(0))
        lppds.append(torch.logsumexp(torch.xlogy(v, r) - r - torch.lgamma(v + 1.0), 0) - math.log(S))
    return torch.cat(means), torch.cat(lppds)


t_new = timed(streaming, a.calls)
t_one = timed(one_cell, a.calls)
t_lib = timed(library_only, a.calls)
t_lib1 = timed(library_one_cell, a.calls)
# the two paths score the same cells: largest difference, relative to the largest value
out = streaming()
t_sum = timed(lambda: heldout.summarize(out["lppd"]), a.calls)
ref_mean, ref_lppd = materialising()
ok = torch.isfinite(out["lppd"][order]) & torch.isfinite(ref_lppd)
agree = {"mean_rel": float((out["mean"][order] - ref_mean).abs().max() / ref_mean.abs().max()),
         "lppd_rel": float((out["lppd"][order] - ref_lppd)[ok].abs().max() / ref_lppd[ok].abs().max()),
         "n_excluded": out["n_excluded"]}
del out, ref_mean, ref_lppd
torch.cuda.empty_cache()
t_old = timed(materialising, a.calls, warmup=1)
res = {"shape": {"rows": B, "D": D, "K": K, "S": S, "cells": N, "nnz": int(sc.nnz), "density": 0.005,
                 "generator": "synth.linear_structure", "scratch_bytes": need},
       "score_cells": t_new, "one_cell": t_one, "library_only": t_lib, "library_one_cell": t_lib1,
       "summary": t_sum,
       "materialising": dict(t_old, chunk_rows=a.chunk_rows, cells_presorted=True),
       "cell_kernel_ms_estimate": round(t_lib["median_ms"] - t_lib1["median_ms"], 3),
       "torch_ms_estimate": round(t_new["median_ms"] - t_lib["median_ms"], 3),
       "agreement": agree,
       "speedup": round(t_old["median_ms"] / t_new["median_ms"], 2)}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
