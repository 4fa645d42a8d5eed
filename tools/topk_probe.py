"""top_k (csrc/topk.hip) against the materialising path at one C3 row shard:
linear_structure(rows=122 880, D=20 000, density=0.005), K = 32, S = 8, k = 10.

Timed with device events after a warm-up, 20 calls each, median and spread (min, max).  The
materialising path is what the library offered before: log_likelihood_components on row chunks that
fit ([S,rows,D] rate and log-likelihood, 8 bytes per cell and draw), mean over the draws, torch.topk
per chunk; it is timed WITHOUT masking the stored cells (which it would need a dense mask for), top_k
with them excluded.  The TFLOP/s figure charges 2 S B D KP flops to the whole top_k call (prep, encode
sweep, bitmap and select), so it is a lower bound on the select kernel's rate.

usage: topk_probe.py [--rows N] [--cols D] [--calls N] [--out FILE]   -> one JSON line, also written to FILE"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spmf_amd import PoissonFactorization, _lib, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=122_880)
ap.add_argument("--cols", type=int, default=20_000)
ap.add_argument("--latent", type=int, default=32)
ap.add_argument("--draws", type=int, default=8)
ap.add_argument("-k", type=int, default=10)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--chunk-rows", type=int, default=4096)
ap.add_argument("--out", default=os.path.join("profiles", "topk_probe.json"))
a = ap.parse_args()

dev = torch.device("cuda", 0)
B, D, K, S, k = a.rows, a.cols, a.latent, a.draws, a.k
sc = synth.linear_structure(B, D, 0.005, dev, panel_rows=a.chunk_rows)
m = PoissonFactorization(latent_dim=K, feature_dim=D, u_tau_scale=1.0 / (B * D) ** 0.5, device=dev,
                         panel_rows=a.chunk_rows)
torch.manual_seed(1)
draws = m.surrogate_distribution.sample(S)
KP = int(_lib.load().spmf_padded_k(m._handle()))


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
    return m.top_k({"counts": sc}, k=k, draws=draws)


def materialising():
    out = []
    for p in range(sc.n_panels):
        rate = m.log_likelihood_components(s=draws["s"], u=draws["u"], v=draws["v"], w=draws["w"],
                                           data={"counts": sc, "panels": (p, p + 1)})["rate"]
        out.append(torch.topk(rate.mean(0), k, dim=1))
        del rate
    return out


t_new = timed(streaming, a.calls)
torch.cuda.empty_cache()
t_old = timed(materialising, a.calls, warmup=1)
flops = 2.0 * S * B * D * KP
res = {"shape": {"rows": B, "D": D, "K": K, "KP": KP, "S": S, "k": k, "nnz": int(sc.nnz), "density": 0.005,
                 "generator": "synth.linear_structure"},
       "top_k": t_new, "materialising": dict(t_old, chunk_rows=a.chunk_rows, stored_cells_masked=False),
       "top_k_tflops_f32_mfma_lower_bound": round(flops / (t_new["median_ms"] * 1e-3) / 1e12, 2),
       "frac_f32_mfma_peak_lower_bound": round(flops / (t_new["median_ms"] * 1e-3) / 1e12 / 157.3, 3),
       "speedup": round(t_old["median_ms"] / t_new["median_ms"], 2)}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
