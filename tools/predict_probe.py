"""predict (csrc/panel.hip) at one mid shape: linear_structure(rows=65 536, D=20 000, density=0.005), K = 32,
S = 16, panels of C = 64, 1024 and all D columns (a seeded choice of columns for the two lists).

Timed with device events after a warm-up, `--calls` calls each, median and spread (min, max); the probe reports,
it asserts nothing:
  predict_mean / predict_all  predict with the mean only / with mean, sd and p_nonzero, per C; the outputs'
                      bytes (B * C * 4 each) divided by the median time;
  top_k               top_k(k=10) on the same inputs: the same draw stage and the same tile work over all D
                      columns, without the output stream;
  draw_stage          embed on the same inputs: prep + encode sweep of the S draws + a small reduction, the part
                      every streaming call pays before its consumer;
  dense_alternative   (C = 64 only) what a user had before: spmf_dense_ll per draw on `--slice-rows` rows (all D
                      columns, rate and log-likelihood, 8 bytes per cell and draw), the listed columns' rates
                      accumulated into a mean; the time scaled to B rows;
  expectation         the mean-only panel at C = D against a top_k sweep plus the time to write B * D * 4 bytes at
                      the rate of a timed fill of that size.

usage: predict_probe.py [--rows N] [--cols D] [--calls N] [--out FILE]
       -> one JSON line, also written to FILE"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=65_536)
ap.add_argument("--cols", type=int, default=20_000)
ap.add_argument("--latent", type=int, default=32)
ap.add_argument("--draws", type=int, default=16)
ap.add_argument("--panels", type=int, nargs="*", default=[64, 1024], help="listed panel sizes (all columns is "
                "always run)")
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--chunk-rows", type=int, default=4096)
ap.add_argument("--slice-rows", type=int, default=4096, help="rows of the dense alternative (whole panels)")
ap.add_argument("--out", default=os.path.join("profiles", "predict_probe.json"))
a = ap.parse_args()

import torch  # noqa: E402

from spmf_amd import PoissonFactorization, synth  # noqa: E402

dev = torch.device("cuda", 0)
B, D, K, S = a.rows, a.cols, a.latent, a.draws
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


def gbs(nbytes, ms):
    return round(nbytes / (statistics.median(ms) * 1e-3) / 1e9, 1)


def dense_alternative(cols):
    """The mean over the draws of the listed columns' rates through spmf_dense_ll on the first --slice-rows rows."""
    part = {"counts": sc, "panels": (0, max(1, a.slice_rows // a.chunk_rows))}
    acc = None
    for i in range(S):
        rate = m.log_likelihood_components(s=draws["s"][i], u=draws["u"][i], v=draws["v"][i], w=draws["w"][i],
                                           data=part)["rate"][:, cols]
        acc = rate if acc is None else acc + rate
    return acc / S


t_topk = timed(lambda: m.top_k(batch, k=10, draws=draws), a.calls)
t_stage = timed(lambda: m.embed(batch, draws=draws), a.calls)
fill = torch.empty(B, D, dtype=torch.float32, device=dev)
t_fill = timed(lambda: fill.fill_(1.0), a.calls)
del fill
torch.cuda.empty_cache()
write_gbs = gbs(B * D * 4, t_fill)

pick = torch.randperm(D, generator=torch.Generator().manual_seed(2))
panels = {}
for Cn in [c for c in a.panels if c < D] + [D]:
    cols = None if Cn == D else pick[:Cn].to(dev)
    t_mean = timed(lambda: m.predict(batch, cols, draws=draws), a.calls)
    t_all = timed(lambda: m.predict(batch, cols, draws=draws, sd=True, p_nonzero=True), a.calls)
    torch.cuda.empty_cache()
    one = B * Cn * 4
    entry = {"C": Cn, "listed": cols is not None, "output_bytes_each": one,
             "predict_mean": dict(stats(t_mean), output_gb_per_s=gbs(one, t_mean)),
             "predict_all": dict(stats(t_all), output_gb_per_s=gbs(3 * one, t_all))}
    if Cn == 64:
        rows = max(1, a.slice_rows // a.chunk_rows) * a.chunk_rows
        got = m.predict({"counts": sc, "panels": (0, rows // a.chunk_rows)}, cols, draws=draws)["mean"]
        ref = dense_alternative(cols)
        rel = ((got - ref).abs() / ref.abs().clamp_min(1e-30)).max()
        t_old = timed(lambda: dense_alternative(cols), max(2, a.calls // 3), warmup=1)
        entry["dense_alternative"] = dict(stats(t_old), slice_rows=rows, scaled_to_rows=B,
                                          scaled_median_ms=round(statistics.median(t_old) * B / rows, 3),
                                          max_relative_difference_of_the_mean=float(rel))
        del got, ref
        torch.cuda.empty_cache()
    panels[str(Cn)] = entry

full = panels[str(D)]["predict_mean"]["median_ms"]
expected = statistics.median(t_topk) + B * D * 4 / (write_gbs * 1e9) * 1e3
res = {"shape": {"rows": B, "D": D, "K": K, "S": S, "nnz": int(sc.nnz), "density": 0.005,
                 "generator": "synth.linear_structure", "chunk_rows": a.chunk_rows},
       "top_k": stats(t_topk), "draw_stage": stats(t_stage),
       "fill_B_x_D_fp32": dict(stats(t_fill), gb_per_s=gbs(B * D * 4, t_fill)),
       "panels": panels,
       "expectation": {"what": "predict_mean at C = D ~ top_k + B*D*4 bytes at the write rate", "write_gb_per_s": write_gbs,
                       "expected_ms": round(expected, 3), "measured_ms": full,
                       "measured_over_expected": round(full / expected, 3)}}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
