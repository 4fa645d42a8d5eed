"""group_means (csrc/groups.hip) on a slice of the C4 shape: synth.scrna_like(rows=32 768, D=4 096), log_transform,
K = 64, S = 8, 12 groups (a seeded label per row, one row in sixteen unlabelled), all columns.

Timed with device events after a warm-up, `--calls` calls each, median and spread (min, max):
  group_means           the call, sums only; group_means_p_nonzero with the second output;
  embed                 the draw stage alone (prep + encode sweep of the 8 draws + a small reduction): what every
                        streaming call pays before its consumer runs;
  predict_index_add     the route of the commit before group_means: predict one draw at a time over all rows and
                        columns (a dense [rows, D] fp32 block per draw), converted to fp64 and summed by label
                        with index_add_ -- S encode sweeps, S dense blocks written and read back.
Agreement: the largest |sum - route's sum| / sum |m| over all (draw, group, column), and whether a repeated call
returns the same bits.

usage: groups_probe.py [--rows N] [--cols D] [--calls N] [--out FILE]   -> one JSON line, also written to FILE"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=32_768)
ap.add_argument("--cols", type=int, default=4_096)
ap.add_argument("--latent", type=int, default=64)
ap.add_argument("--draws", type=int, default=8)
ap.add_argument("--groups", type=int, default=12)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--out", default=os.path.join("profiles", "groups_probe.json"))
a = ap.parse_args()

import torch  # noqa: E402

from spmf_amd import PoissonFactorization, _lib, synth  # noqa: E402

dev = torch.device("cuda", 0)
B, D, K, S, G = a.rows, a.cols, a.latent, a.draws, a.groups
sc = synth.scrna_like(B, D, dev, 20241218 + 4, panel_rows=8192, chunk_rows=8192, target_density=0.03)
m = PoissonFactorization(latent_dim=K, feature_dim=D, u_tau_scale=1.0 / (B * D) ** 0.5, device=dev,
                         log_transform=True, panel_rows=8192)
colsum = torch.zeros(D, dtype=torch.float64, device=dev)
colnnz = torch.zeros(D, dtype=torch.float64, device=dev)
sc.compute_stats(m._handle(), colsum, colnnz)
m.eta_i = (colsum / B).clamp_min(1e-3).reshape(1, D)        # column_norms = gene means (floored), as the C4 caller
m.xi_u_global = float((colsum / B).sum())
torch.manual_seed(1)
draws = m.surrogate_distribution.sample(S)
batch = {"counts": sc}
gen = torch.Generator().manual_seed(5)
labels = torch.randint(0, G, (B,), generator=gen)
labels[torch.rand(B, generator=gen) < 1.0 / 16.0] = -1
labels = labels.to(dev)


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


def route():
    """-> (sums, sums of |m|) fp64 [S, G, D] by the route of the commit before group_means."""
    keep = labels >= 0
    idx = labels[keep].to(torch.int64)
    total = torch.zeros(S, G, D, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(total)
    for s in range(S):
        one = {n: v[s:s + 1] for n, v in draws.items()}
        cells = m.predict(batch, draws=one)["mean"][keep].double()
        total[s].index_add_(0, idx, cells)
        mag[s].index_add_(0, idx, cells.abs())
        del cells
    return total, mag


new = m.group_means(batch, labels, n_groups=G, draws=draws)
again = m.group_means(batch, labels, n_groups=G, draws=draws)
old, mag = route()
rel = ((new["sum"] - old).abs() / mag.clamp_min(1e-300)).max()
same = bool(torch.equal(new["sum"].view(torch.int64), again["sum"].view(torch.int64)))
finite = bool(torch.isfinite(new["sum"]).all())
del again, old, mag
torch.cuda.empty_cache()

t_new = timed(lambda: m.group_means(batch, labels, n_groups=G, draws=draws), a.calls)
t_pnz = timed(lambda: m.group_means(batch, labels, n_groups=G, draws=draws, p_nonzero=True), a.calls)
t_embed = timed(lambda: m.embed(batch, draws=draws), a.calls)
t_old = timed(route, a.calls, warmup=1)
lib, h = _lib.load(), m._handle()
med = statistics.median
res = {"shape": {"rows": B, "D": D, "K": K, "S": S, "groups": G, "nnz": int(sc.nnz), "log_transform": True,
                 "generator": "synth.scrna_like", "labelled_rows": int((labels >= 0).sum()),
                 "groups_scratch_bytes": int(lib.spmf_groups_scratch_bytes(h, B, S, G, D)),
                 "embed_scratch_bytes": int(lib.spmf_embed_scratch_bytes(h, B, S)),
                 "dense_block_bytes_per_draw": B * D * 4},
       "group_means": stats(t_new), "group_means_p_nonzero": stats(t_pnz), "embed": stats(t_embed),
       "predict_index_add": stats(t_old),
       "consumer_ms": round(med(t_new) - med(t_embed), 3),
       "flop_per_call": 2.0 * S * B * D * K,
       "consumer_tflops": round(2.0 * S * B * D * K / (max(med(t_new) - med(t_embed), 1e-6) * 1e-3) / 1e12, 2),
       "speedup_over_predict_index_add": round(med(t_old) / med(t_new), 2),
       "agreement": {"max_abs_diff_over_sum_abs_m": float(rel), "repeat_has_the_same_bits": same,
                     "all_finite": finite}}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
