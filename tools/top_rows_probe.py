"""top_rows (csrc/toprows.hip) against the only other route to its answer: predict on the same panel and draws, a
dense [rows, C] fp32 block, followed by torch.topk(dim=0).

Shape: synth.scrna_like(rows=200 000, D=4 096), K = 32, S = 32, k = 10, a seeded panel of 1 024 columns; and the same
rows with a panel of 64 columns (one column block: the grid is the row slices alone), which shows whether the row
slices fill the device.

The two paths ALTERNATE, `--rounds` times each in one process after one warm-up call of each (device events around
the whole call); per path the median and the spread (max - min).  The bar of the wide panel: top_rows' median is at
most the alternative's median plus the alternative's own spread.  The narrow panel is recorded without a bar.
Stored cells are not excluded in the timed calls, since the alternative knows nothing of them; top_rows with the
exclusion is timed beside them.  Agreement: top_rows' scores equal torch.topk's values bit for bit (both descending),
and its rows equal torch.topk's indices wherever a column's k + 1 best scores are distinct.

usage: top_rows_probe.py [--rows N] [--cols D] [--panel C] [--rounds N] [--out FILE]  -> one JSON line, also in FILE"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=200_000)
ap.add_argument("--cols", type=int, default=4_096)
ap.add_argument("--panel", type=int, default=1_024)
ap.add_argument("--latent", type=int, default=32)
ap.add_argument("--draws", type=int, default=32)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join("profiles", "top_rows_probe.json"))
a = ap.parse_args()

import torch  # noqa: E402

from spmf_amd import PoissonFactorization, _lib, synth  # noqa: E402

dev = torch.device("cuda", 0)
B, D, K, S, k = a.rows, a.cols, a.latent, a.draws, a.k
sc = synth.scrna_like(B, D, dev, 20241218 + 9, panel_rows=8192, chunk_rows=8192, target_density=0.03)
m = PoissonFactorization(latent_dim=K, feature_dim=D, u_tau_scale=1.0 / (B * D) ** 0.5, device=dev, panel_rows=8192)
colsum = torch.zeros(D, dtype=torch.float64, device=dev)
colnnz = torch.zeros(D, dtype=torch.float64, device=dev)
sc.compute_stats(m._handle(), colsum, colnnz)
m.eta_i = (colsum / B).clamp_min(1e-3).reshape(1, D)
m.xi_u_global = float((colsum / B).sum())
torch.manual_seed(1)
draws = m.surrogate_distribution.sample(S)
batch = {"counts": sc}
gen = torch.Generator().manual_seed(5)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3),
            "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def panel_case(C):
    cols = torch.randperm(D, generator=gen)[:C].to(dev)

    def new(exclude=False):
        return m.top_rows(batch, cols=cols, k=k, draws=draws, exclude_stored=exclude)

    def old():
        block = m.predict(batch, cols=cols, draws=draws)["mean"]
        return torch.topk(block, k, dim=0)

    got, want = new(), old()                       # (the warm-up call of each path)
    finite = bool(torch.isfinite(want.values).all())
    same_scores = bool(torch.equal(got["scores"].view(torch.int32), want.values.t().contiguous().view(torch.int32)))
    block = m.predict(batch, cols=cols, draws=draws)["mean"]
    best = torch.topk(block, k + 1, dim=0).values
    distinct = (best[1:] != best[:-1]).all(0)
    same_rows = bool(torch.equal(got["rows"][distinct], want.indices.t()[distinct]))
    again = new()
    repeat = bool(torch.equal(again["rows"], got["rows"]) and torch.equal(again["scores"], got["scores"]))
    del got, want, block, best, again
    torch.cuda.empty_cache()
    t_new, t_old, t_excl = [], [], []
    for _ in range(a.rounds):
        t_new.append(event_ms(new))
        t_old.append(event_ms(old))
    new(True)
    for _ in range(a.rounds):
        t_excl.append(event_ms(lambda: new(True)))
    lib, h = _lib.load(), m._handle()
    sn, so = stats(t_new), stats(t_old)
    return {"panel_columns": C, "top_rows": sn, "predict_topk": so, "top_rows_exclude_stored": stats(t_excl),
            "bar_ms": round(so["median_ms"] + so["spread_ms"], 3),
            "within_bar": sn["median_ms"] <= so["median_ms"] + so["spread_ms"],
            "speedup": round(so["median_ms"] / sn["median_ms"], 2),
            "toprows_scratch_bytes": int(lib.spmf_toprows_scratch_bytes(h, B, S, C)),
            "dense_block_bytes": B * C * 4, "flop_per_call": 2.0 * S * B * C * K,
            "agreement": {"all_finite": finite, "scores_equal_topk_values_bit_for_bit": same_scores,
                          "rows_equal_topk_indices_on_distinct_columns": same_rows,
                          "distinct_columns": int(distinct.sum()), "repeat_has_the_same_bits": repeat}}


res = {"shape": {"rows": B, "D": D, "K": K, "S": S, "k": k, "nnz": int(sc.nnz), "generator": "synth.scrna_like",
                 "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
                 "cus": torch.cuda.get_device_properties(0).multi_processor_count},
       "wide_panel": panel_case(a.panel), "one_column_block": panel_case(64)}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
