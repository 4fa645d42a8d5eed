"""graph_transform (csrc/graph_transform.hip) at one C3 row shard: 122 880 query rows mapped onto the layout of
122 880 reference rows (both from one mixture of 32 centres 4 N(0, I) with unit noise, K = 32; the reference laid out
by graph_layout), k = 15 neighbours, M = 8 negatives, 30 epochs from the weighted-mean start.

Timed with device events after a warm-up; a window holds `--repeats` calls (`--torch-repeats` for torch), `--calls`
windows each, the three alternated, median and spread (min, max) of the time of ONE call:
  one_launch     spmf_graph_transform once: all 30 epochs in one launch;
  thirty_calls   the same epochs as 30 one-epoch calls chained through y_out (the start by a call of no epoch): what
                 a launch per epoch, as graph_layout must have, would cost here;
  torch          the same epochs written in torch on the same card: the neighbours gathered once, per epoch the
                 clipped terms, a sum over the k axis, the negatives from torch.randint and their gather.
The library calls are made through the raw binding on prepared pointers, so that the windows hold the launches and
not the argument checks of the Python method.  Beside the times: whether one_launch and thirty_calls agree bit for
bit, and the largest distance between the library's and torch's positions after the first epoch without repulsion
(they draw different negatives, so later epochs are not comparable).

usage: transform_probe.py [--rows N] [--calls N] [--repeats N] [--epochs N] [--out FILE]
       -> one JSON line, also written to FILE"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=122_880)
ap.add_argument("--latent", type=int, default=32)
ap.add_argument("--k", type=int, default=15)
ap.add_argument("--epochs", type=int, default=30)
ap.add_argument("--negatives", type=int, default=8)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--repeats", type=int, default=100)
ap.add_argument("--torch-repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join("profiles", "transform_probe.json"))
a = ap.parse_args()

import torch  # noqa: E402

from spmf_amd import PoissonFactorization, _lib, graph  # noqa: E402

dev = torch.device("cuda", 0)
N, K, E, M, LR = a.rows, a.latent, a.epochs, a.negatives, 0.25
m = PoissonFactorization(latent_dim=K, feature_dim=64, initialize_distributions=False, device=dev)
gen = torch.Generator(device=dev).manual_seed(4)
centres = 4.0 * torch.randn(32, K, device=dev, generator=gen)


def sample(n):
    return (centres[torch.randint(0, 32, (n,), device=dev, generator=gen)]
            + torch.randn(n, K, device=dev, generator=gen)).contiguous()


ref_pts, qry_pts = sample(N), sample(N)
ab = graph.find_ab(0.1, 1.0)
nn_ref = m.knn(ref_pts, k=a.k)
y_ref = m.graph_layout(m.fuzzy_graph(nn_ref["indices"], nn_ref["distances"]), "pca", points=ref_pts, n_epochs=200,
                       a=ab[0], b=ab[1], n_negatives=M)["embedding"]
nn = m.knn(ref_pts, k=a.k, queries=qry_pts)
idx = nn["indices"].contiguous()
w = graph.query_weights(idx, nn["distances"])["weights"].contiguous()
lib, h = _lib.load(), m._handle()
stream = torch.cuda.current_stream(dev).cuda_stream
out_one, out_thirty = (torch.empty(N, 2, dtype=torch.float32, device=dev) for _ in range(2))


def call(y_in, y_out, epoch0, n_epochs, rate=5.0):
    _lib.check(h, lib.spmf_graph_transform(h, N, a.k, idx.data_ptr(), w.data_ptr(), y_ref.data_ptr(), N,
                                           y_in.data_ptr() if y_in is not None else None, y_out.data_ptr(), 0,
                                           epoch0, n_epochs, E, LR, ab[0], ab[1], 1.0, rate, M, 0, stream),
               "spmf_graph_transform")


def one_launch():
    call(None, out_one, 0, E)


def thirty_calls():
    call(None, out_thirty, 0, 0)
    for e in range(E):
        call(out_thirty, out_thirty, e, 1)


A, B = (torch.tensor(v, dtype=torch.float32, device=dev) for v in ab)
jdx = idx.long().clamp_min(0)


def clipped(d, near):
    """The clipped step of each pair: ``d`` [.., 2] the differences, ``near``: attraction (else repulsion)."""
    d2 = (d * d).sum(-1)
    live = d2 > 0
    s = torch.where(live, d2, torch.ones_like(d2))
    q = A * s ** B
    c = -2.0 * B * q / (s * (1.0 + q)) if near else 2.0 * B / ((0.001 + s) * (1.0 + q))
    return (torch.where(live, c, torch.zeros_like(c)).unsqueeze(-1) * d).clamp(-4.0, 4.0)


def torch_transform(epochs=None, repel=True):
    tg = torch.Generator(device=dev).manual_seed(0)
    yj = y_ref[jdx]                                           # [N, k, 2], once
    wk = w.unsqueeze(-1)
    W = w.sum(1, keepdim=True)
    y = (wk * yj).sum(1) / W
    scale, inv = 5.0 / M * W, 1.0 / W.clamp_min(1.0)
    for e in range(E if epochs is None else epochs):
        alpha = LR * (1.0 - e / E)
        F = (wk * clipped(y.unsqueeze(1) - yj, True)).sum(1)
        if repel:
            r = torch.randint(0, N, (N, M), device=dev, generator=tg)
            F = F + scale * clipped(y.unsqueeze(1) - y_ref[r], False).sum(1)
        y = y + alpha * F * inv
    return y


def timed(fns, repeats, calls):
    """The functions alternated, a window of ``repeats[i]`` calls each: -> milliseconds per call, a list per
    function."""
    for fn in fns:
        fn()
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(calls):
        for which, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(repeats[which]):
                fn()
            e1.record()
            e1.synchronize()
            ms[which].append(e0.elapsed_time(e1) / repeats[which])
    return ms


def stats(ms, repeats):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "windows": len(ms), "calls_per_window": repeats}


reps = [a.repeats, a.repeats, a.torch_repeats]
t_one, t_thirty, t_torch = timed([one_launch, thirty_calls, torch_transform], reps, a.calls)
one_launch()
thirty_calls()
first = torch.empty_like(out_one)
call(None, first, 0, 0)
call(first, first, 0, 1, rate=0.0)
tfirst = torch_transform(1, repel=False)
torch.cuda.synchronize()
placed = torch.isfinite(first).all(1) & torch.isfinite(tfirst).all(1)
med = statistics.median
out = {"shape": {"query_rows": N, "reference_rows": N, "K": K, "k": a.k, "epochs": E, "negatives": M, "lr": LR,
                 "a": ab[0], "b": ab[1], "rows_without_a_neighbour": int((w.sum(1) == 0).sum())},
       "one_launch": stats(t_one, reps[0]), "thirty_calls": stats(t_thirty, reps[1]), "torch": stats(t_torch, reps[2]),
       "thirty_calls_over_one_launch": round(med(t_thirty) / med(t_one), 2),
       "torch_over_one_launch": round(med(t_torch) / med(t_one), 2),
       "one_launch_us_per_epoch": round(med(t_one) * 1e3 / max(E, 1), 3),
       "one_launch_equals_thirty_calls_bit_for_bit": bool(torch.equal(out_one.view(torch.int32),
                                                                      out_thirty.view(torch.int32))),
       "first_epoch_attraction_max_abs_difference_to_torch": float((first - tfirst)[placed].abs().max()),
       "all_finite": bool(torch.isfinite(out_one).all())}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
