#!/usr/bin/env python
"""Time waic() (materialising) against waic_streaming() on synthetic Poisson batches.

    python tools/waic_time.py                 # both steps, each in a child process under a timeout
    python tools/waic_time.py --step shared   # 2000 x 5000, K=16, S=50: both paths fit
    python tools/waic_time.py --step c2       # 20000 x 5000, S=100: waic_streaming alone

Median of 10 timed calls after 3 warm-ups, device synchronised around every timed call, draws
fixed across the calls.  The materialising path is timed as waic() runs it with the draws
passed in (log_likelihood_components -> fp64 -> logsumexp / var).  --once runs a single
streaming call (for a kernel trace).  --cols times waic_streaming(col_scores=True), the call with
the per-column sums.  One JSON line per step."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = {"shared": (2000, 5000, 16, 50, True, 240), "c2": (20000, 5000, 16, 100, False, 420)}


def _problem(B, D, K, S, seed=0, density=0.05):
    import numpy as np
    import torch
    from spmf_amd import PoissonFactorization
    from spmf_amd.sparse import SparseCounts
    rng = np.random.default_rng(seed)
    nnz_row = max(1, int(density * D))
    stride = D // nnz_row                    # one stored column in every run of `stride`: distinct, sorted
    cols = stride * np.arange(nnz_row)[None, :] + rng.integers(0, stride, size=(B, nnz_row))
    indptr = np.arange(B + 1, dtype=np.int64) * nnz_row
    data = (1 + rng.poisson(2.0, size=B * nnz_row)).astype(np.float32)
    m = PoissonFactorization(latent_dim=K, feature_dim=D, u_tau_scale=1 / math.sqrt(B * D),
                             initialize_distributions=False, device="cuda")
    m.xi_u_global = 4.0
    sc = SparseCounts.from_any((indptr, cols.reshape(-1), data, (B, D)), m.device, None, latent_dim=K)
    g = torch.Generator(device="cuda").manual_seed(seed)

    def pos(*shape):
        return torch.exp(0.5 * torch.randn(*shape, device="cuda", generator=g)) * 0.3
    draws = {"u": pos(S, D, K), "v": pos(S, K, D), "w": pos(S, 1, D), "s": pos(S, 2, D) + 0.5}
    return m, {"counts": sc}, draws


def _median_ms(fn, warmup=3, reps=10):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def run_step(name, once=False, cols=False):
    import torch
    B, D, K, S, both, _ = STEPS[name]
    m, batch, draws = _problem(B, D, K, S)
    kw = {"col_scores": True} if cols else {}
    if once:
        out = m.waic_streaming(batch, draws=draws, **kw)
        torch.cuda.synchronize()
        print(json.dumps({"step": name, "once": True, "cols": cols,
                          **{k: out[k] for k in ("lppd", "pwaic", "n", "n_excluded")}}))
        return
    res = {"step": name, "B": B, "D": D, "K": K, "S": S, "cols": cols}
    out = {}

    def streaming():
        out["s"] = m.waic_streaming(batch, draws=draws, **kw)
    med, lo, hi = _median_ms(streaming)
    res.update(streaming_ms=round(med, 3), streaming_min_ms=round(lo, 3), streaming_max_ms=round(hi, 3),
               lppd=out["s"]["lppd"], pwaic=out["s"]["pwaic"], n_excluded=out["s"]["n_excluded"])
    if both:
        def materialising():
            ll = m.log_likelihood_components(s=draws["s"], u=draws["u"], v=draws["v"], w=draws["w"],
                                             data=batch)["log_likelihood"].double()
            lp = torch.logsumexp(ll, 0) - math.log(S)
            pw = ll.var(0, unbiased=True)
            e = lp - pw
            out["m"] = (float(lp.sum()), float(pw.sum()), float(2.0 * torch.sqrt(e.numel() * e.var(unbiased=True))))
        med, lo, hi = _median_ms(materialising)
        res.update(materialising_ms=round(med, 3), materialising_min_ms=round(lo, 3),
                   materialising_max_ms=round(hi, 3), materialising_lppd=out["m"][0],
                   materialising_pwaic=out["m"][1], materialising_se=out["m"][2], streaming_se=out["s"]["se"])
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--cols", action="store_true", help="waic_streaming(col_scores=True)")
    a = ap.parse_args()
    if a.step:
        run_step(a.step, a.once, a.cols)
        return 0
    for name in ("shared", "c2"):       # a fresh child per step, each under its own time limit
        rc = subprocess.run(["timeout", "-k", "10", str(STEPS[name][5]), sys.executable, os.path.abspath(__file__),
                             "--step", name] + (["--cols"] if a.cols else [])).returncode
        if rc != 0:
            print(f"step {name} ended with status {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
