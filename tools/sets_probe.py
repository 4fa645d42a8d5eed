#!/usr/bin/env python
"""Time set_scores (csrc/sets.hip) against the route of the commit before it, at C2's streaming shape: 20 000 x
5 000 Poisson counts (the problem of tools/waic_time.py --step c2), K = 16, S = 32 draws, mean and sd.

Two cases: `fifty` -- 50 sets of 100 seeded columns each, signed weights; `all` -- one set of all columns.
Two routes:
  set_scores   the call;
  predict      predict one draw at a time over the union of the sets' columns (a dense [rows, M] fp32 block per
               draw), converted to fp64 and multiplied with the [M, G] weight matrix in torch, the per-draw scores
               folded into mean and sd by Welford's recurrence -- S encode sweeps, S dense blocks.

    python tools/sets_probe.py                       # every (case, route) in a fresh child process, alternated
                                                     # three times; medians and spreads -> profiles/sets_probe.json
    python tools/sets_probe.py --case fifty --route set_scores      # one child: one JSON line

A child reports the median of 10 timed calls after 3 warm-ups, the device synchronised around every timed call;
the set_scores child also reports the largest |mean - route's mean| / mean sum |w m| once, outside the timing."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

B, D, K, S = 20_000, 5_000, 16, 32
CASES = ("fifty", "all")
ROUTES = ("set_scores", "predict")
CHILD_LIMIT = 300


def _sets(case):
    import numpy as np
    rng = np.random.default_rng(31)
    if case == "all":
        return [np.arange(D)], None
    sets = [rng.choice(D, 100, replace=False) for _ in range(50)]
    weights = [(rng.uniform(0.25, 2.0, 100) * rng.choice([-1.0, 1.0], 100)).astype(np.float32) for _ in sets]
    return sets, weights


def run_child(case, route):
    import numpy as np
    import torch
    from waic_time import _median_ms, _problem
    m, batch, draws = _problem(B, D, K, S)
    sets, weights = _sets(case)
    union = np.unique(np.concatenate(sets))
    W = torch.zeros(len(union), len(sets), dtype=torch.float64, device="cuda")
    for g, cols in enumerate(sets):
        w = np.ones(len(cols)) if weights is None else weights[g].astype(np.float64)
        W[:, g].index_add_(0, torch.as_tensor(np.searchsorted(union, cols), device="cuda"),
                           torch.as_tensor(w, device="cuda"))
    cols_dev = torch.as_tensor(union, device="cuda")
    out = {}

    def new():
        out["new"] = m.set_scores(batch, sets, weights, draws=draws, sd=True)

    def old(mag=False):
        mu = torch.zeros(B, len(sets), dtype=torch.float64, device="cuda")
        q, tot = torch.zeros_like(mu), torch.zeros_like(mu)
        absw = W.abs() if mag else None
        top = torch.zeros_like(mu) if mag else None
        for s in range(S):
            one = {n: v[s:s + 1] for n, v in draws.items()}
            cells = m.predict(batch, None if case == "all" else cols_dev, draws=one)["mean"].double()
            x = cells @ W
            if mag:
                top += cells.abs() @ absw
            del cells
            tot += x
            dl = x - mu
            mu += dl / (s + 1)
            q += dl * (x - mu)
        out["old"] = {"mean": tot / S, "sd": torch.sqrt(q / (S - 1)), "mag": top / S if mag else None}

    res = {"case": case, "route": route, "B": B, "D": D, "K": K, "S": S, "sets": len(sets),
           "listed": int(sum(len(c) for c in sets)), "union": int(len(union))}
    med, lo, hi = _median_ms(new if route == "set_scores" else old)
    res.update(median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3))
    if route == "set_scores":
        old(mag=True)
        torch.cuda.synchronize()
        n, o = out["new"], out["old"]
        res["max_mean_diff_over_mean_sum_abs_wm"] = float(((n["mean"] - o["mean"]).abs()
                                                           / o["mag"].clamp_min(1e-300)).max())
        res["max_sd_diff_over_mean_sum_abs_wm"] = float(((n["sd"] - o["sd"]).abs() / o["mag"].clamp_min(1e-300)).max())
        again = m.set_scores(batch, sets, weights, draws=draws, sd=True)
        res["repeat_has_the_same_bits"] = all(
            bool(torch.equal(again[k].view(torch.int64), n[k].view(torch.int64))) for k in ("mean", "sd"))
        res["all_finite"] = bool(torch.isfinite(n["mean"]).all() and torch.isfinite(n["sd"]).all())
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--route", choices=ROUTES)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sets_probe.json"))
    a = ap.parse_args()
    if a.case or a.route:
        run_child(a.case or "fifty", a.route or "set_scores")
        return 0
    runs = {c: {r: [] for r in ROUTES} for c in CASES}
    for case in CASES:
        for _ in range(a.rounds):
            for route in ROUTES:       # a fresh child per measurement, each under its own time limit
                p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__),
                                    "--case", case, "--route", route], stdout=subprocess.PIPE, text=True)
                if p.returncode != 0:
                    print(f"{case} / {route} ended with status {p.returncode}: stopping", file=sys.stderr)
                    return p.returncode
                line = p.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                runs[case][route].append(json.loads(line))
    res = {"shape": {"rows": B, "D": D, "K": K, "S": S, "problem": "tools/waic_time.py _problem (5 % stored)"},
           "order": "set_scores, predict route, alternated %d times per case, a fresh process each; every figure "
                    "is the child's median over 10 timed calls" % a.rounds, "cases": {}}
    for case in CASES:
        new = [r["median_ms"] for r in runs[case]["set_scores"]]
        old = [r["median_ms"] for r in runs[case]["predict"]]
        first = runs[case]["set_scores"][0]
        res["cases"][case] = {
            "sets": first["sets"], "listed": first["listed"], "union": first["union"],
            "set_scores_ms": new, "predict_route_ms": old,
            "set_scores_median": statistics.median(new), "predict_route_median": statistics.median(old),
            "set_scores_spread": round(max(new) - min(new), 3), "predict_route_spread": round(max(old) - min(old), 3),
            "not_slower_beyond_the_routes_spread":
                statistics.median(new) <= statistics.median(old) + (max(old) - min(old)),
            "agreement": {k: first[k] for k in ("max_mean_diff_over_mean_sum_abs_wm",
                                                "max_sd_diff_over_mean_sum_abs_wm", "repeat_has_the_same_bits",
                                                "all_finite")}}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
