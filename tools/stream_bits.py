"""Do two builds of the library return the same bits from the streaming calls?

    stream_bits.py dump FILE          run top_k, score_cells, rank_cells, embed, predict, top_rows, group_means,
                                      set_scores and waic_streaming at four small cases, and knn at two shapes, with the library
                                      that SPMF_LIB_PATH names (default: the tree's own) and save every output to FILE
    stream_bits.py compare A B [OUT]  compare two dumps tensor by tensor with torch.equal -> one JSON line,
                                      also written to OUT

The cases are problems of tests/_stream_cases.py, (likelihood, B, D, K, S): poisson (131, 197, 16, 7), mixed
(65, 130, 40, 3), bernoulli_log (70, 150, 3, 2) and poisson (40, 70, 128, 3), i.e. KP 16, 64, 4 and 128.
top_k: k = 10 and 64, stored cells excluded and not, columns and scores.  score_cells: every cell listed in a
seeded random order with values 0 .. 3: mean and lppd.  rank_cells: the same list, stored cells excluded: rank,
candidates and score.  embed: mean and (S >= 2) deviation.  predict: mean, (S >= 2) sd and p_nonzero for all
columns and for the list (D - 1, 0, 3, 3, D // 2), which holds a duplicate.  top_rows: k = 10 and 64, stored cells
excluded and not, for all columns and for the same list: rows and scores.  group_means: sum and sum_nonzero for
the labels -1, 0, 1, 2, -1, ... with four groups (group 3 is empty), all columns and the same list.  set_scores:
mean and sd of three sets -- that list (its repeated column counts twice), an empty set and every second column --
with seeded normal weights.  knn: two of tests/test_gpu_knn.py's SHAPES with its
points, (nq, nr, K, k) = (131, 197, 16, 10) Euclidean under both SPMF_KNN_TILE values and (5, 333, 33, 64) cosine:
indices and distances.  waic_streaming (row scores included) is called
TWICE in each dump: its fp64 sums are atomics, so `compare` also reports whether the two calls of one build
agree, which is the bar a comparison across builds has to be read against.

A dump is made in a process of its own per build (a library is loaded once per process); a build from before
embed / knn (predict, top_rows, group_means, set_scores) lacks their entry points and dumps no tensor of theirs."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [("poisson", 131, 197, 16, 7), ("mixed", 65, 130, 40, 3), ("bernoulli_log", 70, 150, 3, 2),
         ("poisson", 40, 70, 128, 3)]
KNN_CASES = [(131, 197, 16, 10, "euclidean", ("0", "1")), (5, 333, 33, 64, "cosine", (None,))]
CALLS = ("top_k", "score_cells", "rank_cells", "embed", "knn", "predict", "top_rows", "group_means", "set_scores")


def dump(path):
    import numpy as np
    import torch
    from spmf_amd import _lib
    have = C.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        print(f"{_lib.LIB_PATH} has no {name}: not bound", file=sys.stderr)
        del _lib.SIGNATURES[name]
    from _stream_cases import _problem
    from _problems import _dense_model
    with_knn = "spmf_knn" in _lib.SIGNATURES and "spmf_embed_rows" in _lib.SIGNATURES
    out = {"lib": os.path.relpath(_lib.LIB_PATH, ROOT), "tree": os.path.basename(ROOT),
           "device": torch.cuda.get_device_name(0)}
    for lik, B, D, K, S in CASES:
        cfg, x, params, mask, _ = _problem(lik, B, D, K, S)
        m = _dense_model(lik, cfg, mask, 32)
        batch = {"counts": x}
        tag = f"{lik}_{B}x{D}_K{K}_S{S}"
        for k in (10, 64):
            for ex in (True, False):
                top = m.top_k(batch, k=k, draws=params, exclude_stored=ex)
                out[f"top_k/{tag}/k{k}/exclude{int(ex)}/columns"] = top["columns"].cpu()
                out[f"top_k/{tag}/k{k}/exclude{int(ex)}/scores"] = top["scores"].cpu()
        cell = np.random.default_rng(5).permutation(B * D)
        sc = m.score_cells(batch, cell // D, cell % D, values=(cell % 4).astype(np.float32), draws=params)
        out[f"score_cells/{tag}/mean"] = sc["mean"].cpu()
        out[f"score_cells/{tag}/lppd"] = sc["lppd"].cpu()
        rk = m.rank_cells(batch, cell // D, cell % D, draws=params)
        for name in ("rank", "candidates", "score"):
            out[f"rank_cells/{tag}/{name}"] = rk[name].cpu()
        if with_knn:
            for name, v in m.embed(batch, draws=params, sd=S >= 2).items():
                out[f"embed/{tag}/{name}"] = v.cpu()
        listed = np.array([D - 1, 0, 3, 3, D // 2])
        for cols, ctag in ((None, "all"), (listed, "listed")):
            if "spmf_predict_columns" in _lib.SIGNATURES:
                for name, v in m.predict(batch, cols=cols, draws=params, sd=S >= 2, p_nonzero=True).items():
                    if name != "columns":
                        out[f"predict/{tag}/{ctag}/{name}"] = v.cpu()
            if "spmf_toprows_columns" in _lib.SIGNATURES:
                for k in (10, 64):
                    for ex in (True, False):
                        top = m.top_rows(batch, cols=cols, k=k, draws=params, exclude_stored=ex)
                        for name in ("rows", "scores"):
                            out[f"top_rows/{tag}/{ctag}/k{k}/exclude{int(ex)}/{name}"] = top[name].cpu()
            if "spmf_group_sums" in _lib.SIGNATURES:
                grp = m.group_means(batch, np.arange(B) % 4 - 1, n_groups=4, cols=cols, draws=params, p_nonzero=True)
                assert grp["count"].tolist()[3] == 0
                for name in ("sum", "sum_nonzero"):
                    out[f"group_means/{tag}/{ctag}/{name}"] = grp[name].cpu()
        if "spmf_set_scores" in _lib.SIGNATURES:
            sets = [listed, np.array([], dtype=np.int64), np.arange(0, D, 2)]
            wts = [np.random.default_rng(7 + i).normal(size=len(s)).astype(np.float32) for i, s in enumerate(sets)]
            sc = m.set_scores(batch, sets, weights=wts, draws=params, sd=True)
            for name in ("mean", "sd"):
                out[f"set_scores/{tag}/{name}"] = sc[name].cpu()
        for call in (0, 1):
            w = m.waic_streaming(batch, draws=params, row_scores=True)
            for name, v in w.items():
                v = v.cpu() if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
                out[f"waic_streaming/{tag}/{name}/call{call}"] = v
    if with_knn:
        from _stream_cases import _points
        for nq, nr, K, k, metric, tiles in KNN_CASES:
            Q, R = _points(nq, nr, K, False)
            for tile in tiles:
                if tile is not None:
                    os.environ["SPMF_KNN_TILE"] = tile
                try:
                    nn = m.knn(torch.as_tensor(R).cuda(), k=k, queries=torch.as_tensor(Q).cuda(), metric=metric)
                finally:
                    os.environ.pop("SPMF_KNN_TILE", None)
                for name in ("indices", "distances"):
                    out[f"knn/{nq}x{nr}_K{K}_k{k}_{metric}/tile{tile}/{name}"] = nn[name].cpu()
    torch.cuda.synchronize()
    torch.save(out, path)
    print(f"{sum(torch.is_tensor(v) for v in out.values())} tensors of {out['lib']} -> {path}")


def _bits(t):
    import torch
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.dtype.is_floating_point else t


def compare(a_path, b_path, out_path=None):
    import torch
    a, b = torch.load(a_path), torch.load(b_path)
    keys = sorted(k for k in a if torch.is_tensor(a[k]))
    assert keys == sorted(k for k in b if torch.is_tensor(b[k])), "the two dumps hold different outputs"
    res = {"a": a["lib"], "b": b["lib"], "a_tree": a.get("tree"), "b_tree": b.get("tree"), "device": a["device"], "cases": ["%s %dx%d K=%d S=%d" % c for c in CASES],
           "knn_cases": ["%dx%d K=%d k=%d %s, SPMF_KNN_TILE %s" % (*c[:5], " and ".join(t or "unset" for t in c[5]))
                         for c in KNN_CASES]}
    for call in CALLS:
        mine = [k for k in keys if k.startswith(call + "/")]
        differ = [k for k in mine if not torch.equal(_bits(a[k]), _bits(b[k]))]
        res[call] = {"tensors": len(mine), "equal": len(mine) - len(differ), "differ": differ}
    # waic_streaming: call 0 of A against call 0 of B, beside call 0 against call 1 inside each build
    mine = [k[:-len("/call0")] for k in keys if k.startswith("waic_streaming/") and k.endswith("/call0")]

    def rel(x, y):
        ne = (_bits(x) != _bits(y)).reshape(-1)
        x, y = x.double().reshape(-1)[ne], y.double().reshape(-1)[ne]
        d = torch.nan_to_num((x - y).abs() / x.abs().clamp_min(1e-300), nan=float("inf"))
        return float(d.max()) if d.numel() else 0.0
    w = {"tensors": len(mine)}
    for name, (p, q, i, j) in {"across_builds": (a, b, 0, 0), "two_calls_of_a": (a, a, 0, 1),
                               "two_calls_of_b": (b, b, 0, 1)}.items():
        eq = [torch.equal(_bits(p[f"{k}/call{i}"]), _bits(q[f"{k}/call{j}"])) for k in mine]
        w[name] = {"equal": sum(eq), "largest_relative_difference":
                   max(rel(p[f"{k}/call{i}"], q[f"{k}/call{j}"]) for k in mine)}
    res["waic_streaming"] = w
    line = json.dumps(res)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return 0 if not any(res[c]["differ"] for c in CALLS) else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) in (4, 5) and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
