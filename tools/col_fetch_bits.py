"""Do two builds of the library return the same bits from a deterministic-mode step?

    col_fetch_bits.py dump FILE          run one deterministic step per case with the library that SPMF_LIB_PATH
                                         names (default: the tree's own) and save its 14 parts and 12 gradients
    col_fetch_bits.py compare A B [OUT]  compare two dumps tensor by tensor with torch.equal -> one JSON line,
                                         also written to OUT

The column pass adds an item's entries into its sums in list order, four at a time, whatever the width of the
list fetch; the deterministic mode has no atomics, so a change of the fetch must leave every bit where it was.
Cases: a C3-shaped shard (250 000 x 20 000, K = 32, balanced panels: work items of up to 256 entries), run twice
(the second run against the first is the mode's own bar), and the list problems of tests/test_gpu_col_fetch.py at
K = 2 ... 64 with their lists cut as a production shape cuts them.  A dump is made in a process of its own per
build (a library is loaded once per process)."""
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dump(path, rows=250_000):
    import torch
    from spmf_amd import PoissonFactorization, _lib, synth
    from spmf_amd.sparse import balanced_panel_rows
    out = {"lib": os.path.relpath(_lib.LIB_PATH, ROOT), "device": torch.cuda.get_device_name(0)}
    dev = torch.device("cuda", 0)

    def keep(tag, step):
        parts, grads, _ = step
        for k, v in parts.items():
            out[f"{tag}/part_{k}"] = v.cpu().clone()
        for k, v in grads.items():
            out[f"{tag}/grad_{k}"] = v.cpu().clone()

    D, K = 20_000, 32
    sc = synth.linear_structure(rows, D, 0.005, dev, panel_rows=balanced_panel_rows(rows, K))
    with contextlib.redirect_stdout(sys.stderr):
        m = PoissonFactorization(latent_dim=K, feature_dim=D, u_tau_scale=1.0 / (rows * D) ** 0.5, device=dev,
                                 deterministic=True)
    colsum = torch.zeros(D, dtype=torch.float64, device=dev)
    colnnz = torch.zeros_like(colsum)
    sc.compute_stats(m._handle(), colsum, colnnz)
    cm = colsum / colnnz
    m.eta_i = torch.where(cm > 1, cm, torch.ones_like(cm)).reshape(1, D)
    m.xi_u_global = float(torch.nansum(cm))
    torch.manual_seed(7)
    params = m.surrogate_distribution.sample(1)
    for call in (0, 1):
        keep(f"shard_{rows}x{D}_K{K}/call{call}", m.energy_and_grads({"counts": sc}, params))
    out["shard_segment"] = int(getattr(sc, "segment", 0))
    del sc, m

    import _pass_cases as T
    from _problems import build_model
    for K in (2, 4, 8, 16, 32, 64):
        cfg, X, params, _ = T._list_case(K)
        m = build_model(cfg, T.R)
        m.deterministic = True
        keep(f"lists_K{K}", m.energy_and_grads({"counts": T._packed(X)}, params))
    torch.cuda.synchronize()
    torch.save(out, path)
    print(f"{sum(torch.is_tensor(v) for v in out.values())} tensors of {out['lib']} -> {path}")


def compare(a_path, b_path, out_path=None):
    import torch
    a, b = torch.load(a_path), torch.load(b_path)
    keys = sorted(k for k in a if torch.is_tensor(a[k]))
    assert keys == sorted(k for k in b if torch.is_tensor(b[k])), "the two dumps hold different outputs"

    def bits(t):
        return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.dtype.is_floating_point else t
    res = {"a": a["lib"], "b": b["lib"], "device": a["device"], "shard_segment": a.get("shard_segment")}
    cases = sorted({k.rsplit("/", 1)[0] for k in keys})
    for c in cases:
        mine = [k for k in keys if k.rsplit("/", 1)[0] == c]
        differ = [k for k in mine if not torch.equal(bits(a[k]), bits(b[k]))]
        res[c] = {"tensors": len(mine), "equal": len(mine) - len(differ), "differ": differ}
    # the mode's own bar: two calls of one build
    for name, d in (("a", a), ("b", b)):
        first = [k for k in keys if "/call0/" in k]
        res[f"two_calls_of_{name}_equal"] = all(torch.equal(bits(d[k]), bits(d[k.replace("/call0/", "/call1/")]))
                                                for k in first)
    line = json.dumps(res)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return 0 if not any(res[c]["differ"] for c in cases) else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) in (4, 5) and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
