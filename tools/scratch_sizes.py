"""Do two builds of the library report the same workspace and scratch sizes?

    scratch_sizes.py dump FILE          call every size function of the library that SPMF_LIB_PATH names (default:
                                        the tree's own) over the grid below and save the integers to FILE as JSON
    scratch_sizes.py compare A B [OUT]  compare two dumps value by value -> one JSON line, also written to OUT

Every size function is the library's layout of that memory run without memory (spmf_amd/csrc/arena.h), so equal
sizes over a grid that reaches every conditional buffer say the layouts agree region by region in their totals.

The grid.  Contexts (K, D, flags): (3, 17, 0), (16, 197, 0), (32, 20000, SCALE_ROWS), (50, 350, 0), (128, 70, 0),
(40, 130, MIXED), (64, 6000, LOG_TRANSFORM | SCALE_ROWS) and the same after spmf_ctx_set_e_cap(1 MiB),
(3, 150, BERNOULLI | LOG_TRANSFORM), and (32, 5000, 0) after spmf_ctx_set_column_split(2500) -- which the library
refuses, a split being a multiple of 32: that context has none -- and after spmf_ctx_set_column_split(2496); a
setting's return code is part of its context's name.  Rows 0, 1, 63, 64, 65, 2048, 2049, 4096, 100000, 2^20;
S 1, 2, 7, 20.  spmf_workspace_bytes and the waic / topk / cells / rank /
predict / embed sizes: every context x rows x S.  Groups: G 1, 4, 1025, 2^24 x n_cols 0, 5, D on top of that.  Top
rows: n_cols 0, 5, 64, 65, D on top of that (64 / 65 where D allows).  Sets:
set_ptr (0), (0, 0), (0, 4), (0, 64, 65, 65, 200) on top of that.  knn (context-free but for the device):
(n_query, n_ref, row_len) (0, 0, 8), (131, 197, 16), (5, 333, 33), (100000, 100000, 256).  Deterministic-mode
scratch: n_items 0, 1, 1000 x S 1, 2 per context.  One call with an invalid argument per function: it returns 0.

No GPU is needed, except for spmf_layout_sizes_k (it asks rocPRIM for its temporary storage on the device): its
sizes, for LAYOUTS below, are dumped only where a device is present, and "layout_sizes_dumped" says whether.
The top-k, top-rows and knn sizes depend on the device's CU count (256 is assumed without a device): compare dumps made on
the same machine."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = (0, 1, 63, 64, 65, 2048, 2049, 4096, 100000, 1 << 20)
DRAWS = (1, 2, 7, 20)
GROUPS = (1, 4, 1025, 1 << 24)
SETS = ((0,), (0, 0), (0, 4), (0, 64, 65, 65, 200))
KNN = ((0, 0, 8), (131, 197, 16), (5, 333, 33), (100000, 100000, 256))
DET = [(n, s) for n in (0, 1, 1000) for s in (1, 2)]
# (n_rows, nnz, n_cols, panel_rows, latent_dim)
LAYOUTS = ((0, 0, 17, 32, 0), (131, 2000, 197, 32, 16), (2049, 100000, 350, 100000, 3),
           (100000, 5000000, 20000, 4096, 32), (1 << 20, 50000000, 6000, 65536, 64))
ROW_S_CALLS = ("spmf_workspace_bytes", "spmf_waic_scratch_bytes", "spmf_topk_scratch_bytes",
               "spmf_cells_scratch_bytes", "spmf_rank_scratch_bytes", "spmf_predict_scratch_bytes",
               "spmf_embed_scratch_bytes")


def _contexts(lib):
    from spmf_amd import _lib
    SR, LT, BE, MX = _lib.FLAG_SCALE_ROWS, _lib.FLAG_LOG_TRANSFORM, _lib.FLAG_BERNOULLI, _lib.FLAG_MIXED
    specs = [(3, 17, 0, None), (16, 197, 0, None), (32, 20000, SR, None), (50, 350, 0, None), (128, 70, 0, None),
             (40, 130, MX, None), (64, 6000, LT | SR, None), (64, 6000, LT | SR, ("e_cap", 1 << 20)),
             (3, 150, BE | LT, None), (32, 5000, 0, ("column_split", 2500)), (32, 5000, 0, ("column_split", 2496))]
    for K, D, flags, setting in specs:
        h = C.c_void_p()
        assert lib.spmf_ctx_create(0, K, D, flags, C.byref(h)) == 0, (K, D, flags)
        tag = f"K{K}_D{D}_flags{flags}"
        if setting:
            rc = getattr(lib, "spmf_ctx_set_" + setting[0])(h, setting[1])
            tag += f"_{setting[0]}{setting[1]}_rc{rc}"
        yield tag, h, D
        lib.spmf_ctx_destroy(h)


def dump(path):
    from spmf_amd import _lib
    lib = _lib.load()
    out = {}
    for tag, h, D in _contexts(lib):
        for rows in ROWS:
            for S in DRAWS:
                at = f"{tag}/rows{rows}/S{S}"
                for fn in ROW_S_CALLS:
                    out[f"{fn}/{at}"] = getattr(lib, fn)(h, rows, S)
                for G in GROUPS:
                    for n_cols in (0, 5, D):
                        out[f"spmf_groups_scratch_bytes/{at}/G{G}/C{n_cols}"] = \
                            lib.spmf_groups_scratch_bytes(h, rows, S, G, n_cols)
                for n_cols in sorted({n for n in (0, 5, 64, 65, D) if n <= D}):
                    out[f"spmf_toprows_scratch_bytes/{at}/C{n_cols}"] = lib.spmf_toprows_scratch_bytes(h, rows, S, n_cols)
                for ptr in SETS:
                    arr = (C.c_int64 * len(ptr))(*ptr)
                    out[f"spmf_sets_scratch_bytes/{at}/ptr{'_'.join(map(str, ptr))}"] = \
                        lib.spmf_sets_scratch_bytes(h, rows, S, len(ptr) - 1, arr)
        for nq, nr, row_len in KNN:
            out[f"spmf_knn_scratch_bytes/{tag}/{nq}x{nr}_len{row_len}"] = lib.spmf_knn_scratch_bytes(h, nq, nr, row_len)
        for n_items, S in DET:
            out[f"spmf_det_scratch_bytes/{tag}/items{n_items}/S{S}"] = lib.spmf_det_scratch_bytes(h, n_items, S)
        # one invalid argument each: every one of these is 0
        for fn in ROW_S_CALLS:
            out[f"{fn}/{tag}/invalid_rows-1"] = getattr(lib, fn)(h, -1, 2)
        out[f"spmf_toprows_scratch_bytes/{tag}/invalid_C-1"] = lib.spmf_toprows_scratch_bytes(h, 64, 2, -1)
        out[f"spmf_groups_scratch_bytes/{tag}/invalid_G0"] = lib.spmf_groups_scratch_bytes(h, 64, 2, 0, 5)
        bad = (C.c_int64 * 3)(0, 9, 4)
        out[f"spmf_sets_scratch_bytes/{tag}/invalid_ptr_decreasing"] = lib.spmf_sets_scratch_bytes(h, 64, 2, 2, bad)
        out[f"spmf_knn_scratch_bytes/{tag}/invalid_len0"] = lib.spmf_knn_scratch_bytes(h, 5, 5, 0)
        out[f"spmf_det_scratch_bytes/{tag}/invalid_S0"] = lib.spmf_det_scratch_bytes(h, 10, 0)
    assert all(v == 0 for k, v in out.items() if "/invalid_" in k), "an invalid call returned a size"
    dumped = True
    for shape in LAYOUTS:
        lb, sb = C.c_size_t(), C.c_size_t()
        if lib.spmf_layout_sizes_k(0, *shape, C.byref(lb), C.byref(sb)) != 0:
            dumped = False      # no device to ask
            break
        at = "rows%d_nnz%d_D%d_P%d_K%d" % shape
        out[f"spmf_layout_sizes_k/{at}/layout"] = lb.value
        out[f"spmf_layout_sizes_k/{at}/scratch"] = sb.value
    res = {"lib": os.path.relpath(_lib.LIB_PATH, ROOT), "layout_sizes_dumped": dumped, "sizes": out}
    with open(path, "w") as f:
        json.dump(res, f)
    print(f"{len(out)} sizes of {res['lib']} -> {path} (layout sizes {'dumped' if dumped else 'not dumped: no device'})")


def compare(a_path, b_path, out_path=None):
    with open(a_path) as f:
        a = json.load(f)
    with open(b_path) as f:
        b = json.load(f)
    assert sorted(a["sizes"]) == sorted(b["sizes"]), "the two dumps hold different calls"
    res = {"a": a["lib"], "b": b["lib"],
           "layout_sizes_dumped": a["layout_sizes_dumped"] and b["layout_sizes_dumped"]}
    differ = []
    for fn in sorted({k.split("/")[0] for k in a["sizes"]}):
        mine = [k for k in a["sizes"] if k.split("/")[0] == fn]
        bad = [k for k in mine if a["sizes"][k] != b["sizes"][k]]
        res[fn] = {"values": len(mine), "equal": len(mine) - len(bad), "invalid_calls_zero":
                   all(a["sizes"][k] == 0 and b["sizes"][k] == 0 for k in mine if "/invalid_" in k),
                   "largest": max(a["sizes"][k] for k in mine), "differ": bad[:20]}
        differ += bad
    res["all_equal"] = not differ
    line = json.dumps(res)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return 0 if not differ else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) in (4, 5) and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
