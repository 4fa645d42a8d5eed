"""What the tests of the streaming calls share: the cached problems of the GPU files, the host helpers of the
*_host.py files (library, cpu_model, no_library, host_ctx) and, for the C-ABI, ONE contract table of the
draw-stage entry points, every one that include/spmf_hip.h declares (waic_streaming / spmf_waic_accumulate and
spmf_waic_accumulate_cols, top_k / spmf_topk_rows, score_cells / spmf_score_cells, rank_cells / spmf_rank_cells,
predict / spmf_predict_columns, group_means / spmf_group_sums, embed / spmf_embed_rows, top_rows /
spmf_toprows_columns, set_scores / spmf_set_scores): each entry as a raw ctypes call with a dict of good
arguments -- dummy addresses without a device (host_good_call), real buffers with one (gpu_good_call) -- plus the
error contract of the draw stage they have in common (include/spmf_hip.h), asserted by one function on a device
(test_gpu_stream_abi.py) and without one (test_stream_host.py).  A new draw-stage call adds one row to ENTRIES
and one branch to each of the two good calls.  spmf_knn and spmf_kmeans_step are no draw-stage calls: each has
its argument list, raw call and error contract here once, behind the table's.
"""
import collections
import ctypes as C
import fnmatch
import functools
import os
import re

import numpy as np
import torch

from oracle import spmf_oracle as O
from _problems import _dense_model, _dense_problem

T = torch.as_tensor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BERN_DAMP = {"bernoulli": 1.0 / 64.0, "bernoulli_log": 1.0 / 8.0}

# the shape of the contract tests: a ragged 64-row block, K padded 3 -> 4, two draws so that sd is defined
B, D, K, S = 70, 45, 3, 2
# the list of predict / groups / toprows in the good calls: four columns, one of them twice
PANEL_COLS = (7, 0, 7, 44)
# the sets of the GPU good call over those columns, one of them empty, and their weights (one set has some)
PANEL_SETS = ((7, 0), (), (44, 7, 7))
PANEL_WEIGHTS = ((0.5, -1.25), (), (1.0, 1.0, 1.0))

# One row per entry point: the call, its scratch size, the smallest S, the Python method, `own`: the arguments
# between `eta` and `scratch` in the header's order with their ctypes, `size_args`: those of `own` the size
# function takes behind (rows, S), `header_args`: the argument counts of (scratch size, call) in include/spmf_hip.h
Entry = collections.namedtuple("Entry", "call size min_S method own size_args header_args")
_P, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64
ENTRIES = {
    "waic": Entry("spmf_waic_accumulate", "spmf_waic_scratch_bytes", 2, "waic_streaming",
                  (("sums", _P), ("rows", _P)), (), (3, 10)),
    "topk": Entry("spmf_topk_rows", "spmf_topk_scratch_bytes", 1, "top_k",
                  (("k", C.c_int), ("flags", C.c_uint), ("cols", _P), ("scores", _P)), (), (3, 12)),
    "cells": Entry("spmf_score_cells", "spmf_cells_scratch_bytes", 1, "score_cells",
                   (("n", _I64), ("row", _P), ("col", _P), ("val", _P), ("mean", _P), ("lppd", _P)), (), (3, 14)),
    "rank": Entry("spmf_rank_cells", "spmf_rank_scratch_bytes", 1, "rank_cells",
                  (("n", _I64), ("row", _P), ("col", _P), ("flags", C.c_uint), ("rank", _P), ("cand", _P),
                   ("score", _P)), (), (3, 15)),
    "predict": Entry("spmf_predict_columns", "spmf_predict_scratch_bytes", 1, "predict",
                     (("n", _I32), ("cols", _P), ("mean", _P), ("sd", _P), ("pnz", _P)), (), (3, 13)),
    "groups": Entry("spmf_group_sums", "spmf_groups_scratch_bytes", 1, "group_means",
                    (("labels", _P), ("G", _I32), ("n", _I32), ("cols", _P), ("sum", _P), ("nz", _P)), ("G", "n"),
                    (5, 14)),
    "embed": Entry("spmf_embed_rows", "spmf_embed_scratch_bytes", 1, "embed", (("mean", _P), ("sd", _P)), (),
                   (3, 10)),
    "waic_cols": Entry("spmf_waic_accumulate_cols", "spmf_waic_scratch_bytes", 2, "waic_streaming",
                       (("sums", _P), ("rows", _P), ("colsum", _P)), (), (3, 11)),
    "toprows": Entry("spmf_toprows_columns", "spmf_toprows_scratch_bytes", 1, "top_rows",
                     (("n", _I32), ("cols", _P), ("k", C.c_int), ("flags", C.c_uint), ("rows", _P), ("scores", _P)),
                     ("n",), (4, 14)),
    # set_ptr is a HOST array the entry reads before anything else: a real int64 array in both good calls
    "sets": Entry("spmf_set_scores", "spmf_sets_scratch_bytes", 1, "set_scores",
                  (("n_sets", _I32), ("set_ptr", _P), ("cols", _P), ("weights", _P), ("ld", _I64), ("mean", _P),
                   ("sd", _P)), ("n_sets", "set_ptr"), (5, 15)),
}


# ---- what the *_host.py files share ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def library():
    """The loaded library, built first where the shared object is missing."""
    import __graft_entry__ as ge
    from spmf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def cpu_model(**kw):
    """-> (a CPU-only Poisson model of 6 columns and K = 2, seeded counts [8, 6], two seeded draws)."""
    from spmf_amd import PoissonFactorization
    m = PoissonFactorization(latent_dim=2, feature_dim=6, initialize_distributions=False, device="cpu", **kw)
    rng = np.random.default_rng(0)
    x = rng.poisson(1.0, size=(8, 6)).astype(np.float64)
    draws = {"u": rng.random((2, 6, 2)), "v": rng.random((2, 2, 6)), "w": rng.random((2, 1, 6)),
             "s": rng.random((2, 2, 6))}
    return m, x, draws


def no_library(monkeypatch):
    """Any load of the library from here on fails the test."""
    from spmf_amd import _lib

    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def host_ctx(lib, k, flags=0, d=D):
    h = C.c_void_p()
    assert lib.spmf_ctx_create(0, k, d, flags, C.byref(h)) == 0
    return h


def assert_declared_exported_bound(name, nargs):
    """``name`` is declared in include/spmf_hip.h with ``nargs`` arguments, matched by the export list and
    bound in spmf_amd._lib with as many."""
    from spmf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spmf_hip.h")).read(), flags=re.S)
    exports = open(os.path.join(ROOT, "spmf_amd", "csrc", "exports.map")).read()
    exports = re.sub(r"/\*.*?\*/", "", exports, flags=re.S)
    globs = re.search(r"global:\s*([^}]*?)local:", exports, re.S).group(1)
    patterns = [p.strip() for p in globs.split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
    assert name in _lib.SIGNATURES, name
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/spmf_hip.h"
    declared = len([a for a in m.group(1).split(",") if a.strip()])
    assert len(_lib.SIGNATURES[name][1]) == declared == nargs, name
    assert "define SPMF_ABI_VERSION 6" in hdr and _lib.ABI_VERSION == 6


def _bern_cols(lik, mask, D):
    if lik.startswith("bernoulli"):
        return np.ones(D, dtype=bool)
    return np.asarray(mask, dtype=bool) if mask is not None else np.zeros(D, dtype=bool)


def _oracle_scores(cfg, x, params, bern):
    """fp64 [B,D]: mean over the draws of the rate (Poisson column) / sigmoid(logit) (Bernoulli)."""
    rate = O.log_likelihood_components(cfg, T(x), T(params["s"]), T(params["u"]), T(params["v"]),
                                       T(params["w"]))["rate"]
    if rate.dim() == 2:
        rate = rate.unsqueeze(0)
    m = torch.where(T(bern), torch.sigmoid(rate), rate)
    return m.mean(0).numpy()


@functools.lru_cache(maxsize=None)
def _problem(lik, B, D, K, S, seed=None, density=0.3):
    """The problem of a case and its oracle scores, computed once and shared (read-only)."""
    cfg, x, params, mask = _dense_problem(lik, B, D, K, S, 9100 + B + K if seed is None else seed,
                                          density=density)
    if lik in BERN_DAMP:
        params["u"] = params["u"] * BERN_DAMP[lik]
        params["w"] = params["w"] * BERN_DAMP[lik]
    score = _oracle_scores(cfg, x, params, _bern_cols(lik, mask, D))
    return cfg, x, params, mask, score


# ---- predict's cases, which group_means and set_scores are held against too ------------------------------------
# (B, D, K, S): the three shapes of test_gpu_topk.SHAPES -- ragged 64 x 64 blocks and 32 x 32 tiles, K padded
# 3 -> 4, K = 16, K = 33 -> 64 (two K chunks)
SHAPES = [(70, 45, 3, 2), (131, 197, 16, 7), (5, 333, 33, 3)]
PNZ_DAMP = {70: 2.0 ** -8, 131: 2.0 ** -14, 5: 2.0 ** -16}      # by B of SHAPES
OUTS = ("mean", "sd", "p_nonzero")


def _bar(v, smax):
    return 1e-5 * np.abs(v) + 1e-5 * smax


def _lists(D):
    """The column lists of a shape: all columns, one column, a seeded permutation, and min(D, 65) columns that
    start D-1, 0, 0: a duplicate, a 64-block edge crossed, both ends touched."""
    rng = np.random.default_rng(77 + D)
    n = min(D, 65)
    mixed = np.concatenate([[D - 1, 0, 0], rng.integers(0, D, size=n - 3)]).astype(np.int64)
    return {"all": None, "one": np.array([D - 1]), "perm": rng.permutation(D), "dup": mixed}


def _per_draw(cfg, x, params, bern):
    """fp64 [S,B,D]: the oracle's rate and m_s of every draw."""
    rate = O.log_likelihood_components(cfg, T(x), T(params["s"]), T(params["u"]), T(params["v"]),
                                       T(params["w"]))["rate"]
    if rate.dim() == 2:
        rate = rate.unsqueeze(0)
    m = torch.where(T(bern), torch.sigmoid(rate), rate)
    return rate.numpy(), m.numpy()


@functools.lru_cache(maxsize=None)
def _case(lik, B, D, K, S):
    """The problem of test_gpu_topk at this shape, its per-draw oracle values, the model and the full
    prediction with all outputs; computed once and shared (read-only)."""
    cfg, x, params, mask, score = _problem(lik, B, D, K, S)
    bern = _bern_cols(lik, mask, D)
    rate, ms = _per_draw(cfg, x, params, bern)
    np.testing.assert_allclose(ms.mean(0), score, rtol=1e-12, atol=0)
    m = _dense_model(lik, cfg, mask, 32)
    full = m.predict({"counts": x}, draws=params, sd=True, p_nonzero=True)
    assert set(full) == set(OUTS)
    for n in OUTS:
        assert full[n].dtype == torch.float32 and tuple(full[n].shape) == (B, D) and full[n].is_cuda, n
    return dict(cfg=cfg, x=x, params=params, mask=mask, bern=bern, score=score, rate=rate, ms=ms, m=m, full=full)


@functools.lru_cache(maxsize=None)
def _damped_case(lik, B, D, K, S):
    """poisson / mixed with u and w scaled by PNZ_DAMP[B]: rates small enough for P(x > 0) to say something."""
    cfg, x, params, mask = _dense_problem(lik, B, D, K, S, 9100 + B + K)
    params = dict(params)
    params["u"] = params["u"] * PNZ_DAMP[B]
    params["w"] = params["w"] * PNZ_DAMP[B]
    bern = _bern_cols(lik, mask, D)
    rate, ms = _per_draw(cfg, x, params, bern)
    return dict(cfg=cfg, x=x, params=params, mask=mask, bern=bern, rate=rate, ms=ms)


@functools.lru_cache(maxsize=None)
def _points(nq, nr, K, self_case, shift=0.0):
    """The seeded query and reference rows of the knn tests (fp32; self_case: one set)."""
    rng = np.random.default_rng(7300 + nq + K)
    R = rng.standard_normal((nr, K))
    Q = R if self_case else rng.standard_normal((nq, K))
    R32 = (R + shift).astype(np.float32)
    Q32 = R32 if self_case else (Q + shift).astype(np.float32)
    return Q32, R32


def abi_call(entry, good):
    """-> call(**overrides): the entry point through a binding of its own with plain pointers, so that
    NULL can stand for `params` and `counts` too, with the arguments of ``good`` (keys h, ct, S, pin, eta,
    the entry's own of ENTRIES, ptr, nbytes, stream) unless overridden."""
    from spmf_amd import _lib
    own = ENTRIES[entry].own
    fn = getattr(C.CDLL(_lib.LIB_PATH), ENTRIES[entry].call)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [t for _, t in own] + [
        C.c_void_p, C.c_size_t, C.c_void_p]

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], C.byref(a["ct"]) if a["ct"] is not None else None, a["S"], a["pin"], a["eta"],
                  *[a[n] for n, _ in own], a["ptr"], a["nbytes"], a["stream"])
    return call


def scratch_need(lib, entry, h, rows, s, own):
    """The entry's scratch size for ``rows`` rows and ``s`` draws, with its extra size arguments out of ``own``."""
    e = ENTRIES[entry]
    return int(getattr(lib, e.size)(h, rows, s, *[own[n] for n in e.size_args]))


def host_good_call(lib, entry):
    """A valid-looking call of ``entry`` that needs no device: a context of spmf_ctx_create (K = 3, D = 45), a
    hand-filled descriptor of 70 empty rows and dummy aligned addresses -- nothing in it may be dereferenced, so
    only refused and empty calls may be made with it.  -> (good, need, pin_without_u, mixed_ctx_without_types,
    cleanup); ``cleanup()`` destroys the two contexts."""
    from spmf_amd import _lib
    from spmf_amd._lib import VAR_ORDER
    h, raw = host_ctx(lib, K), host_ctx(lib, K, _lib.FLAG_MIXED)

    def cleanup():
        lib.spmf_ctx_destroy(h)
        lib.spmf_ctx_destroy(raw)
    try:
        cs = _lib.CountsStruct()
        cs.struct_size = C.sizeof(_lib.CountsStruct)
        cs.n_cols, cs.n_rows, cs.nnz, cs.row_ptr = D, B, 0, 0x10000
        slots = {n: 0x100000 * (i + 1) for i, n in enumerate(VAR_ORDER) if n in ("s", "u", "v", "w")}
        own = {"waic": dict(sums=0x2000000, rows=None),
               "topk": dict(k=5, flags=1, cols=0x2000000, scores=0x3000000),
               "cells": dict(n=4, row=0x2000000, col=0x3000000, val=0x4000000, mean=0x5000000, lppd=0x6000000),
               "rank": dict(n=4, row=0x2000000, col=0x3000000, flags=1, rank=0x4000000, cand=0x5000000,
                            score=0x6000000),
               "predict": dict(n=4, cols=0x2000000, mean=0x3000000, sd=0x4000000, pnz=0x5000000),
               "groups": dict(labels=0x6000000, G=4, n=4, cols=0x2000000, sum=0x3000000, nz=0x5000000),
               "embed": dict(mean=0x2000000, sd=0x3000000),
               "waic_cols": dict(sums=0x2000000, rows=None, colsum=0x3000000),
               "toprows": dict(n=4, cols=0x2000000, k=5, flags=1, rows=0x3000000, scores=0x4000000),
               "sets": dict(n_sets=2, set_ptr=(C.c_int64 * 3)(0, 4, 9), cols=0x2000000, weights=0x3000000, ld=2,
                            mean=0x4000000, sd=0x5000000)}[entry]
        need = scratch_need(lib, entry, h, B, S, own)
        assert need > 0 and need % 256 == 0
        good = dict(h=h, ct=cs, S=S, pin=_lib.PtrArray(*[slots.get(n) for n in VAR_ORDER]), eta=0x7000000,
                    ptr=0x8000000, nbytes=need, stream=None, **own)
        no_u = _lib.PtrArray(*[slots.get(n) if n != "u" else None for n in VAR_ORDER])
    except BaseException:
        cleanup()
        raise
    return good, need, no_u, raw, cleanup


def gpu_good_call(entry, m, x, params, k=5, sets=None):
    """The arguments of a valid call of ``entry`` on model ``m`` for the batch ``x`` and the draws ``params``,
    with an exactly sized scratch of zeros and outputs filled with the sentinel -7: -> (good, need, outputs,
    scratch, pin_without_u).  topk and toprows: ``k``.  cells and rank: every cell once, row by row (cells: with
    values 0, 1, 2, 0, ...).  predict, groups and toprows: the columns PANEL_COLS; groups: G = 3 and the labels
    -1, 0, 1, 2, -1, ... .  sets: ``sets`` = (lists, weights, ld), else PANEL_SETS with PANEL_WEIGHTS and
    ld = n_sets.  ``outputs`` holds the device tensors by argument name; ``good["keep"]`` keeps the inputs alive
    (the lists of an entry that has some come last, as a dict by argument name)."""
    from spmf_amd import _lib
    from spmf_amd._lib import VAR_ORDER
    lib, h = _lib.load(), m._handle()
    _, cs = m._batch({"counts": x})
    n_draws, P = m._pack_params(params, names=("s", "u", "v", "w"))
    pin = _lib.PtrArray(*[P[n].data_ptr() if n in P else None for n in VAR_ORDER])
    no_u = _lib.PtrArray(*[P[n].data_ptr() if n in P and n != "u" else None for n in VAR_ORDER])
    eta = m._eta_device()
    rows, width = x.shape

    def full(shape, dtype):
        return torch.full(shape, -7, dtype=dtype, device="cuda")

    def ptrs(*dicts):
        return {n: t.data_ptr() for d in dicts for n, t in d.items()}
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    lists = {}
    if entry in ("waic", "waic_cols"):
        out = {"sums": full((6,), f64), "rows": full((rows, 2), f64)}
        if entry == "waic_cols":
            out["colsum"] = full((width, 5), f64)
        own = ptrs(out)
    elif entry == "topk":
        out = {"cols": full((rows, k), i32), "scores": full((rows, k), f32)}
        own = dict(k=k, flags=1, **ptrs(out))
    elif entry in ("cells", "rank"):
        N = rows * width
        cell = torch.arange(N, device="cuda")
        lists = {"row": (cell // width).to(i32), "col": (cell % width).to(i32)}
        if entry == "cells":
            lists["val"] = (cell % 3).to(f32)
            out = {"mean": full((N,), f32), "lppd": full((N,), f32)}
            own = dict(n=N, **ptrs(lists, out))
        else:
            out = {"rank": full((N,), i32), "cand": full((N,), i32), "score": full((N,), f32)}
            own = dict(n=N, flags=1, **ptrs(lists, out))
    elif entry == "predict":
        lists = {"cols": torch.tensor(PANEL_COLS, dtype=i32, device="cuda")}
        out = {n: full((rows, len(PANEL_COLS)), f32) for n in ("mean", "sd", "pnz")}
        own = dict(n=len(PANEL_COLS), **ptrs(lists, out))
    elif entry == "groups":
        lists = {"labels": (torch.arange(rows, device="cuda") % 4 - 1).to(i32),
                 "cols": torch.tensor(PANEL_COLS, dtype=i32, device="cuda")}
        out = {n: full((n_draws, 3, len(PANEL_COLS)), f64) for n in ("sum", "nz")}
        own = dict(G=3, n=len(PANEL_COLS), **ptrs(lists, out))
    elif entry == "toprows":
        lists = {"cols": torch.tensor(PANEL_COLS, dtype=i32, device="cuda")}
        out = {"rows": full((len(PANEL_COLS), k), i32), "scores": full((len(PANEL_COLS), k), f32)}
        own = dict(n=len(PANEL_COLS), k=k, flags=1, **ptrs(lists, out))
    elif entry == "sets":
        members, weights, ld = sets or (PANEL_SETS, PANEL_WEIGHTS, len(PANEL_SETS))
        set_ptr = np.concatenate([[0], np.cumsum([len(s) for s in members])]).astype(np.int64)
        lists = {"cols": torch.tensor([j for s in members for j in s], dtype=i32, device="cuda"),
                 "weights": torch.tensor([w for s in weights for w in s], dtype=f32, device="cuda")}
        out = {n: full((rows, ld), f64) for n in ("mean", "sd")}
        own = dict(n_sets=len(members), set_ptr=set_ptr.ctypes.data, ld=ld, **ptrs(lists, out))
        lists["set_ptr"] = set_ptr
    else:
        out = {n: full((rows, m.latent_dim), f32) for n in ("mean", "sd")}
        own = ptrs(out)
    need = scratch_need(lib, entry, h, int(cs.n_rows), n_draws, own)
    assert need > 0 and need % 256 == 0
    scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    good = dict(h=h, ct=cs, S=n_draws, pin=pin, eta=eta.data_ptr(),
                ptr=scratch.data_ptr() + (-scratch.data_ptr()) % 256, nbytes=need,
                stream=torch.cuda.current_stream().cuda_stream, keep=[P, eta, lists], **own)
    return good, need, out, scratch, no_u


def assert_shared_errors(lib, entry, good, need, pin_without_u, mixed_ctx_without_types, after=lambda: None):
    """The error contract of the draw stage for one entry point; every call here returns before a launch, and
    ``after`` is run behind each (the GPU files check their sentinels there).  ``good``: arguments of a valid
    call whose scratch holds exactly ``need`` bytes.  Every refusal's message, read from the context the call was
    made on, starts with the entry's name; the descriptor's own two are check_counts', worded for every call
    alike.  -> the raw call."""
    call = abi_call(entry, good)
    own_prefix = ENTRIES[entry].call[len("spmf_"):] + ": "

    def refused(code, why=None, prefix=own_prefix, **kw):
        assert call(**kw) == code, why or kw
        msg = lib.spmf_last_error(kw.get("h", good["h"])).decode()
        assert msg.startswith(prefix), (why or kw, msg)
        after()
        return msg
    refused(-1, "S below the minimum", S=ENTRIES[entry].min_S - 1)
    refused(-1, S=65536)
    for name in ("pin", "eta", "ptr"):
        refused(-1, **{name: None})
    refused(-1, prefix="counts is null", ct=None)
    refused(-1, "slot u missing", pin=pin_without_u)
    assert "aligned" in refused(-1, "scratch off by 4 bytes", ptr=good["ptr"] + 4)
    bad = type(good["ct"]).from_buffer_copy(good["ct"])
    bad.struct_size += 8
    refused(-1, "struct_size + 8", prefix="counts.struct_size is ", ct=bad)
    assert "column_types" in refused(-1, h=mixed_ctx_without_types)
    assert str(need) in refused(-3, nbytes=need - 256)
    return call


# ---- spmf_knn, spmf_kmeans_step and spmf_embed_rows: their own argument errors, with and without a device ----------
KNN_ARGS = (("q", C.c_void_p), ("nq", C.c_int64), ("r", C.c_void_p), ("nr", C.c_int64), ("row_len", C.c_int),
            ("k", C.c_int), ("flags", C.c_uint), ("self_offset", C.c_int64), ("idx", C.c_void_p),
            ("dist", C.c_void_p), ("ptr", C.c_void_p), ("nbytes", C.c_size_t), ("stream", C.c_void_p))


def knn_raw_call(good):
    """-> call(**overrides): spmf_knn through a binding of its own with the arguments of ``good``."""
    from spmf_amd import _lib
    fn = C.CDLL(_lib.LIB_PATH).spmf_knn
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [t for _, t in KNN_ARGS]

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], *[a[n] for n, _ in KNN_ARGS])
    return call


def assert_knn_errors(lib, good, need, after=lambda: None):
    """The error contract of spmf_knn; every call here returns before a launch or a memset, and ``after`` is
    run behind each (the GPU file checks its sentinels there)."""
    call, h = knn_raw_call(good), good["h"]

    def refused(code, **kw):
        assert call(**kw) == code, kw
        assert lib.spmf_last_error(h).decode().startswith("knn: "), lib.spmf_last_error(h).decode()
        after()
    for k in (0, 65, -3):
        refused(-1, k=k)
    for row_len in (0, 257, -1):
        refused(-1, row_len=row_len)
    refused(-1, flags=2)
    refused(-1, flags=3)
    assert "flag" in lib.spmf_last_error(h).decode()
    refused(-1, nr=2 ** 31)
    assert "int32" in lib.spmf_last_error(h).decode()
    refused(-1, nq=-1)
    refused(-1, nr=-1)
    refused(-1, self_offset=-2)
    for name in ("q", "r", "idx", "dist", "ptr"):
        refused(-1, **{name: None})
    refused(-1, ptr=good["ptr"] + 4)
    assert "aligned" in lib.spmf_last_error(h).decode()
    refused(-3, nbytes=need - 256)
    assert str(need) in lib.spmf_last_error(h).decode()
    refused(-3, nq=0, nbytes=0)             # errors come before the empty return
    assert call(h=None) == -1


KMEANS_ARGS = (("x", C.c_void_p), ("n", C.c_int64), ("row_len", C.c_int), ("cent", C.c_void_p), ("G", C.c_int32),
               ("prev", C.c_void_p), ("labels", C.c_void_p), ("dist", C.c_void_p), ("sums", C.c_void_p),
               ("counts", C.c_void_p), ("stats", C.c_void_p), ("ptr", C.c_void_p), ("nbytes", C.c_size_t),
               ("stream", C.c_void_p))


def kmeans_raw_call(good):
    """-> call(**overrides): spmf_kmeans_step through a binding of its own with the arguments of ``good``."""
    from spmf_amd import _lib
    fn = C.CDLL(_lib.LIB_PATH).spmf_kmeans_step
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [t for _, t in KMEANS_ARGS]

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], *[a[n] for n, _ in KMEANS_ARGS])
    return call


def assert_kmeans_errors(lib, good, need, after=lambda: None):
    """The error contract of spmf_kmeans_step; every call here returns before a launch or a memset, and ``after``
    is run behind each (the GPU file checks its sentinels there)."""
    call, h = kmeans_raw_call(good), good["h"]

    def refused(code, **kw):
        assert call(**kw) == code, kw
        msg = lib.spmf_last_error(h).decode()
        assert msg.startswith("kmeans_step: "), msg
        after()
        return msg
    for g in (0, -1, 65537):
        assert "n_clusters" in refused(-1, G=g)
    for w in (0, 257, -1):
        assert "row_len" in refused(-1, row_len=w)
    for rows in (-1, 2 ** 31 - 63, 2 ** 40):
        assert "n_rows" in refused(-1, n=rows)
    assert "prev_labels" in refused(-1, prev=good["labels"])
    for name in ("x", "cent", "labels", "sums", "counts", "stats", "ptr"):
        assert "null" in refused(-1, **{name: None})
    for name in ("sums", "counts", "stats", "ptr"):
        refused(-1, n=0, **{name: None})
    assert "aligned" in refused(-1, ptr=good["ptr"] + 4)
    assert str(need) in refused(-3, nbytes=need - 256)
    refused(-3, n=0, nbytes=0)               # errors come before the empty return
    assert call(h=None) == -1


def assert_embed_own_errors(lib, call, good, after=lambda: None):
    """The argument errors of spmf_embed_rows beyond the draw stage's; ``call`` is the raw call of ``good``
    (abi_call), every call returns before a launch and ``after`` is run behind each."""
    assert call(mean=None) == -1
    after()
    one = good["sd"] if good["sd"] is not None else 0x6000000
    assert call(S=1, sd=one) == -1
    assert "sd_out" in lib.spmf_last_error(good["h"]).decode()
    after()
