"""What the tests of the three streaming calls share (waic_streaming / spmf_waic_accumulate, top_k /
spmf_topk_rows, score_cells / spmf_score_cells): the cached problems of the GPU files and, for the
C-ABI, each entry point as a raw ctypes call with a dict of good arguments plus the error contract
of the draw stage they have in common (include/spmf_hip.h), asserted by one function on a device
(test_gpu_stream_abi.py) and without one (test_stream_host.py).
"""
import ctypes as C
import functools

import numpy as np
import torch

T = torch.as_tensor

BERN_DAMP = {"bernoulli": 1.0 / 64.0, "bernoulli_log": 1.0 / 8.0}

# entry point -> (the call, its scratch size, smallest S, the Python method, the arguments between `eta` and
# `scratch` in the header's order with their ctypes)
ENTRIES = {
    "waic": ("spmf_waic_accumulate", "spmf_waic_scratch_bytes", 2, "waic_streaming",
             (("sums", C.c_void_p), ("rows", C.c_void_p))),
    "topk": ("spmf_topk_rows", "spmf_topk_scratch_bytes", 1, "top_k",
             (("k", C.c_int), ("flags", C.c_uint), ("cols", C.c_void_p), ("scores", C.c_void_p))),
    "cells": ("spmf_score_cells", "spmf_cells_scratch_bytes", 1, "score_cells",
              (("n", C.c_int64), ("row", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p),
               ("mean", C.c_void_p), ("lppd", C.c_void_p))),
}


def _bern_cols(lik, mask, D):
    if lik.startswith("bernoulli"):
        return np.ones(D, dtype=bool)
    return np.asarray(mask, dtype=bool) if mask is not None else np.zeros(D, dtype=bool)


def _oracle_scores(cfg, x, params, bern):
    """fp64 [B,D]: mean over the draws of the rate (Poisson column) / sigmoid(logit) (Bernoulli)."""
    from oracle import spmf_oracle as O
    rate = O.log_likelihood_components(cfg, T(x), T(params["s"]), T(params["u"]), T(params["v"]),
                                       T(params["w"]))["rate"]
    if rate.dim() == 2:
        rate = rate.unsqueeze(0)
    m = torch.where(T(bern), torch.sigmoid(rate), rate)
    return m.mean(0).numpy()


@functools.lru_cache(maxsize=None)
def _problem(lik, B, D, K, S, seed=None, density=0.3):
    """The problem of a case and its oracle scores, computed once and shared (read-only)."""
    from test_gpu_dense import _dense_problem
    cfg, x, params, mask = _dense_problem(lik, B, D, K, S, 9100 + B + K if seed is None else seed,
                                          density=density)
    if lik in BERN_DAMP:
        params["u"] = params["u"] * BERN_DAMP[lik]
        params["w"] = params["w"] * BERN_DAMP[lik]
    score = _oracle_scores(cfg, x, params, _bern_cols(lik, mask, D))
    return cfg, x, params, mask, score


def abi_call(entry, good):
    """-> call(**overrides): the entry point through a binding of its own with plain pointers, so that
    NULL can stand for `params` and `counts` too, with the arguments of ``good`` (keys h, ct, S, pin, eta,
    the entry's own of ENTRIES, ptr, nbytes, stream) unless overridden."""
    from spmf_amd import _lib
    name, _, _, _, own = ENTRIES[entry]
    fn = getattr(C.CDLL(_lib.LIB_PATH), name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [t for _, t in own] + [
        C.c_void_p, C.c_size_t, C.c_void_p]

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], C.byref(a["ct"]) if a["ct"] is not None else None, a["S"], a["pin"], a["eta"],
                  *[a[n] for n, _ in own], a["ptr"], a["nbytes"], a["stream"])
    return call


def gpu_good_call(entry, m, x, params, k=5):
    """The arguments of a valid call of ``entry`` on model ``m`` for the batch ``x`` and the draws ``params``,
    with an exactly sized scratch of zeros and outputs filled with the sentinel -7: -> (good, need, outputs,
    scratch, pin_without_u).  The cell list is every cell once, row by row, with values 0, 1, 2, 0, ...
    ``outputs`` holds the device tensors by argument name; ``good["keep"]`` keeps the inputs alive."""
    from spmf_amd import _lib
    from spmf_amd._lib import VAR_ORDER
    lib, h = _lib.load(), m._handle()
    _, cs = m._batch({"counts": x})
    S, P = m._pack_params(params, names=("s", "u", "v", "w"))
    pin = _lib.PtrArray(*[P[n].data_ptr() if n in P else None for n in VAR_ORDER])
    no_u = _lib.PtrArray(*[P[n].data_ptr() if n in P and n != "u" else None for n in VAR_ORDER])
    eta = m._eta_device()
    B, D = x.shape
    need = int(getattr(lib, ENTRIES[entry][1])(h, int(cs.n_rows), S))
    assert need > 0 and need % 256 == 0
    scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")

    def full(shape, dtype):
        return torch.full(shape, -7, dtype=dtype, device="cuda")
    keep = [P, eta]
    if entry == "waic":
        out = {"sums": full((6,), torch.float64), "rows": full((B, 2), torch.float64)}
        own = {n: t.data_ptr() for n, t in out.items()}
    elif entry == "topk":
        out = {"cols": full((B, k), torch.int32), "scores": full((B, k), torch.float32)}
        own = dict(k=k, flags=1, **{n: t.data_ptr() for n, t in out.items()})
    else:
        N = B * D
        cell = torch.arange(N, device="cuda")
        lists = {"row": (cell // D).to(torch.int32), "col": (cell % D).to(torch.int32),
                 "val": (cell % 3).to(torch.float32)}
        keep.append(lists)
        out = {"mean": full((N,), torch.float32), "lppd": full((N,), torch.float32)}
        own = dict(n=N, **{n: t.data_ptr() for n, t in {**lists, **out}.items()})
    good = dict(h=h, ct=cs, S=S, pin=pin, eta=eta.data_ptr(), ptr=scratch.data_ptr() + (-scratch.data_ptr()) % 256,
                nbytes=need, stream=torch.cuda.current_stream().cuda_stream, keep=keep, **own)
    return good, need, out, scratch, no_u


def assert_shared_errors(lib, entry, good, need, pin_without_u, mixed_ctx_without_types):
    """The error contract of the draw stage for one entry point; every call here returns before a launch.
    ``good``: arguments of a valid call whose scratch holds exactly ``need`` bytes."""
    call = abi_call(entry, good)
    min_S = ENTRIES[entry][2]
    h = good["h"]
    assert call(S=min_S - 1) == -1, "S below the minimum"
    assert call(S=65536) == -1
    assert call(pin=None) == -1 and call(eta=None) == -1 and call(ptr=None) == -1 and call(ct=None) == -1
    assert call(pin=pin_without_u) == -1, "slot u missing"
    assert call(ptr=good["ptr"] + 4) == -1, "scratch off by 4 bytes"
    bad = type(good["ct"]).from_buffer_copy(good["ct"])
    bad.struct_size += 8
    assert call(ct=bad) == -1, "struct_size + 8"
    assert call(h=mixed_ctx_without_types) == -1
    assert "column_types" in lib.spmf_last_error(mixed_ctx_without_types).decode()
    assert call(nbytes=need - 256) == -3
    msg = lib.spmf_last_error(h).decode()
    assert str(need) in msg, msg
    return call
