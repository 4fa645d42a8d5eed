"""Harness for the finish kernels (spmf_amd/csrc/finish_body.h, finish.hip, the prior half inside prep.hip's
begin_kernel) -- TEST INFRASTRUCTURE ONLY.

Drives the C ABI directly on a model's context, in the style of tests/_sur_table.py (whose Guarded it reuses):

  1. a data pass on a tiny batch binds the workspace (and lets the prep launch write its column sums from
     the parameters under test);
  2. optionally the packed accumulators are overwritten through spmf_acc_ptr / spmf_acc_len, the public point
     the row-shard all-reduce uses (padded columns k >= K stay zero, as the layout documents);
  3. the finish runs on parameter and gradient buffers of the harness.

Three routes over the same accumulators: "a" spmf_finish alone, "b" spmf_prior_async then spmf_finish, "c"
spmf_step_begin, injection, spmf_step_end.  Every gradient buffer, parts[S][14] and n_nonfinite[2S] is a Guarded
allocation pre-filled with NaN (a slot nobody wrote is seen); counts are checked on the host before any call and
the margins after every call.

The numpy half (regime draws, accumulator packing, references and yardsticks) needs no GPU: the host suite
(tests/test_finish_reference_host.py) pins it.
"""
import ctypes as C
import math

import numpy as np
import torch

from oracle import sparse_exact as SE
from oracle import spmf_oracle as O

VAR_ORDER = O.VAR_ORDER
FP32_RANGE = 1e37          # a gradient entry whose fp64 yardstick reaches this is outside the finish's domain
C0 = SE.HALF_LOG_2_OVER_PI

# ---- 3.1: the magnitude regimes (log-uniform per entry; "benign" is oracle.random_params) ---------------------
REGIMES = {
    "shrunk": {"uvw": (1e-8, 1.0), "eta": (1e-3, 1e2), "u_tau": (1e-6, 1.0), "s_tau": (1e-3, 1e1),
               "s": (1e-4, 1e1), "a": (1e-3, 1e4)},
    "wide": {"uvw": (1e-6, 1e3), "eta": (1e-6, 1e3), "u_tau": (1e-8, 1.0), "s_tau": (1e-6, 1e3),
             "s": (1e-6, 1e3), "a": (1e-6, 1e3)},
}
SEEDS = {"benign": 11, "shrunk": 12, "wide": 13}      # the fixed draws of the GPU test and of the host count
# (regime, K, decay) at D = 33, S = 2.  decay = 0.5 at K = 16 (decay^15 = 3e-5) runs on the benign and the shrunk
# regime: on the wide one it moves 2.5 % of the u chain past 1e37, above the 2 % cap of the input condition.
REGIME_CASES = [(r, 5, d) for r in ("benign", "shrunk", "wide") for d in (0.99, 1.0)] + \
               [("benign", 16, 0.5), ("shrunk", 16, 0.5)]
_RANGE_OF = {"u": "uvw", "v": "uvw", "w": "uvw", "u_eta": "eta", "s_eta": "eta", "u_tau": "u_tau",
             "s_tau": "s_tau", "s": "s", "u_eta_a": "a", "u_tau_a": "a", "s_eta_a": "a", "s_tau_a": "a"}


def f32(a):
    """Round to values an fp32 holds exactly (kept as fp64)."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def prior_scales(cfg, params, prior_weight=1.0):
    """The prior's entry-wise gradient yardstick (oracle.energy_grad_scales, data=False) as numpy arrays."""
    x = np.zeros((1, cfg.feature_dim))
    sc = O.energy_grad_scales(cfg, x, params, prior_weight=prior_weight, data=False)
    return {n: v.numpy() for n, v in sc.items()}


def draw_regime(cfg, S, regime, seed):
    """Twelve [S, *shape] fp32-exact arrays of one regime and the share of every variable's entries that was
    redrawn.

    Input condition of the issue: a gradient entry of any variable whose fp64 yardstick is >= 1e37 is outside
    what fp32 can return; every input entry that contributes to it is replaced by its benign draw.  For an
    element-wise chain (u, u_eta, u_eta_a at (d, k); s, s_eta, s_eta_a at (r, d)) the contributors are the
    chain's entries at that index.  d/d u_tau[k] and d/d s_tau[d] are SUMS (over d, over the two rows): their
    contributors are the summands that carry the sum, (q^2 + 1) / tau >= 1e37 / (number of summands) -- if
    every summand is below that the sum is below 1e37 -- and, when no summand does, u_tau / u_tau_a (s_tau /
    s_tau_a) themselves."""
    benign = O.random_params(cfg, S, seed, fp32_exact=True)
    if regime == "benign":
        return benign, {n: 0.0 for n in VAR_ORDER}
    rng = np.random.default_rng(seed + 7919)
    p = {}
    for n in VAR_ORDER:
        lo, hi = REGIMES[regime][_RANGE_OF[n]]
        p[n] = f32(10.0 ** rng.uniform(math.log10(lo), math.log10(hi), benign[n].shape))
    K, D = cfg.latent_dim, cfg.feature_dim
    dec = cfg.symmetry_breaking_decay ** np.arange(K)
    changed = {n: np.zeros(p[n].shape, dtype=bool) for n in VAR_ORDER}

    def redraw(names, mask):
        for n in names:
            m = np.broadcast_to(mask, p[n].shape)
            p[n] = np.where(m, benign[n], p[n])
            changed[n] |= m

    for _ in range(8):
        sc = prior_scales(cfg, p)
        bad = {n: sc[n] >= FP32_RANGE for n in VAR_ORDER}
        if not any(b.any() for b in bad.values()):
            break
        redraw(("u", "u_eta", "u_eta_a"), bad["u"] | bad["u_eta"] | bad["u_eta_a"])
        redraw(("s", "s_eta", "s_eta_a"), bad["s"] | bad["s_eta"] | bad["s_eta_a"])
        bk = bad["u_tau"] | bad["u_tau_a"]                               # [S,1,K]
        if bk.any():
            q = p["u"] / (p["u_eta"] * p["u_tau"] * dec)
            carry = ((q * q + 1.0) / p["u_tau"] >= FP32_RANGE / D) & bk
            redraw(("u", "u_eta", "u_eta_a"), carry)
            redraw(("u_tau", "u_tau_a"), bk & ~carry.any(1, keepdims=True))
        bd = bad["s_tau"] | bad["s_tau_a"]                               # [S,1,D]
        if bd.any():
            q = p["s"] / (p["s_eta"] * p["s_tau"])
            carry = ((q * q + 1.0) / p["s_tau"] >= FP32_RANGE / 2) & bd
            redraw(("s", "s_eta", "s_eta_a"), carry)
            redraw(("s_tau", "s_tau_a"), bd & ~carry.any(1, keepdims=True))
    else:
        raise AssertionError("the redraw did not bring every yardstick below 1e37")
    return p, {n: float(changed[n].mean()) for n in VAR_ORDER}


def draw_abs_horseshoe(cfg, S, seed):
    """3.3: v, w benign, u log-uniform in [1e-30, 1e6], s in [1e-6, 1e3]."""
    p = O.random_params(cfg, S, seed, fp32_exact=True)
    rng = np.random.default_rng(seed + 104729)
    p["u"] = f32(10.0 ** rng.uniform(-30, 6, p["u"].shape))
    p["s"] = f32(10.0 ** rng.uniform(-6, 3, p["s"].shape))
    return p


# ---- references ------------------------------------------------------------------------------------------------
def prior_reference(cfg, params):
    """-> (parts name -> [S], grads name -> [S,*shape], part yardsticks name -> [S]): oracle/sparse_exact.prior_term
    per draw (the default model) or fp64 autograd of the oracle's densities (AbsHorseshoe), and the sum of the
    absolute additive terms of every part (oracle.prior_log_prob_terms)."""
    S = params["u"].shape[0]
    pt = {k: torch.as_tensor(np.asarray(v, dtype=np.float64)) for k, v in params.items()}
    terms = O.prior_log_prob_terms(cfg, pt)
    yard = {n: sum(t.abs() * torch.ones_like(pt[n]) for t in ts).sum((-1, -2)).numpy() for n, ts in terms.items()}
    if cfg.horseshoe_plus and cfg.likelihood == "poisson":
        dec = cfg.symmetry_breaking_decay ** np.arange(cfg.latent_dim)
        outs = [SE.prior_term({k: v[s] for k, v in params.items()}, cfg.u_tau_scale, cfg.s_tau_scale, dec)
                for s in range(S)]
        parts = {n: np.array([o[0][n] for o in outs]) for n in outs[0][0]}
        grads = {n: np.stack([o[1][n] for o in outs]) for n in outs[0][1]}
        return parts, grads, yard
    pg = {k: v.clone().requires_grad_(True) for k, v in pt.items()}
    pp = O.prior_log_prob_parts(cfg, pg)
    g = torch.autograd.grad(sum(v.sum() for v in pp.values()), [pg[n] for n in pg], allow_unused=True)
    grads = {n: (gi if gi is not None else torch.zeros_like(pg[n])).numpy() for n, gi in zip(pg, g)}
    return {n: v.detach().numpy() for n, v in pp.items()}, grads, yard


def data_reference(acc, B_global, lgamma_sum, eta, p):
    """One draw: oracle/sparse_exact.finish_from_acc and, beside it, the yardsticks -- the sum of the absolute
    additive pieces of every gradient entry and of parts 'x', 'z'."""
    u, v, w, s = p["u"], p["v"], p["w"], p["s"]
    D, K = u.shape
    KP = SE.padded_k(K)
    ref = SE.finish_from_acc(acc, B_global, lgamma_sum, eta, u, v, w, s)
    a = acc.astype(np.float64)
    gA = a[:D * KP].reshape(D, KP)[:, :K]
    gV = a[D * KP:2 * D * KP].reshape(D, KP)[:, :K]
    gphi = a[2 * D * KP:2 * D * KP + D]
    tail = a[2 * D * KP + D:].reshape(-1, 2).sum(1)
    llx, zsq, zsum = tail[0], tail[1], tail[SE.TAIL_HEAD:SE.TAIL_HEAD + K]
    eta = np.broadcast_to(np.asarray(eta, dtype=np.float64).reshape(-1), (D,))
    T = s[0] + s[1]
    w1, w2 = s[0] / T, s[1] / T
    wv = w.reshape(D)
    sc = {"u": np.abs(w1[:, None] * gA / eta[:, None]),
          "v": ((np.abs(gV) + np.abs(zsum)[None, :]) * eta[:, None]).T,
          "w": (eta * w2 * (np.abs(gphi) + B_global))[None, :]}
    pieces = np.abs(u * gA / eta[:, None]).sum(1) + eta * np.abs(wv) * (np.abs(gphi) + B_global)
    sc["s"] = np.stack([pieces * s[1] / T ** 2, pieces * s[0] / T ** 2])
    veta = (v * eta[None, :]).sum(1)
    yard = {"x": abs(llx) + abs(lgamma_sum) + np.abs(zsum * veta).sum() + B_global * np.abs(eta * w2 * wv).sum(),
            "z": B_global * K * abs(C0) + 0.5 * abs(zsq)}
    return ref, sc, yard


# ---- packed accumulators -----------------------------------------------------------------------------------------
def pack_acc(gA, gV, gphi, scalars, zsum):
    """One draw's accumulators in the layout of include/spmf_hip.h (no column split), fp32:
    [gA'(D*KP) | gV'(D*KP) | gphi(D) | tail]; scalars: the six fp64 head values of the tail."""
    D, K = gA.shape
    KP = SE.padded_k(K)
    A = np.zeros((D, KP), dtype=np.float32)
    V = np.zeros((D, KP), dtype=np.float32)
    A[:, :K], V[:, :K] = gA, gV
    sc = np.zeros(SE.TAIL_HEAD + KP)
    sc[:SE.TAIL_HEAD] = scalars
    sc[SE.TAIL_HEAD:SE.TAIL_HEAD + K] = zsum
    hi = sc.astype(np.float32)
    lo = (sc - hi.astype(np.float64)).astype(np.float32)
    return np.concatenate([A.reshape(-1), V.reshape(-1), np.asarray(gphi, dtype=np.float32),
                           np.stack([hi, lo], 1).reshape(-1)]).astype(np.float32)


def split_layout(acc, D, K, Dh):
    """The same accumulators laid out per spmf_acc_split: [cols < Dh: gA'|gV'|gphi][cols >= Dh: ...][tail]."""
    KP = SE.padded_k(K)
    A = acc[:D * KP].reshape(D, KP)
    V = acc[D * KP:2 * D * KP].reshape(D, KP)
    ph = acc[2 * D * KP:2 * D * KP + D]
    out = [A[:Dh].reshape(-1), V[:Dh].reshape(-1), ph[:Dh], A[Dh:].reshape(-1), V[Dh:].reshape(-1), ph[Dh:],
           acc[2 * D * KP + D:]]
    return np.concatenate(out).astype(np.float32)


def random_acc(D, K, B_global, rng, big=1e9):
    """3.4: gA', gV' ~ N(0, 1e3^2) with exact zeros and one empty column; gphi = B (1 +- 1e-3); llx and
    sum z^2 around `big` with a fraction an fp32 cannot hold; zsum of mixed sign; counts 3 and 7."""
    gA = rng.normal(0, 1e3, (D, K))
    gV = rng.normal(0, 1e3, (D, K))
    gA[rng.random((D, K)) < 0.1] = 0.0
    gV[rng.random((D, K)) < 0.1] = 0.0
    gphi = B_global * (1.0 + 1e-3 * rng.uniform(-1, 1, D))
    e = int(rng.integers(D))
    gA[e], gV[e], gphi[e] = 0.0, 0.0, 0.0                # a column without a stored entry
    scal = [-big * rng.uniform(0.5, 2.0) - 0.123456789, big * rng.uniform(0.5, 2.0) + 0.987654321, 3.0, 0.0, 7.0, 0.0]
    zsum = rng.normal(0, 50.0, K)
    return pack_acc(f32(gA), f32(gV), f32(gphi), scal, zsum)


# ---- the device side ---------------------------------------------------------------------------------------------
class FinishRun:
    """One model context, S draws of parameters, a tiny batch.  run(route, ...) -> dict(parts [S,14], grads
    name -> [S,*shape], nnf [2S] or None)."""

    def __init__(self, model, params, x):
        from spmf_amd import _lib
        from _sur_table import Guarded
        self._lib, self.G = _lib, Guarded
        self.m, self.lib, self.h = model, _lib.load(), model._handle()
        self.dev = model.device
        self.D, self.K = int(model.feature_dim), int(model.latent_dim)
        self.names = tuple(model.var_order)
        self.shapes = O.var_shapes(self.D, self.K)
        self.S = int(np.asarray(params["u"]).shape[0])
        self.P = {}
        for n in self.names:
            a = np.asarray(params[n], dtype=np.float64)
            if a.shape != (self.S,) + self.shapes[n]:
                raise ValueError(f"{n}: shape {a.shape}")
            if not (a.astype(np.float32).astype(np.float64) == a).all():
                raise ValueError(f"{n}: not fp32-exact")
            self.P[n] = torch.as_tensor(a.astype(np.float32)).to(self.dev).contiguous()
        self.sc, self.cs = model._batch({"counts": np.asarray(x, dtype=np.float64)})
        model._ensure_workspace(self.cs.n_rows, self.S)
        self.eta = model._eta_device()
        self.KP = int(self.lib.spmf_padded_k(self.h))
        if self.KP != SE.padded_k(self.K):
            raise ValueError("padded K of the library and of the reference differ")
        self.n_acc = int(self.lib.spmf_acc_len(self.h, 1))
        if self.n_acc != 2 * self.D * self.KP + self.D + 2 * (SE.TAIL_HEAD + self.KP):
            raise ValueError("accumulator length of the library and of the reference differ")
        self.rows, self.lgamma = int(self.cs.n_rows), float(self.cs.lgamma_sum)

    def _outputs(self, with_nnf):
        nan = float("nan")
        g = {n: self.G(self.S * int(np.prod(self.shapes[n])), device=self.dev,
                       fill=np.full(self.S * int(np.prod(self.shapes[n])), nan)) for n in self.names}
        parts = self.G(self.S * 14, torch.float64, device=self.dev, fill=np.full(self.S * 14, nan))
        nnf = self.G(2 * self.S, torch.float64, device=self.dev, fill=np.full(2 * self.S, nan)) if with_nnf else None
        return g, parts, nnf

    def _check(self, g, parts, nnf):
        from _sur_table import _need
        for n in self.names:
            _need(self.P[n], torch.float32, self.S * int(np.prod(self.shapes[n])), f"param {n}")
            _need(g[n].t, torch.float32, self.S * int(np.prod(self.shapes[n])), f"grad {n}")
        _need(parts.t, torch.float64, self.S * 14, "parts")
        if nnf is not None:
            _need(nnf.t, torch.float64, 2 * self.S, "n_nonfinite")
        _need(self.eta, torch.float32, self.D, "eta")

    def _inject(self, acc):
        """acc: [S, n_acc] fp32 host array in the DEVICE layout (split_layout applied by the caller)."""
        from spmf_amd.poisson import _wrap_f32
        acc = np.ascontiguousarray(acc, dtype=np.float32)
        if acc.shape != (self.S, self.n_acc):
            raise ValueError(f"accumulators {acc.shape}, expected {(self.S, self.n_acc)}")
        ptr = self.lib.spmf_acc_ptr(self.h)
        if not ptr or int(self.lib.spmf_acc_len(self.h, self.S)) != acc.size:
            raise ValueError("no bound accumulators of this size")
        _wrap_f32(ptr, acc.size, self.dev, self.m._ws).copy_(torch.as_tensor(acc.reshape(-1)))

    def run(self, route, acc=None, prior_weight=1.0, rows=None, lgamma=None, with_nnf=True):
        lib, h, _lib = self.lib, self.h, self._lib
        g, parts, nnf = self._outputs(with_nnf)
        self._check(g, parts, nnf)
        pin = _lib.PtrArray(*[self.P[n].data_ptr() if n in self.P else None for n in VAR_ORDER])
        gout = _lib.PtrArray(*[g[n].ptr if n in g else None for n in VAR_ORDER])
        st = torch.cuda.current_stream(self.dev).cuda_stream
        rows = self.rows if rows is None else int(rows)
        lgamma = self.lgamma if lgamma is None else float(lgamma)
        nptr = nnf.ptr if nnf is not None else None
        eta = self.eta.data_ptr()
        if route in ("a", "b"):
            _lib.check(h, lib.spmf_data_pass(h, C.byref(self.cs), self.S, pin, eta, st), "spmf_data_pass")
            if acc is not None:
                self._inject(acc)
            if route == "b":
                _lib.check(h, lib.spmf_prior_async(h, self.S, float(prior_weight), pin, eta, parts.ptr, gout, st),
                           "spmf_prior_async")
            _lib.check(h, lib.spmf_finish(h, self.S, rows, lgamma, float(prior_weight), pin, eta, parts.ptr, gout,
                                          nptr, st), "spmf_finish")
        elif route == "c":
            _lib.check(h, lib.spmf_step_begin(h, C.byref(self.cs), self.S, float(prior_weight), pin, eta, parts.ptr,
                                              gout, nptr, st), "spmf_step_begin")
            if acc is not None:
                self._inject(acc)
            _lib.check(h, lib.spmf_step_end(h, rows, lgamma, st), "spmf_step_end")
        else:
            raise ValueError(route)
        torch.cuda.synchronize()
        bad = [n for n, b in list(g.items()) + [("parts", parts), ("nnf", nnf)] if b is not None and not b.intact()]
        assert not bad, f"route {route}: a canary margin was written ({bad})"
        return {"parts": parts.get().reshape(self.S, 14),
                "grads": {n: g[n].get().reshape((self.S,) + self.shapes[n]) for n in self.names},
                "bits": {n: g[n].bits().cpu().numpy() for n in self.names},
                "nnf": nnf.get() if nnf is not None else None}

    def read_acc(self):
        """The accumulators a data pass left (device layout), [S, n_acc]."""
        from spmf_amd.poisson import _wrap_f32
        n = self.S * self.n_acc
        return _wrap_f32(self.lib.spmf_acc_ptr(self.h), n, self.dev, self.m._ws).cpu().numpy().reshape(self.S, -1).copy()


def tiny_batch(D, rng, rows=5):
    """A handful of rows with a few counts each (binds the workspace; its own accumulators are replaced)."""
    x = ((rng.random((rows, D)) < 0.3) * (1 + rng.poisson(2.0, size=(rows, D)))).astype(np.float64)
    x[0, 0] = 1.0
    return x
