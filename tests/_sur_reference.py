"""fp64 restatement of the surrogate, optimiser and gate kernels -- TEST INFRASTRUCTURE ONLY.

Written from the header comment of spmf_amd/csrc/surrogate.hip and the formulas of
tests/_vi_reference.py, in plain numpy:

    kind 0  y = t0 + softplus(t1) eps,  theta = softplus(y)    (ident[i] != 0: theta = y)
    kind 1  same, theta = y
    kind 2  a = softplus(t0), b = softplus(t1), y = b / g, theta = softplus(y)
    log q = log q_y(y) - log sigmoid(y)     (no Jacobian where theta = y)
    loss  = -(1/(S B)) sum_s [sum gtheta theta - c log q_s]

Every function takes the fp32 inputs the kernels are handed, widened to fp64.  Beside each
result comes its yardstick in the convention of tests/_gradcheck.py: the sum of the absolute
values of what is added up (the additive terms of log q, or the derivative of each of them).
"""
import functools
import math

import numpy as np
import scipy.special as sps

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def softplus(x):
    return np.logaddexp(0.0, np.asarray(x, dtype=np.float64))


def softplus_inv(y):
    """raw value whose softplus is y (fp64)."""
    y = np.asarray(y, dtype=np.float64)
    return y + np.log(-np.expm1(-y))


def sigmoid(x):
    return sps.expit(np.asarray(x, dtype=np.float64))


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _soft_mask(kind, ident, n):
    """True where theta = softplus(y)."""
    if kind == 1:
        return np.zeros(n, dtype=bool)
    if kind == 0 and ident is not None:
        return np.asarray(ident).reshape(n) == 0
    return np.ones(n, dtype=bool)


def fwd_ref(kind, t0, t1, noise, ident=None):
    """One variable.  t0, t1: [n]; noise: [S, n] (eps, or g for kind 2).
    -> dict theta [S,n], l [S,n] (log q per element and draw), Y [S,n] (sum of |additive pieces of l|),
       th_scale [S,n] (yardstick of theta: sigma(y) (|t0| + |softplus(t1) eps|) for the normal kinds, 0 for kind 2)."""
    t0, t1, nz = _f64(t0), _f64(t1), _f64(noise)
    n = t0.size
    soft = _soft_mask(kind, ident, n)
    if kind == 2:
        a, b = softplus(t0), softplus(t1)
        y = b / nz
        pieces = [a * np.log(b) + 0 * y, -sps.gammaln(a) + 0 * y, -(a + 1.0) * np.log(y), -b / y]
        th_scale = np.zeros_like(y)
    else:
        sg = softplus(t1)
        y = t0 + sg * nz
        pieces = [-0.5 * nz * nz, -np.log(sg) + 0 * y, np.full_like(y, -HALF_LOG_2PI)]
        th_scale = np.where(soft, sigmoid(y), 1.0) * (np.abs(t0) + np.abs(sg * nz))
    with np.errstate(over="ignore"):
        pieces.append(np.where(soft, softplus(-y), 0.0))        # -log sigmoid(y)
        theta = np.where(soft, softplus(y), y)
    l = sum(pieces)
    Y = sum(np.abs(p) for p in pieces)
    return {"theta": theta, "l": l, "Y": Y, "y": y, "th_scale": th_scale}


def bwd_ref(kind, t0, t1, noise, gtheta, inv_sb, c, dgda=None, ident=None):
    """d loss / d(t0, t1) per element of one variable, and the per-element yardsticks (sum over draws of
    the absolute values of the additive pieces).  -> g0, g1, sc0, sc1  ([n] each)."""
    t0, t1, nz, ge = _f64(t0), _f64(t1), _f64(noise), _f64(gtheta)
    n = t0.size
    soft = _soft_mask(kind, ident, n)
    if kind == 2:
        a, b = softplus(t0), softplus(t1)
        dg = _f64(dgda)
        y = b / nz
        sig, oms = sigmoid(y), sigmoid(-y)
        dy_da = -(b / nz) / nz * dg
        dy_db = 1.0 / nz
        # d loss / dy: the energy term and the three terms of log q that hold y
        py = [-inv_sb * ge * sig, -inv_sb * c * (a + 1.0) / y, inv_sb * c * (b / y) / y, -inv_sb * c * oms]
        # explicit d/da, d/db of log q at fixed y
        pa = [inv_sb * c * np.log(b) + 0 * y, -inv_sb * c * sps.digamma(a) + 0 * y, -inv_sb * c * np.log(y)]
        pb = [inv_sb * c * a / b + 0 * y, -inv_sb * c / y]
        p0 = [p * dy_da for p in py] + pa
        p1 = [p * dy_db for p in py] + pb
        s0, s1 = sigmoid(t0), sigmoid(t1)
    else:
        sg = softplus(t1)
        y = t0 + sg * nz
        dth = np.where(soft, sigmoid(y), 1.0)
        oms = np.where(soft, sigmoid(-y), 0.0)
        py = [-inv_sb * ge * dth, -inv_sb * c * oms]
        p0 = py
        p1 = [p * nz for p in py] + [-inv_sb * c / sg + 0 * y]
        s0, s1 = 1.0, sigmoid(t1)
    g0 = s0 * sum(p.sum(0) for p in p0)
    g1 = s1 * sum(p.sum(0) for p in p1)
    sc0 = np.abs(s0) * sum(np.abs(p).sum(0) for p in p0)
    sc1 = np.abs(s1) * sum(np.abs(p).sum(0) for p in p1)
    return g0, g1, sc0, sc1


def adam_ref(p, m, v, g, t=None, clip=0.0, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7, b1t=None, b2t=None):
    """One tf.keras-style Adam step in fp64 from the given state.  t is 1-based; b1t / b2t give beta^t
    directly (the device path reads them from its state).
    -> dict p, m, v (new values) and the yardsticks ym = |b1 m| + |(1-b1) g|, yv = v_new,
       ystep = lr ym / c1 / (sqrt(v_new / c2) + eps)."""
    p, m, v, g = _f64(p), _f64(m), _f64(v), _f64(g)
    if clip > 0.0:
        g = np.clip(g, -clip, clip)
    c1 = 1.0 - (b1 ** t if b1t is None else b1t)
    c2 = 1.0 - (b2 ** t if b2t is None else b2t)
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    den = np.sqrt(v2 / c2) + eps
    p2 = p - lr * (m2 / c1) / den
    ym = np.abs(b1 * m) + np.abs((1.0 - b1) * g)
    return {"p": p2, "m": m2, "v": v2, "ym": ym, "yv": v2, "ystep": lr * ym / c1 / den, "den": den, "c1": c1,
            "c2": c2}


def gate_ref(state, parts, logq, nnf, S, c, rows):
    """The state update of vi_gate_kernel in fp64: -> new state (16 doubles).
    loss = -mean_s[x + z + c (prior - log q)] / rows; applied when the loss is finite and no stored cell's
    log-pmf was not."""
    st = np.array(state, dtype=np.float64, copy=True)
    parts = _f64(parts).reshape(S, 14)
    logq = _f64(logq).reshape(S)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = 0.0
        for s in range(S):
            prior = 0.0
            for i in range(12):
                prior += parts[s, i]
            acc += parts[s, 13] + parts[s, 12] + c * (prior - logq[s])
        loss = -(acc / S) / rows
    bad = float(np.sum(_f64(nnf)[:S])) if nnf is not None else 0.0
    sat = float(np.sum(_f64(nnf)[S:2 * S])) if nnf is not None else 0.0
    ok = bool(np.isfinite(loss)) and bad == 0.0
    st[14] += sat
    st[13] += 1.0
    st[8] = loss
    st[9] = 1.0 if ok else 0.0
    if ok:
        st[5] *= st[1]
        st[6] *= st[2]
        st[7] += 1.0
        st[10] += loss
        st[11] += 1.0
    else:
        st[12] += 1.0
    return st


@functools.lru_cache(maxsize=None)
def dgda_ref(a, g, digits=60):
    """d g / d a of g ~ Gamma(a, 1) at fixed probability: -(dP/da)(a, g) / p(g; a), P the regularised lower
    incomplete gamma function -- mpmath.diff of gammainc(..., regularized=True) at `digits` digits.  In the
    right tail the upper function Q = 1 - P is differentiated instead (dP/da = -dQ/da; P itself is 1 to all
    the digits there)."""
    import mpmath as mp
    with mp.workdps(digits):
        a_, g_ = mp.mpf(float(a)), mp.mpf(float(g))
        if g_ > a_ + 1:
            dP = -mp.diff(lambda t: mp.gammainc(t, g_, mp.inf, regularized=True), a_)
        else:
            dP = mp.diff(lambda t: mp.gammainc(t, 0, g_, regularized=True), a_)
        logp = (a_ - 1) * mp.log(g_) - g_ - mp.loggamma(a_)
        return float(-dP / mp.exp(logp))


def dgda_small(a, g):
    """Leading term of dgda for g << 1: P = g^a / Gamma(a+1) (1 + O(g)) gives
    dg/da = -(g/a) (log g - psi(a+1)) (1 + O(g)).  Used only to hand the chain-rule kernels a finite value
    of the right magnitude where mpmath would be slow; the kernels are handed dgda."""
    a, g = _f64(a), _f64(g)
    return -(g / a) * (np.log(g) - sps.digamma(a + 1.0))
