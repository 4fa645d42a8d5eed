"""GPU: surrogate_fwd / surrogate_bwd / the fused chain rule + Adam of spmf_amd/csrc/surrogate.hip against the
fp64 reference of tests/_sur_reference.py, over tables whose sizes sit on the block edges of every kernel
(1024 elements per block forward, 256 backward and in the sampler's transform), with skipped slots, noise
as column slices of a wider buffer, all three kinds and the ident mask -- on a GRID of parameters (raw
scales -20..20, concentrations 1e-3..300, draws down to the sampler's clamp 1e-30), not a perturbation of
the initial point.  Every output buffer has canary margins (tests/_sur_table.py).

The two log-q reduction branches the per-context scratch (2^20 doubles) decides are at the end.

The largest error observed on an MI355X, as a share of its bound, is written beside each assertion.
"""
import functools

import numpy as np
import pytest
import torch

import _sur_reference as R
import _sur_table as T
from _gradcheck import assert_grads_entrywise, worst_entry

pytestmark = pytest.mark.gpu

FLT_MIN = 1.2e-38
U = 2.0 ** -23
RATIOS = {}


def _note(key, val):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(val))
    print(f"[ratio] {key}: {float(val):.3e} of its bound (largest so far {RATIOS[key]:.3e})")


@pytest.fixture(scope="module")
def handle():
    from spmf_amd import PoissonFactorization
    m = PoissonFactorization(latent_dim=2, feature_dim=8, u_tau_scale=0.1, device="cuda")
    yield m._handle()
    del m
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _grid(inv_sb, c):
    grid = T.gamma_grid(inv_sb, c)
    # 27 of the 360 combinations (7.5 %) leave the fp32 range at these inv_sb, c: counted on the CPU too
    # (tests/test_sur_reference_host.py)
    assert sum(not k[4] for k in grid) <= 0.10 * len(grid)
    return grid


# (n, kind, ident) per slot; ident: None, "mixed", "zeros", "ones" (kind 0 only).  The largest n first, in
# the middle, last: the blocks past a variable's end occur at every slot position.
LAYOUTS = {
    "one": [(4097, 0, "mixed")],
    "five_first": [(4097, 2, None), (257, 0, None), (1023, 1, None), (1, 2, None), (1025, 0, "ones")],
    "twelve_middle": [(1, 0, None), (255, 2, None), (256, 1, None), (257, 0, "zeros"), (1023, 2, None),
                      (2049, 0, "mixed"), (4097, 2, None), (1024, 0, None), (1025, 1, None), (1, 2, None),
                      (255, 0, "mixed"), (2049, 2, None)],
    "five_last": [(1, 1, None), (1024, 2, None), (255, 0, "mixed"), (2049, 1, None), (4097, 0, None)],
}
# (layout, S, noise_ld > n, B of inv_sb = 1 / (S B), c, slots skipped in the forward call)
CASES = [
    ("one", 1, False, 256, 1.0, ()),
    ("five_first", 2, True, 1000, 1e-3, (0, 2, 4)),
    ("twelve_middle", 7, True, 256, 1.0, (0, 6, 11)),
    ("five_last", 2, False, 256, 1e-3, (4,)),
]


def _ident(mode, n, rng):
    if mode is None:
        return None
    if mode == "mixed":
        return (rng.random(n) < 0.5).astype(np.uint8)
    return np.full(n, 1 if mode == "ones" else 0, dtype=np.uint8)


def _make(handle, layout, S, wide, inv_sb, c, seed):
    """-> (SurTable, per-slot host inputs) with grid parameters."""
    rng = np.random.default_rng(seed)
    slots, inputs, changed = [], [], 0
    for j, (n, kind, idm) in enumerate(LAYOUTS[layout]):
        ident = _ident(idm, n, rng)
        ge = T.gtheta_inputs(S, n, rng)
        if kind == 2:
            t0, t1, nz, dg = T.gamma_slot_inputs(n, S, _grid(inv_sb, c), rng)
        else:
            t0, t1, nz = T.normal_slot_inputs(n, S, rng)
            dg = None
        # An entry whose yardstick is below 1e-30 asks fp32 for a number it does not have (1e-5 of it is below
        # FLT_MIN): gtheta = 0 in every draw of an element with y >> 0 leaves only c (1 - sigmoid(y)) / (S B),
        # 1e-55 at y = 120.  Such elements get a non-zero gtheta.  (A yardstick of exactly 0 stays: the
        # identity elements with gtheta = 0, which must come out exactly 0.)
        # At most 1 % of a slot's elements (of 12 for the tiny slots) are changed.
        for _ in range(2):
            g0, g1, s0, s1 = R.bwd_ref(kind, t0, t1, nz, ge, inv_sb, c, dg, ident)
            tiny = ((s0 > 0) & (s0 < 1e-30)) | ((s1 > 0) & (s1 < 1e-30))
            if not tiny.any():
                break
            changed += int(tiny.sum())
            assert tiny.sum() <= 0.01 * max(n, 12), (layout, j, int(tiny.sum()), n)
            ge[:, tiny] = np.float32(1e-3)
        assert not tiny.any()
        ld = n + 3 + 16 * (j % 3) if wide and j % 2 == 0 else None
        slots.append(T.SurSlot(S, n, kind, t0, t1, nz, dg, ge, ident, ld))
        inputs.append(dict(n=n, kind=kind, t0=t0, t1=t1, noise=nz, dgda=dg, gtheta=ge, ident=ident,
                           g0=g0, g1=g1, s0=s0, s1=s1))
    print(f"[inputs] {layout}: gtheta made non-zero in {changed} of {sum(x['n'] for x in inputs)} elements")
    return T.SurTable(handle, S, slots), inputs


def _check_fwd(tab, inputs, S, skip, tag):
    logq, Y = np.zeros(S), np.zeros(S)
    lmin = np.inf
    for j, (sl, x) in enumerate(zip(tab.slots, inputs)):
        if j in skip:
            continue
        f = R.fwd_ref(x["kind"], x["t0"], x["t1"], x["noise"], x["ident"])
        logq += f["l"].sum(1)
        Y += f["Y"].sum(1)
        lmin = min(lmin, float(np.abs(f["l"]).min()))
        th = sl.theta.get().astype(np.float64).reshape(S, -1)
        assert np.isfinite(th).all(), (tag, j)
        bound = 1e-5 * np.maximum(np.abs(f["theta"]), f["th_scale"]) + FLT_MIN
        r = float((np.abs(th - f["theta"]) / bound).max())
        _note("theta", r)
        assert r <= 1.0, (tag, j, r)          # largest observed on an MI355X: 0.011 of the bound
    got = tab.logq.get()
    r = float((np.abs(got - logq) / (1e-5 * Y)).max())
    _note("logq", r)
    assert r <= 1.0, (tag, got, logq, Y)       # largest observed: 0.0044 of the bound
    return lmin, Y


@pytest.mark.parametrize("layout,S,wide,B,c,skip", CASES, ids=[k[0] for k in CASES])
def test_forward_backward_and_fused_step_on_the_grid(handle, layout, S, wide, B, c, skip):
    inv_sb = 1.0 / (S * B)
    tab, inputs = _make(handle, layout, S, wide, inv_sb, c, seed=len(layout) + S)
    tag = (layout, S)
    # forward with slots handed over as n = 0: their theta stays untouched, log q is the others' share
    if skip:
        tab.fwd(skip=skip)
        for j in skip:
            sl = tab.slots[j]
            assert bool((sl.theta.bits() == T._SENT[torch.float32][1]).all()), (tag, j, "a skipped slot was written")
        _check_fwd(tab, inputs, S, skip, tag + ("skip",))
    tab.logq.t.fill_(float("nan"))
    tab.fwd()
    _check_fwd(tab, inputs, S, (), tag)
    # chain rule
    tab.bwd(inv_sb, c)
    got, ref, sc = {}, {}, {}
    for j, (sl, x) in enumerate(zip(tab.slots, inputs)):
        g0, g1, s0, s1 = x["g0"], x["g1"], x["s0"], x["s1"]
        for nm, h, r, s in (("g0", sl.g0.get(), g0, s0), ("g1", sl.g1.get(), g1, s1)):
            assert np.isfinite(h).all(), (tag, j, nm, "non-finite gradient")
            k = f"slot{j}.kind{x['kind']}.{nm}"
            got[k], ref[k], sc[k] = h, r, s
            _note("grad entry-wise", worst_entry(h, r, s)[0] / 1e-5)
            _note("grad array norm", np.abs(h.astype(np.float64) - r).max() / (1e-5 * np.abs(r).max()))
    # largest observed: 0.19 of the entry-wise bound, 0.031 of the array-norm bound
    assert_grads_entrywise(got, ref, sc, tol=1e-5, tag=str(tag))
    # fused chain rule + Adam: gated off changes nothing, gated on equals adam_ref fed with bwd_ref
    rng = np.random.default_rng(99)
    tab.attach_adam(rng)
    lr, b1, b2, eps, t = 0.05, 0.9, 0.999, 1e-7, 3
    st = torch.zeros(16, dtype=torch.float64)
    st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7] = lr, b1, b2, eps, 0.0, b1 ** t, b2 ** t, t
    state = st.cuda()
    before = [[g.bits() for g in (sl.t0, sl.t1) + sl.m + sl.v] for sl in tab.slots]
    host = [[g.get().astype(np.float64) for g in (sl.t0, sl.t1) + sl.m + sl.v] for sl in tab.slots]
    tab.bwd_adam(inv_sb, c, state)                                  # state[9] = 0: skipped
    for sl, b in zip(tab.slots, before):
        for g, bits in zip((sl.t0, sl.t1) + sl.m + sl.v, b):
            assert torch.equal(g.bits(), bits), (tag, "a gated-off step changed a bit")
    state[9] = 1.0
    tab.bwd_adam(inv_sb, c, state)
    for j, (sl, x, h) in enumerate(zip(tab.slots, inputs, host)):
        for k, (gref, scale) in enumerate(((x["g0"], x["s0"]), (x["g1"], x["s1"]))):
            p0, m0, v0 = h[k], h[2 + k], h[4 + k]
            dg = 1e-5 * scale                       # what the gradient itself is allowed
            a = R.adam_ref(p0, m0, v0, gref, lr=lr, b1=b1, b2=b2, eps=eps, b1t=b1 ** t, b2t=b2 ** t)
            # Adam in fp32 holds |g| <= 1e18 (g^2 leaves the range above, in any fp32 Adam: see test_gpu_adam_edges)
            dom = np.abs(gref) + dg <= 1e18
            pn, mn, vn = (g.get().astype(np.float64) for g in ((sl.t0, sl.t1)[k], sl.m[k], sl.v[k]))
            assert np.isfinite(pn).all(), (tag, j, k)
            # the gradient's allowance carried through the update: m is linear in g; v lies between its
            # values at the ends of [g - dg, g + dg] (0 inside when the interval holds 0); the step is
            # m / D with D = sqrt(v / c2) + eps, |m/D - m_ref/D_ref| <= dm / D_lo + |m_ref| (1/D_lo - 1/D_hi)
            glo = np.where(np.abs(gref) > dg, np.abs(gref) - dg, 0.0)
            v_lo = b2 * v0 + (1 - b2) * glo ** 2
            v_hi = b2 * v0 + (1 - b2) * (np.abs(gref) + dg) ** 2
            bm = 4 * U * a["ym"] + (1 - b1) * dg
            bv = 4 * U * a["yv"] + (v_hi - v_lo)
            d_lo, d_hi = np.sqrt(v_lo / a["c2"]) + eps, np.sqrt(v_hi / a["c2"]) + eps
            bp = (U * np.abs(a["p"]) + 1e-5 * a["ystep"]
                  + lr / a["c1"] * ((1 - b1) * dg / d_lo + np.abs(a["m"]) * (1 / d_lo - 1 / d_hi)))
            for nm, hv, rv, bb in (("m", mn, a["m"], bm), ("v", vn, a["v"], bv), ("p", pn, a["p"], bp)):
                err = np.abs(hv - rv)[dom]
                r = float((err / np.where(bb[dom] > 0, bb[dom], 1.0))[(bb[dom] > 0) | (err > 0)].max(initial=0.0))
                _note(f"fused adam {nm}", r)
                assert (err <= bb[dom]).all(), (tag, j, k, nm, r)    # largest observed: m 0.29, v 0.26, p 0.49


BENIGN = {
    # block-edge tables for the log-q sum: every |l_i| is far above the sum's allowance, so a lost or a doubled
    # element cannot hide in it.  None: a skipped slot (first, middle, last).
    "five_first": ([(4097, 0), (1, 2), (257, 1), (1023, 0), (255, 2)], 1, False),
    "twelve_skips": ([None, (1025, 0), (1, 2), (256, 1), None, (2049, 0), (255, 2), (1024, 1), (257, 0), (1023, 0),
                      (1, 1), None], 7, True),
    "five_last": ([(1, 0), (255, 1), (1025, 0), (257, 2), (4097, 1)], 2, True),
}


@pytest.mark.parametrize("name", list(BENIGN))
def test_no_element_is_lost_or_doubled_in_log_q_at_the_block_edges(handle, name):
    """sigma = softplus(-20) = 2e-9 and |eps| <= 1 give l_i of about 19 with pieces of about 21 (kind 2:
    a = 3, b = 1e8, g in [1, 2]: l_i about -19), so with fewer than 6000 elements 1e-5 Y_s is below a tenth of
    the smallest |l_i| -- asserted below from the reference."""
    layout, S, wide = BENIGN[name]
    rng = np.random.default_rng(len(name))
    slots, inputs = [], []
    for j, spec in enumerate(layout):
        if spec is None:
            slots.append(None)
            inputs.append(None)
            continue
        n, kind = spec
        if kind == 2:
            t0, t1 = np.full(n, T.raw_of(3.0)), np.full(n, T.raw_of(1e8))
            nz = rng.uniform(1.0, 2.0, (S, n)).astype(np.float32)
            dg = np.ones((S, n), dtype=np.float32)
        else:
            t0 = rng.uniform(2.0, 6.0, n).astype(np.float32)
            t1 = np.full(n, -20.0, dtype=np.float32)
            nz, dg = rng.uniform(-1.0, 1.0, (S, n)).astype(np.float32), None
        ld = n + 5 + 8 * (j % 2) if wide and j % 2 else None
        slots.append(T.SurSlot(S, n, kind, t0, t1, nz, dg, None, None, ld))
        inputs.append(dict(n=n, kind=kind, t0=t0, t1=t1, noise=nz, ident=None))
    tab = T.SurTable(handle, S, slots)
    tab.logq.t.fill_(float("nan"))
    tab.fwd()
    skip = tuple(j for j, s in enumerate(slots) if s is None)
    lmin, Y = _check_fwd(tab, inputs, S, skip, (name,))
    assert lmin >= 10 * 1e-5 * Y.max(), (lmin, Y.max())           # a condition on the inputs, not on the kernel


# ---- the two reduction branches the scratch size decides -----------------------------------------

def _big_table(handle, S, seed):
    """One slot of n = 4096 among 12, the others n = 1, kind 0, benign parameters; noise is drawn on the
    device (90 M elements at S = 21846)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    slots = []
    for j in range(12):
        n = 4096 if j == 5 else 1
        rng = np.random.default_rng(j)
        sl = T.SurSlot(S, n, 0, rng.uniform(-2, 2, n).astype(np.float32), np.full(n, -7.6, dtype=np.float32),
                       None, None, None, None, None, big=True)
        sl.noise_w.t.copy_(torch.randn(S * n, generator=gen, device="cuda", dtype=torch.float32))
        slots.append(sl)
    return T.SurTable(handle, S, slots)


def test_sample_transform_falls_back_to_two_launches_beyond_the_scratch(handle):
    """16 x 12 workgroup columns x S = 5462 draws = 1 048 704 per-block slots > 2^20: spmf_sample_transform
    runs the two separate launches.  Same bits of noise and theta as the two calls, log q to 1e-13."""
    S = 5462
    assert 16 * 12 * S > 2 ** 20 >= 4 * 12 * S
    a, b = _big_table(handle, S, 1), _big_table(handle, S, 2)
    a.sample_noise(seed=71, counter=3)
    a.fwd()
    b.sample_transform(seed=71, counter=3)
    for x, y in zip(a.slots, b.slots):
        assert torch.equal(x.noise_w.bits(), y.noise_w.bits()) and torch.equal(x.theta.bits(), y.theta.bits())
    la, lb = a.logq.get(), b.logq.get()
    assert np.isfinite(la).all()
    r = float(np.abs(la - lb).max() / (1e-13 * np.abs(la).max()))
    _note("logq one launch vs two, beyond the scratch", r)
    assert r <= 1.0                                     # observed: 0 (the fall-back runs the same two kernels)
    del a, b
    torch.cuda.empty_cache()


def test_forward_adds_log_q_atomically_beyond_the_scratch(handle):
    """4 x 12 workgroups x S = 21 846 = 1 048 608 > 2^20: surrogate_fwd zeroes logq itself and its blocks add
    to logq[s] with same-address fp64 atomics.  The reference is torch fp64 on the device, 512 draws at a time."""
    S = 21846
    assert 4 * 12 * S > 2 ** 20
    tab = _big_table(handle, S, 3)
    tab.logq.t.fill_(-1.2345e300)                                  # garbage: the branch zeroes it itself
    tab.fwd()
    ref, Y = torch.zeros(S, dtype=torch.float64, device="cuda"), torch.zeros(S, dtype=torch.float64, device="cuda")
    sp = torch.nn.functional.softplus
    for sl in tab.slots:
        t0, sg = sl.t0.t.double(), sp(sl.t1.t.double())
        nz_all = sl.noise_w.t.view(S, sl.n)
        for s0 in range(0, S, 512):
            nz = nz_all[s0:s0 + 512].double()
            y = t0 + sg * nz
            pieces = (-0.5 * nz * nz, (-torch.log(sg)).expand_as(y), torch.full_like(y, -R.HALF_LOG_2PI), sp(-y))
            ref[s0:s0 + 512] += sum(pieces).sum(1)
            Y[s0:s0 + 512] += sum(p.abs() for p in pieces).sum(1)
            if sl.n > 1 and s0 == 0:
                th = sl.theta.t.view(S, sl.n)[:512].double()
                assert float(((th - sp(y)).abs() / sp(y)).max()) <= 1e-5
    r = float(((tab.logq.t - ref).abs() / (1e-5 * Y)).max())
    _note("logq, atomic branch", r)
    assert r <= 1.0                                     # largest observed: 0.0056 of the bound
    del tab, ref, Y
    torch.cuda.empty_cache()
