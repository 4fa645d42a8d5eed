"""GPU: the Philox sampler of spmf_amd/csrc/surrogate.hip (spmf_sample_noise, spmf_sample_transform) at its
edges: the implicit gamma derivative against mpmath over a in [0.02, 3500] (3500 is the end of the domain
include/spmf_hip.h states), the distribution of the draws (boost a < 1, both fp32 neighbours of 1, large a,
the clamp at 1e-30), the counter layout, and the one-launch sample + transform against the fp64 reference
at block edges, with skipped slots and noise as column slices.

Fixed seeds make the outcome deterministic.  Ten KS tests at p > 1e-4 fail a correct sampler with
probability below 1e-3.
"""
import numpy as np
import pytest
import scipy.stats as sst
import torch

import _sur_reference as R
import _sur_table as T

pytestmark = pytest.mark.gpu

ONE_LO = float(np.nextafter(np.float32(1), np.float32(0)))
ONE_HI = float(np.nextafter(np.float32(1), np.float32(2)))


@pytest.fixture(scope="module")
def handle():
    from spmf_amd import PoissonFactorization
    m = PoissonFactorization(latent_dim=2, feature_dim=8, u_tau_scale=0.1, device="cuda")
    yield m._handle()
    del m
    torch.cuda.empty_cache()


def _gamma_slot(S, a, n=None, ld=None):
    t0 = np.full(n, T.raw_of(a)) if n is not None else np.asarray([T.raw_of(x) for x in a], dtype=np.float32)
    return T.SurSlot(S, t0.size, 2, t0, np.zeros(t0.size, dtype=np.float32), ld=ld)


def _a32(t0):
    """softplus of the fp32 raw value IN fp32, widened: what the kernel is handed, up to one ulp."""
    t0 = np.asarray(t0, dtype=np.float32)
    return (np.maximum(t0, np.float32(0)) + np.log1p(np.exp(-np.abs(t0)))).astype(np.float32).astype(np.float64)


def test_implicit_gradient_against_mpmath_over_the_stated_domain(handle):
    S = 64
    a = np.concatenate([np.geomspace(0.02, 1000.0, 98), [3500.0, 3500.0]])
    sl = _gamma_slot(S, a)
    tab = T.SurTable(handle, S, [sl])
    tab.sample_noise(seed=2024, counter=1)
    g, dg = sl.noise().astype(np.float64), sl.dgda().astype(np.float64)
    assert np.isfinite(g).all() and np.isfinite(dg).all() and (g >= 1e-30 * (1 - 1e-6)).all()
    a32 = _a32(sl.t0.get())
    worst, pairs = 0.0, 0
    for i in range(a.size):
        for s in {int(np.argmin(g[:, i])), int(np.argmax(g[:, i])), int(np.argsort(g[:, i])[S // 2])}:
            ref = R.dgda_ref(float(a32[i]), float(g[s, i]))
            rel = abs(dg[s, i] - ref) / abs(ref)
            worst, pairs = max(worst, rel), pairs + 1
            assert rel <= 1e-5, (a32[i], g[s, i], dg[s, i], ref)      # largest observed on an MI355X: 1.8e-7
    print(f"[ratio] dgda vs mpmath: {worst / 1e-5:.3e} of its bound over {pairs} pairs")
    assert pairs >= 280
    # the draws of the largest admitted a stay inside the series' 4000 terms
    assert g[:, -2:].max() < 3998.0


@pytest.fixture(scope="module")
def gamma_draws(handle):
    """400 000 draws (n = 2000, S = 200) at each concentration, one slot each, one launch: the moments are
    taken over all of them, the KS tests and the clamp count over the first ten draws (20 000 values)."""
    conc = (0.05, 0.1, 0.3, 0.7, ONE_LO, ONE_HI, 1.5, 20.0, 300.0)
    S = 200
    slots = [_gamma_slot(S, a, n=2000, ld=2000 + 7 * (j % 2)) for j, a in enumerate(conc)]
    tab = T.SurTable(handle, S, slots)
    tab.sample_noise(seed=31337, counter=0)
    out = {a: (sl.noise().astype(np.float64).ravel(), sl.dgda().astype(np.float64).ravel(), _a32(sl.t0.get())[0])
           for a, sl in zip(conc, slots)}
    del tab, slots
    return out


@pytest.mark.parametrize("a", [0.1, 0.3, 0.7, ONE_LO, ONE_HI, 1.5, 20.0, 300.0])
def test_gamma_draws_pass_ks_and_moments(gamma_draws, a):
    g, dg, a32 = gamma_draws[a]
    assert g.size == 400000 and np.isfinite(g).all() and np.isfinite(dg).all() and (g >= 1e-30 * (1 - 1e-6)).all()
    z = (g - a32) / np.sqrt(a32)
    # standardised moments at the tolerances of test_hip_sampler_statistics_and_implicit_gradient.  The sample
    # variance of z has the standard error sqrt((2 + 6 / a) / N) (gamma: excess kurtosis 6 / a): over the
    # 400 000 draws 0.012 at a = 0.1, so 0.06 is 4.8 standard errors there and more at every larger a.
    assert abs(z.mean()) < 0.03, (a, z.mean())
    assert abs(z.var() - 1.0) < 0.06, (a, z.var())
    print(f"[moments] gamma a = {a}: mean {z.mean():+.4f}, var - 1 {z.var() - 1.0:+.4f}")
    g = g[:20000]
    p = sst.kstest(g, "gamma", args=(a32,)).pvalue
    print(f"[ks] gamma a = {a}: p = {p:.3e}")
    assert p > 1e-4, (a, p)


def test_draws_at_the_clamp(gamma_draws):
    """a = 0.05: 3 % of the mass lies below the clamp 1e-30, which a KS test rightly rejects; the share of
    draws AT the clamp is the gamma CDF there."""
    g, dg, a32 = gamma_draws[0.05]
    assert (g >= 1e-30 * (1 - 1e-6)).all() and np.isfinite(g).all() and np.isfinite(dg).all()
    g = g[:20000]
    share = sst.gamma.cdf(float(np.float32(1e-30)), a32)
    at = np.mean(g == float(np.float32(1e-30)))
    se = np.sqrt(share * (1 - share) / g.size)
    assert abs(at - share) <= 3 * se, (at, share, se)


def test_four_million_normal_draws(handle):
    S, n = 64, 65536
    sl = T.SurSlot(S, n, 0, np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32))
    tab = T.SurTable(handle, S, [sl])
    tab.sample_noise(seed=5, counter=9)
    e = sl.noise_w.t
    assert bool(torch.isfinite(e).all()) and float(e.abs().max()) <= 6.0
    x = e.double()
    assert abs(float(x.mean())) < 0.02 and abs(float(x.std()) - 1.0) < 0.02
    p = sst.kstest(x.cpu().numpy(), "norm").pvalue
    print(f"[ks] normal, {x.numel()} draws: p = {p:.3e}")
    assert p > 1e-4
    del tab, sl, e, x
    torch.cuda.empty_cache()


def test_counter_layout(handle):
    S, n = 4, 512

    def table(nvars, a=0.5, skip_none=()):
        slots = []
        for j in range(nvars):
            if j in skip_none:
                slots.append(None)
            elif j % 2 == 0:
                slots.append(T.SurSlot(S, n, 0, np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)))
            else:
                slots.append(_gamma_slot(S, a, n=n))
        return T.SurTable(handle, S, slots)

    full = table(12)
    full.sample_noise(seed=77, counter=5)
    nz = [sl.noise() for sl in full.slots]
    # equal n, equal parameters: other slot, other draw, other element -> other bits
    assert not np.array_equal(nz[0], nz[2]) and not np.array_equal(nz[1], nz[3])
    assert (nz[0] != nz[2]).mean() > 0.99 and (nz[1] != nz[3]).mean() > 0.99
    for k in (0, 1):
        assert (nz[k][0] != nz[k][1]).mean() > 0.99
        assert np.unique(nz[k][0]).size > 0.99 * n
    # the same (seed, counter, slot, draw, element): the same bits whatever nvars and whichever slots are skipped
    part = table(4, skip_none=(0, 2))
    part.sample_noise(seed=77, counter=5, skip=(1,))
    assert np.array_equal(part.slots[3].noise(), nz[3]) and np.array_equal(part.slots[3].dgda(), full.slots[3].dgda())
    assert bool((part.slots[1].noise_w.bits() == T._SENT[torch.float32][1]).all())      # handed over as n = 0
    # ... and the device step counter adds to the host's
    st = torch.zeros(16, dtype=torch.float64)
    st[13] = 3.0
    part2 = table(4)
    part2.sample_noise(seed=77, counter=2, state=st.cuda())
    for j in range(4):
        assert np.array_equal(part2.slots[j].noise(), nz[j]), j
    other = table(4)
    other.sample_noise(seed=77, counter=6)
    assert (other.slots[0].noise() != nz[0]).mean() > 0.99
    # the boost uniform of a < 1: a = 0.5 and a = 1.5 run the SAME Marsaglia-Tsang draw G (both at a + 1 = 1.5 or
    # a = 1.5, same counter), so g(0.5) / g(1.5) = ub^2 recovers the boost uniform: it must be uniform and must
    # not follow G, whose words it shares (it is taken from their low bytes)
    big = table(4, a=1.5)
    big.sample_noise(seed=77, counter=5)
    G = np.concatenate([big.slots[j].noise().astype(np.float64).ravel() for j in (1, 3)])
    gb = np.concatenate([nz[j].astype(np.float64).ravel() for j in (1, 3)])
    ub = np.sqrt(gb / G)
    assert (ub > 0).all() and (ub < 1 + 1e-6).all()
    p = sst.kstest(ub, "uniform").pvalue
    rho = sst.spearmanr(ub, G)[0]
    print(f"[ks] boost uniform: p = {p:.3e}, spearman with the Marsaglia-Tsang draw {rho:.3e}")
    assert p > 1e-4
    assert abs(rho) <= 4.5 / np.sqrt(ub.size)                  # 4.5 standard errors of rho under independence
    assert abs(sst.spearmanr(gb, G)[0]) < 0.9                  # g is not a monotone function of G


@pytest.mark.parametrize("S,wide", [(1, False), (3, True)])
def test_sample_and_transform_in_one_launch_against_the_reference(handle, S, wide):
    """sample_fwd_kernel (256 elements per block, one draw per block): theta and log q from ITS noise against
    fwd_ref, sizes on the block edges, a skipped slot first / in the middle / last."""
    sizes = [None, 257, 1, 1025, None, 256, 255, 4097, 1024, 2049, 1023, None]
    rng = np.random.default_rng(S)
    slots, meta = [], []
    for j, n in enumerate(sizes):
        if n is None:
            slots.append(None)
            meta.append(None)
            continue
        kind = (0, 2, 1)[j % 3]
        if kind == 2:
            t0 = np.asarray([T.raw_of(x) for x in rng.choice([0.3, ONE_LO, 3.0, 50.0], n)], dtype=np.float32)
            t1 = np.asarray([T.raw_of(x) for x in rng.choice([7e-3, 1.0, 20.0], n)], dtype=np.float32)
        else:
            t0 = rng.uniform(-30, 30, n).astype(np.float32)
            t1 = rng.choice(np.asarray(T.NORMAL_T1, dtype=np.float32), n)
        ident = (rng.random(n) < 0.5).astype(np.uint8) if kind == 0 and j % 2 else None
        slots.append(T.SurSlot(S, n, kind, t0, t1, ident=ident, ld=n + 9 if wide and j % 2 else None))
        meta.append((kind, t0, t1, ident))
    tab = T.SurTable(handle, S, slots)
    tab.logq.t.fill_(float("nan"))
    tab.sample_transform(seed=99, counter=4)
    logq, Y, worst = np.zeros(S), np.zeros(S), 0.0
    for sl, mt in zip(slots, meta):
        if sl is None:
            continue
        nz = sl.noise()
        assert np.isfinite(nz).all()
        f = R.fwd_ref(mt[0], mt[1], mt[2], nz, mt[3])
        logq += f["l"].sum(1)
        Y += f["Y"].sum(1)
        th = sl.theta.get().astype(np.float64).reshape(S, -1)
        bound = 1e-5 * np.maximum(np.abs(f["theta"]), f["th_scale"]) + 1.2e-38
        worst = max(worst, float((np.abs(th - f["theta"]) / bound).max()))
    r = float((np.abs(tab.logq.get() - logq) / (1e-5 * Y)).max())
    print(f"[ratio] one launch: theta {worst:.3e}, logq {r:.3e} of their bounds")
    assert worst <= 1.0 and r <= 1.0              # largest observed: theta 0.011, log q 0.00064 of the bound


def test_one_launch_loses_and_doubles_no_element_of_log_q(handle):
    """sample_fwd_kernel's own log-q sum (256 elements and one draw per block, per-block slots) on parameters
    where every |l_i| is far above the sum's allowance: sigma = softplus(-30) = 9e-14 gives l_i = 29 - eps^2 / 2
    with pieces of about 31 (kind 2: a = 3, b = 1e8: l_i = -19.1 + 4 log g - g <= -17.5), so with fewer than
    5000 elements a lost or a doubled element cannot hide in 1e-5 Y_s -- asserted below from the reference on
    the noise the kernel drew.  Sizes on the block edges, a skipped slot first, in the middle and last."""
    S = 2
    layout = [None, (257, 0), (1, 2), (1025, 1), None, (256, 0), (65, 2), (2049, 0), (1023, 1), None]
    rng = np.random.default_rng(17)
    slots, meta = [], []
    for j, spec in enumerate(layout):
        if spec is None:
            slots.append(None)
            meta.append(None)
            continue
        n, kind = spec
        if kind == 2:
            t0, t1 = np.full(n, T.raw_of(3.0)), np.full(n, T.raw_of(1e8))
        else:
            t0, t1 = rng.uniform(2.0, 6.0, n).astype(np.float32), np.full(n, -30.0, dtype=np.float32)
        slots.append(T.SurSlot(S, n, kind, t0, t1, ld=n + 5 if j % 2 else None))
        meta.append((kind, t0, t1))
    tab = T.SurTable(handle, S, slots)
    tab.logq.t.fill_(float("nan"))
    tab.sample_transform(seed=123, counter=8)
    logq, Y, lmin = np.zeros(S), np.zeros(S), np.inf
    for sl, mt in zip(slots, meta):
        if sl is None:
            continue
        f = R.fwd_ref(mt[0], mt[1], mt[2], sl.noise())
        logq += f["l"].sum(1)
        Y += f["Y"].sum(1)
        lmin = min(lmin, float(np.abs(f["l"]).min()))
    assert lmin >= 10 * 1e-5 * Y.max(), (lmin, Y.max())           # a condition on the inputs, not on the kernel
    r = float((np.abs(tab.logq.get() - logq) / (1e-5 * Y)).max())
    print(f"[ratio] one launch, benign: logq {r:.3e} of its bound (smallest |l_i| {lmin:.2f}, allowance {1e-5 * Y.max():.3f})")
    assert r <= 1.0
