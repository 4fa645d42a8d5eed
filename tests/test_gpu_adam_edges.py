"""GPU: spmf_adam_step and spmf_adam_step_dev (adam_block of spmf_amd/csrc/surrogate.hip) against adam_ref in
fp64: sizes on both sides of the 2048 elements a block covers, the float4 branch and the scalar branch in one
launch (each of p, m, v, g in turn one element into its buffer), steps far from and at bias correction 1,
clipping, and gradients from exact 0 to 1e15.  Five steps in a row, each checked ONE step ahead from the
device's own fp32 p, m, v, so every bound belongs to one step.  Canary margins around p, m, v, g.

|g| above 1e18 is out of scope: g * g leaves the fp32 range there in any fp32 Adam.
"""
import numpy as np
import pytest
import torch

import _sur_reference as R
import _sur_table as T

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
SIZES = (1, 2, 3, 4, 5, 1023, 2047, 2048, 2049, 2052, 4100)
LR, B1, B2, EPS = 0.05, 0.9, 0.999, 1e-7
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


def _gradient(n, rng):
    """Exact zeros, +-1e-30, +-1, +-1e15 and a spread between."""
    g = rng.normal(0, 1, n) * 10.0 ** rng.uniform(-8, 8, n)
    special = np.array([0.0, 1e-30, -1e-30, 1.0, -1.0, 1e15, -1e15])
    idx = rng.permutation(n)[:min(n, 7 * max(1, n // 20))]
    g[idx] = special[np.arange(idx.size) % 7] if n > 1 else special[rng.integers(7)]
    return g.astype(np.float32)


def _tensors(sizes, rng, shifts):
    out = []
    for j, n in enumerate(sizes):
        g = _gradient(n, rng)
        m = rng.normal(0, 1, n) * 10.0 ** rng.uniform(-6, 2, n)
        # v >= 1e-12 where g is tiny: (1 - b2) g^2 = 1e-63 for g = 1e-30, not an fp32 number, so a bound
        # relative to v_ref can only be asked where v_ref is one
        v = 10.0 ** rng.uniform(-12, 2, n)
        zero = g == 0.0
        m[zero], v[zero] = 0.0, 0.0                       # exact zeros with m = v = 0: p must not move
        out.append(dict(n=n, p=rng.normal(0, 1, n).astype(np.float32), m=m.astype(np.float32),
                        v=v.astype(np.float32), g=g, shift=shifts[j % len(shifts)]))
    return out


def _check_step(tab, before, grads, tag, **ref_kw):
    for j, r in enumerate(tab.rec):
        a = R.adam_ref(before["p"][j], before["m"][j], before["v"][j], grads[j], lr=LR, b1=B1, b2=B2, eps=EPS,
                       **ref_kw)
        got = {k: r[k].get().astype(np.float64) for k in "pmv"}
        assert all(np.isfinite(got[k]).all() for k in "pmv"), (tag, j)
        # largest observed on an MI355X, as a share of the bound: m 0.29, v 0.52, p 0.50
        # (a build of the kernel that forms 1 - beta2 in fp32 is at 27 x the bound of v)
        bounds = {"m": 4 * U * a["ym"],
                  "v": 4 * U * a["yv"],
                  "p": U * np.abs(a["p"]) + 1e-5 * a["ystep"]}
        for k in "mvp":
            err, b = np.abs(got[k] - a[k]), bounds[k]
            ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
            _note(f"adam {k}", ratio.max())
            assert (err <= b).all(), (tag, j, k, int(np.argmax(ratio)), float(ratio.max()))
        zero = (grads[j] == 0.0) & (before["m"][j] == 0.0) & (before["v"][j] == 0.0)
        assert np.array_equal(got["p"][zero], before["p"][j][zero].astype(np.float64))


# each of p, m, v, g in turn one element into its buffer (scalar branch although n % 4 == 0), and all aligned
SHIFTS = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1))


@pytest.mark.parametrize("dev", [False, True], ids=["host_scalars", "device_state"])
@pytest.mark.parametrize("t0,clip", [(1, 0.0), (2, 1e-3), (1000, "equal"), (100000, 0.0)])
def test_adam_steps_one_step_ahead_of_the_fp64_reference(handle, dev, t0, clip):
    rng = np.random.default_rng(t0 + 7 * dev)
    sizes = list(SIZES) + [2048, 4100, 2052, 4]            # the multiples of 4 again, under other shifts
    tens = _tensors(sizes, rng, SHIFTS)
    if clip == "equal":
        # a clip value that IS one of the |g|, half of them above: the median |g| of tensor 10 (n = 4100, all
        # four arrays aligned: the float4 branch), planted with both signs in tensor 5 (n = 1023: the scalar
        # branch) and tensor 11 (n = 2048 with p one element in: the scalar branch although n % 4 == 0)
        assert tens[10]["n"] % 4 == 0 and tens[10]["shift"] == (0, 0, 0, 0) and tens[11]["shift"] != (0, 0, 0, 0)
        ag = np.sort(np.abs(tens[10]["g"]))
        clip = float(ag[ag.size // 2])
        assert 0 < clip < float(ag[-1])
        for j in (5, 11):
            k = np.flatnonzero(tens[j]["g"] != 0.0)[:2]
            tens[j]["g"][k] = (clip, -clip)
        assert all((np.abs(tens[j]["g"]) == np.float32(clip)).any() for j in (5, 10, 11))
    tab = T.AdamTable(handle, tens)
    st = torch.zeros(16, dtype=torch.float64)
    for step in range(5):
        t = t0 + step
        before = {k: tab.host(k) for k in "pmv"}
        # step 0's gradients again in step 3 (the clip value meets its |g| a second time, on other m, v)
        grads = [_gradient(r["n"], rng) for r in tab.rec] if step not in (0, 3) else [x["g"].copy() for x in tens]
        for j, (r, g) in enumerate(zip(tab.rec, grads)):
            # where v is still 0 a tiny g would ask for v_ref = (1 - b2) g^2 below the fp32 range (see _tensors)
            g[(before["v"][j] == 0.0) & (np.abs(g) < 1e-15)] = 0.0
            r["g"].set(g)
        if dev:
            st[0], st[1], st[2], st[3], st[4] = LR, B1, B2, EPS, clip
            st[5], st[6], st[7], st[9] = B1 ** (t - 1), B2 ** (t - 1), t - 1, 1.0
            # the gate multiplies [5], [6] by beta before the update reads them
            st[5] *= B1
            st[6] *= B2
            state = st.cuda()
            tab.step_dev(state)
            _check_step(tab, before, grads, (dev, t, clip), clip=clip, b1t=float(st[5]), b2t=float(st[6]))
        else:
            tab.step(LR, B1, B2, EPS, t, clip)
            _check_step(tab, before, grads, (dev, t, clip), clip=clip, t=t)


@pytest.mark.parametrize("ntensors", [1, 24])
def test_one_and_twentyfour_tensors(handle, ntensors):
    rng = np.random.default_rng(ntensors)
    sizes = [SIZES[(3 * j + 7) % len(SIZES)] for j in range(ntensors)]
    if ntensors == 1:
        sizes = [2049]
    tens = _tensors(sizes, rng, SHIFTS)
    tab = T.AdamTable(handle, tens)
    before = {k: tab.host(k) for k in "pmv"}
    tab.step(LR, B1, B2, EPS, 3, 0.0)
    _check_step(tab, before, [x["g"] for x in tens], ("ntensors", ntensors), t=3)


def test_a_gated_off_device_step_changes_no_bit(handle):
    rng = np.random.default_rng(5)
    tab = T.AdamTable(handle, _tensors(SIZES, rng, SHIFTS))
    bits = [[r[k].bits() for k in "pmvg"] for r in tab.rec]
    st = torch.zeros(16, dtype=torch.float64)
    st[0], st[1], st[2], st[3], st[5], st[6], st[7], st[9] = LR, B1, B2, EPS, B1, B2, 1, 0.0
    tab.step_dev(st.cuda())
    for r, b in zip(tab.rec, bits):
        for k, x in zip("pmvg", b):
            assert torch.equal(r[k].bits(), x)
