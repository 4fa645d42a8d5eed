"""CPU: the fp64 reference of the surrogate / optimiser / gate kernels (tests/_sur_reference.py) pinned
against independent computations, so that the GPU edge tests compare the kernels with something that is
itself checked: torch fp64 autograd, the torch Adam of _vi_reference, scipy's inverse incomplete gamma
function and a case worked by hand.  The fp32 defect of the parent's dy/da and the share of the gamma grid
left out for range are on record here too."""
import math

import numpy as np
import pytest
import torch

import _sur_reference as R
import _sur_table as T


class _GammaGiven(torch.autograd.Function):
    """g with d g / d a handed in (as the kernel is handed dgda)."""

    @staticmethod
    def forward(ctx, g, a, dgda):
        ctx.save_for_backward(dgda)
        return g

    @staticmethod
    def backward(ctx, grad):
        (dgda,) = ctx.saved_tensors
        return None, grad * dgda, None


def _torch_loss(kind, t0, t1, nz, ge, inv_sb, c, dgda, ident):
    sp = torch.nn.functional.softplus
    if kind == 2:
        a, b = sp(t0), sp(t1)
        g = _GammaGiven.apply(nz, a.expand(nz.shape), dgda)
        y = b / g
        lq = a * torch.log(b) - torch.lgamma(a) - (a + 1) * torch.log(y) - b / y
    else:
        sg = sp(t1)
        y = t0 + sg * nz
        lq = -0.5 * nz ** 2 - torch.log(sg) - 0.5 * math.log(2 * math.pi)
    soft = torch.ones_like(t0, dtype=torch.bool) if kind != 1 else torch.zeros_like(t0, dtype=torch.bool)
    if kind == 0 and ident is not None:
        soft = torch.as_tensor(ident) == 0
    th = torch.where(soft, sp(y), y)
    lq = lq - torch.where(soft, torch.nn.functional.logsigmoid(y), torch.zeros_like(y))
    return -((ge * th).sum() - c * lq.sum()) * inv_sb, th, lq


@pytest.mark.parametrize("kind,masked", [(0, False), (0, True), (1, False), (2, False)])
def test_fwd_and_bwd_reference_equal_torch_fp64_autograd(kind, masked):
    rng = np.random.default_rng(7 + kind)
    S, n, inv_sb, c = 3, 40, 1.0 / (3 * 50), 0.25
    t0 = rng.uniform(-3, 3, n).astype(np.float32)
    t1 = rng.uniform(-6, 2, n).astype(np.float32)
    ge = (rng.normal(0, 1, (S, n)) * 10.0 ** rng.uniform(-3, 3, (S, n))).astype(np.float32)
    ident = (rng.random(n) < 0.4).astype(np.uint8) if masked else None
    if kind == 2:
        nz = rng.gamma(R.softplus(t0), size=(S, n)).clip(1e-30).astype(np.float32)
        dg = rng.normal(0, 1, (S, n)).astype(np.float32)
    else:
        nz, dg = rng.normal(0, 1, (S, n)).astype(np.float32), None
    f = R.fwd_ref(kind, t0, t1, nz, ident)
    g0, g1, s0, s1 = R.bwd_ref(kind, t0, t1, nz, ge, inv_sb, c, dg, ident)
    tt0 = torch.tensor(t0, dtype=torch.float64, requires_grad=True)
    tt1 = torch.tensor(t1, dtype=torch.float64, requires_grad=True)
    loss, th, lq = _torch_loss(kind, tt0, tt1, torch.tensor(nz, dtype=torch.float64),
                               torch.tensor(ge, dtype=torch.float64), inv_sb, c,
                               None if dg is None else torch.tensor(dg, dtype=torch.float64), ident)
    r0, r1 = torch.autograd.grad(loss, (tt0, tt1))
    np.testing.assert_allclose(f["theta"], th.detach().numpy(), rtol=1e-13, atol=0)
    assert np.abs(f["l"] - lq.detach().numpy()).max() <= 1e-13 * f["Y"].max()
    assert (f["Y"] >= np.abs(f["l"]) * (1 - 1e-15)).all()
    assert (np.abs(g0 - r0.numpy()) <= 1e-12 * s0).all() and (np.abs(g1 - r1.numpy()) <= 1e-12 * s1).all()
    assert (s0 >= np.abs(g0) * (1 - 1e-12)).all() and (s1 >= np.abs(g1) * (1 - 1e-12)).all()


def test_adam_reference_equals_the_torch_adam_in_fp64():
    from _vi_reference import Adam
    rng = np.random.default_rng(3)
    n = 50
    p = rng.normal(0, 1, n)
    m, v = np.zeros(n), np.zeros(n)
    tp = torch.tensor(p.copy())
    opt = Adam([tp], 0.05)
    for t in range(1, 6):
        g = rng.normal(0, 1, n) * 10.0 ** rng.uniform(-4, 4, n)
        opt.step([torch.tensor(g)])
        r = R.adam_ref(p, m, v, g, t=t, lr=0.05)
        p, m, v = r["p"], r["m"], r["v"]
        np.testing.assert_allclose(p, tp.numpy(), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(m, opt.m[0].numpy(), rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(v, opt.v[0].numpy(), rtol=1e-13, atol=1e-300)
    # clipping, and beta^t handed in as the device state holds it
    r = R.adam_ref(p, m, v, g, clip=1e-3, b1t=0.9 ** 7, b2t=0.999 ** 7)
    r2 = R.adam_ref(p, m, v, np.clip(g, -1e-3, 1e-3), t=7)
    assert all(np.array_equal(r[k], r2[k]) for k in "pmv")


def test_dgda_reference_equals_the_derivative_of_the_quantile_function():
    """d g / d a at fixed probability, by central differences of scipy's gammaincinv (gammainccinv in the
    upper tail) at steps h and h / 2, h = 2e-4 a, extrapolated to O(h^4): at a = 0.05 the quantile behaves as
    exp(-138 / a) in the lower tail and the plain quotient is 3e-5 off, the extrapolated one below 1e-7."""
    import scipy.special as sps
    for a in (0.05, 0.1, 0.3, 0.7, 1.0, 1.5, 3.0, 20.0, 50.0, 300.0):
        for pr in (1e-3, 0.05, 0.5, 0.95, 1 - 1e-3):
            g = float(sps.gammaincinv(a, pr))
            if pr > 0.5:
                inv, q = sps.gammainccinv, float(sps.gammaincc(a, g))
            else:
                inv, q = sps.gammaincinv, float(sps.gammainc(a, g))
            h = 2e-4 * a
            d1 = (inv(a + h, q) - inv(a - h, q)) / (2 * h)
            d2 = (inv(a + h / 2, q) - inv(a - h / 2, q)) / h
            fd = (4 * d2 - d1) / 3
            ref = R.dgda_ref(a, g)
            assert abs(ref - fd) <= 1e-6 * abs(fd), (a, pr, g, ref, fd)
    # the small-g leading term handed to the chain-rule kernels is of the right magnitude
    for a in (1e-3, 0.1, 3.0):
        assert abs(R.dgda_small(a, 1e-20) / R.dgda_ref(a, 1e-20) - 1.0) < 1e-6


def test_gate_reference_on_a_hand_case():
    S, c, rows = 2, 0.5, 10.0
    parts = np.zeros((S, 14))
    parts[0, :12] = 1.0            # prior 12
    parts[0, 12], parts[0, 13] = -3.0, -20.0
    parts[1, 0], parts[1, 12], parts[1, 13] = 2.0, -1.0, -10.0
    logq = np.array([4.0, -2.0])
    # draw 0: -20 - 3 + .5 (12 - 4) = -19; draw 1: -10 - 1 + .5 (2 + 2) = -9; loss = 14 / 10
    st = np.zeros(16)
    st[1], st[2], st[5], st[6] = 0.9, 0.999, 0.81, 0.998001
    out = R.gate_ref(st, parts, logq, None, S, c, rows)
    assert out[8] == 1.4 and out[9] == 1.0 and out[7] == 1 and out[11] == 1 and out[12] == 0 and out[13] == 1
    assert out[5] == 0.81 * 0.9 and out[6] == 0.998001 * 0.999 and out[10] == 1.4
    # a non-finite stored cell skips the step; the saturation counts are added up either way
    out2 = R.gate_ref(out, parts, logq, np.array([0.0, 1.0, 3.0, 4.0]), S, c, rows)
    assert out2[9] == 0.0 and out2[12] == 1 and out2[13] == 2 and out2[14] == 7 and out2[7] == 1
    assert out2[5] == out[5] and out2[10] == 1.4
    parts[1, 3] = np.inf
    out3 = R.gate_ref(out2, parts, logq, None, S, c, rows)
    assert out3[9] == 0.0 and out3[12] == 2 and out3[13] == 3 and not np.isfinite(out3[8])


def test_the_square_of_a_small_draw_is_the_defect_and_the_quotient_form_is_not():
    """(a, b, g) = (0.1, 1, 1e-20): dy/da = -b / g^2 * dg/da is about -4.6e22.  In fp32 g * g is 0 (below
    3.7e-23), so the form the chain rule had, -b / (g * g) * dgda, is not finite; -(y * dgda) / g with
    y = b / g is the reference's value to fp32 rounding."""
    f = np.float32
    a, b, g = 0.1, f(1.0), f(1e-20)
    dg = f(R.dgda_ref(a, float(g)))
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        old = -b / (g * g) * dg
        y = b / g
        new = -(y * dg) / g
    exact = -float(b) / float(g) / float(g) * float(dg)
    assert -4.8e22 < exact < -4.4e22
    assert not np.isfinite(old)
    assert np.isfinite(new) and abs(float(new) - exact) <= 4 * 2.0 ** -24 * abs(exact)
    # and through bwd_ref: the t0 gradient of that element is finite and holds that factor
    t0, t1 = T.raw_of(a), T.raw_of(1.0)
    g0, _, s0, _ = R.bwd_ref(2, [t0], [t1], [[g]], [[1.0]], 1.0, 0.0, [[dg]])
    bb = float(R.softplus(np.float64(t1)))         # softplus of the fp32 raw value: 1 to 1e-9
    expect = -R.sigmoid(np.float64(t0)) * R.sigmoid(bb / float(g)) * exact * bb
    assert np.isfinite(g0[0]) and abs(g0[0] - expect) <= 1e-12 * abs(expect) and s0[0] >= abs(g0[0]) * (1 - 1e-12)


# the (1 / (S B), c) of the four grid cases of tests/test_gpu_surrogate_edges.py
@pytest.mark.parametrize("inv_sb,c", [(1.0 / 256, 1.0), (1.0 / (2 * 1000), 1e-3), (1.0 / (7 * 256), 1.0),
                                      (1.0 / (2 * 256), 1e-3)])
def test_at_most_a_tenth_of_the_gamma_grid_leaves_the_fp32_range(inv_sb, c):
    grid = T.gamma_grid(inv_sb, c)
    assert len(grid) == len(T.GAMMA_A) * len(T.GAMMA_B) * len(T.GAMMA_G) == 360
    out = sum(not k[4] for k in grid)
    assert out <= 0.10 * len(grid), out
    # every (a, b) pair keeps draws, the small ones g <= 1e-20 with a <= 0.3 among them
    ng = len(T.GAMMA_G)
    assert all(any(k[4] for k in grid[p:p + ng]) for p in range(0, len(grid), ng))
    small = [k for k in grid if k[4] and k[2] <= 1.0001e-20 and R.softplus(np.float64(k[0])) <= 0.31]
    assert len(small) >= 20
