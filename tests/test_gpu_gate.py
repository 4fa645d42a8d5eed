"""GPU: spmf_vi_gate (vi_gate_kernel of spmf_amd/csrc/surrogate.hip) against gate_ref.  All of it is fp64, so the
loss is held to 1e-14 relative and the counters exactly; the state sits between canary margins."""
import numpy as np
import pytest
import torch

import _sur_reference as R
import _sur_table as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    from spmf_amd import PoissonFactorization
    m = PoissonFactorization(latent_dim=2, feature_dim=8, u_tau_scale=0.1, device="cuda")
    yield m._handle()
    del m


def _state():
    st = np.zeros(16)
    st[0], st[1], st[2], st[3], st[5], st[6] = 0.05, 0.9, 0.999, 1e-7, 1.0, 1.0
    return st


def _inputs(S, rng):
    # log-probabilities: every part negative, log q positive (a tight normal), so the loss adds terms of one
    # sign and "1e-14 relative" is a bound on rounding, not on cancellation
    parts = -rng.uniform(1.0, 1e4, (S, 14))
    logq = rng.uniform(1.0, 1e5, S)
    return parts, logq


def _run(handle, st, parts, logq, nnf, S, c, rows):
    g = T.Guarded(16, torch.float64, fill=st)
    T.vi_gate(handle, g, torch.tensor(parts, dtype=torch.float64).reshape(-1).cuda(),
              torch.tensor(logq, dtype=torch.float64).cuda(),
              None if nnf is None else torch.tensor(nnf, dtype=torch.float64).cuda(), S, c, rows)
    return g.get()


def _same(got, ref):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])       # the same infinity
    rel = np.abs(got[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1e-300)
    assert rel.max() <= 1e-14, (got, ref)                   # observed on an MI355X: 0 (the same doubles)
    for k in (7, 9, 11, 12, 13, 14):
        assert got[k] == ref[k], k
    return float(rel.max())


@pytest.mark.parametrize("S", [1, 3, 20])
@pytest.mark.parametrize("nnf_mode", ["null", "zero", "one_draw", "saturation"])
def test_gate_state_update(handle, S, nnf_mode):
    rng = np.random.default_rng(S)
    parts, logq = _inputs(S, rng)
    nnf = None
    if nnf_mode != "null":
        nnf = np.zeros(2 * S)
        if nnf_mode == "one_draw":
            nnf[S - 1] = 2.0
        if nnf_mode == "saturation":
            nnf[S:] = rng.integers(0, 50, S)
    st = _state()
    st[13], st[14], st[7], st[10], st[11] = 41.0, 5.0, 40.0, 123.5, 40.0
    c, rows = 0.37, 250.0
    got, ref = _run(handle, st, parts, logq, nnf, S, c, rows), R.gate_ref(st, parts, logq, nnf, S, c, rows)
    r = _same(got, ref)
    print(f"[ratio] gate: {r / 1e-14:.3e} of its bound")
    assert ref[9] == (0.0 if nnf_mode == "one_draw" else 1.0)
    assert got[14] == 5.0 + (nnf[S:].sum() if nnf is not None else 0.0)


@pytest.mark.parametrize("where", ["parts", "logq"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_loss_skips_the_step(handle, where, value):
    S = 3
    parts, logq = _inputs(S, np.random.default_rng(1))
    if where == "parts":
        parts[1, 4] = value
    else:
        logq[2] = value
    st = _state()
    got, ref = _run(handle, st, parts, logq, None, S, 1.0, 10.0), R.gate_ref(st, parts, logq, None, S, 1.0, 10.0)
    _same(got, ref)
    assert got[9] == 0.0 and got[12] == 1.0 and got[13] == 1.0 and got[7] == 0.0 and got[5] == 1.0 and got[6] == 1.0
    assert not np.isfinite(got[8])


def test_two_thousand_gated_steps_every_seventh_skipped(handle):
    S, c, rows = 3, 0.5, 100.0
    rng = np.random.default_rng(2)
    parts, logq = _inputs(S, rng)
    bad = parts.copy()
    bad[0, 13] = np.nan
    dp, db = (torch.tensor(x, dtype=torch.float64).reshape(-1).cuda() for x in (parts, bad))
    dl = torch.tensor(logq, dtype=torch.float64).cuda()
    g = T.Guarded(16, torch.float64, fill=_state())
    lib, h = T._lib.load(), handle
    stream = torch.cuda.current_stream().cuda_stream
    steps, skipped = 2000, 0
    for i in range(steps):
        skip = i % 7 == 6
        skipped += skip
        T._need(g.t, torch.float64, 16, "state")
        T._lib.check(h, lib.spmf_vi_gate(h, (db if skip else dp).data_ptr(), dl.data_ptr(), None, S, c, rows, g.ptr,
                                         stream), "spmf_vi_gate")
    torch.cuda.synchronize()
    assert g.intact()
    st = g.get()
    applied = steps - skipped
    assert st[7] == applied and st[11] == applied and st[12] == skipped and st[13] == steps
    assert abs(st[5] - 0.9 ** applied) <= 1e-12 * 0.9 ** applied
    assert abs(st[6] - 0.999 ** applied) <= 1e-12 * 0.999 ** applied
    loss = R.gate_ref(_state(), parts, logq, None, S, c, rows)[8]
    assert abs(st[10] - applied * loss) <= 1e-12 * abs(applied * loss)
