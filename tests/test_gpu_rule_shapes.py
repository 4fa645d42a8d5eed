"""The non-finite replacement rule (poisson.py:606-616) at real shapes: values against the literal
oracle (oracle.unormalized_log_prob_parts), gradients against fp64 autograd through _rule_energy
(tests/_problems.py), on batches with a known set of rate-0 stored cells per draw
(tests/_rule_cases.py).

What the cases reach that the 24 x 15 problem of test_gpu_rule_and_surface.py cannot: the minimum
in a draw other than the first (s* decoding), bad cells in several draws (N is the total, nlg per
draw), the minimum on a row of more than 64 stored entries (the gA' chain), KP = 4 ... 256, the
log_transform decoder, scale_rows off, the cross-block CAS minimum and the grid-stride loop of the
reductions, index_base across row chunks, row_base != 0, both column-split halves, deterministic
mode, and draws run back to back.

Poisson only.  The Bernoulli, mixed and Bernoulli + log_transform branches of
nonfinite_patch_kernel cannot be reached with finite parameters: a Bernoulli log-pmf
x * l - softplus(l) is finite for every finite logit, so such a model never has a non-finite cell
and never calls the rule.  Those branches are not exercised here, and no input is made up for them."""
import functools

import numpy as np
import pytest
import torch

import _rule_cases as RC
from oracle import spmf_oracle as O
from _energy_check import MIN_GAP, assert_same_bits, check_rule
from _problems import _rule_energy, build_model

gpu = pytest.mark.gpu
T = torch.as_tensor


@functools.lru_cache(maxsize=4)
def _reference(name):
    """(cfg, x of the batch's rows, params, literal parts, rule gradients) of a case."""
    c = next(k for k in RC.ALL if k.name == name)
    cfg, x, params = RC.build(c)
    xb = x[RC.rows_of(c)]
    ref_v = O.unormalized_log_prob_parts(cfg, xb, params)
    rparts, rgrads = _rule_energy(cfg, xb, params)
    np.testing.assert_allclose(rparts["x"].numpy(), ref_v["x"].numpy(), rtol=1e-12)
    return c, cfg, x, xb, params, ref_v, rgrads


@pytest.mark.parametrize("case", RC.ALL, ids=lambda c: c.name)
def test_cases_are_well_posed(case):
    """Oracle only (no GPU): every rate-0 cell is a stored cell, each draw holds the planted count, the
    reference gradients are finite, and the minimum over the finite cells is unique with a relative
    gap of at least 1e-3 to the runner-up -- and sits where the case says it does."""
    c, cfg, x, xb, params, ref_v, rgrads = _reference(case.name)
    ll, rate, bad, (s, b, d), gap = RC.minimum_of(cfg, xb, params)
    assert not ((rate <= 0) & ~(xb > 0)[None]).any(), "an unstored cell has rate 0"
    assert (bad == ((rate <= 0) & (xb > 0)[None])).all()
    assert bad.sum((1, 2)).tolist() == RC.planted_counts(c) and bad.sum() > 0
    assert (xb > 0).sum(1).min() > 0, "empty row"
    for k, g in rgrads.items():
        assert np.isfinite(g).all(), k
    for k, v in ref_v.items():
        assert torch.isfinite(v).all(), k
    assert gap >= MIN_GAP, gap
    if c.logt:
        z = O.encode(cfg, T(xb), T(params["u"]), T(params["s"]))
        assert float((torch.matmul(z, T(params["v"])) * cfg.eta_i).max()) <= 8.0
    e = c.expect
    nnz = int((xb[b] > 0).sum())
    print(f"{c.name}: minimum {ll[s, b, d]:.4f} at draw {s} row {b} col {d}, {nnz} stored entries on "
          f"its row, gap {gap:.2e}, planted {RC.planted_counts(c)}")
    assert e.get("draw", s) == s
    assert nnz >= e.get("row_nnz", 0)
    assert d < e.get("col_lt", c.D) and d >= e.get("col_ge", 0)
    assert e.get("panel", b // c.panel_rows) == b // c.panel_rows
    if c.deep is not None:
        r0 = RC.rows_of(c).start
        assert (s, b + r0, d) == (c.deep[0], c.deep[1] % c.B, c.deep[2])
    # the minimum's draw holds bad cells in another draw too, or the bad cells are all elsewhere
    assert bad.sum() > bad[s].sum() or c.S == 1 or bad[s].sum() == bad.sum()


def test_cases_reach_what_they_are_there_for():
    ks = {c.K for c in RC.ALL}
    assert ks >= {3, 16, 40, 64, 100, 200}
    assert {c.logt for c in RC.ALL} == {True, False} and {c.scale_rows for c in RC.ALL} == {True, False}
    assert any(c.expect.get("draw") == 0 and any(s > 0 for s in c.plants) for c in RC.ALL)
    assert any(c.expect.get("draw", 0) > 0 for c in RC.ALL)
    assert any(c.expect.get("row_nnz", 0) > 64 for c in RC.ALL)
    assert RC.MANY_CELLS.B * RC.MANY_CELLS.D > 2048 * 1024
    assert all(c.B * c.D * c.S > 1024 for c in RC.ALL)
    assert all(c.K <= 64 and not c.logt for c in RC.DETERMINISTIC)


def _batch(c, x, model=None):
    if c.panels is None:
        return {"counts": x}
    from spmf_amd import SparseCounts
    sc = SparseCounts.from_any(x, "cuda", c.panel_rows, getattr(model, "column_split", 0))
    return {"counts": sc, "panels": c.panels}


def _run(case, **model_kw):
    c, cfg, x, xb, params, ref_v, rgrads = _reference(case.name)
    m = build_model(cfg, c.panel_rows)
    for k, v in model_kw.items():
        setattr(m, k, v)
    return (c, m, _batch(c, x, m), params, ref_v, rgrads)


@gpu
@pytest.mark.parametrize("case", RC.CASES + [RC.MANY_CELLS, RC.TALL, RC.BACK_TO_BACK], ids=lambda c: c.name)
def test_rule_value_and_gradient_at_shape(case):
    check_rule(*_run(case))


@gpu
@pytest.mark.parametrize("case", [RC.MINIBATCH, RC.MINIBATCH_WIDE], ids=lambda c: c.name)
def test_rule_on_a_panel_range_minibatch(case):
    """panels = (p0, p1), p0 > 0, against the oracle on that row slice; planted rows outside the
    range do not count."""
    c, m, batch, params, ref_v, rgrads = _run(case)
    assert sum(RC.planted_counts(c)) < sum(len(r) * len(k) for r, k in c.plants.values())
    check_rule(c, m, batch, params, ref_v, rgrads)


@gpu
@pytest.mark.parametrize("case", [RC.CHUNKED, RC.CHUNKED_LOGT, RC.MINIBATCH], ids=lambda c: c.name)
def test_rule_with_the_scan_cut_into_row_chunks(case, monkeypatch):
    """_nonfinite_scan over chunks of one panel and of two panels (index_base != 0; the minimum's
    chunk is neither the first nor one with bad cells) == the unchunked scan to 1e-12 on 'x', and
    each == the oracle."""
    c, m, batch, params, ref_v, rgrads = _run(case)
    whole, gwhole = check_rule(c, m, batch, params, ref_v, rgrads, "unchunked")
    scan = m._nonfinite_scan
    for panels_per_chunk in (1, 2):
        calls = []

        def counted(*a, _n=panels_per_chunk, **kw):
            calls.append(_n)
            return scan(*a, max_cells=_n * c.panel_rows * c.D, **kw)
        monkeypatch.setattr(m, "_nonfinite_scan", counted)
        parts, grads = check_rule(c, m, batch, params, ref_v, rgrads, f"{panels_per_chunk} panel(s) per chunk")
        assert calls, "the scan did not run"
        np.testing.assert_allclose(parts["x"].cpu().numpy(), whole["x"].cpu().numpy(), rtol=1e-12)
        for k in gwhole:
            assert float((grads[k] - gwhole[k]).abs().max()) <= 1e-6 * float(gwhole[k].abs().max()), k
    n_panels = -(-(RC.rows_of(c).stop - RC.rows_of(c).start) // c.panel_rows)
    assert n_panels >= 6 and c.expect["panel"] not in (0, n_panels - 1)


@gpu
@pytest.mark.parametrize("case", [RC.SPLIT_LOW, RC.SPLIT_HIGH], ids=lambda c: c.name)
def test_rule_with_column_split_accumulators(case):
    """enable_column_split on one device: the patch adds to the half (Dh, hfs) that holds the minimum's
    column, and the gA' chain to the half of every stored column of its row."""
    c, cfg, x, xb, params, ref_v, rgrads = _reference(case.name)
    m = build_model(cfg, c.panel_rows)
    assert m.enable_column_split(64) == 64
    check_rule(c, m, {"counts": x}, params, ref_v, rgrads)


@gpu
@pytest.mark.parametrize("case", RC.DETERMINISTIC, ids=lambda c: c.name)
def test_rule_in_deterministic_mode_is_bit_reproducible(case):
    c, m, batch, params, ref_v, rgrads = _run(case, deterministic=True)
    runs = []
    for rep in range(2):
        parts, grads = check_rule(c, m, batch, params, ref_v, rgrads, f"run {rep}")
        torch.cuda.synchronize()
        runs.append(({k: v.clone() for k, v in parts.items()}, {k: v.clone() for k, v in grads.items()}))
    assert_same_bits(runs[0], runs[1])
