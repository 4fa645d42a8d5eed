"""References and bars of the GPU tests of energy_and_grads.  The contract (north_star): 1e-5 relative, fp32
kernels.  Parts are compared at rtol = atol = 1e-5; gradients ENTRY by entry against 1e-5 of the sum of the absolute
contributions to that entry (tests/_gradcheck.py, oracle.energy_grad_scales): entries of a sparse gradient cancel
to ~0, so the yardstick is what was added up."""
import numpy as np
import torch

import _rule_cases as RC
from oracle import spmf_oracle as O
from oracle import sparse_exact as SE
from _chunked_oracle import data_term as dense_data_term, prior_scales
from _gradcheck import assert_grads_entrywise

RTOL = 1e-5
MIN_GAP = 1e-3          # fp32 cells must pick the fp64 argmin: relative gap to the runner-up


def assert_close_parts(got, ref, rtol=RTOL, tag=""):
    for k in ref:
        g = got[k].detach().cpu().numpy()
        r = ref[k].numpy()
        np.testing.assert_allclose(g, r, rtol=rtol, atol=rtol, err_msg=f"{tag} part {k}")


def assert_close_grads(got, ref, scales, rtol=RTOL, tag=""):
    """Entry-wise: |hip - oracle| <= rtol * sum of |contributions| to that entry."""
    assert_grads_entrywise(got, ref, scales, rtol, tag)


def check_dense_oracle(model, cfg, x, params, batch=None, tag=""):
    """The standard comparison with the dense fp64 oracle on ``x``: no non-finite cell, every part and every
    gradient entry at the contract.  ``batch``: what the model is given where that is not {"counts": x} (a
    SparseCounts of x, a panel range whose rows x holds).  -> (parts, grads) of the model."""
    pref, gref, _ = O.energy_and_grads(cfg, x, params)
    parts, grads, nnf = model.energy_and_grads({"counts": x} if batch is None else batch, params)
    assert float(nnf.sum()) == 0, tag
    assert_close_parts(parts, pref, tag=tag)
    assert_close_grads(grads, gref, O.energy_grad_scales(cfg, x, params), tag=tag)
    return parts, grads


def sparse_reference(cfg, X, params, s=0, chunk=8192):
    """(sparse-exact data term, total gradients of the 12 variables, their entry-wise yardsticks) of draw s: the
    fp64 port of the linear decoder's passes (oracle/sparse_exact.py); yardstick: the dense oracle in row chunks."""
    one = {k: np.asarray(v[s], dtype=np.float64) for k, v in params.items()}
    eta = cfg.eta_i.numpy().reshape(-1)
    ref = SE.data_term(X, eta, float(cfg.xi_u_global), cfg.scale_rows, one["u"], one["v"], one["w"], one["s"])
    assert ref["n_nonfinite"] == 0
    _, pg = SE.prior_term(one, cfg.u_tau_scale, cfg.s_tau_scale,
                          cfg.symmetry_breaking_decay ** np.arange(cfg.latent_dim))
    grads = {k: pg[k] + ref["grads"].get(k, 0.0) for k in pg}
    p64 = {k: np.asarray(v[s:s + 1], dtype=np.float64) for k, v in params.items()}
    dense = dense_data_term(cfg, X, p64, chunk=chunk, scales=True)
    psc = prior_scales(cfg, p64)
    scales = {k: psc[k][0] + (dense["scales"][k][0] if k in dense["scales"] else 0.0) for k in pg}
    return ref, grads, scales


def check_sparse(cfg, X, params, batch, model, tag, ref=None, chunk=8192):
    """One evaluation against the sparse-exact reference, draw by draw: 'x' and 'z' at 1e-5 (rtol and atol), the
    gradients entry by entry at 1e-5 of their yardsticks.  ``ref``: the reference of a single-draw problem, where
    several evaluations share it.  -> (parts, grads) of the model."""
    parts, grads, nnf = model.energy_and_grads(batch, params)
    assert float(nnf.sum()) == 0, tag
    S = next(iter(params.values())).shape[0]
    assert ref is None or S == 1
    for s in range(S):
        data, grads_ref, scales = sparse_reference(cfg, X, params, s, chunk) if ref is None else ref
        for k in ("x", "z"):
            got = float(parts[k][s])
            print(tag, "draw", s, k, got, data[k])
            np.testing.assert_allclose(got, data[k], rtol=RTOL, atol=RTOL, err_msg=f"{tag} draw {s} part {k}")
        assert_grads_entrywise({k: v[s] for k, v in grads.items()}, grads_ref, scales, RTOL, f"{tag} draw {s}")
    return parts, grads


def assert_same_bits(first, second):
    """Two (parts, grads) of one deterministic-mode model on one batch: equal bit for bit."""
    for a, b, what in zip(first, second, ("part", "grad")):
        for k in a:
            assert torch.equal(a[k], b[k]), (what, k)


def check_rule(c, m, batch, params, ref_v, rgrads, tag=""):
    """The non-finite rule on one evaluation of the rule case ``c`` (tests/_rule_cases.py): the planted counts per
    draw, values against the literal oracle ``ref_v``, gradients against fp64 autograd through _rule_energy
    (``rgrads``) at 1e-5 of each variable's largest entry, and the class surface."""
    parts, grads, nnf = m.energy_and_grads(batch, params, nonfinite="rule")
    assert nnf.cpu().tolist() == RC.planted_counts(c), tag
    for k, r in ref_v.items():
        np.testing.assert_allclose(parts[k].cpu().numpy(), r.numpy(), rtol=1e-5, err_msg=f"{tag} {k}")
    for k, r in rgrads.items():
        g = grads[k].cpu().double().numpy().reshape(r.shape)
        assert np.isfinite(g).all(), (tag, k)
        err = np.abs(g - r).max()
        print(f"{c.name} {tag} grad {k}: max err {err:.3e}, bar {1e-5 * np.abs(r).max():.3e}")
        assert err <= 1e-5 * np.abs(r).max(), (tag, k, err, np.abs(r).max())
    got = m.unormalized_log_prob_parts(batch, **params)
    np.testing.assert_allclose(got["x"].cpu().numpy(), ref_v["x"].numpy(), rtol=1e-5, err_msg=tag)
    return parts, grads
