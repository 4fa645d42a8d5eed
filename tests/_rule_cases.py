"""Problems for the non-finite replacement rule (poisson.py:606-616) at real shapes: batches with a
known set of stored rate-0 cells per draw, and -- where a case needs the minimum's cell at a given
place -- one deep cell that holds the minimum over the finite cells.

Construction of a planted set (draw s, rows R, columns C):
    u[s, C, :] = 0 and w[s, 0, C] = 0    the columns of C feed nothing into z and have phi = 0
    x[R, :] = 0, then x[R, C] > 0        the rows of R store exactly the columns of C
so z_R = 0 in draw s and exactly |R| * |C| stored cells have rate 0 there.  No column of v is zeroed
and no row is left empty: an UNSTORED rate-0 cell is 0 * log 0 and makes fp64 autograd NaN.

With these parameters the smallest log-pmf of a batch belongs to the cell with the LARGEST rate (-rate
dominates x log r - lgamma(x+1)).  A deep cell (s, b, d, count[, fill]) puts it where a case needs it:
row b's counts times 4 (optionally after storing a fraction ``fill`` of its columns, for a long row),
so z_b is the largest encoding; x[b, d] = count; v[s, :, d] and w[s, 0, d] times 8 (exact in fp32), so
column d of draw s alone has the largest decoder row.
"""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from oracle import spmf_oracle as O

T = torch.as_tensor


@dataclass
class RuleCase:
    name: str
    B: int
    D: int
    K: int
    S: int
    seed: int
    density: float
    plants: dict                      # draw -> (rows, columns); negative rows count from B
    logt: bool = False
    scale_rows: bool = True
    deep: tuple = None                # (draw, row, column, count[, fill])
    panel_rows: int = 64
    panels: tuple = None              # (p0, p1): the batch is this panel range of the resident matrix
    expect: dict = field(default_factory=dict)   # what the well-posedness test pins about the minimum


def build(c: RuleCase):
    """-> (cfg, x, params) of the WHOLE resident matrix (a minibatch case slices rows itself)."""
    rng = np.random.default_rng(c.seed)
    B, D, K, S = c.B, c.D, c.K, c.S
    mask = rng.random((B, D)) < c.density
    x = (mask * (1 + rng.poisson(2.0, size=(B, D)))).astype(np.float64)
    cfg = O.OracleConfig(latent_dim=K, feature_dim=D, scale_rows=c.scale_rows, log_transform=c.logt,
                         u_tau_scale=1.0 / math.sqrt(B * D))
    cfg.eta_i = T(rng.uniform(0.5, 3.0, size=(1, D)))
    cfg.xi_u_global = float(rng.uniform(2.0, 6.0))
    params = O.random_params(cfg, S, c.seed + 1, fp32_exact=True)
    for s, (rows, cols) in c.plants.items():
        rows = [r % B for r in rows]
        params["u"][s, cols, :] = 0.0
        params["w"][s, 0, cols] = 0.0
        x[rows, :] = 0.0
        for r in rows:
            x[r, cols] = 1 + rng.poisson(2.0, size=len(cols))
    # every other row keeps z > 0 in every draw: it stores at least one column outside the planted ones
    planted_cols = sorted({d for _, cols in c.plants.values() for d in cols})
    planted_rows = sorted({r % B for rows, _ in c.plants.values() for r in rows})
    free = np.setdiff1d(np.arange(D), planted_cols)
    lone = np.setdiff1d(np.flatnonzero((x[:, free] > 0).sum(1) == 0), planted_rows)
    x[lone, free[lone % len(free)]] = 1.0
    if c.deep is not None:
        s, b, d, count = c.deep[:4]
        b %= B
        if len(c.deep) > 4:
            fill = rng.random(D) < c.deep[4]
            x[b, fill] = 1 + rng.poisson(2.0, size=int(fill.sum()))
        x[b, :] *= 4.0
        x[b, d] = float(count)
        params["v"][s, :, d] *= 8.0
        params["w"][s, 0, d] *= 8.0
    if c.logt:
        # exponents at or below 8 (tests/test_gpu_parity.py test_row_lengths_around_the_chunk_boundaries)
        z = O.encode(cfg, T(x), T(params["u"]), T(params["s"]))
        top = float((torch.matmul(z, T(params["v"])) * cfg.eta_i).max())
        params["v"] = (params["v"] * (7.99 / top)).astype(np.float32).astype(np.float64)
    return cfg, x, params


def rows_of(c: RuleCase):
    """Row slice of the resident matrix that the case's batch covers."""
    if c.panels is None:
        return slice(0, c.B)
    return slice(c.panels[0] * c.panel_rows, min(c.panels[1] * c.panel_rows, c.B))


def planted_counts(c: RuleCase):
    """Expected non-finite stored cells per draw inside the batch's rows."""
    sl = rows_of(c)
    out = [0.0] * c.S
    for s, (rows, cols) in c.plants.items():
        out[s] = float(sum(sl.start <= r % c.B < sl.stop for r in rows) * len(cols))
    return out


def minimum_of(cfg, x, params):
    """The oracle's finite cells: (ll [S,B,D], bad mask, (s, b, d) of the minimum, relative gap to
    the second smallest)."""
    out = O.log_likelihood_components(cfg, T(x), T(params["s"]), T(params["u"]), T(params["v"]),
                                      T(params["w"]))
    ll, rate = out["log_likelihood"].numpy(), out["rate"].numpy()
    bad = ~np.isfinite(ll)
    flat = np.where(bad, np.inf, ll).reshape(-1)
    i0, i1 = np.argpartition(flat, 1)[:2]
    if flat[i1] < flat[i0]:
        i0, i1 = i1, i0
    gap = (flat[i1] - flat[i0]) / abs(flat[i0])
    return ll, rate, bad, np.unravel_index(i0, ll.shape), float(gap)


# ---------------------------------------------------------------------------------------------
# The cases.  ``expect`` is asserted by the well-posedness test (CPU, oracle only):
#   draw      the draw that holds the minimum
#   row_nnz   lower bound on the stored entries of the minimum's row
#   col_lt / col_ge   the minimum's column is below / at or above this (column-split halves)
#   panel     the minimum's row lies in this panel of the batch
# ---------------------------------------------------------------------------------------------
_R = [3, 64, 65, -1]
_C = [7, 70, 140]

CASES = [
    # seed-chosen minima (no deep cell): the shapes of the issue's probe table
    RuleCase("k16_s3_min_in_draw1", 300, 150, 16, 3, 900 + 300 + 16, 0.25,
             {1: (_R, _C), 2: ([10, 200], [5, 99])}, expect={"draw": 1}),
    RuleCase("k100_min_in_draw0_bad_in_draw1", 520, 200, 100, 2, 900 + 520 + 100, 0.12,
             {1: (_R, _C)}, expect={"draw": 0}),
    RuleCase("k40_logt", 300, 150, 40, 2, 900 + 300 + 40, 0.25, {1: (_R, _C)}, logt=True,
             expect={"draw": 1}),
    RuleCase("k200_long_row", 70, 330, 200, 2, 900 + 70 + 200, 0.35, {1: ([3, 64, 65, -1], _C)},
             panel_rows=32, expect={"row_nnz": 65}),
    # placed minima
    RuleCase("k3_no_row_scale", 130, 90, 3, 3, 11, 0.3, {0: ([0, 129], [1, 64]), 2: ([50], [88])},
             scale_rows=False, deep=(1, 77, 65, 3), panel_rows=16, expect={"draw": 1}),
    RuleCase("k64_logt_no_row_scale_long_row", 90, 300, 64, 2, 12, 0.5, {0: (_R, _C)}, logt=True,
             scale_rows=False, deep=(1, 40, 250, 5, 0.7), panel_rows=32, expect={"draw": 1, "row_nnz": 65}),
    RuleCase("k16_long_row_last_draw", 200, 330, 16, 3, 13, 0.6, {0: (_R, _C), 1: ([100], [0, 329])},
             deep=(2, 150, 300, 0, 0.8), expect={"draw": 2, "row_nnz": 150}),
]

# the chunked scan: panel_rows 32 -> ten panels; the planted rows lie in panels 0, 2 and 9, the
# minimum's row in panel 5
CHUNKED = RuleCase("chunked", 300, 150, 16, 3, 21, 0.25, {0: (_R, _C), 2: ([70, 290], [5, 99])},
                   deep=(1, 5 * 32 + 9, 101, 3), panel_rows=32, expect={"draw": 1, "panel": 5})
CHUNKED_LOGT = RuleCase("chunked_logt", 300, 150, 40, 2, 22, 0.25, {1: (_R, _C)}, logt=True,
                        deep=(0, 5 * 32 + 9, 101, 0), panel_rows=32, expect={"draw": 0, "panel": 5})

# a panel range with p0 > 0 (rows 64..255 of 300); one planted row lies outside the batch
MINIBATCH = RuleCase("minibatch", 300, 150, 16, 3, 23, 0.25, {0: ([3, 64, 65, 254], _C), 2: ([100, 290], [5, 99])},
                     deep=(1, 200, 20, 3), panel_rows=32, panels=(2, 8), expect={"draw": 1, "panel": 4})
MINIBATCH_WIDE = RuleCase("minibatch_k100", 200, 150, 100, 2, 24, 0.25, {1: ([10, 64, 65, 150], _C)},
                          deep=(0, 130, 20, 2), panel_rows=32, panels=(1, 6), expect={"draw": 0, "panel": 3})

# column split at Dh = 64 of D = 150 (S = 1: the split flow is a single-draw flow)
SPLIT_LOW = RuleCase("split_min_in_lower_half", 300, 150, 16, 1, 25, 0.25, {0: (_R, _C)},
                     deep=(0, 120, 20, 3), expect={"col_lt": 64, "draw": 0})
SPLIT_HIGH = RuleCase("split_min_in_upper_half", 300, 150, 100, 1, 26, 0.25, {0: (_R, _C)},
                      deep=(0, 120, 101, 0), expect={"col_ge": 64, "draw": 0})

# deterministic mode (Poisson / linear, K <= 64)
DETERMINISTIC = [
    RuleCase("det_k16", 300, 150, 16, 3, 27, 0.25, {0: (_R, _C), 2: ([10, 200], [5, 99])},
             deep=(1, 120, 101, 3), expect={"draw": 1}),
    RuleCase("det_k64_long_row", 200, 330, 64, 2, 28, 0.6, {0: (_R, _C)},
             deep=(1, 150, 300, 2, 0.8), expect={"draw": 1, "row_nnz": 150}),
]

# more than 2048 blocks of 1024 cells: the reductions' grid stride loops (9000 x 300 = 2.7e6 cells)
MANY_CELLS = RuleCase("many_cells", 9000, 300, 8, 1, 29, 0.05, {0: ([3, 64, 65, 4500, -1], [7, 70, 140, 299])},
                      deep=(0, 8000, 250, 3), panel_rows=1024, expect={"draw": 0, "panel": 7})

# B > 262 140 with five columns: one dense_ll call of the scan covers every row
TALL = RuleCase("tall_narrow", 270000, 5, 2, 1, 30, 0.6, {0: ([3, 64, 65, 140000, -1], [1])},
                panel_rows=4096, expect={"draw": 0})

# the shape of test_draws_in_turn_on_a_batch_too_big_for_one_launch_per_kernel (tests/test_gpu_widek.py)
BACK_TO_BACK = RuleCase("draws_in_turn", 2100, 1700, 128, 2, 31, 0.01, {0: ([3, 64, 65, -1], [7, 70, 1400]),
                        1: ([1100], [900])}, deep=(1, 2000, 1500, 3, 0.05), panel_rows=1024,
                        expect={"draw": 1, "panel": 1})

ALL = CASES + [CHUNKED, CHUNKED_LOGT, MINIBATCH, MINIBATCH_WIDE, SPLIT_LOW, SPLIT_HIGH] + DETERMINISTIC + \
    [MANY_CELLS, TALL, BACK_TO_BACK]
