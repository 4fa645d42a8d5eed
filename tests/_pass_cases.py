"""The matrices of the row-pass and column-pass tests that more than one file uses: tests/test_gpu_col_fetch.py and
tests/test_gpu_row_prefetch.py build their cases on them, and tools/col_fetch_bits.py and tools/row_prefetch_bits.py
dump the same problems' bits."""
import functools

import numpy as np
import scipy.sparse as sp
import torch

from _energy_check import sparse_reference
from _problems import _config, _counts, _csr

# ---- column pass: lists around the fetch and segment boundaries (col_pass.hip) ----------------------------------
R, LIST_D = 320, 24                                   # rows of a panel, columns of the list problems


def _fe(K):
    """Entries per fetch and lane group of the packed lists at latent dimension K."""
    kp = 4 * -(-K // 4)
    return (8 if kp <= 32 else 4) * (kp // 4)


def _list_lengths(K):
    fe = _fe(K)
    return sorted({0, 1, fe - 1, fe, fe + 1, 2 * fe - 1, 2 * fe, 2 * fe + 1, 255, 256, 257})


def _list_matrix(K, seed):
    """Two panels of R rows.  Panel 0 is ordinary; panel 1 holds nothing but the lists of _list_lengths(K) in the
    LAST columns, ascending: the list of 257 entries (two segments of SEGMENT_ENTRIES = 256: 256 + 1) is the last
    list of the panel-CSC arrays, so its fetches run into the padding.  Panel 1 has 10 non-empty lists = 11 work
    items: no multiple of the 64, 32, 16, 8 or 4 items of a wave, so its last wave has lane groups without an item."""
    rng = np.random.default_rng(seed)
    x = np.zeros((2 * R, LIST_D))
    x[:R] = (rng.random((R, LIST_D)) < 0.05) * (1 + rng.poisson(1.5, size=(R, LIST_D)))
    L = _list_lengths(K)
    for j, n in enumerate(L):
        rows = R + np.sort(rng.choice(R, size=n, replace=False))
        x[rows, LIST_D - len(L) + j] = 1 + rng.poisson(1.5, size=n)
    return x


@functools.lru_cache(maxsize=None)
def _list_case(K):
    X = sp.csr_matrix(_list_matrix(K, 800 + K))
    cfg, params = _config(X, K, 810 + K)
    return cfg, X, params, sparse_reference(cfg, X, params)


def _whole_lists(sc):
    """The work items of a production shape: a batch as small as these is cut into segments of 16 entries, so
    that it offers a few thousand items; the shapes the pass is built for (C3: 1M x 20k) reach SEGMENT_ENTRIES =
    256, where a list of up to 256 entries is ONE item and runs the fetch loop over its whole length.  Cut this
    batch's lists the same way."""
    from spmf_amd.sparse import SEGMENT_ENTRIES
    ptr = sc.pc_ptr.view(sc.n_panels, sc.n_cols + 1).to(torch.int64)
    sc._build_items((ptr[:, 1:] - ptr[:, :-1]).reshape(-1), ptr[:, :-1].reshape(-1), seg=SEGMENT_ENTRIES)
    sc.__dict__.pop("_hp", None)
    assert not sc._struct_cache
    return sc


def _packed(X, panel_rows=R):
    sc = _whole_lists(_counts(X, panel_rows))
    assert sc.pc_ent is not None and sc.pc_pad >= 7
    return sc


# ---- row pass: row lengths around the warm-up's windows (row_pass.hip issue_next) -------------------------------
# empty rows first, last and in runs; every window boundary (31 ... 33, 63 ... 65, 127 ... 129); a 129- and a 300-entry
# row directly before and after short ones, and next to each other
LENGTHS = [0, 0, 1, 31, 32, 33, 0, 63, 64, 65, 129, 127, 300, 128, 1, 129, 300, 0, 0, 0, 33, 300, 129, 64, 0, 31, 128,
           65, 127, 63, 32, 1, 0]


@functools.lru_cache(maxsize=None)
def _mixed_lengths(B=len(LENGTHS)):
    """The lengths above, tiled to B rows of 320 columns (the last row is empty whenever B is a multiple of their
    number)."""
    return _csr([LENGTHS[b % len(LENGTHS)] for b in range(B)], 320, np.random.default_rng(9001))


def _fractional(X):
    X = X.copy()
    X.data[5] = 2.5                         # one non-integer value: the canonical col / val arrays
    return X
