"""The streaming posterior queries of the model classes: ``StreamingQueries`` is the mixin that gives
PoissonFactorization (and through it the Bernoulli and mixed classes) waic_streaming, top_k, score_cells,
rank_cells, predict, top_rows, group_means, set_scores, embed, knn, neighbors, kmeans, cluster, silhouette,
fuzzy_graph, graph_layout, umap, graph_transform, umap_transform, spectral and spectral_cluster.

Every draw-stage query is the same three pieces around its own kernel (include/spmf_hip.h, csrc/api_stream.hip "the
draw stage"): ``_Draws``, the checked draws and the one place a library call is spelled; a driver that walks
the batches and row chunks (``_stream_rows`` for [rows, width] outputs, ``_stream_cells`` for a cell list);
and the check of the query's own arguments, which comes first.  A new query is one method here, one row in
tests/_stream_cases.py's ENTRIES and its own error cases.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._lib import VAR_ORDER
from .sparse import SparseCounts


def _is_one_batch(data):
    """``data`` is ONE batch (a dict, counts or an array), not an iterable of batches or a factory."""
    return not callable(data) and (isinstance(data, (dict, SparseCounts)) or hasattr(data, "shape"))


def _batches(data):
    """``data`` -- one batch, an iterable of batches or a data-factory callable -- as an iterable of batches."""
    if callable(data):
        return data()
    return (data,) if _is_one_batch(data) else data


def _vector(name, what, t, integer=True):
    """``t`` (numpy, torch or a sequence) as a 1-D tensor; with ``integer`` float and bool are refused."""
    if not isinstance(t, torch.Tensor):
        t = np.asarray(t)
        if t.size == 0 and integer:                 # [] has no dtype of its own
            t = t.astype(np.int64)
        t = torch.as_tensor(t)
    if t.dim() != 1:
        raise ValueError(f"{name}: {what} must be 1-D, got shape {tuple(t.shape)}")
    if integer and (t.dtype.is_floating_point or t.dtype == torch.bool):
        raise ValueError(f"{name}: {what} must hold integers, got {t.dtype}")
    return t


def fold_top_rows(rows, scores, new_rows, new_scores, offset):
    """The running best k of ``top_rows`` with one more row chunk: ``rows`` int64 / ``scores`` float32 [C, k] are
    the best so far (padding: row -1 / score -inf at the tail), ``new_rows`` int32 / ``new_scores`` [C, k] the
    chunk's result with rows relative to the chunk's first row, global row ``offset``.  Chunks arrive in ascending
    row order and each is ordered by (score descending, row ascending), so a stable sort of [running | new] by
    score keeps equal scores in ascending row order and the padding at the tail.  -> (rows, scores)."""
    k = scores.shape[1]
    new_rows = new_rows.to(torch.int64)
    both_r = torch.cat([rows, torch.where(new_rows >= 0, new_rows + int(offset), new_rows)], 1)
    both_s = torch.cat([scores, new_scores], 1)
    both_s, order = torch.sort(both_s, dim=1, descending=True, stable=True)
    return both_r.gather(1, order)[:, :k].contiguous(), both_s[:, :k].contiguous()


class _Scratch:
    """The grow-only device scratch of one streaming call."""

    def __init__(self, device):
        self.device, self.buf = device, None

    def fit(self, need_bytes):
        """-> (256-byte aligned pointer, usable bytes >= need_bytes).  An outgrown buffer is dropped
        before the larger one is allocated."""
        if self.buf is None or self.buf.numel() < need_bytes + 256:
            self.buf = None
            self.buf = torch.empty(need_bytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self.buf.data_ptr()) % 256
        return self.buf.data_ptr() + off, self.buf.numel() - off


class _Draws:
    """What one streaming call (``name``) hands the library's draw stage: ``S`` draws in ``pin``, the C-ABI's
    twelve parameter slots (it keeps the packed tensors it points into alive), ``eta``, the stream, the padded
    K ``KP``, the library and the context, and the call's scratch.  ``draws``: dict with 's','u','v','w' of
    shape [S,...] (None: ``surrogate_distribution.sample(nsamples)``), at least ``min_draws`` of them."""

    def __init__(self, model, name, draws, nsamples, min_draws, dense_alternative):
        if model._custom_codec is not None:
            raise NotImplementedError(f"{name}: custom encoder/decoder callables have no kernel "
                                      f"(use {dense_alternative}, which evaluates them densely)")
        why = " (the variance over the draws)" if min_draws > 1 else ""
        if draws is None:
            if int(nsamples) < min_draws:
                raise ValueError(f"{name} needs nsamples >= {min_draws}{why}")
            draws = model.surrogate_distribution.sample(int(nsamples))
        self.S, P = model._pack_params(draws, names=("s", "u", "v", "w"))
        if self.S < min_draws:
            raise ValueError(f"{name} needs at least {min_draws} draws{why}")
        self.lib, self.h = _lib.load(), model._handle()
        self.pin = _lib.PtrArray(*[P[n].data_ptr() if n in P else None for n in VAR_ORDER])
        self.pin.tensors = P
        self.eta = model._eta_device().data_ptr()
        self.stream = torch.cuda.current_stream(model.device).cuda_stream
        self.KP = int(self.lib.spmf_padded_k(self.h))
        self.scratch = _Scratch(model.device)

    def call(self, fn, size_fn, sub, *own, size_args=()):
        """The entry point ``fn`` on the batch struct ``sub`` with the entry's ``own`` arguments, in a scratch
        of ``size_fn(h, rows, S, *size_args)`` bytes."""
        need = getattr(self.lib, size_fn)(self.h, int(sub.n_rows), self.S, *size_args)
        _lib.check(self.h, getattr(self.lib, fn)(self.h, C.byref(sub), self.S, self.pin, self.eta, *own,
                                                 *self.scratch.fit(need), self.stream), fn)


class StreamingQueries:
    """The streaming calls of the model classes.  The host class supplies ``device``, ``feature_dim``,
    ``latent_dim``, ``surrogate_distribution``, ``_custom_codec`` and ``_batch`` / ``_batch_rows`` /
    ``_pack_params`` / ``_handle`` / ``_eta_device``."""

    _GROUP_OUT_CAP = 1 << 30          # bytes of one [S, G, C] fp64 output of group_means

    # ------------------------------------------------------------------
    # the drivers
    # ------------------------------------------------------------------
    def _row_chunks(self, data, row_bytes, max_rows):
        """The batch and row-chunk iteration of the streaming calls.
        ``data``: one batch (dict / counts), an iterable of batches or a data-factory callable; a
        ``{"counts": sc, "panels": (p0, p1)}`` batch is the rows of those panels.  Yields
        ``(n_rows, chunks)`` per batch; ``chunks`` yields ``(r0, sub)``: the batch struct of the
        next non-empty chunk of whole panels and its first row inside the batch.  A chunk has at
        most ``max_rows`` rows (default: 1 GiB of scratch at ``row_bytes`` per row)."""
        for batch in _batches(data):
            sc, cs = self._batch(batch)
            p0, p1 = sc.panel_range(batch.get("panels") if isinstance(batch, dict) else None)
            cap = int(max_rows) if max_rows else max(1, (1 << 30) // int(row_bytes))
            step = max(1, cap // sc.panel_rows)

            def chunks(sc=sc, p0=p0, p1=p1, step=step):
                for q0 in range(p0, p1, step):
                    sub = sc.struct(q0, min(q0 + step, p1))
                    if sub.n_rows == 0:
                        continue
                    yield (q0 - p0) * sc.panel_rows, sub
            yield int(cs.n_rows), chunks()

    def _stream_rows(self, data, row_bytes, max_rows, outputs, call):
        """[rows, width] outputs streamed over the batches and row chunks of ``data``.  ``outputs``: name ->
        (width, dtype, zero-filled or not), allocated whole per batch; ``call(sub, ptr)`` serves one chunk,
        ``ptr[name]`` being the output's address at the chunk's first row (``call`` None: nothing to compute,
        the outputs are allocated all the same).  -> name -> the rows of all batches: the tensor of a single
        batch itself, the concatenation of several, [0, width] for none."""
        parts = {n: [] for n in outputs}
        for n_rows, chunks in self._row_chunks(data, row_bytes, max_rows):
            out = {n: (torch.zeros if zero else torch.empty)(n_rows, width, dtype=dtype, device=self.device)
                   for n, (width, dtype, zero) in outputs.items()}
            for r0, sub in chunks if call is not None else ():
                call(sub, {n: t[r0:].data_ptr() for n, t in out.items()})
            for n, t in out.items():
                parts[n].append(t)
        return {n: p[0] if len(p) == 1 else torch.cat(p) if p else
                torch.empty(0, outputs[n][0], dtype=outputs[n][1], device=self.device) for n, p in parts.items()}

    def _stream_cells(self, dr, data, cells, row_bytes, max_rows, outputs, call):
        """Per-cell outputs of the checked list ``cells`` (``_cell_list``), which is consumed: sorted by row and
        cut into the segments of ``_cell_segments``.  ``outputs``: name -> (dtype, fill), the value of a cell no
        chunk serves; ``call(sub, n, row_ptr, col_ptr, val_ptr, ptr)`` serves the ``n`` cells of one segment,
        ``ptr[name]`` being the output's address at the segment's first cell.  -> name -> [N] in the caller's
        order.  Every intermediate, the scratch of ``dr`` included, is released as soon as it has been read, and the
        outputs are put back in order one at a time."""
        N = int(cells.rows.numel())
        rows, cols, vals, order, segments = self._cell_segments(data, cells.rows, cells.cols, cells.vals,
                                                                cells.n_rows, row_bytes, max_rows)
        cells.rows = cells.cols = cells.vals = None      # only the sorted copies live on
        out = {n: torch.full((N,), fill, dtype=dtype, device=self.device) for n, (dtype, fill) in outputs.items()}
        for sub, rel, lo, hi in segments:
            call(sub, hi - lo, rel.data_ptr(), cols[lo:hi].data_ptr(),
                 vals[lo:hi].data_ptr() if vals is not None else None,
                 {n: t[lo:hi].data_ptr() for n, t in out.items()})
        del rows, cols, vals, segments
        dr.scratch.buf = None
        res = {}
        for n in outputs:
            t = out.pop(n)
            res[n] = torch.empty_like(t).index_copy_(0, order, t)
            del t
        return res

    def _cell_list(self, name, data, rows, cols, values=None):
        """The cell list of ``score_cells`` / ``rank_cells`` (``name``), checked before any library call:
        ``data`` is one batch, ``rows`` / ``cols`` (/ ``values``) are 1-D and of equal length, the indices
        integers inside the batch.  -> rows, cols, vals (or None) on the device and n_rows, the rows of the
        batch, as the attributes of one object (``_stream_cells`` consumes it)."""
        if not _is_one_batch(data):
            raise ValueError(f"{name} takes ONE batch (a dict or counts), not an iterable or a factory")
        rows = _vector(name, "rows", rows).to(device=self.device)
        cols = _vector(name, "cols", cols).to(device=self.device)
        vals = None
        if values is not None:
            vals = _vector(name, "values", values, integer=False).to(device=self.device, dtype=torch.float32)
        N = int(rows.numel())
        if cols.numel() != N or (vals is not None and vals.numel() != N):
            raise ValueError(f"{name}: rows, cols and values must have equal length, got {N}, "
                             f"{int(cols.numel())}" + (f", {int(vals.numel())}" if vals is not None else ""))
        # the index check: one device-side min / max and one read-back, before any library call
        # (the batch's row count is read off its shape, not off the library's descriptor)
        n_rows = self._batch_rows(data)
        if n_rows > 2 ** 31 - 1:
            raise ValueError(f"{name}: a batch of {n_rows} rows is beyond the int32 row index of the list; "
                             "score it by panel ranges")
        if N:
            r_lo, r_hi, c_lo, c_hi = torch.stack(
                [t.to(torch.int64) for t in (*torch.aminmax(rows), *torch.aminmax(cols))]).tolist()
            if r_lo < 0 or r_hi >= n_rows:
                raise ValueError(f"{name}: rows must lie in [0, {n_rows}), got {r_lo} .. {r_hi}")
            if c_lo < 0 or c_hi >= self.feature_dim:
                raise ValueError(f"{name}: cols must lie in [0, {self.feature_dim}), got {c_lo} .. {c_hi}")
        return SimpleNamespace(rows=rows, cols=cols, vals=vals, n_rows=n_rows)

    def _cell_segments(self, data, rows, cols, vals, n_rows, row_bytes, max_rows):
        """The checked list of ``_cell_list`` cut along the row chunks of ``_row_chunks``: the cells sorted by
        row (stable), so that a chunk's cells are one contiguous segment.  -> (rows, cols, vals as int32 / int32 /
        float32 in sorted order, order, segments); ``order[i]`` is the caller's position of sorted cell i and
        ``segments`` lists ``(sub, rel, lo, hi)`` per chunk with cells: the chunk's batch struct, its cells' rows
        relative to the chunk's first row, and its slice of the sorted list."""
        (lib_rows, chunks), = self._row_chunks(data, row_bytes, max_rows)
        assert lib_rows == n_rows, (lib_rows, n_rows)
        N = int(rows.numel())
        rows, order = torch.sort(rows.to(torch.int32), stable=True)
        cols = cols.to(torch.int32)[order]
        if vals is not None:
            vals = vals[order]
        chunks = list(chunks)
        # a chunk's segment, from its first and its last row: both fit the int32 of the list
        first = torch.tensor([r0 for r0, _ in chunks] or [0], dtype=torch.int32, device=self.device)
        last = torch.tensor([r0 + int(sub.n_rows) - 1 for r0, sub in chunks] or [0], dtype=torch.int32,
                            device=self.device)
        edges = torch.stack([torch.searchsorted(rows, first), torch.searchsorted(rows, last, right=True)],
                            1).tolist() if N else []
        segments = [(sub, rows[lo:hi] - r0 if r0 else rows[lo:hi], lo, hi)
                    for (r0, sub), (lo, hi) in zip(chunks, edges) if hi > lo]
        return rows, cols, vals, order, segments

    def _column_list(self, name, cols):
        """The column list of ``predict`` (``name``), checked before any library call: None (all columns) or
        1-D integers inside [0, D), at most D of them, duplicates kept.  -> int32 on the device, or None."""
        if cols is None:
            return None
        D = self.feature_dim
        cols = _vector(name, "cols", cols)
        if cols.numel() > D:
            raise ValueError(f"{name}: cols lists {int(cols.numel())} columns, more than the {D} there are")
        if cols.numel():
            lo, hi = int(cols.min()), int(cols.max())
            if lo < 0 or hi >= D:
                raise ValueError(f"{name}: cols must lie in [0, {D}), got {lo} .. {hi}")
        return cols.to(device=self.device, dtype=torch.int32).contiguous()

    def _group_labels(self, name, data, labels, n_groups):
        """The labels of ``group_means`` (``name``), checked before any library call: 1-D integers in
        {-1, 0 .. n_groups - 1}, one per row of all batches.  The rows are counted off the batches' shapes: a
        factory is called once for the count and once for the run, a list is walked twice, and no batch is kept
        alive in between; a one-shot iterator cannot be walked twice, so its length is checked as its batches
        arrive (``counted`` False).  -> (int32 labels on the device, n_groups, counted)."""
        labels = _vector(name, "labels", labels)
        batches = _batches(data)
        counted = callable(data) or iter(batches) is not batches
        if counted:
            n_rows = sum(self._batch_rows(b) for b in batches)
            if int(labels.numel()) != n_rows:
                raise ValueError(f"{name}: labels must have one entry per row, got {int(labels.numel())} for "
                                 f"{n_rows} rows")
        n_groups = self._label_range(name, labels, n_groups, "n_groups")
        return labels.to(device=self.device, dtype=torch.int32).contiguous(), n_groups, counted

    @staticmethod
    def _label_range(name, labels, n_groups, what):
        """``n_groups`` (None: max(labels) + 1) with the 1-D integer ``labels`` checked to lie in
        {-1, 0 .. n_groups - 1} -> n_groups."""
        lo, hi = (int(labels.min()), int(labels.max())) if labels.numel() else (-1, -1)
        if n_groups is None:
            n_groups = hi + 1
        n_groups = int(n_groups)
        if n_groups < 1:
            raise ValueError(f"{name}: {what} must be at least 1, got {n_groups}")
        if lo < -1 or hi >= n_groups:
            raise ValueError(f"{name}: labels must lie in [-1, {n_groups}) (-1: no group), got {lo} .. {hi}")
        return n_groups

    # ------------------------------------------------------------------
    # the queries
    # ------------------------------------------------------------------
    def waic_streaming(self, data, nsamples=100, draws=None, row_scores=False, max_rows=None, col_scores=False):
        """``waic`` at any size: per-cell lppd_i / pwaic_i over the draws are formed in
        registers (csrc/waic.hip) and only their sums over the cells leave the kernel, so
        nothing of size S*B*D or B*D is written.

        ``data``: one batch (dict / counts), an iterable of batches or a data-factory
        callable; the sums are added across batches.  ``draws``: dict with 's','u','v','w' of
        shape [S,...] (default: ``surrogate_distribution.sample(nsamples)``), the same for every
        batch.  ``row_scores=True`` adds 'row_lppd' / 'row_pwaic', fp64 tensors concatenated
        over the batches.  ``max_rows`` caps the rows of one kernel call (whole panels), which
        bounds the scratch of the encoded rows (S * rows * K floats; default 1 GiB of them).

        Returns {'waic','se','lppd','pwaic','n','n_excluded'} (spmf_amd.waic.combine): a cell
        with a non-finite log-pmf in any draw (NaN count, rate 0 under a positive count) is
        left out of the sums and counted in 'n_excluded', where ``waic`` returns NaN / -inf.

        ``col_scores=True`` adds the same criterion per column -- which genes or items the model
        fits badly -- as device tensors of length D (spmf_amd.waic.combine_columns): 'col_n' and
        'col_n_excluded' (int64), 'col_lppd', 'col_pwaic', 'col_waic' = -2 (lppd - pwaic) and
        'col_se' (fp64; NaN where a column has at most one counted cell).  Columns ADD across
        batches and row chunks, where the row scores concatenate.  The exclusion rule holds per
        column: an excluded cell is left out of its column's sums and counted in its
        'col_n_excluded'; a NaN count makes every cell of its row non-finite, so it takes one
        cell out of EVERY column.  A column in which nothing is stored is scored like any other
        (all its counts are 0).  The column sums are fp64 atomics, as the totals are: equal to
        rounding from call to call, not bit-reproducible."""
        from . import waic as _waic
        dr = _Draws(self, "waic_streaming", draws, nsamples, 2, "waic()")
        sums = torch.zeros(_waic.NSUMS, dtype=torch.float64, device=self.device)
        if col_scores:
            cols = torch.zeros(self.feature_dim, _waic.NCOLSUMS, dtype=torch.float64, device=self.device)

            def call(sub, ptr):
                dr.call("spmf_waic_accumulate_cols", "spmf_waic_scratch_bytes", sub, sums.data_ptr(),
                        ptr.get("rows"), cols.data_ptr())
        else:
            def call(sub, ptr):
                dr.call("spmf_waic_accumulate", "spmf_waic_scratch_bytes", sub, sums.data_ptr(), ptr.get("rows"))
        rows = self._stream_rows(
            data, dr.S * dr.KP * 4, max_rows, {"rows": (2, torch.float64, True)} if row_scores else {}, call)
        out = _waic.combine(sums)
        if row_scores:
            out["row_lppd"], out["row_pwaic"] = rows["rows"][:, 0].contiguous(), rows["rows"][:, 1].contiguous()
        if col_scores:
            out.update(_waic.combine_columns(cols))
        return out

    def top_k(self, data, k=10, nsamples=32, draws=None, exclude_stored=True, max_rows=None):
        """Per row the ``k`` columns with the largest posterior predictive mean
        score_bd = mean_s m_s(b, d), m_s = the rate of draw s on a Poisson column and
        sigmoid(logit) on a Bernoulli one, without a [B,D] array: the scores are formed and
        selected in csrc/topk.hip and only [B,k] leaves the kernel.

        ``data``, ``draws`` and ``max_rows`` as in ``waic_streaming`` (``draws`` may hold a single
        draw, e.g. a point estimate from ``calibrated_expectations``; ``max_rows`` also bounds the
        bitmap of the stored cells, rows * D / 8 bytes).  ``exclude_stored``: cells the batch
        stores are no candidates.  A cell with a non-finite score is none either (a NaN count
        takes its whole row out).

        Returns {'columns': int32 [B,k], 'scores': float32 [B,k]} on the device, the rows of all
        batches concatenated: score descending, equal scores by ascending column, a row with
        fewer than k candidates padded with column -1 / score -inf.  Bit-reproducible."""
        k = int(k)
        if not 1 <= k <= 64:
            raise ValueError("top_k needs 1 <= k <= 64")
        dr = _Draws(self, "top_k", draws, nsamples, 1, "log_likelihood_components")
        flags = 1 if exclude_stored else 0
        return self._stream_rows(
            data, dr.S * dr.KP * 4 + (self.feature_dim + 31) // 32 * 4, max_rows,
            {"columns": (k, torch.int32, False), "scores": (k, torch.float32, False)},
            lambda sub, ptr: dr.call("spmf_topk_rows", "spmf_topk_scratch_bytes", sub, k, flags, ptr["columns"],
                                     ptr["scores"]))

    def score_cells(self, data, rows, cols, values=None, nsamples=32, draws=None, max_rows=None):
        """Held-out evaluation: the posterior predictive mean and, with ``values``, the log
        pointwise predictive density lppd_i = log mean_s p(value_i | theta_s) of the listed cells
        ``(rows[i], cols[i])``, without a [S,B,D] array (csrc/cells.hip).  'mean' is the score of
        ``top_k``: the mean over the draws of the rate on a Poisson column and of sigmoid(logit) on
        a Bernoulli one.

        ``data`` is ONE batch (dict / counts; ``{"counts": sc, "panels": (p0, p1)}`` is the rows
        of those panels).  The batch conditions the scores: its stored counts encode the rows, as
        everywhere else, and the listed values are only scored.  A held-out cell should therefore
        not also be stored in ``data`` with its true value, or it informs its own row's encoding;
        that is the caller's split and is not checked.  ``rows`` are relative to the first row of
        the batch (of the panel range); ``rows``, ``cols``, ``values`` are 1-D and of equal length,
        numpy or torch on any device, in any order, duplicates and zeros allowed.  ``draws`` /
        ``nsamples`` as in ``top_k`` (a single draw is allowed), ``max_rows`` as in
        ``waic_streaming``.

        Returns {'mean': float32 [N]} on the device in the caller's order and, with values,
        'lppd': float32 [N] plus the summary of ``spmf_amd.heldout.summarize``: 'lppd_sum',
        'lppd_mean', 'se', 'n', 'n_excluded'.  A cell with a non-finite log-pmf in any draw (NaN
        value, rate 0 under a positive value) has lppd NaN and is counted in 'n_excluded'; a NaN
        count in the batch makes every score of its row NaN.  A cell's scores do not depend on
        the order of the list or on ``max_rows``.  Bit-reproducible."""
        from . import heldout as _heldout
        cells = self._cell_list("score_cells", data, rows, cols, values)
        dr = _Draws(self, "score_cells", draws, nsamples, 1, "log_likelihood_components")
        nan = (torch.float32, float("nan"))
        out = self._stream_cells(
            dr, data, cells, dr.S * dr.KP * 4, max_rows,
            {"mean": nan, "lppd": nan} if values is not None else {"mean": nan},
            lambda sub, n, row, col, val, ptr: dr.call("spmf_score_cells", "spmf_cells_scratch_bytes", sub, n, row,
                                                       col, val, ptr["mean"], ptr.get("lppd")))
        if values is not None:
            out.update(_heldout.summarize(out["lppd"]))
        return out

    def rank_cells(self, data, rows, cols, k=(1, 5, 10, 20, 50), nsamples=32, draws=None, exclude_stored=True,
                   max_rows=None):
        """Held-out ranking: where the listed cells ``(rows[i], cols[i])`` land in the ranking of ``top_k``,
        without a [B,D] array (csrc/rank.hip).  Score, order and candidates are ``top_k``'s: the mean over the
        draws of the rate on a Poisson column and of sigmoid(logit) on a Bernoulli one; score descending, equal
        scores by ascending column; the candidates of a row are its columns with a finite score that, with
        ``exclude_stored``, the batch does not store.  A listed cell may or may not be a candidate itself.

        ``data`` is ONE batch and ``rows`` / ``cols`` are as in ``score_cells`` (any order, duplicates allowed,
        any number of cells per row); ``draws`` / ``nsamples`` as in ``top_k``, ``max_rows`` as in ``top_k``.
        ``k``: the cut-offs of the summary's hit rates (an int or a sequence of ints).

        Returns, on the device and in the caller's order, 'rank': int32 [N], the number of the row's other
        candidates that precede the cell (0 is the best; -1 for a non-finite score, e.g. a row with a NaN
        count), 'candidates': int32 [N], the number of the row's candidates beside the cell, and 'score':
        float32 [N], bit for bit the score ``top_k`` reports for that cell -- so for a cell that is not stored,
        ``rank < k`` exactly when ``top_k(k)["columns"][row, rank]`` is its column.  Plus the summary of
        ``spmf_amd.heldout.rank_summary``: 'n', 'n_excluded', 'hit_rate' {k: share}, 'mrr', 'auc'.  A cell's
        result does not depend on the order of the list, on its other cells or on ``max_rows``.
        Bit-reproducible.  Cost: about two ``top_k`` sweeps while no row lists more than 32 cells; the kernel
        serves 32 listed cells per row and round, so a row with n listed cells costs its block of 64 rows
        ceil(n / 32) such double sweeps (listing every column of a row is correct but slow)."""
        from . import heldout as _heldout
        cells = self._cell_list("rank_cells", data, rows, cols)
        ks = (int(k),) if isinstance(k, (int, np.integer)) else tuple(int(v) for v in k)
        if any(v < 1 for v in ks):
            raise ValueError(f"rank_cells: the cut-offs k must be >= 1, got {ks}")
        dr = _Draws(self, "rank_cells", draws, nsamples, 1, "log_likelihood_components")
        flags = 1 if exclude_stored else 0
        out = self._stream_cells(
            dr, data, cells, dr.S * dr.KP * 4 + (self.feature_dim + 31) // 32 * 4, max_rows,
            {"rank": (torch.int32, -1), "candidates": (torch.int32, 0), "score": (torch.float32, float("nan"))},
            lambda sub, n, row, col, val, ptr: dr.call("spmf_rank_cells", "spmf_rank_scratch_bytes", sub, n, row,
                                                       col, flags, ptr["rank"], ptr["candidates"], ptr["score"]))
        out.update(_heldout.rank_summary(out["rank"], out["candidates"], ks))
        return out

    def predict(self, data, cols=None, nsamples=32, draws=None, sd=False, p_nonzero=False, max_rows=None):
        """The reconstruction: the posterior predictive mean of every cell of the rows of ``data`` and the
        columns ``cols`` as a dense block, without a [S,B,D] array (csrc/panel.hip).  'mean' is the score of
        ``top_k`` / ``rank_cells``, bit for bit: the mean over the draws of m_s, the rate on a Poisson column
        and sigmoid(logit) on a Bernoulli one.

        ``data``, ``draws`` and ``max_rows`` as in ``top_k`` (``draws`` may hold a single draw); the rows of
        all batches are concatenated.  ``cols``: None (all D columns) or 1-D integers in [0, D), numpy or
        torch on any device, at most D of them, in any order, duplicates kept: output column j is column
        ``cols[j]``.  ``sd=True`` adds the unbiased standard deviation of m_s over the draws (at least two
        draws; Welford in draw order).  ``p_nonzero=True`` adds P(x > 0) under the predictive mixture:
        mean_s (1 - exp(-rate_s)) on a Poisson column, formed as -expm1(-rate_s) so that small rates keep
        their digits, and the mean itself on a Bernoulli column.

        Returns device tensors {'mean': float32 [B, C]} plus 'sd' and 'p_nonzero' when asked for and, with a
        list, 'columns': the int32 list as used.  Memory: every output is B * C * 4 bytes and is allocated
        whole -- bound it with the column list or, over the rows, with a ``{"counts": sc, "panels": (p0, p1)}``
        range per call; the scratch is bounded by ``max_rows`` as in ``top_k``.  A row with a NaN count is NaN.
        A value depends on its cell alone: not on the list, on the other outputs asked for or on
        ``max_rows``.  Bit-reproducible."""
        cols = self._column_list("predict", cols)
        dr = _Draws(self, "predict", draws, nsamples, 2 if sd else 1, "log_likelihood_components")
        n_cols = self.feature_dim if cols is None else int(cols.numel())
        cols_ptr = cols.data_ptr() if cols is not None else None
        names = ("mean",) + (("sd",) if sd else ()) + (("p_nonzero",) if p_nonzero else ())

        def call(sub, ptr):
            dr.call("spmf_predict_columns", "spmf_predict_scratch_bytes", sub, n_cols, cols_ptr, ptr["mean"],
                    ptr.get("sd"), ptr.get("p_nonzero"))
        res = self._stream_rows(data, dr.S * dr.KP * 4, max_rows, {n: (n_cols, torch.float32, False) for n in names},
                                call if n_cols else None)       # (an empty list has no pointer to pass)
        if cols is not None:
            res["columns"] = cols
        return res

    def top_rows(self, data, cols=None, k=10, nsamples=32, draws=None, exclude_stored=True, max_rows=None):
        """Per column the ``k`` rows with the largest posterior predictive mean -- the cells that most express a
        marker gene, the audience of an item -- without a [B, C] block (csrc/toprows.hip): ``top_k`` along the
        other axis.  The score of a cell is ``predict``'s 'mean', bit for bit: the mean over the draws of the rate
        on a Poisson column and of sigmoid(logit) on a Bernoulli one.

        ``data``, ``draws`` / ``nsamples`` and ``max_rows`` as in ``top_k`` (one batch, an iterable or a factory;
        ``draws`` may hold a single draw); the rows are numbered across all batches in arrival order, as
        ``predict`` concatenates them.  ``cols`` as in ``predict``: None (all D columns) or 1-D integers in
        [0, D), in any order, duplicates kept; output row j belongs to column ``cols[j]``.  ``exclude_stored``:
        a row that stores the column in its batch is no candidate for that column.  A row with a non-finite
        score is no candidate for any column (a NaN count takes its row out everywhere).

        Returns device tensors {'rows': int64 [C, k], 'scores': float32 [C, k]} and, with a list, 'columns': the
        int32 list as used.  Within a column: score descending, equal scores by ascending row; a column with
        fewer than k candidates is padded at the tail with row -1 / score -inf.  Every row chunk is selected in
        the kernel and folded into the running best k (``fold_top_rows``), so at most 2 * C * k candidates are
        alive.  The result does not depend on ``max_rows``, on how the rows are split into batches or on the other
        listed columns.  Bit-reproducible."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"top_rows: k must be an integer, got {k!r}")
        k = int(k)
        if not 1 <= k <= 64:
            raise ValueError(f"top_rows needs 1 <= k <= 64, got {k}")
        cols = self._column_list("top_rows", cols)
        dr = _Draws(self, "top_rows", draws, nsamples, 1, "predict")
        n_cols = self.feature_dim if cols is None else int(cols.numel())
        cols_ptr = cols.data_ptr() if cols is not None else None
        flags = 1 if exclude_stored else 0
        rows = torch.full((n_cols, k), -1, dtype=torch.int64, device=self.device)
        scores = torch.full((n_cols, k), float("-inf"), dtype=torch.float32, device=self.device)
        new_rows = torch.empty(n_cols, k, dtype=torch.int32, device=self.device)
        new_scores = torch.empty(n_cols, k, dtype=torch.float32, device=self.device)
        off = 0
        for n_rows, chunks in self._row_chunks(data, dr.S * dr.KP * 4 + (self.feature_dim + 31) // 32 * 4, max_rows):
            for r0, sub in chunks if n_cols else ():
                dr.call("spmf_toprows_columns", "spmf_toprows_scratch_bytes", sub, n_cols, cols_ptr, k, flags,
                        new_rows.data_ptr(), new_scores.data_ptr(), size_args=(n_cols,))
                rows, scores = fold_top_rows(rows, scores, new_rows, new_scores, off + r0)
            off += n_rows
        res = {"rows": rows, "scores": scores}
        if cols is not None:
            res["columns"] = cols
        return res

    def group_means(self, data, labels, n_groups=None, cols=None, nsamples=32, draws=None, p_nonzero=False,
                    max_rows=None):
        """The posterior predictive reduced over rows: per draw, the mean over the rows of every group of
        m_s(b, d) -- the cell of ``predict`` for draw s, the rate on a Poisson column and sigmoid(logit) on a
        Bernoulli one -- without a [rows, C] block per draw (csrc/groups.hip).  What a cluster, cell type or
        segment expresses, with the draws kept apart so that a non-linear contrast between groups
        (``spmf_amd.groups.contrast``: a log fold change) has a posterior of its own.

        ``data``, ``draws``, ``cols`` and ``max_rows`` as in ``predict``; batches are streamed, never held
        together (a factory is called twice, first for the row count alone; for a one-shot iterator the length
        of ``labels`` is checked batch by batch instead of up front).  ``labels``: 1-D integers, numpy or torch on any device, one per row of all batches in
        arrival order, in {-1, 0 .. n_groups - 1}; -1 is "no group".  ``n_groups`` defaults to
        max(labels) + 1.  ``p_nonzero=True`` adds the expected fraction of the group with x > 0 (the sum of
        ``predict``'s P(x > 0) terms per draw).

        Returns device tensors: 'draws' fp64 [S, G, C] (sum / count), 'mean' [G, C] and, with two draws or
        more, 'sd' [G, C] (unbiased) over the draws, 'count' int64 [G], 'sum' fp64 [S, G, C] (the raw sums:
        shards add up), with ``p_nonzero`` 'p_nonzero_draws' [S, G, C] / 'p_nonzero' [G, C] and their raw
        sums 'sum_nonzero', with a list 'columns'.  An empty group has NaN means and count 0.  A row with a NaN count makes its own group
        NaN and no other.  Every sum is fp64 from the first addition on, in an order fixed by the arguments:
        bit-reproducible; ``max_rows`` and the split into batches change the order of the fp64 additions
        only.  Memory: each [S, G, C] array is S * G * C * 8 bytes and at most 1 GiB -- bound it with
        ``cols``.  ``max_rows`` bounds the two copies of the encoded rows and the per-row part of the ordering;
        the scratch also holds 64 pad rows per group (S * 64 * G * K floats), which no row limit bounds."""
        labels, G, _ = self._group_labels("group_means", data, labels, n_groups)
        cols = self._column_list("group_means", cols)
        n_cols = self.feature_dim if cols is None else int(cols.numel())
        if draws is not None and self._custom_codec is None:
            n_draws = int(next(iter(draws.values())).shape[0])
        else:
            n_draws = int(nsamples)
        if n_draws * G * n_cols * 8 > self._GROUP_OUT_CAP:
            raise ValueError(f"group_means: an output of {n_draws} draws x {G} groups x {n_cols} columns is "
                             f"{n_draws * G * n_cols * 8} bytes, above the cap of {self._GROUP_OUT_CAP}: pass "
                             "fewer columns at a time with cols")
        dr = _Draws(self, "group_means", draws, nsamples, 1, "predict")
        S = dr.S
        total = torch.zeros(S, G, n_cols, dtype=torch.float64, device=self.device)
        nonzero = torch.zeros_like(total) if p_nonzero else None
        off = 0
        # per row: the encoded rows twice (arrival order, group order), rank and slot, its share of the chunk table
        row_bytes = 2 * S * dr.KP * 4 + 8 + (G + 1023) // 1024 * 4
        for n_rows, chunks in self._row_chunks(data, row_bytes, max_rows):
            if off + n_rows > int(labels.numel()):
                raise ValueError(f"group_means: labels must have one entry per row, got {int(labels.numel())} "
                                 f"for at least {off + n_rows} rows")
            for r0, sub in chunks if n_cols else ():
                dr.call("spmf_group_sums", "spmf_groups_scratch_bytes", sub, labels[off + r0:].data_ptr(), G, n_cols,
                        cols.data_ptr() if cols is not None else None, total.data_ptr(),
                        nonzero.data_ptr() if nonzero is not None else None, size_args=(G, n_cols))
            off += n_rows
        if off != int(labels.numel()):
            raise ValueError(f"group_means: labels must have one entry per row, got {int(labels.numel())} for "
                             f"{off} rows")
        count = torch.bincount(labels[labels >= 0].to(torch.int64), minlength=G)
        n = count.to(torch.float64).masked_fill(count == 0, float("nan"))[None, :, None]
        res = {"draws": total / n, "count": count, "sum": total}
        res["mean"] = res["draws"].mean(0)
        if S >= 2:
            res["sd"] = res["draws"].std(0, unbiased=True)
        if nonzero is not None:
            res["sum_nonzero"] = nonzero
            res["p_nonzero_draws"] = nonzero / n
            res["p_nonzero"] = res["p_nonzero_draws"].mean(0)
        if cols is not None:
            res["columns"] = cols
        return res

    def set_scores(self, data, sets, weights=None, nsamples=32, draws=None, sd=False, max_rows=None,
                   max_listed=None):
        """The posterior predictive reduced over columns: per row the weighted sum over each column set of
        m_s(b, d) -- the cell of ``predict`` for draw s, the rate on a Poisson column and sigmoid(logit) on a
        Bernoulli one -- averaged over the draws, without a [rows, columns] block (csrc/sets.hip).  A gene-set
        or signature score per cell, a category affinity per user, the expected row total (the set of all
        columns); with ``sd=True`` its posterior standard deviation, which a sum of ``predict``'s per-cell
        deviations cannot give.

        ``data``, ``draws`` and ``max_rows`` as in ``predict``; the rows of all batches are concatenated.
        ``sets``: a sequence of 1-D integer arrays (numpy / torch / lists) of columns in [0, D), in any order; a
        column listed twice counts twice, sets may overlap, a set may be empty.  ``weights``: None (all 1) or a
        sequence of as many float arrays, each as long as its set, finite; signed weights make a contrast of two
        signatures one set with a posterior sd of its own.  ``sd=True`` needs two draws.

        Returns device tensors {'mean': fp64 [B, G]} plus 'sd': fp64 [B, G] (unbiased, over the per-draw
        scores) when asked for, and 'sizes': int64 [G], the length of every list.  Every sum is fp64 from the
        first addition on (each fp32 cell and weight is converted first) and runs in an order fixed by the
        set's own list and the number of draws: a set's column has the same bits whatever the other sets, its
        position, ``max_rows`` or ``max_listed``.  An empty set scores 0 (sd 0); a row with a NaN count is NaN
        in every non-empty set.  Bit-reproducible.

        Memory and cost: the sets are served in runs of whole sets whose lists, each padded to whole 64-column
        blocks, stay within ``max_listed`` columns (default: 256 MiB of compacted decoding rows at S draws; a
        single larger set is a run of its own), and the rows in chunks of ``max_rows``.  The draw stage --
        the tables of the S draws and the encoding of the chunk's rows -- runs once per (row chunk, run): with
        many runs prefer a larger ``max_listed``."""
        from . import sets as _sets
        set_ptr, cols, wts = _sets.pack(sets, weights, self.feature_dim)
        dr = _Draws(self, "set_scores", draws, nsamples, 2 if sd else 1, "predict")
        G = len(set_ptr) - 1
        sizes = np.diff(set_ptr)
        padded = (sizes + 63) // 64 * 64
        cap = int(max_listed) if max_listed else max(64, (256 << 20) // (dr.S * dr.KP * 4) // 64 * 64)
        runs, g0, load = [], 0, 0           # (first set, end set, the run's own set_ptr on the host)
        for g in range(G + 1):
            if g == G or (g > g0 and load + int(padded[g]) > cap):
                if g > g0:
                    runs.append((g0, g, np.ascontiguousarray(set_ptr[g0:g + 1] - set_ptr[g0])))
                g0, load = g, 0
            if g < G:
                load += int(padded[g])
        cols = cols.to(self.device)
        wts = wts.to(self.device) if wts is not None else None
        names = ("mean", "sd") if sd else ("mean",)

        def call(sub, ptr):
            for a, b, run_ptr in runs:
                first = int(set_ptr[a])
                dr.call("spmf_set_scores", "spmf_sets_scratch_bytes", sub, b - a, run_ptr.ctypes.data,
                        cols.data_ptr() + 4 * first, wts.data_ptr() + 4 * first if wts is not None else None, G,
                        ptr["mean"] + 8 * a, ptr["sd"] + 8 * a if sd else None,
                        size_args=(b - a, run_ptr.ctypes.data))
        res = self._stream_rows(data, dr.S * dr.KP * 4, max_rows, {n: (G, torch.float64, False) for n in names},
                                call if G else None)
        res["sizes"] = torch.as_tensor(sizes, dtype=torch.int64, device=self.device)
        return res

    def embed(self, data, nsamples=32, draws=None, sd=False, max_rows=None):
        """The rows of ``data`` in the latent space, at any size: the posterior mean encoding
        e_b = (1/S) sum_s z_sb, where z_sb is what ``encode(x, u_s, s_s)`` returns for draw s (the
        draw stage's encode sweep; csrc/knn.hip reduces it over the draws, so [S,B,K] never leaves
        the scratch).

        ``data``, ``draws`` and ``max_rows`` as in ``waic_streaming`` (``draws`` may hold a single
        draw); the rows of all batches are concatenated.  Returns {'mean': float32 [N, latent_dim]}
        on the device and, with ``sd=True``, 'sd': the unbiased standard deviation over the draws
        (at least two draws).  fp32: the sum in draw order times 1/S, Welford in draw order for the
        deviation.  A row with a NaN count is NaN.  Bit-reproducible and independent of
        ``max_rows``."""
        dr = _Draws(self, "embed", draws, nsamples, 2 if sd else 1, "encode")
        return self._stream_rows(
            data, dr.S * dr.KP * 4, max_rows,
            {n: (self.latent_dim, torch.float32, False) for n in (("mean", "sd") if sd else ("mean",))},
            lambda sub, ptr: dr.call("spmf_embed_rows", "spmf_embed_scratch_bytes", sub, ptr["mean"], ptr.get("sd")))

    @staticmethod
    def _knn_args(name, k, metric):
        """k and the metric of ``knn`` / ``neighbors``, checked before any library call -> (k, flags)."""
        from . import neighbors as _neighbors
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"{name}: k must be an integer, got {k!r}")
        if not 1 <= int(k) <= 64:
            raise ValueError(f"{name} needs 1 <= k <= 64, got {k}")
        if metric not in _neighbors.METRICS:
            raise ValueError(f"{name}: metric must be one of {_neighbors.METRICS}, got {metric!r}")
        return int(k), 1 if metric == "cosine" else 0

    @staticmethod
    def _knn_rows(name, what, t):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: {what} must be a torch tensor, got {type(t).__name__}")
        if t.dim() != 2:
            raise ValueError(f"{name}: {what} must be 2-D [rows, width], got shape {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: {what} must be float32, got {t.dtype}")
        if not 1 <= t.shape[1] <= 256:
            raise ValueError(f"{name}: the width of {what} must be in 1..256, got {t.shape[1]}")
        return t

    def knn(self, points, k=15, queries=None, metric="euclidean", include_self=False):
        """The exact ``k`` nearest rows of ``points`` [Nr, Kx] for every row of ``queries`` [Nq, Kx]
        (default: ``points`` itself), without an [Nq, Nr] array (csrc/knn.hip).  Both are float32
        tensors on the model's device, 1 <= Kx <= 256 whatever the model's latent_dim, 1 <= k <= 64.
        ``metric``: 'euclidean' or 'cosine' (the distance 1 - cos).  Without ``queries`` (or with
        ``queries=points``) a row is no neighbour of its own unless ``include_self``.

        Returns {'indices': int32 [Nq,k], 'distances': float32 [Nq,k]} on the device: distance
        ascending, equal distances by ascending index, a query with fewer than k candidates padded
        with -1 / +inf at the tail.  A non-finite row of ``points`` is nobody's neighbour; a non-finite
        query (or a zero row under 'cosine') has none.  The selection runs on the matrix cores over
        centred (or unit) rows; the reported distances are recomputed from the rows as given
        (include/spmf_hip.h spmf_knn has the definition).  Bit-reproducible; a query's result does
        not depend on the other queries.  ``spmf_amd.neighbors.to_csr`` turns the result into the
        CSR arrays of a neighbour graph."""
        k, flags = self._knn_args("knn", k, metric)
        pts = self._knn_rows("knn", "points", points)
        same = queries is None or queries is points or (
            isinstance(queries, torch.Tensor) and queries.shape == points.shape and queries.dtype == points.dtype
            and queries.device == points.device and queries.data_ptr() == points.data_ptr()
            and queries.stride() == points.stride())
        qry = pts if same else self._knn_rows("knn", "queries", queries)
        if qry.shape[1] != pts.shape[1]:
            raise ValueError(f"knn: queries have width {qry.shape[1]}, points {pts.shape[1]}")
        if pts.shape[0] > 2 ** 31 - 1:
            raise ValueError(f"knn: {pts.shape[0]} points are beyond the int32 index of the result")
        dev = torch.device(self.device)
        for what, t in (("points", pts), ("queries", qry)):
            if t.device.type != "cuda" or (dev.index is not None and t.device != dev):
                raise ValueError(f"knn: {what} must be on the model's device {self.device}, got {t.device}")
        pts = pts.contiguous()
        qry = pts if same else qry.contiguous()
        nq, nr, width = int(qry.shape[0]), int(pts.shape[0]), int(pts.shape[1])
        lib, h = _lib.load(), self._handle()
        idx = torch.empty(nq, k, dtype=torch.int32, device=pts.device)
        dist = torch.empty(nq, k, dtype=torch.float32, device=pts.device)
        scratch = _Scratch(pts.device)
        _lib.check(h, lib.spmf_knn(
            h, qry.data_ptr(), nq, pts.data_ptr(), nr, width, k, flags, 0 if same and not include_self else -1,
            idx.data_ptr(), dist.data_ptr(), *scratch.fit(lib.spmf_knn_scratch_bytes(h, nq, nr, width)),
            torch.cuda.current_stream(pts.device).cuda_stream), "spmf_knn")
        return {"indices": idx, "distances": dist}

    def neighbors(self, data, k=15, query=None, metric="euclidean", include_self=False, nsamples=32, draws=None,
                  max_rows=None):
        """The neighbour graph of the rows of ``data`` in the model's latent space: ``embed`` on
        ``data`` -- and on ``query``, when given, with the SAME draws -- then ``knn`` on the posterior
        mean encodings.  Without ``query`` every row of ``data`` gets its k nearest other rows (itself
        too with ``include_self``); with ``query`` every row of ``query`` gets its k nearest rows of
        ``data``.  ``data`` / ``query``, ``nsamples`` / ``draws`` and ``max_rows`` as in ``embed``;
        ``k`` and ``metric`` as in ``knn``.

        Returns {'indices': int32 [Nq,k], 'distances': float32 [Nq,k]} on the device, bit for bit
        ``knn(embed(data, draws=draws)["mean"], k, ...)``."""
        self._knn_args("neighbors", k, metric)
        if not 1 <= self.latent_dim <= 256:
            raise ValueError(f"neighbors: latent_dim {self.latent_dim} is beyond the 256 columns of knn")
        if draws is None and self._custom_codec is None:
            if int(nsamples) < 1:
                raise ValueError("neighbors needs nsamples >= 1")
            draws = self.surrogate_distribution.sample(int(nsamples))      # once: data and query share them
        ref = self.embed(data, nsamples=nsamples, draws=draws, max_rows=max_rows)["mean"]
        if query is None:
            return self.knn(ref, k=k, metric=metric, include_self=include_self)
        qry = self.embed(query, nsamples=nsamples, draws=draws, max_rows=max_rows)["mean"]
        return self.knn(ref, k=k, queries=qry, metric=metric, include_self=True)

    def kmeans(self, points, n_clusters, init="k-means++", max_iter=100, seed=0):
        """Deterministic k-means (Lloyd's iteration) of the rows of ``points`` [N, Kx], a float32 tensor on the
        model's device with 1 <= Kx <= 256 whatever the model's latent_dim, into 1 <= ``n_clusters`` <= 65536
        clusters.  One library call per iteration (include/spmf_hip.h spmf_kmeans_step, csrc/kmeans.hip): the
        assignment is ``knn``'s -- the label of a row is, bit for bit,
        ``knn(centroids, k=min(4, G), queries=points)["indices"][:, 0]`` -- and the clusters' sums are fp64 in
        a fixed order, so two runs of an iteration give the same centroids.

        ``init``: 'k-means++' (``spmf_amd.cluster.init_plus_plus`` with ``seed``), 'first' (the first
        ``n_clusters`` finite rows) or a float32 [n_clusters, Kx] tensor on the device.  The loop: a step on
        the current centroids; stop when no label changed; else centroids = sums / counts in fp64 rounded to
        float32, an empty cluster keeping its centroid; at most ``max_iter`` steps.  One read-back of three
        numbers per iteration.

        Returns {'labels': int32 [N] (-1: a non-finite row), 'distances': float32 [N] (+inf beside -1),
        'centroids': float32 [G, Kx], 'counts': int64 [G]} on the device and 'inertia' (the sum of the squared
        distances), 'n_iter', 'converged', 'n_unassigned'.  Every output refers to the returned centroids, at
        ``max_iter`` too.  Bit-reproducible for a tensor or 'first' init; for 'k-means++' the same seed gives
        the same result on the same machine."""
        from . import cluster as _cluster
        G, max_iter = _cluster.check_args("kmeans", n_clusters, max_iter, init)
        pts = self._knn_rows("kmeans", "points", points)
        if isinstance(init, torch.Tensor):
            _cluster.check_init_tensor("kmeans", init, G, pts)
        if pts.shape[0] > 2 ** 31 - 64:
            raise ValueError(f"kmeans: {pts.shape[0]} points are beyond one call of the library")
        dev = torch.device(self.device)
        if pts.device.type != "cuda" or (dev.index is not None and pts.device != dev):
            raise ValueError(f"kmeans: points must be on the model's device {self.device}, got {pts.device}")
        pts = pts.contiguous()
        if isinstance(init, torch.Tensor):
            start = init
        elif init == "first":
            start = _cluster.init_first(pts, G)
        else:
            start = _cluster.init_plus_plus(pts, G, seed)
        return _cluster.lloyd(self._handle(), pts, start, max_iter)

    def silhouette(self, points, labels, n_clusters=None, metric="euclidean"):
        """The exact silhouette of the rows of ``points`` [N, Kx] under ``labels``: per row its mean distance to
        the other rows of its cluster (a), the smallest mean distance to the rows of another cluster (b, that
        cluster in 'nearest') and s = (b - a) / max(a, b); per cluster the mean of s; and their overall mean, the
        score that answers "how many clusters?" where ``kmeans``' inertia only falls.  One library call
        (include/spmf_hip.h spmf_silhouette has the definition, csrc/silhouette.hip): every pair of rows on the
        matrix cores, fp64 sums in a fixed order, no [N, N] or [N, G] array.

        ``points``: a float32 tensor on the model's device with 1 <= Kx <= 256 whatever the model's latent_dim.
        ``labels``: 1-D integers (numpy or torch on any device), one per row, in {-1, 0 .. n_clusters - 1}; -1 is
        "no cluster" (what ``kmeans`` gives a non-finite row).  ``n_clusters`` (at most 65536) defaults to
        max(labels) + 1.  ``metric``: 'euclidean' or 'cosine' (the distance 1 - cos).  A row with label -1 or a
        non-finite value (under 'cosine' a zero row too) is no member of any cluster: its outputs are NaN /
        nearest -1 and it changes no bit of any other row's result.

        Returns device tensors 'silhouette', 'a', 'b' (float32 [N]), 'nearest' (int32 [N]), 'cluster_mean'
        (fp64 [G], NaN for an empty cluster) and 'counts' (int64 [G], the members), and the host values 'score'
        (the sum of the clusters' fp64 sums of s over the number of members; NaN with fewer than two non-empty
        clusters) and 'n_scored' (the members).  A singleton cluster's row has s = 0.  Bit-reproducible.

        Cost and accuracy: N^2 pairs -- sample rows (``points[idx]``, ``labels[idx]``) where that is too many.
        Distances come from the fp32 expansion |x_i|^2 + |x_j|^2 - 2 <x_i, x_j> of centred (or unit) rows: the
        absolute error of one squared distance is about 2^-24 * KP * (|x'_i|^2 + |x'_j|^2), with KP the width
        rounded up to 4, 8, .., 256, so distances far below the rows' norms are coarse.  Separated clusters are
        scored to fp32 accuracy; a near-collinear cloud with large norms (an untrained model's embedding) is
        scored coarsely."""
        from . import neighbors as _neighbors
        pts = self._knn_rows("silhouette", "points", points)
        if metric not in _neighbors.METRICS:
            raise ValueError(f"silhouette: metric must be one of {_neighbors.METRICS}, got {metric!r}")
        if n_clusters is not None:
            if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)):
                raise ValueError(f"silhouette: n_clusters must be an integer, got {n_clusters!r}")
        labels = _vector("silhouette", "labels", labels)
        N, width = int(pts.shape[0]), int(pts.shape[1])
        if int(labels.numel()) != N:
            raise ValueError(f"silhouette: labels must have one entry per row, got {int(labels.numel())} for "
                             f"{N} rows")
        G = self._label_range("silhouette", labels, n_clusters, "n_clusters")
        if G > 65536:
            raise ValueError(f"silhouette: n_clusters must be at most 65536, got {G}")
        if N > 2 ** 31 - 64:
            raise ValueError(f"silhouette: {N} points are beyond one call of the library")
        dev = torch.device(self.device)
        if pts.device.type != "cuda" or (dev.index is not None and pts.device != dev):
            raise ValueError(f"silhouette: points must be on the model's device {self.device}, got {pts.device}")
        pts = pts.contiguous()
        labels = labels.to(device=pts.device, dtype=torch.int32).contiguous()
        lib, h = _lib.load(), self._handle()
        sil, a, b = (torch.empty(N, dtype=torch.float32, device=pts.device) for _ in range(3))
        nearest = torch.empty(N, dtype=torch.int32, device=pts.device)
        sums = torch.empty(G, dtype=torch.float64, device=pts.device)
        counts = torch.empty(G, dtype=torch.int64, device=pts.device)
        scratch = _Scratch(pts.device)
        _lib.check(h, lib.spmf_silhouette(
            h, pts.data_ptr(), N, width, labels.data_ptr(), G, 1 if metric == "cosine" else 0, sil.data_ptr(),
            a.data_ptr(), b.data_ptr(), nearest.data_ptr(), sums.data_ptr(), counts.data_ptr(),
            *scratch.fit(lib.spmf_silhouette_scratch_bytes(h, N, G, width)),
            torch.cuda.current_stream(pts.device).cuda_stream), "spmf_silhouette")
        n = counts.to(torch.float64)
        mean = sums / n.masked_fill(counts == 0, float("nan"))
        total, members, nonempty = torch.stack([sums.sum(), n.sum(), (counts > 0).sum().to(torch.float64)]).tolist()
        score = total / members if nonempty >= 2 else float("nan")
        return {"silhouette": sil, "a": a, "b": b, "nearest": nearest, "cluster_mean": mean, "counts": counts,
                "score": score, "n_scored": int(members)}

    def fuzzy_graph(self, indices, distances):
        """The symmetric fuzzy neighbour graph of a ``knn`` result (``knn(points)`` on one set of rows): UMAP's
        graph, scanpy's ``obsp["connectivities"]``.  ``spmf_amd.graph.fuzzy_graph`` has the definition; plain
        torch in fp64 on the tensors' device, one stable sort and no scatter-add, so reproducible.  Returns
        {'indptr': int64 [N+1], 'indices': int32, 'weights': float32, 'sigma', 'rho': fp64 [N]}: what
        ``graph_layout`` takes, and ``spmf_amd.graph.to_csr`` turns it into the numpy CSR arrays."""
        from . import graph as _graph
        return _graph.fuzzy_graph(indices, distances)

    @staticmethod
    def _layout_args(name, n_epochs, min_dist, spread, a, b, n_negatives, negative_rate, repulsion, learning_rate,
                     seed, init, starts=None):
        """The layout arguments of ``graph_layout`` / ``umap`` / ``graph_transform`` that need no graph, checked
        before any library call -> namespace(n_epochs (or None), a, b, M, rate, gamma, lr, seed).  ``starts``: the
        values of ``init`` beside a tensor (default: ``spmf_amd.graph.INITS``)."""
        from . import graph as _graph

        def integer(what, v, lo, hi):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"{name}: {what} must be an integer in {lo}..{hi}, got {v!r}")
            return int(v)

        def weight(what, v, positive=False):
            ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)
            if not ok or not np.isfinite(v) or v < 0 or v > 3.0e38 or (positive and v <= 0):
                raise ValueError(f"{name}: {what} must be a finite number {'> 0' if positive else '>= 0'}, got {v!r}")
            return float(v)
        if n_epochs is not None:
            n_epochs = integer("n_epochs", n_epochs, 0, 2 ** 31 - 1)
        M = integer("n_negatives", n_negatives, 1, _graph.MAX_NEGATIVES)
        seed = integer("seed", seed, 0, 2 ** 64 - 1)
        rate, gamma = weight("negative_rate", negative_rate), weight("repulsion", repulsion)
        lr = weight("learning_rate", learning_rate)
        if (a is None) != (b is None):
            raise ValueError(f"{name}: a and b go together (both, or neither for the fit to min_dist and spread)")
        if a is None:
            try:
                a, b = _graph.find_ab(min_dist, spread)
            except (TypeError, ValueError) as e:
                raise ValueError(f"{name}: {e}") from None
        else:
            a, b = weight("a", a, positive=True), weight("b", b, positive=True)
        starts = _graph.INITS if starts is None else starts
        if not isinstance(init, torch.Tensor) and not (isinstance(init, (str, type(None))) and init in starts):
            raise ValueError(f"{name}: init must be one of {starts} or a float32 [N, 2] tensor, got {init!r}")
        return SimpleNamespace(n_epochs=n_epochs, a=a, b=b, M=M, rate=rate, gamma=gamma, lr=lr, seed=seed)

    @staticmethod
    def _graph_tensors(name, graph):
        """The graph dict of ``graph_layout`` / ``spectral``, its types and shapes checked -> (indptr, indices,
        weights, N, nnz)."""
        if not isinstance(graph, dict) or any(n not in graph for n in ("indptr", "indices", "weights")):
            raise ValueError(f"{name}: graph must be a dict with 'indptr', 'indices' and 'weights' (fuzzy_graph)")
        want = {"indptr": torch.int64, "indices": torch.int32, "weights": torch.float32}
        for n, dt in want.items():
            t = graph[n]
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != dt:
                raise ValueError(f"{name}: graph['{n}'] must be a 1-D {dt} tensor")
        indptr, indices, weights = (graph[n] for n in want)
        if indptr.numel() < 1:
            raise ValueError(f"{name}: graph['indptr'] must have N + 1 entries")
        N, nnz = int(indptr.numel()) - 1, int(indices.numel())
        if int(weights.numel()) != nnz:
            raise ValueError(f"{name}: graph['weights'] has {int(weights.numel())} entries, graph['indices'] {nnz}")
        if N > 2 ** 31 - 64:
            raise ValueError(f"{name}: {N} rows are beyond one call of the library")
        if indices.device != indptr.device or weights.device != indptr.device:
            raise ValueError(f"{name}: the graph's tensors must be on one device")
        return indptr, indices, weights, N, nnz

    @staticmethod
    def _graph_numbers(name, indptr, indices, N, nnz):
        """The graph's numbers -- an indptr rising from 0 to nnz, indices in [0, N) -- checked before any library
        call: one device-side reduction and one read-back."""
        ends = torch.stack([indptr[0], indptr[-1]])
        step = torch.diff(indptr).amin().reshape(1) if N else torch.zeros(1, dtype=torch.int64, device=indptr.device)
        span = torch.stack(list(torch.aminmax(indices))).to(torch.int64) if nnz else \
            torch.zeros(2, dtype=torch.int64, device=indptr.device)
        first, last, step, lo, hi = torch.cat([ends, step, span]).tolist()
        if first != 0 or last != nnz or step < 0:
            raise ValueError(f"{name}: graph['indptr'] must rise from 0 to the {nnz} entries, got {first} .. {last}"
                             + (" with a falling step" if step < 0 else ""))
        if nnz and (lo < 0 or hi >= N):
            raise ValueError(f"{name}: graph['indices'] must lie in [0, {N}), got {lo} .. {hi}")

    def _graph_on_device(self, name, indptr):
        dev = torch.device(self.device)
        if indptr.device.type != "cuda" or (dev.index is not None and indptr.device != dev):
            raise ValueError(f"{name}: the graph must be on the model's device {self.device}, got {indptr.device}")

    def graph_layout(self, graph, init="pca", points=None, n_epochs=None, min_dist=0.1, spread=1.0, a=None, b=None,
                     n_negatives=8, negative_rate=5.0, repulsion=1.0, learning_rate=1.0, seed=0):
        """A deterministic 2-D layout of a weighted graph: the full-batch form of UMAP's objective, one kernel
        launch per epoch (include/spmf_hip.h spmf_graph_layout has the definition, csrc/graph_layout.hip).  Every
        epoch moves every row at once from the positions of the epoch before: along its edges towards its
        neighbours, weighted by the edge, and away from ``n_negatives`` rows drawn by a counter-based generator
        from (``seed``, row, epoch); the step is divided by max(1, the row's summed weight), which keeps the
        simultaneous update from overshooting.  No atomics: two runs give the same bits.

        ``graph``: what ``fuzzy_graph`` returns -- 'indptr' int64 [N+1] (monotone from 0 to nnz), 'indices' int32
        in [0, N), 'weights' float32, on the model's device.  ``init``: a float32 [N, 2] tensor on the device;
        'pca': the two leading principal axes of ``points`` [N, Kx] (``spmf_amd.graph.init_pca``: fp64 covariance
        of the finite rows, max |coordinate| = 10, a non-finite row starts NaN and stays); 'random': uniform
        [-10, 10] from a CPU generator seeded with ``seed``.  ``n_epochs``: None is 500 for N <= 10 000, else 200.
        (``a``, ``b``): the curve 1 / (1 + a d^(2b)); None fits them to (``min_dist``, ``spread``) as umap-learn
        does.  ``negative_rate``: negatives per visit of an edge (umap-learn's negative_sample_rate), spread over
        the ``n_negatives`` (1..64) draws of a row; ``repulsion``: their strength; ``learning_rate``: the first
        epoch's step, falling linearly to 0.

        Returns {'embedding': float32 [N, 2] on the device, 'a', 'b', 'n_epochs'}.  Bit-reproducible for a tensor or
        'pca' init on one machine; for 'random' the same seed gives the same result."""
        from . import graph as _graph
        name = "graph_layout"
        la = self._layout_args(name, n_epochs, min_dist, spread, a, b, n_negatives, negative_rate, repulsion,
                               learning_rate, seed, init)
        indptr, indices, weights, N, nnz = self._graph_tensors(name, graph)
        if isinstance(init, torch.Tensor):
            if init.dim() != 2 or tuple(init.shape) != (N, 2) or init.dtype != torch.float32:
                raise ValueError(f"{name}: an init tensor must be float32 of shape {(N, 2)}, got {init.dtype} "
                                 f"{tuple(init.shape)}")
            if init.device != indptr.device:
                raise ValueError(f"{name}: an init tensor must be on the device of the graph {indptr.device}, got "
                                 f"{init.device}")
        elif init == "pca":
            if not isinstance(points, torch.Tensor) or points.dim() != 2 or not points.dtype.is_floating_point \
                    or int(points.shape[0]) != N or int(points.shape[1]) < 1:
                raise ValueError(f"{name}: init='pca' needs points, a floating-point [N, Kx] tensor with N = {N} rows")
            if points.device != indptr.device:
                raise ValueError(f"{name}: points must be on the device of the graph {indptr.device}, got "
                                 f"{points.device}")
        self._graph_numbers(name, indptr, indices, N, nnz)
        self._graph_on_device(name, indptr)
        total = _graph.default_epochs(N) if la.n_epochs is None else la.n_epochs
        if isinstance(init, torch.Tensor):
            start = init.contiguous()
        elif init == "pca":
            start = _graph.init_pca(points)
        else:
            start = _graph.init_random(N, la.seed, indptr.device)
        indptr, indices, weights = indptr.contiguous(), indices.contiguous(), weights.contiguous()
        lib, h = _lib.load(), self._handle()
        out = torch.empty(N, 2, dtype=torch.float32, device=indptr.device)
        scratch = _Scratch(indptr.device)
        _lib.check(h, lib.spmf_graph_layout(
            h, N, nnz, indptr.data_ptr(), indices.data_ptr(), weights.data_ptr(), start.data_ptr(), out.data_ptr(),
            0, total, total, la.lr, la.a, la.b, la.gamma, la.rate, la.M, la.seed,
            *scratch.fit(lib.spmf_graph_layout_scratch_bytes(h, N)),
            torch.cuda.current_stream(indptr.device).cuda_stream), "spmf_graph_layout")
        return {"embedding": out, "a": la.a, "b": la.b, "n_epochs": total}

    def umap(self, data, k=15, metric="euclidean", nsamples=32, draws=None, max_rows=None, init="pca", n_epochs=None,
             min_dist=0.1, spread=1.0, a=None, b=None, n_negatives=8, negative_rate=5.0, repulsion=1.0,
             learning_rate=1.0, seed=0):
        """The 2-D map of the rows of ``data``: ``embed`` on ``data``, ``knn`` on the posterior mean encodings,
        ``fuzzy_graph`` on their result and ``graph_layout`` on the graph ('pca' starts from the encodings) --
        the coordinates scanpy keeps in ``obsm["X_umap"]``, on which clusters, factor scores and genes are looked
        at.  ``data``, ``nsamples`` / ``draws`` and ``max_rows`` as in ``embed`` (the rows of all batches are
        concatenated); ``k`` and ``metric`` as in ``knn``; the layout arguments as in ``graph_layout`` (``init``: a
        tensor, 'pca' or 'random').

        Returns what ``graph_layout`` returns, bit for bit the four calls made by hand, and 'graph' (the fuzzy
        graph), 'latent' (the encoding, float32 [N, latent_dim]) and the 'indices' / 'distances' of ``knn``.
        Bit-reproducible for given draws with a tensor or 'pca' init on one machine; for 'random' the same seed
        gives the same result."""
        self._knn_args("umap", k, metric)
        self._layout_args("umap", n_epochs, min_dist, spread, a, b, n_negatives, negative_rate, repulsion,
                          learning_rate, seed, init)
        if not 1 <= self.latent_dim <= 256:
            raise ValueError(f"umap: latent_dim {self.latent_dim} is beyond the 256 columns of knn")
        emb = self.embed(data, nsamples=nsamples, draws=draws, max_rows=max_rows)["mean"]
        nn = self.knn(emb, k=k, metric=metric)
        g = self.fuzzy_graph(nn["indices"], nn["distances"])
        res = self.graph_layout(g, init=init, points=emb, n_epochs=n_epochs, min_dist=min_dist, spread=spread, a=a,
                                b=b, n_negatives=n_negatives, negative_rate=negative_rate, repulsion=repulsion,
                                learning_rate=learning_rate, seed=seed)
        res.update(graph=g, latent=emb, indices=nn["indices"], distances=nn["distances"])
        return res

    def spectral(self, graph, n_components=2, tol=1e-4, max_iter=100, seed=0):
        """The ``n_components`` + 1 leading eigenvectors of S = D^-1/2 A D^-1/2 of a weighted graph: the spectral
        embedding of its rows (sklearn's ``SpectralEmbedding``, the start of umap-learn's layout, with
        ``spmf_amd.spectral.diffusion_map`` scanpy's ``tl.diffmap``).  Chebyshev-filtered subspace iteration on a
        block of 16 columns (``spmf_amd.spectral`` has the algorithm): the products with the graph and the two
        small fp64 reductions are the library's (include/spmf_hip.h spmf_graph_spmm, csrc/spectral.hip), the
        16 x 16 eigenproblems are ``eigh`` on the CPU.  No atomics and a seeded CPU start: two runs give the same
        bits.

        ``graph``: as in ``graph_layout``, what ``fuzzy_graph`` returns; it should be symmetric (an asymmetric one
        is not refused, it does not converge).  1 <= ``n_components`` <= 12.  The iteration stops when
        |S v - l v| <= ``tol`` for the n_components + 1 leading columns, or after ``max_iter`` outer iterations.
        At least 32 rows must have a valid edge: below that a dense ``eigh`` is the tool.

        Returns what ``spmf_amd.spectral.solve`` returns, tensors on the device: 'values', 'vectors', 'embedding'
        (``vectors[:, 1:]``), 'residuals', 'converged', 'n_iter', 'n_products', 'scale', 'n_unit'.  In a degenerate
        eigenspace the basis is whatever the seeded start gives: reproducible, not canonical.  Pass
        ``spmf_amd.spectral.layout_init(res['embedding'], seed)`` as ``graph_layout(init=...)`` for the spectral
        start of a layout."""
        from . import spectral as _spectral
        name = "spectral"
        _spectral.check_args(name, n_components, tol, max_iter, seed)
        indptr, indices, weights, N, nnz = self._graph_tensors(name, graph)
        self._graph_numbers(name, indptr, indices, N, nnz)
        # the rows with a valid edge, in plain torch: the library is not needed to refuse a small graph
        ok = (torch.isfinite(weights) & (weights > 0)).to(torch.int64)
        run = torch.cat([torch.zeros(1, dtype=torch.int64, device=ok.device), torch.cumsum(ok, 0)])
        n_live = int(((run[indptr[1:]] - run[indptr[:-1]]) > 0).sum())
        if n_live < _spectral.MIN_ROWS:
            raise _spectral.too_few_rows(name, n_live)
        self._graph_on_device(name, indptr)
        ops = _spectral.LibraryOps(_lib.load(), self._handle(), indptr, indices, weights)
        return _spectral.solve(ops, n_components, tol, max_iter, seed, name=name)

    def spectral_cluster(self, graph, n_clusters, tol=1e-4, max_iter=100, seed=0, kmeans_init="k-means++",
                         kmeans_max_iter=100):
        """Spectral clustering of the rows of a graph (Ng, Jordan, Weiss): ``spectral(n_components =
        n_clusters - 1)``, the rows of the ``n_clusters`` leading eigenvectors scaled to unit length
        (``spmf_amd.spectral.cluster_features``), then ``kmeans`` of those rows.  It separates clusters that are
        not convex in the latent space -- two concentric rings -- where ``cluster``'s k-means of the points
        cannot.  2 <= ``n_clusters`` <= 13; a row without a valid edge gets the label -1.

        Returns what ``kmeans`` returns (for the features) and 'spectral' (the result of ``spectral``) and
        'features'.  Bit-reproducible for a given seed on one machine."""
        from . import cluster as _cluster
        from . import spectral as _spectral
        name = "spectral_cluster"
        if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)) \
                or not 2 <= int(n_clusters) <= _spectral.MAX_COMPONENTS + 1:
            raise ValueError(f"{name}: n_clusters must be an integer in 2..{_spectral.MAX_COMPONENTS + 1}, got "
                             f"{n_clusters!r}")
        _spectral.check_args(name, int(n_clusters) - 1, tol, max_iter, seed)
        _cluster.check_args(name, int(n_clusters), kmeans_max_iter, kmeans_init)
        res = self.spectral(graph, n_components=int(n_clusters) - 1, tol=tol, max_iter=max_iter, seed=seed)
        feats = _spectral.cluster_features(res, int(n_clusters))
        out = self.kmeans(feats, int(n_clusters), init=kmeans_init, max_iter=kmeans_max_iter, seed=seed)
        out.update(spectral=res, features=feats)
        return out

    def communities(self, graph, resolution=1.0, max_levels=32, max_sweeps=100, tol=1e-7):
        """Louvain clustering of the rows of a weighted graph by modularity (scanpy's ``tl.louvain`` /
        ``tl.leiden`` on ``obsp["connectivities"]``): it finds the number of clusters itself, where ``cluster`` and
        ``spectral_cluster`` are told it.  ``spmf_amd.communities`` has the algorithm: the weights become int64
        fixed point (rint(w 2^24)), so every sum is exact in any order; a level is a run of synchronous sweeps, each
        one library call (include/spmf_hip.h spmf_graph_move, csrc/graph_move.hip) that moves every row at once from
        the labels of the sweep before, upwards in label on even sweeps and downwards on odd ones; between levels the
        communities become the rows of a coarser graph.  No atomics on floats anywhere: two runs give the same
        bits, which are also the bits of the numpy backend (``spmf_amd.communities.NumpyOps``).

        ``graph``: as in ``graph_layout``, what ``fuzzy_graph`` returns; it should be symmetric (an asymmetric one
        is not refused).  ``resolution`` > 0: the gamma of Q = in / M2 - gamma sum_c (tot_c / M2)^2, larger for
        more and smaller communities.  A level keeps its best labelling (Q above the best so far by more than
        ``tol``) and ends after an up and a down sweep that moved nothing, 4 sweeps without a new best or
        ``max_sweeps``; the levels end when one merged nothing, or after ``max_levels``.

        Returns what ``spmf_amd.communities.solve`` returns, tensors on the device: 'labels' int64 [N], communities
        numbered by descending size (ties by smallest member row), -1 for a row without a valid entry -- what
        ``group_means``, ``silhouette`` and ``neighbors.vote`` take; 'n_communities', 'sizes', 'modularity',
        'levels' (per level 'n_nodes', 'n_communities', 'modularity', 'n_sweeps', 'hit_max_sweeps') and
        'resolution'."""
        from . import communities as _communities
        name = "communities"
        _communities.check_args(name, resolution, max_levels, max_sweeps, tol)
        indptr, indices, weights, N, nnz = self._graph_tensors(name, graph)
        self._graph_numbers(name, indptr, indices, N, nnz)
        self._graph_on_device(name, indptr)
        ops = _communities.LibraryOps(_lib.load(), self._handle(), indptr, indices, weights)
        return _communities.solve(ops, resolution, max_levels, max_sweeps, tol, name=name)

    def graph_transform(self, indices, distances, reference_layout, weights=None, init=None, n_epochs=None,
                        min_dist=0.1, spread=1.0, a=None, b=None, n_negatives=8, negative_rate=5.0, repulsion=1.0,
                        learning_rate=0.25, seed=0, row_offset=0):
        """New rows on a fitted layout, the reference rows held where they are (umap-learn's ``transform``): all
        epochs in one kernel launch (include/spmf_hip.h spmf_graph_transform has the definition,
        csrc/graph_transform.hip).  A new row starts at the weighted mean of its neighbours' positions and is
        then pulled towards them and pushed away from ``n_negatives`` reference rows drawn per epoch from
        (``seed``, the row's number, epoch).  A row's position is a function of that row alone: rows may be mapped
        in chunks of any size with the same bits, ``row_offset`` being the number of a chunk's first row.

        ``indices`` int [Q, k] and ``distances`` float [Q, k]: what ``knn(reference_points, queries=...)`` returned
        (k <= 64, padding -1 / +inf); ``reference_layout``: float32 [n_ref, 2], the 'embedding' of ``graph_layout``
        / ``umap``; all on the model's device.  ``weights``: float32 [Q, k] memberships, None for
        ``spmf_amd.graph.query_weights(indices, distances)``.  ``init``: None for the weighted mean, or a float32
        [Q, 2] tensor.  ``n_epochs``: None is umap-learn's rule for transform, 100 up to 10 000 rows, else 30.
        (``a``, ``b``) should be the reference layout's; None fits them to (``min_dist``, ``spread``).  The other
        arguments as in ``graph_layout``; the default ``learning_rate`` is a quarter of its, as in umap-learn.

        Returns {'embedding': float32 [Q, 2] on the device (NaN: a row without a valid neighbour), 'weights',
        'sigma' (None with given ``weights``), 'a', 'b', 'n_epochs'}.  Bit-reproducible."""
        from . import graph as _graph
        name = "graph_transform"
        la = self._layout_args(name, n_epochs, min_dist, spread, a, b, n_negatives, negative_rate, repulsion,
                               learning_rate, seed, init, starts=(None,))
        if isinstance(row_offset, bool) or not isinstance(row_offset, (int, np.integer)) or int(row_offset) < 0:
            raise ValueError(f"{name}: row_offset must be an integer >= 0, got {row_offset!r}")
        for what, t in (("indices", indices), ("distances", distances), ("reference_layout", reference_layout)):
            if not isinstance(t, torch.Tensor) or t.dim() != 2:
                raise ValueError(f"{name}: {what} must be a 2-D torch tensor")
        if indices.dtype.is_floating_point or indices.dtype == torch.bool:
            raise ValueError(f"{name}: indices must hold integers, got {indices.dtype}")
        if not distances.dtype.is_floating_point or distances.shape != indices.shape:
            raise ValueError(f"{name}: distances must be floating point of the shape of indices "
                             f"{tuple(indices.shape)}, got {distances.dtype} {tuple(distances.shape)}")
        Q, k = int(indices.shape[0]), int(indices.shape[1])
        if not 1 <= k <= 64:
            raise ValueError(f"{name} needs 1 <= k <= 64 neighbours per row, got {k}")
        if reference_layout.dtype != torch.float32 or int(reference_layout.shape[1]) != 2:
            raise ValueError(f"{name}: reference_layout must be float32 of shape [n_ref, 2], got "
                             f"{reference_layout.dtype} {tuple(reference_layout.shape)}")
        n_ref = int(reference_layout.shape[0])
        if n_ref > 2 ** 31 - 1:
            raise ValueError(f"{name}: {n_ref} reference rows are beyond the int32 index of a neighbour")
        if int(row_offset) + Q > 2 ** 32:
            raise ValueError(f"{name}: row_offset + the {Q} rows must stay within 2^32, got row_offset={row_offset}")
        if weights is not None:
            if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 \
                    or weights.shape != indices.shape:
                raise ValueError(f"{name}: weights must be a float32 tensor of shape {tuple(indices.shape)}")
        if isinstance(init, torch.Tensor) and (tuple(init.shape) != (Q, 2) or init.dtype != torch.float32):
            raise ValueError(f"{name}: an init tensor must be float32 of shape {(Q, 2)}, got {init.dtype} "
                             f"{tuple(init.shape)}")
        dev = torch.device(self.device)
        for what, t in (("indices", indices), ("distances", distances), ("reference_layout", reference_layout),
                        ("weights", weights), ("init", init)):
            if t is not None and (t.device.type != "cuda" or (dev.index is not None and t.device != dev)):
                raise ValueError(f"{name}: {what} must be on the model's device {self.device}, got {t.device}")
        total = _graph.default_transform_epochs(Q) if la.n_epochs is None else la.n_epochs
        sigma = None
        if weights is None:
            qw = _graph.query_weights(indices, distances)
            weights, sigma = qw["weights"], qw["sigma"]
        # (an index beyond int32 is no row of the reference: it stays outside [0, n_ref) through the cast)
        idx = indices.clamp(-1, n_ref).to(torch.int32).contiguous()
        w, ref = weights.contiguous(), reference_layout.contiguous()
        start = init.contiguous() if init is not None else None
        lib, h = _lib.load(), self._handle()
        out = torch.empty(Q, 2, dtype=torch.float32, device=idx.device)
        _lib.check(h, lib.spmf_graph_transform(
            h, Q, k, idx.data_ptr(), w.data_ptr(), ref.data_ptr(), n_ref,
            start.data_ptr() if start is not None else None, out.data_ptr(), int(row_offset), 0, total, total,
            la.lr, la.a, la.b, la.gamma, la.rate, la.M, la.seed,
            torch.cuda.current_stream(idx.device).cuda_stream), "spmf_graph_transform")
        return {"embedding": out, "weights": weights, "sigma": sigma, "a": la.a, "b": la.b, "n_epochs": total}

    def umap_transform(self, data, reference, k=15, metric="euclidean", nsamples=32, draws=None, max_rows=None,
                       labels=None, n_classes=None, n_epochs=None, learning_rate=0.25, n_negatives=8,
                       negative_rate=5.0, repulsion=1.0, seed=0):
        """The rows of ``data`` on the map of ``reference`` (what ``umap`` returned: its 'latent', 'embedding', 'a'
        and 'b' are used): ``embed`` on ``data``, ``knn`` of the encodings among the reference's, then
        ``graph_transform`` with the reference's curve -- umap-learn's ``transform``, scanpy's ``ingest``.  The
        reference map does not move.  ``data``, ``nsamples`` / ``draws`` and ``max_rows`` as in ``embed``; ``k``
        and ``metric`` as in ``knn``; the layout arguments as in ``graph_transform``.  ``labels``: an integer per
        reference row (-1: none), e.g. the labels of ``cluster``; every new row then gets the class with the
        largest summed membership among its neighbours (``spmf_amd.neighbors.vote``; ``n_classes`` as there).

        Returns what ``graph_transform`` returns, bit for bit the calls made by hand, and 'latent' (the encoding,
        float32 [Q, latent_dim]), the 'indices' / 'distances' of ``knn`` and, with ``labels``, 'labels' int64 [Q]
        (-1: no voting neighbour) and 'label_share' fp64 [Q].  Bit-reproducible for given draws."""
        from . import neighbors as _neighbors
        name = "umap_transform"
        self._knn_args(name, k, metric)
        if not isinstance(reference, dict) or any(n not in reference for n in ("latent", "embedding", "a", "b")):
            raise ValueError(f"{name}: reference must be what umap returned: a dict with 'latent', 'embedding', "
                             f"'a' and 'b'")
        self._layout_args(name, n_epochs, 0.1, 1.0, reference["a"], reference["b"], n_negatives, negative_rate,
                          repulsion, learning_rate, seed, None, starts=(None,))
        lat, ref = reference["latent"], reference["embedding"]
        if not isinstance(lat, torch.Tensor) or lat.dim() != 2 or lat.dtype != torch.float32 \
                or int(lat.shape[1]) != self.latent_dim:
            raise ValueError(f"{name}: reference['latent'] must be a float32 [n_ref, {self.latent_dim}] tensor")
        if not isinstance(ref, torch.Tensor) or ref.dtype != torch.float32 \
                or tuple(ref.shape) != (int(lat.shape[0]), 2):
            raise ValueError(f"{name}: reference['embedding'] must be a float32 {(int(lat.shape[0]), 2)} tensor")
        if not 1 <= self.latent_dim <= 256:
            raise ValueError(f"{name}: latent_dim {self.latent_dim} is beyond the 256 columns of knn")
        if labels is not None:
            labels = _vector(name, "labels", labels)
            if int(labels.numel()) != int(lat.shape[0]):
                raise ValueError(f"{name}: labels must have one entry per reference row, got {int(labels.numel())} "
                                 f"for {int(lat.shape[0])} rows")
            if n_classes is not None and (isinstance(n_classes, bool) or not isinstance(n_classes, (int, np.integer))
                                          or int(n_classes) < 0):
                raise ValueError(f"{name}: n_classes must be an integer >= 0, got {n_classes!r}")
        emb = self.embed(data, nsamples=nsamples, draws=draws, max_rows=max_rows)["mean"]
        nn = self.knn(lat, k=k, queries=emb, metric=metric)
        res = self.graph_transform(nn["indices"], nn["distances"], ref, n_epochs=n_epochs, a=reference["a"],
                                   b=reference["b"], n_negatives=n_negatives, negative_rate=negative_rate,
                                   repulsion=repulsion, learning_rate=learning_rate, seed=seed)
        res.update(latent=emb, indices=nn["indices"], distances=nn["distances"])
        if labels is not None:
            res["labels"], res["label_share"] = _neighbors.vote(nn["indices"], res["weights"],
                                                                labels.to(emb.device), n_classes)
        return res

    def cluster(self, data, n_clusters, nsamples=32, draws=None, max_rows=None, init="k-means++", max_iter=100,
                seed=0):
        """k-means of the rows of ``data`` in the model's latent space: ``embed`` on ``data``, then ``kmeans``
        on the posterior mean encodings, with no labelling leaving the device in between.  ``data``,
        ``nsamples`` / ``draws`` and ``max_rows`` as in ``embed`` (the rows of all batches are concatenated);
        ``n_clusters``, ``init``, ``max_iter`` and ``seed`` as in ``kmeans``.

        Returns what ``kmeans`` returns, bit for bit ``kmeans(embed(data, draws=draws)["mean"], ...)``, and
        'embedding': float32 [N, latent_dim].  The labels are those ``group_means`` takes, and
        ``silhouette(res["embedding"], res["labels"], n_clusters)`` scores the clustering."""
        from . import cluster as _cluster
        G, max_iter = _cluster.check_args("cluster", n_clusters, max_iter, init)
        if not 1 <= self.latent_dim <= 256:
            raise ValueError(f"cluster: latent_dim {self.latent_dim} is beyond the 256 columns of kmeans")
        if isinstance(init, torch.Tensor):        # (its device is checked against the embedding's, in kmeans)
            if init.dim() != 2 or tuple(init.shape) != (G, self.latent_dim):
                raise ValueError(f"cluster: an init tensor must have shape {(G, self.latent_dim)}, got "
                                 f"{tuple(init.shape)}")
            if init.dtype != torch.float32:
                raise ValueError(f"cluster: an init tensor must be float32, got {init.dtype}")
        emb = self.embed(data, nsamples=nsamples, draws=draws, max_rows=max_rows)["mean"]
        res = self.kmeans(emb, G, init=init, max_iter=max_iter, seed=seed)
        res["embedding"] = emb
        return res
