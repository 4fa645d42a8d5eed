"""The streaming posterior queries of the model classes: ``StreamingQueries`` is the mixin that gives
PoissonFactorization (and through it the Bernoulli and mixed classes) waic_streaming, top_k, score_cells,
rank_cells, predict, top_rows, group_means, set_scores and embed.  (The calls on rows and graphs as given, and the
composites that start from ``embed``, are ``spmf_amd.analysis``.)

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

from . import _args, _lib
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
        self.scratch = _lib.Scratch(model.device)

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
        k = _args.integer("top_rows", "k", k)
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
