"""Device-resident sparse count matrix for the HIP path.

The reference feeds dense ``[B, D]`` tensors under ``data[count_key]``
(mederrata_spmf/poisson.py:170,182; tests/spmf_test.py:17-22).  For the
linear decoder the energy only needs the stored entries, so
the HIP path keeps one shard of the matrix as

  * row-major CSR   ``row_ptr[N+1] int32, col_idx[nnz] int32, val[nnz] f32``
  * panel-CSC       for each panel of ``panel_rows`` consecutive rows a CSC of
                    that panel: ``pc_ptr[n_panels*(D+1)]``, ``pc_row``, ``pc_val``
  * per-row         ``row_sum`` (f32), ``row_lgamma`` = sum lgamma(x+1) (f64)

A *batch* is a contiguous range of panels, so minibatching never re-sorts.
On the HIP device the layout is built by the library (``spmf_layout_build``,
``spmf_dense_row_ptr`` / ``spmf_dense_fill_csr`` for dense batches,
``spmf_counts_stats`` / ``spmf_counts_colstats`` / ``spmf_counts_gvals`` for the
statistics and the log_transform streams): torch is storage.  The torch
construction of the same arrays below is the host-side statement of the layout
(CPU tensors, and the reference the library is compared with bit for bit in
tests/test_gpu_layout.py; ``SPMF_NATIVE_LAYOUT=0`` selects it on the GPU).
"""
from __future__ import annotations


import ctypes as C
import os

import numpy as np
import torch

from . import _lib

DEFAULT_PANEL_ROWS = 8192      # without a latent_dim hint
PANEL_TABLE_BYTES = 3 << 20    # z and xi*gz rows of one panel: what an XCD's 4 MB L2 should hold


def balanced_panel_rows(n_rows, latent_dim, table_bytes=PANEL_TABLE_BYTES):
    """Rows per panel for a shard of ``n_rows`` at latent dimension ``latent_dim``.

    The column pass gathers z_b and xi*gz_b (2 x KP floats per row) of ONE panel at a time on
    each XCD (col_pass.hip: workgroup -> panel by blockIdx % 8), so a panel's pair of tables
    should fit that XCD's L2 with room for the entry stream (3 MB of 4: measured optimum on C3
    and C4), and the panel count should be a multiple of 8 so that every XCD walks the same
    number of panels (123 panels on C3 left two XCDs with 16 and six with 15: 4 % of the pass).
    A shard of up to two such panels stays one panel (fewer than 8 panels are shared by all XCDs)."""
    n_rows = int(max(1, n_rows))
    kp = 4
    while kp < int(latent_dim):
        kp *= 2
    target = max(1024, int(table_bytes) // (8 * kp))
    if kp > 64 and table_bytes == PANEL_TABLE_BYTES:
        # the whole-wave column pass of csrc/widek.hip (one wave and one set of 2*KP float atomics per work
        # item): longer lists pay more than L2 residency -- C2's matrix at K = 256: 3.43 ms per step with
        # 1408-row panels, 1.81 with 10 240 (profiles/r05_widek_probe.txt)
        target = 10240
    if n_rows <= 2 * target:
        return n_rows
    n_panels = 8 * -(-n_rows // (8 * target))
    rows = -(-n_rows // n_panels)
    for g in (64, 8):                       # a round number, if it keeps the panel count
        r = -(-rows // g) * g
        if -(-n_rows // r) == n_panels:
            return r
    return rows
SEGMENT_ENTRIES = 256     # longest run of one column a single lane group streams
#: zero entries appended to pc_row / pc_val / pc_gval: the column pass reads list entries
#: four per lane (spmf_counts.pc_pad, include/spmf_hip.h) and may run this far past a list
PC_PAD = 64


def _as_csr_arrays(x):
    """Accept scipy CSR, (indptr, indices, data), dense ndarray / tensor."""
    try:
        import scipy.sparse as sp
        if sp.issparse(x):
            x = x.tocsr()
            x.sum_duplicates()
            return (np.asarray(x.indptr), np.asarray(x.indices),
                    np.asarray(x.data), x.shape)
    except ImportError:  # pragma: no cover
        pass
    if isinstance(x, (tuple, list)) and len(x) == 4:
        return x
    return None


def _layout_check(lib, rc, what):
    """Raise on a failed spmf_layout_* / spmf_dense_* call (context-free entry points: the message
    is the calling thread's spmf_layout_last_error)."""
    if rc != 0:
        msg = lib.spmf_layout_last_error()
        raise _lib.SpmfError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


class SparseCounts:
    """One row shard of the count matrix in the layout the kernels read."""

    def __init__(self, row_ptr, col_idx, val, n_rows, n_cols,
                 panel_rows=None, col_split=0, latent_dim=None):
        """``panel_rows`` None / 0: chosen by balanced_panel_rows when ``latent_dim`` is given,
        DEFAULT_PANEL_ROWS otherwise."""
        if not panel_rows:
            panel_rows = balanced_panel_rows(n_rows, latent_dim) if latent_dim else DEFAULT_PANEL_ROWS
        dev = val.device
        self.device = dev
        self.n_rows = int(n_rows)
        self.n_cols = int(n_cols)
        self.row_ptr = row_ptr.to(torch.int32).contiguous()
        self.col_idx = col_idx.to(torch.int32).contiguous()
        self.val = val.to(torch.float32).contiguous()
        self.nnz = int(self.val.numel())
        if self.nnz >= 2 ** 31:
            raise ValueError("nnz per shard must fit int32")
        self.panel_rows = int(max(1, min(panel_rows, max(self.n_rows, 1))))
        self.n_panels = max(1, -(-self.n_rows // self.panel_rows))
        # multi-GPU overlap: work items of a panel sorted by column half first
        # (columns < col_split, then the rest); 0 = no split
        self.col_split = int(col_split)
        # the model's latent dimension when the caller knows it: small K asks for more, shorter work items
        # (include/spmf_hip.h spmf_layout_build_k); 0 = unknown
        self.latent_dim_hint = int(latent_dim) if latent_dim else 0
        # the lists, the work items and the packed streams: the library's builder on the HIP
        # device (csrc/layout.hip), the torch operators below for host-side tensors (CPU tests)
        # or when SPMF_NATIVE_LAYOUT=0 asks for them (tests/test_gpu_layout.py compares the two)
        self.native_layout = False
        if dev.type == "cuda" and os.environ.get("SPMF_NATIVE_LAYOUT", "1") != "0":
            self._build_native()
        else:
            self._build_panel_csc()
            self._build_packed_rows()
        self.row_sum = None
        self.row_lgamma = None
        self.row_scale = None      # xi_b, set by PoissonFactorization
        self._xi_key = None
        self.gval = None           # g(x) = log(x/eta+1) per entry (log_transform only)
        self.pc_gval = None
        self._g_key = None
        self._struct_cache = {}    # ((p0, p1), _xi_key, _g_key) -> descriptor (struct)
        self._keep = []

    # ---- construction ----------------------------------------------------
    @classmethod
    def from_any(cls, x, device=None, panel_rows=None, col_split=0, latent_dim=None):
        if isinstance(x, SparseCounts):
            return x
        device = torch.device(device if device is not None else
                              ("cuda" if torch.cuda.is_available() else "cpu"))
        if isinstance(x, torch.Tensor) and x.layout in (torch.sparse_csr, torch.sparse_coo):
            # a torch sparse tensor (CSR, or COO coalesced to CSR): its index / value tensors are taken where
            # they are -- on the device: no host round trip
            xc = x.coalesce().to_sparse_csr() if x.layout == torch.sparse_coo else x
            if xc.dim() != 2:
                raise ValueError("counts must be [rows, features]")
            return cls(xc.crow_indices().to(device), xc.col_indices().to(device),
                       xc.values().to(device=device, dtype=torch.float32), xc.shape[0], xc.shape[1],
                       panel_rows, col_split, latent_dim)
        csr = _as_csr_arrays(x)
        if csr is not None:
            indptr, indices, data, shape = csr
            # 4-byte offsets / indices over the host link when they fit (they must, to be a shard)
            it = np.int32 if (len(indptr) == 0 or int(indptr[-1]) < 2 ** 31) and shape[1] < 2 ** 31 else np.int64
            return cls(torch.as_tensor(np.asarray(indptr, dtype=it)).to(device),
                       torch.as_tensor(np.asarray(indices, dtype=it)).to(device),
                       torch.as_tensor(np.asarray(data, dtype=np.float32)).to(device),
                       shape[0], shape[1], panel_rows, col_split, latent_dim)
        return cls.from_dense(x, device, panel_rows, col_split, latent_dim)

    @classmethod
    def from_dense(cls, x, device=None, panel_rows=None, col_split=0, latent_dim=None):
        device = torch.device(device if device is not None else
                              ("cuda" if torch.cuda.is_available() else "cpu"))
        if hasattr(x, "numpy") and not isinstance(x, torch.Tensor):
            x = x.numpy()
        t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
        t = t.to(device)
        if t.dim() != 2:
            raise ValueError("counts must be [rows, features]")
        N, D = t.shape
        if t.device.type == "cuda" and os.environ.get("SPMF_NATIVE_LAYOUT", "1") != "0":
            # the library's compaction (csrc/layout.hip): count, offsets, fill -- three passes over
            # the dense batch instead of mask / nonzero / index with int64 intermediates
            lib = _lib.load()
            t = t.to(torch.float32).contiguous()
            idx = t.device.index if t.device.index is not None else torch.cuda.current_device()
            st = torch.cuda.current_stream(t.device).cuda_stream

            def ok(rc, what):
                _layout_check(lib, rc, what)

            row_ptr = torch.empty(N + 1, dtype=torch.int32, device=t.device)
            nb = int(lib.spmf_dense_scratch_bytes(N))
            scratch = torch.empty((nb + 7) // 8, dtype=torch.int64, device=t.device)
            ok(lib.spmf_dense_row_ptr(idx, N, D, t.data_ptr(), D, row_ptr.data_ptr(), scratch.data_ptr(),
                                      scratch.numel() * 8, st), "spmf_dense_row_ptr")
            nnz = int(row_ptr[N])
            if nnz >= 2 ** 31 - 1:
                raise ValueError("nnz per shard must fit int32")
            col = torch.empty(nnz, dtype=torch.int32, device=t.device)
            val = torch.empty(nnz, dtype=torch.float32, device=t.device)
            if nnz > 0:
                ok(lib.spmf_dense_fill_csr(idx, N, D, t.data_ptr(), D, row_ptr.data_ptr(), col.data_ptr(),
                                           val.data_ptr(), st), "spmf_dense_fill_csr")
            return cls(row_ptr, col, val, N, D, panel_rows, col_split, latent_dim)
        mask = t != 0
        counts = mask.sum(1)
        row_ptr = torch.zeros(N + 1, dtype=torch.int64, device=device)
        row_ptr[1:] = torch.cumsum(counts, 0)
        nz = mask.nonzero(as_tuple=False)      # row-major order
        col = nz[:, 1]
        val = t[mask].to(torch.float32)
        return cls(row_ptr, col, val, N, D, panel_rows, col_split, latent_dim)

    def _build_native(self):
        """spmf_layout_build (include/spmf_hip.h): one caller-owned buffer holds every derived
        array; the attributes below are views into it."""
        lib = _lib.load()
        dev = self.device
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        lb, sb = C.c_size_t(), C.c_size_t()

        def ok(rc, what):
            _layout_check(lib, rc, what)

        ok(lib.spmf_layout_sizes_k(idx, self.n_rows, self.nnz, self.n_cols, self.panel_rows, self.latent_dim_hint,
                                   C.byref(lb), C.byref(sb)), "spmf_layout_sizes_k")
        with torch.cuda.device(idx):
            layout = torch.empty(max(lb.value, 256), dtype=torch.uint8, device=dev)
            scratch = torch.empty(max(sb.value, 256), dtype=torch.uint8, device=dev)
            cs, info = _lib.CountsStruct(), _lib.LayoutInfo()
            info.struct_size = C.sizeof(_lib.LayoutInfo)
            ok(lib.spmf_layout_build_k(idx, self.n_rows, self.nnz, self.n_cols, self.row_ptr.data_ptr(),
                                       self.col_idx.data_ptr(), self.val.data_ptr(), self.panel_rows,
                                       self.col_split, self.latent_dim_hint, layout.data_ptr(), layout.numel(),
                                       scratch.data_ptr(), scratch.numel(), C.byref(cs), C.byref(info),
                                       torch.cuda.current_stream(dev).cuda_stream), "spmf_layout_build_k")
        del scratch
        base = layout.data_ptr()

        def view(ptr, n, dtype=torch.int32):
            off = int(ptr) - base
            return layout[off:off + 4 * n].view(dtype)

        nP, D, nnz = int(info.n_panels), self.n_cols, self.nnz
        assert nP == self.n_panels and int(info.panel_rows) == self.panel_rows
        self._layout_buf = layout
        self.pc_ptr = view(cs.pc_ptr, nP * (D + 1))
        self.pc_row = view(cs.pc_row, nnz + PC_PAD)
        self.pc_val = view(cs.pc_val, nnz + PC_PAD, torch.float32)
        self.pc_pad = int(cs.pc_pad)
        packed = os.environ.get("SPMF_PACKED_ENTRIES", "1") != "0"
        self.pc_ent = view(cs.pc_ent, nnz + PC_PAD) if cs.pc_ent and packed else None
        self.ent = view(cs.ent, nnz) if cs.ent and packed else None
        n_items = int(info.n_items)
        self.items = view(cs.items, 4 * n_items).view(n_items, 4)
        self.item_ptr = view(cs.item_ptr, nP + 1)
        self.item_mid = view(cs.item_mid, nP)
        self.list_first = view(cs.list_first, nP * D + 1)     # deterministic mode: items in generation order
        self.item_pos = view(cs.item_pos, n_items)
        per_panel = view(info.items_per_panel, nP).to(torch.int64)
        lower = view(info.items_lower, nP).to(torch.int64)
        self.items_per_panel = per_panel
        self.items_per_half = torch.stack([lower, per_panel - lower], 0)
        self.segment = int(info.segment)
        self.native_layout = True

    def _build_packed_rows(self):
        # packed copy of the CSR entries for the row pass (spmf_counts.ent): col << 16 | count,
        # when the columns fit 16 bits and every stored value is an integer count below 65536
        self.ent = None
        if self.nnz > 0 and self.n_cols <= 65536 and os.environ.get("SPMF_PACKED_ENTRIES", "1") != "0":
            v = self.val
            if bool(((v >= 0) & (v <= 65535.0) & (v == torch.floor(v))).all()):
                w = (self.col_idx.to(torch.int64) << 16) | v.to(torch.int64)
                # bit pattern of a uint32 in an int32 tensor (torch has no uint32 arithmetic)
                self.ent = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()

    def _build_panel_csc(self):
        dev, N, D, P = self.device, self.n_rows, self.n_cols, self.panel_rows
        nP = self.n_panels
        lens = (self.row_ptr[1:] - self.row_ptr[:-1]).to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(N, device=dev, dtype=torch.int64), lens)
        key = (rows // P) * D + self.col_idx.to(torch.int64)
        # stable: ties keep CSR (ascending row) order -> deterministic lists
        order = torch.sort(key, stable=True).indices
        self.pc_row = torch.cat([rows[order].to(torch.int32),
                                 torch.zeros(PC_PAD, dtype=torch.int32, device=dev)]).contiguous()
        self.pc_val = torch.cat([self.val[order],
                                 torch.zeros(PC_PAD, dtype=torch.float32, device=dev)]).contiguous()
        self.pc_pad = PC_PAD       # what batch_struct reports (0 selects the entry-at-a-time fetch)
        # packed lists for the column pass (spmf_counts.pc_ent): row inside its panel << 16 | count
        self.pc_ent = None
        if self.nnz > 0 and P <= 65536 and os.environ.get("SPMF_PACKED_ENTRIES", "1") != "0":
            v = self.pc_val[:self.nnz]
            if bool(((v >= 0) & (v <= 65535.0) & (v == torch.floor(v))).all()):
                w = ((rows[order] % P) << 16) | v.to(torch.int64)
                w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
                self.pc_ent = torch.cat([w, torch.zeros(PC_PAD, dtype=torch.int32, device=dev)]).contiguous()
        cnt = torch.bincount(key, minlength=nP * D)
        excl = torch.zeros(nP * D + 1, dtype=torch.int64, device=dev)
        excl[1:] = torch.cumsum(cnt, 0)
        ptr = torch.empty(nP, D + 1, dtype=torch.int64, device=dev)
        ptr[:, :D] = excl[:-1].view(nP, D)
        ptr[:, D] = excl[D::D]
        self.pc_ptr = ptr.to(torch.int32).contiguous().view(-1)
        self._build_items(cnt, excl[:-1])

    def _build_items(self, cnt, starts, seg=None):
        """Column-pass work items {start, len, column, 0}: every non-empty
        (panel, column) list cut into segments of <= seg entries; inside a
        panel sorted by length (descending) so the lane groups of a wave get
        items of similar length.  Deterministic (stable sorts)."""
        dev, D, nP = self.device, self.n_cols, self.n_panels
        if seg is None:
            # a panel should offer a few thousand items: small or nearly dense
            # batches (few, long column lists) are otherwise a handful of serial
            # 256-entry walks -- 128 us of latency for a 1000 x 30 batch
            seg, per_panel = 16, self.nnz / max(1, nP)
            k = getattr(self, "latent_dim_hint", 0)        # csrc/layout.hip make_geo: the same rule
            want = 32768 if 1 <= k <= 4 else (16384 if 5 <= k <= 8 else 4096)
            while seg < SEGMENT_ENTRIES and per_panel / seg > want:
                seg *= 2
            seg = min(seg, SEGMENT_ENTRIES)
        seg = int(seg)
        nseg = (cnt + seg - 1) // seg                       # segments per list
        lists = torch.nonzero(nseg > 0, as_tuple=False).view(-1)
        rep = nseg[lists]
        lid = torch.repeat_interleave(lists, rep)           # list id of every item
        first = torch.cumsum(rep, 0) - rep
        k = torch.arange(lid.numel(), device=dev, dtype=torch.int64) - \
            torch.repeat_interleave(first, rep)             # segment index inside its list
        start = starts[lid] + k * seg
        length = torch.minimum(cnt[lid] - k * seg, torch.full_like(k, seg))
        panel = lid // D
        col = lid % D
        # sort by (panel asc, [column half asc,] length desc); ties keep (column, segment) order
        half = (col >= self.col_split).to(torch.int64) if self.col_split > 0 else torch.zeros_like(col)
        key = (panel * 2 + half) * (seg + 1) + (seg - length)
        order = torch.sort(key, stable=True).indices
        items = torch.stack([start[order], length[order], col[order],
                             torch.zeros_like(col[order])], 1)
        self.items = items.to(torch.int32).contiguous()
        # the items in generation order -- (panel, column, segment) -- for the deterministic mode:
        # first raw item of every list, and where each raw item went in the sort
        lf = torch.zeros(nseg.numel() + 1, dtype=torch.int64, device=dev)
        lf[1:] = torch.cumsum(nseg, 0)
        self.list_first = lf.to(torch.int32).contiguous()
        pos = torch.empty(order.numel(), dtype=torch.int64, device=dev)
        pos[order] = torch.arange(order.numel(), device=dev, dtype=torch.int64)
        self.item_pos = pos.to(torch.int32).contiguous()
        per_panel = torch.bincount(panel, minlength=nP)
        ip = torch.zeros(nP + 1, dtype=torch.int64, device=dev)
        ip[1:] = torch.cumsum(per_panel, 0)
        self.item_ptr = ip.to(torch.int32).contiguous()
        self.items_per_panel = per_panel
        lower = torch.bincount(panel[half == 0], minlength=nP)
        self.item_mid = (ip[:-1] + lower).to(torch.int32).contiguous()
        self.items_per_half = torch.stack([lower, per_panel - lower], 0)

    # ---- statistics (HIP pre-pass) ---------------------------------------
    def compute_stats(self, ctx_handle, colsum=None, colnnz=None):
        """row_sum / row_lgamma via spmf_counts_stats; optionally accumulate
        compute_scales' column sums (poisson.py:118-135) into colsum/colnnz
        (float64 device tensors of length D)."""
        lib = _lib.load()
        if self.device.type != "cuda":
            raise _lib.SpmfError("SparseCounts statistics need the HIP device")
        self.row_sum = torch.empty(self.n_rows, dtype=torch.float32, device=self.device)
        self.row_lgamma = torch.empty(self.n_rows, dtype=torch.float64, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = lib.spmf_counts_stats(
            ctx_handle, self.n_rows, self.row_ptr.data_ptr(), self.col_idx.data_ptr(),
            self.val.data_ptr(), None, None,
            self.row_sum.data_ptr(), self.row_lgamma.data_ptr(), stream)
        _lib.check(ctx_handle, rc, "spmf_counts_stats")
        if colsum is not None or colnnz is not None:
            # the column half from the panel-CSC lists: one atomic per list, not per entry
            cs = self.batch_struct()
            rc = lib.spmf_counts_colstats(
                ctx_handle, C.byref(cs),
                colsum.data_ptr() if colsum is not None else None,
                colnnz.data_ptr() if colnnz is not None else None, stream)
            _lib.check(ctx_handle, rc, "spmf_counts_colstats")

    # The spmf_counts descriptors cached per (panel range, xi key, g key) hold RAW
    # device pointers to row_scale / gval / pc_gval.  Two models with different
    # xi_u_global or eta may share one SparseCounts (key A -> key B -> key A), so the
    # tensors of every key that still has a cached descriptor (or a captured graph)
    # are kept alive here, and evicting a key drops its descriptors with it.
    _MAX_XI_KEYS = 8
    _MAX_G_KEYS = 2          # gval + pc_gval are nnz sized

    def _drop_structs(self, pos, key):
        for k in [k for k in self._struct_cache if k[pos] == key]:
            del self._struct_cache[k]

    def set_row_scale(self, xi_u_global, scale_rows):
        """xi_b = rowsum_b / xi_u_global (poisson.py:644-649)."""
        key = (float(xi_u_global), bool(scale_rows))
        if key == self._xi_key:
            return
        held = self.__dict__.setdefault("_row_scales", {})
        if key not in held:
            held[key] = ((self.row_sum / float(xi_u_global)).contiguous()
                         if scale_rows else None)
            while len(held) > self._MAX_XI_KEYS:
                old = next(iter(held))
                del held[old]
                self._drop_structs(1, old)
        self.row_scale = held[key]
        self._xi_key = key

    def set_log_transform(self, eta_dev, ctx_handle=None):
        """g(x) = log(x/eta_d + 1) per stored entry (encoder_function,
        poisson.py:41-42), in CSR and panel-CSC order.  Data side: depends on
        the counts and the fixed column scales only.  With a context handle on the
        HIP device: spmf_counts_gvals; torch operators otherwise (host-side tensors)."""
        held = self.__dict__.setdefault("_gvals", {})
        # identity of the eta tensor (a strong reference is kept, so its id cannot be
        # recycled while the entry lives) + its in-place version counter
        key = (id(eta_dev), int(eta_dev._version))
        if self._g_key == key:
            return
        if key not in held:
            eta = eta_dev.to(self.device, torch.float32).contiguous()
            if ctx_handle is not None and self.device.type == "cuda" and self.nnz > 0:
                gval = torch.empty(self.nnz, dtype=torch.float32, device=self.device)
                pc_gval = torch.zeros(self.nnz + PC_PAD, dtype=torch.float32, device=self.device)
                cs = self.batch_struct()
                rc = _lib.load().spmf_counts_gvals(
                    ctx_handle, C.byref(cs), eta.data_ptr(), gval.data_ptr(), pc_gval.data_ptr(),
                    torch.cuda.current_stream(self.device).cuda_stream)
                _lib.check(ctx_handle, rc, "spmf_counts_gvals")
                held[key] = (eta_dev, gval, pc_gval, eta)
                self._trim_gvals(held)
                _, self.gval, self.pc_gval = held[key][:3]
                self._g_key = key
                return
            gval = torch.log1p(self.val / eta[self.col_idx.to(torch.int64)]).contiguous()
            nP, D = self.n_panels, self.n_cols
            ptr = self.pc_ptr.view(nP, D + 1).to(torch.int64)
            cnt = (ptr[:, 1:] - ptr[:, :-1]).reshape(-1)
            cols = torch.repeat_interleave(
                torch.arange(nP * D, device=self.device, dtype=torch.int64) % D, cnt)
            pc_gval = torch.cat([torch.log1p(self.pc_val[:self.nnz] / eta[cols]),
                                 torch.zeros(PC_PAD, dtype=torch.float32,
                                             device=self.device)]).contiguous()
            held[key] = (eta_dev, gval, pc_gval)
            self._trim_gvals(held)
        _, self.gval, self.pc_gval = held[key][:3]
        self._g_key = key

    def _trim_gvals(self, held):
        while len(held) > self._MAX_G_KEYS:
            old = next(iter(held))
            del held[old]
            self._drop_structs(2, old)

    # ---- batches ---------------------------------------------------------
    def n_batches(self, batch_rows):
        ppb = max(1, batch_rows // self.panel_rows)
        return -(-self.n_panels // ppb)

    def _host_panels(self):
        """Host mirrors of the per-panel numbers a descriptor needs (first stored entry of every
        panel, items per panel and per column half, Σ lgamma(x+1) per panel): read back ONCE, so
        that cutting a descriptor for a panel range is host arithmetic -- a fresh minibatch of a
        resident shard costs no device synchronisation (it was six: 0.2-0.3 ms beside a 0.13 ms
        step)."""
        hp = self.__dict__.get("_hp")
        if hp is None:
            nP, P = self.n_panels, self.panel_rows
            edges = torch.clamp(torch.arange(nP + 1, dtype=torch.int64) * P, max=self.n_rows).to(self.device)
            starts = self.row_ptr[edges].to(torch.int64).cpu().numpy()
            ipp = self.items_per_panel.cpu().numpy()
            iph = self.items_per_half.cpu().numpy()
            iptr = np.concatenate([[0], np.cumsum(ipp)]).astype(np.int64)
            hp = self._hp = {"starts": starts, "ipp": ipp, "iph": iph, "iptr": iptr, "lg": None, "lg_of": None}
        if self.row_lgamma is not None and hp["lg_of"] is not self.row_lgamma:
            nP, P = self.n_panels, self.panel_rows
            pad = nP * P - self.n_rows
            lg = self.row_lgamma if pad == 0 else torch.cat(
                [self.row_lgamma, torch.zeros(pad, dtype=torch.float64, device=self.device)])
            hp["lg"] = lg.view(nP, P).sum(1).cpu().numpy() if self.n_rows else np.zeros(nP)
            hp["lg_of"] = self.row_lgamma
        return hp

    def panel_range(self, pr):
        """A batch's ``'panels'`` entry (None: every panel) as ``(p0, p1)``, p1 clipped to the panels there are."""
        p0, p1 = pr or (0, None)
        return int(p0), self.n_panels if p1 is None else min(int(p1), self.n_panels)

    def struct(self, p0=0, p1=None):
        """``batch_struct(p0, p1)`` under the current row scale and g(x), built once per key and
        kept until that row scale or g(x) is evicted (``_drop_structs``)."""
        key = ((p0, p1), self._xi_key, self._g_key)
        cs = self._struct_cache.get(key)
        if cs is None:
            cs = self._struct_cache[key] = self.batch_struct(p0, p1)
        return cs

    def batch_struct(self, p0=0, p1=None):
        """spmf_counts descriptor of panels [p0, p1)."""
        p1 = self.n_panels if p1 is None else min(p1, self.n_panels)
        r0 = p0 * self.panel_rows
        r1 = min(p1 * self.panel_rows, self.n_rows)
        hp = self._host_panels()
        cs = _lib.CountsStruct()
        cs.struct_size = C.sizeof(_lib.CountsStruct)      # ABI guard, verified by the library
        cs.n_rows = r1 - r0
        lo = int(hp["starts"][p0]) if self.nnz else 0
        hi = int(hp["starts"][p1]) if self.nnz else 0
        cs.nnz = hi - lo
        cs.n_cols = self.n_cols
        cs.n_panels = p1 - p0
        cs.panel_rows = self.panel_rows
        cs.row_base = r0
        cs.row_ptr = self.row_ptr.data_ptr() + 4 * r0
        cs.col_idx = self.col_idx.data_ptr()
        cs.val = self.val.data_ptr()
        cs.row_scale = (self.row_scale.data_ptr() + 4 * r0
                        if self.row_scale is not None else None)
        cs.pc_ptr = self.pc_ptr.data_ptr() + 4 * p0 * (self.n_cols + 1)
        cs.pc_row = self.pc_row.data_ptr()
        cs.pc_val = self.pc_val.data_ptr()
        cs.lgamma_sum = (float(hp["lg"][p0:p1].sum())
                         if self.row_lgamma is not None and p1 > p0 else 0.0)
        cs.item_ptr = self.item_ptr.data_ptr() + 4 * p0
        cs.items = self.items.data_ptr()
        cs.max_items_per_panel = (int(hp["ipp"][p0:p1].max())
                                  if self.items.numel() and p1 > p0 else 0)
        cs.pc_pad = int(self.pc_pad)
        if self.col_split > 0:
            cs.item_mid = self.item_mid.data_ptr() + 4 * p0
            cs.col_split = self.col_split
            for h in range(2):
                cs.max_items_half[h] = (int(hp["iph"][h, p0:p1].max())
                                        if self.items.numel() and p1 > p0 else 0)
        if getattr(self, "list_first", None) is not None:
            cs.list_first = self.list_first.data_ptr() + 4 * p0 * self.n_cols
            cs.item_pos = self.item_pos.data_ptr()
            cs.n_items = int(hp["iptr"][p1] - hp["iptr"][p0])
        cs.gval = self.gval.data_ptr() if self.gval is not None else None
        cs.ent = self.ent.data_ptr() if getattr(self, "ent", None) is not None else None
        cs.pc_ent = self.pc_ent.data_ptr() if getattr(self, "pc_ent", None) is not None else None
        cs.pc_gval = self.pc_gval.data_ptr() if self.pc_gval is not None else None
        return cs

    def to_dense(self):
        out = torch.zeros(self.n_rows, self.n_cols, dtype=torch.float32, device=self.device)
        lens = (self.row_ptr[1:] - self.row_ptr[:-1]).to(torch.int64)
        rows = torch.repeat_interleave(
            torch.arange(self.n_rows, device=self.device), lens)
        out[rows, self.col_idx.to(torch.int64)] = self.val
        return out
