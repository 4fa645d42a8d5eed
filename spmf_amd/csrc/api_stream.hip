// api_stream.hip -- the streaming calls behind the C-ABI (include/spmf_hip.h): the draw stage, its consumers'
// entries, spmf_knn, spmf_kmeans_step, spmf_silhouette, spmf_graph_layout, spmf_graph_transform and the graph
// products of spectral.hip (spmf_graph_scale, spmf_graph_spmm, spmf_block_gram, spmf_block_rotate) and the sweep of
// graph_move.hip (spmf_graph_move).  Host-side orchestration only (ctx.h).
#include <stdlib.h>

#include "ctx.h"

using namespace spmf;

extern "C" {

// ---- the draw stage of the streaming calls ---------------------------------------------------
// spmf_waic_accumulate (and its _cols form), spmf_topk_rows, spmf_score_cells, spmf_rank_cells, spmf_predict_columns,
// spmf_toprows_columns, spmf_group_sums, spmf_set_scores and spmf_embed_rows are one stage and a consumer each (spmf_knn, at the end of the section,
// takes rows as given and shares the scratch and launch helpers only).
// The stage: for S draws the per-draw tables (prep) and the encoded rows z[S,B,KP] go into the caller's scratch;
// the consumer kernel then reads z, V' and phi of every draw (kernels.h DrawTables).  The context's workspace is
// not used, so a step that is bound (or half way: spmf_step_begin .. spmf_step_end) keeps everything it has.
// Scratch of a call = one arena (arena.h): the draw tables first, the consumer's own buffers behind them.  Each
// call has one layout function, which takes the arena and the call's argument struct and names every buffer
// once; its spmf_*_scratch_bytes is that function on an arena without memory.
// An entry is: draw_check, its layout on the caller's scratch and byte count with the SPMF_E_WORKSPACE failure
// where that does not fit (scratch_too_small), its own argument checks -- in front of the layout where it depends
// on them --, its empty returns, draw_stage, `launched`.  What two entries need alike is written once:
// draw_tables, stored_layout, panel_tables, check_column_list.
static void draw_tables(Arena& a, const spmf_ctx* c, int64_t rows, int S, Tables& T) {
  const size_t KP = c->KP, D = c->D, nS = S;
  T.Ap = a.take<float>(nS * D * KP);
  T.Vp = a.take<float>(nS * D * KP);
  T.phi = a.take<float>(nS * D);
  T.dprep = a.take<double>(nS * kPrepSeg * (KP + 1));
  T.dacc = a.take<double>((size_t)kDaccRep * (kDaccHead + KP));
  T.z = T.gzs = a.take<float>(nS * (size_t)rows * KP);
}
static size_t draw_tables_bytes(const spmf_ctx* c, int64_t rows, int S) {
  Arena a;
  Tables T;
  draw_tables(a, c, rows, S, T);
  return a.used;
}

// The SPMF_E_WORKSPACE failure of a call `fn` whose scratch holds `have` bytes where its layout takes `need` for
// the shape `detail` ("rows=70 S=2").
static int scratch_too_small(spmf_ctx* c, const char* fn, size_t need, size_t have, const std::string& detail) {
  return fail(c, SPMF_E_WORKSPACE, std::string(fn) + ": scratch too small: need " + std::to_string(need) +
      " bytes for " + detail + ", have " + std::to_string(have));
}
static std::string rows_S(const spmf_counts* ct, int S) {
  return "rows=" + std::to_string((long long)ct->n_rows) + " S=" + std::to_string(S);
}
// The end of every entry: `ok` is what its launcher returned, `no_kernel` the entry's text for false.
static int launched(spmf_ctx* c, bool ok, const char* no_kernel) {
  if (!ok) return fail(c, SPMF_E_UNSUPPORTED, no_kernel);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

// What every streaming call `fn` checks before anything is launched: S in min_S..65535, the shared pointers, the
// scratch's alignment, the column types of a mixed context and the counts.  Behind it the context, the counts and
// S are fit to run the call's layout on: the scratch's size is the entry's next check, or, where the layout
// depends on further arguments, the one behind their checks.
static int draw_check(spmf_ctx* c, const char* fn, const spmf_counts* ct, int S, int min_S,
    const float* const params[SPMF_NVARS], const float* eta, const void* scratch) {
  if (!c) return SPMF_E_ARG;
  const std::string f = std::string(fn) + ": ";
  if (S < min_S || S > 65535) return fail(c, SPMF_E_ARG, f + (min_S == 2 ? "S must be in 2..65535 (the variance "
      "over the draws needs two)" : "S must be in 1..65535"));
  if (!params || !eta || !scratch) return fail(c, SPMF_E_ARG, f + "null argument");
  if (!params[2] || !params[0] || !params[1] || !params[7]) return fail(c, SPMF_E_ARG, f + "params u, v, w, s "
      "(slots 2, 0, 1, 7) must be set, each [S, ...]");
  if ((uintptr_t)scratch & 255) return fail(c, SPMF_E_ARG, f + "scratch must be 256-byte aligned");
  if (likelihood_code(c) == 3 && !c->ctype) return fail(c, SPMF_E_ARG, f + "spmf_ctx_set_column_types was not "
      "called");
  const int rc = check_counts(c, ct);   // (the scratch is sized by the batch; encode_rows checks the rest)
  if (rc) return rc;
  // the encode sweep of S draws gathers z with 32-bit byte offsets per draw; the consumers' row blocks are a
  // 31-bit grid extent, a listed cell's row an int32
  if (ct->n_rows > ((int64_t)1 << 31) - 64) return fail(c, SPMF_E_ARG, f + "too many rows in one call");
  return SPMF_OK;
}

// The stage of a checked call: the tables T inside its scratch (draw_tables), filled by the prep launch (S draws)
// and the encode sweep, which writes z and nothing else: gzs and the scalar block are never touched.  `dt` is
// what the consumer reads.  Nothing is launched for an empty batch.
static int draw_stage(spmf_ctx* c, const char* fn, const spmf_counts* ct, int S,
    const float* const params[SPMF_NVARS], const float* eta, const Tables& T, hipStream_t st, DrawTables& dt) {
  dt = DrawTables{ct->n_rows, c->D, c->KP, S, likelihood_code(c), T.z, T.Vp, T.phi, c->ctype};
  return encode_rows(c, fn, ct, S, &T, params[2], params[0], params[1], params[7], eta, st);
}
// waic_accumulate, score_cells and embed_rows, whose scratch is the draw tables alone: draw_check, and the tables
// T laid out in the scratch with the size check
static int draw_only_check(spmf_ctx* c, const char* fn, const spmf_counts* ct, int S, int min_S,
    const float* const params[SPMF_NVARS], const float* eta, void* scratch, size_t scratch_bytes, Tables& T) {
  const int rc = draw_check(c, fn, ct, S, min_S, params, eta, scratch);
  if (rc) return rc;
  Arena a(scratch, scratch_bytes);
  draw_tables(a, c, ct->n_rows, S, T);
  return a.fits() ? SPMF_OK : scratch_too_small(c, fn, a.used, scratch_bytes, rows_S(ct, S));
}

// ---- streaming WAIC (waic.hip) ------------------------------------------------------------
size_t spmf_waic_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int S) {
  if (!c || n_rows < 0 || S < 2) return 0;
  return draw_tables_bytes(c, n_rows, S);
}

// The body of the two entries; `fn` stands in front of every message, col_out may be NULL.
static int waic_accumulate(spmf_ctx* c, const char* fn, const spmf_counts* ct, int S,
    const float* const params[SPMF_NVARS], const float* eta, double* sums6, double* row_out, double* col_out,
    void* scratch, size_t scratch_bytes, void* stream) {
  Tables T;
  int rc = draw_only_check(c, fn, ct, S, 2, params, eta, scratch, scratch_bytes, T);
  if (rc) return rc;
  const std::string f = std::string(fn) + ": ";
  if (!sums6) return fail(c, SPMF_E_ARG, f + "null argument");
  if ((int64_t)(c->D + 63) / 64 > 65535) return fail(c, SPMF_E_UNSUPPORTED, f + "D above 65535 * 64");
  hipStream_t st = (hipStream_t)stream;
  DrawTables dt;
  rc = draw_stage(c, fn, ct, S, params, eta, T, st, dt);
  if (rc || ct->n_rows == 0) return rc;
  WaicArgs wa{dt, ct->nnz, ct->row_ptr, ct->col_idx, ct->val, sums6, row_out, col_out};
  return launched(c, launch_waic(wa, st), (f + "no kernel for this K / likelihood").c_str());
}

int spmf_waic_accumulate(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS],
    const float* eta, double* sums6, double* row_out, void* scratch, size_t scratch_bytes, void* stream) {
  return waic_accumulate(c, "waic_accumulate", ct, S, params, eta, sums6, row_out, nullptr, scratch, scratch_bytes,
      stream);
}

int spmf_waic_accumulate_cols(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS],
    const float* eta, double* sums6, double* row_out, double* col_out, void* scratch, size_t scratch_bytes,
    void* stream) {
  return waic_accumulate(c, "waic_accumulate_cols", ct, S, params, eta, sums6, row_out, col_out, scratch,
      scratch_bytes, stream);
}

// ---- streaming per-row top-k of the posterior predictive mean (topk.hip) ---------------------
static int device_cus(const spmf_ctx* c) {
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || n < 1) {
    (void)hipGetLastError();
    n = 256;   // no device to ask (a host-only caller sizing a scratch): an MI355X
  }
  return n;
}
// Column slices (gridDim.y) of the select launch.  A workgroup owns 64 rows and sweeps the column blocks of its
// slice, and two workgroups are resident per CU at the widest candidate buffer: with fewer than 2 * CUs row
// blocks the columns are split until the grid has that many workgroups -- never into more slices than column
// blocks or than the merge kernel holds (kTopkMaxSlices) -- and the count is then lowered to the slices that
// ceil(blocks / slices) blocks each leave non-empty.  At 2 * CUs row blocks and above: one slice, no merge.
static int topk_slices(int64_t n_rows, int D, int cus) {
  const int64_t rb = (n_rows + 63) / 64, cb = ((int64_t)D + 63) / 64;
  if (rb < 1 || rb >= 2 * (int64_t)cus) return 1;
  int64_t nsl = (2 * (int64_t)cus + rb - 1) / rb;
  if (nsl > kTopkMaxSlices) nsl = kTopkMaxSlices;
  if (nsl > cb) nsl = cb;
  const int64_t per = (cb + nsl - 1) / nsl;
  return (int)((cb + per - 1) / per);
}
// Scratch of rank_cells, and the head of top-k's: the draw tables and the bitmap of the stored cells of `rows` rows,
// a bit per column in 32-bit words (topk_mark_kernel), whatever the call's flags; `slices` of the select launch
static size_t stored_words(const spmf_ctx* c, int64_t rows) { return (size_t)rows * ((c->D + 31) / 32); }
static void stored_layout(Arena& a, const spmf_ctx* c, int64_t rows, int S, Tables& T, uint32_t*& stored, int& slices) {
  draw_tables(a, c, rows, S, T);
  stored = a.take<uint32_t>(stored_words(c, rows));
  slices = topk_slices(rows, c->D, device_cus(c));
}
// The bitmap of a laid-out call: zeroed on the stream when flag bit 0 (exclude stored cells) is set, else NULL.
static int stored_bits(spmf_ctx* c, unsigned flags, int64_t rows, hipStream_t st, uint32_t*& stored) {
  if (!(flags & 1u)) stored = nullptr;
  else HIPCHK(c, hipMemsetAsync(stored, 0, stored_words(c, rows) * sizeof(uint32_t), st));
  return SPMF_OK;
}

// Scratch of one top-k call: the draw tables, the bitmap and the slices' results (sized for k = kTopkMaxK: the size
// does not depend on the call's k or flags)
static void topk_layout(Arena& a, const spmf_ctx* c, int64_t rows, int S, Tables& T, TopkArgs& ta) {
  stored_layout(a, c, rows, S, T, ta.stored, ta.slices);
  const size_t part = ta.slices > 1 ? (size_t)ta.slices * rows * kTopkMaxK : 0;
  ta.part_cols = a.take<int32_t>(part);
  ta.part_scores = a.take<float>(part);
}

size_t spmf_topk_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int S) {
  if (!c || n_rows < 0 || S < 1) return 0;
  Arena a;
  Tables T;
  TopkArgs ta{};
  topk_layout(a, c, n_rows, S, T, ta);
  return a.used;
}

int spmf_topk_rows(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS], const float* eta,
    int k, unsigned flags, int32_t* cols_out, float* score_out, void* scratch, size_t scratch_bytes, void* stream) {
  int rc = draw_check(c, "topk_rows", ct, S, 1, params, eta, scratch);
  if (rc) return rc;
  Tables T;
  TopkArgs ta{};
  Arena a(scratch, scratch_bytes);
  topk_layout(a, c, ct->n_rows, S, T, ta);
  if (!a.fits()) return scratch_too_small(c, "topk_rows", a.used, scratch_bytes, rows_S(ct, S));
  if (k < 1 || k > kTopkMaxK) return fail(c, SPMF_E_ARG, "topk_rows: k must be in 1..64");
  if (flags & ~1u) return fail(c, SPMF_E_ARG, "topk_rows: unknown flag (bit 0: exclude stored cells)");
  if (!cols_out || !score_out) return fail(c, SPMF_E_ARG, "topk_rows: null argument");
  hipStream_t st = (hipStream_t)stream;
  rc = draw_stage(c, "topk_rows", ct, S, params, eta, T, st, ta.t);
  if (rc || ct->n_rows == 0) return rc;
  ta.nnz = ct->nnz; ta.k = k;
  ta.row_ptr = ct->row_ptr; ta.col = ct->col_idx;
  rc = stored_bits(c, flags, ct->n_rows, st, ta.stored);
  if (rc) return rc;
  ta.cols = cols_out; ta.scores = score_out;
  return launched(c, launch_topk(ta, st), "topk_rows: no kernel for this K / likelihood");
}

// ---- posterior predictive mean / lppd of a list of cells (cells.hip) --------------------------
// Scratch of one call: the draw tables alone.
size_t spmf_cells_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int S) {
  if (!c || n_rows < 0 || S < 1) return 0;
  return draw_tables_bytes(c, n_rows, S);
}

int spmf_score_cells(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS], const float* eta,
    int64_t n_cells, const int32_t* cell_row, const int32_t* cell_col, const float* cell_val, float* mean_out,
    float* lppd_out, void* scratch, size_t scratch_bytes, void* stream) {
  Tables T;
  int rc = draw_only_check(c, "score_cells", ct, S, 1, params, eta, scratch, scratch_bytes, T);
  if (rc) return rc;
  if (n_cells < 0) return fail(c, SPMF_E_ARG, "score_cells: n_cells is negative");
  if (n_cells > 0 && (!cell_row || !cell_col || !mean_out)) return fail(c, SPMF_E_ARG, "score_cells: cell_row, "
      "cell_col and mean_out must be set for a non-empty list");
  if ((cell_val == nullptr) != (lppd_out == nullptr)) return fail(c, SPMF_E_ARG, "score_cells: cell_val and lppd_out "
      "go together (both NULL: the mean only)");
  // the cell kernel's grid is a 31-bit extent of 256-cell workgroups
  if (n_cells > ((int64_t)1 << 38)) return fail(c, SPMF_E_ARG, "score_cells: too many cells in one call");
  if (n_cells == 0 || ct->n_rows == 0) return SPMF_OK;   // (no row: no valid cell; the Python surface lists none)
  hipStream_t st = (hipStream_t)stream;
  DrawTables dt;
  rc = draw_stage(c, "score_cells", ct, S, params, eta, T, st, dt);
  if (rc) return rc;
  CellsArgs ca{dt, n_cells, cell_row, cell_col, cell_val, mean_out, lppd_out};
  return launched(c, launch_cells(ca, st), "score_cells: no kernel for this K / likelihood");
}

// ---- rank of listed cells among their row's candidates (rank.hip) ------------------------------
// Scratch of one call: stored_layout (the size does not depend on the flags); the kernel keeps everything else in
// LDS and in the caller's outputs.
size_t spmf_rank_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int S) {
  if (!c || n_rows < 0 || S < 1) return 0;
  Arena a;
  Tables T;
  RankArgs ra{};
  stored_layout(a, c, n_rows, S, T, ra.stored, ra.slices);
  return a.used;
}

int spmf_rank_cells(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS], const float* eta,
    int64_t n_cells, const int32_t* cell_row, const int32_t* cell_col, unsigned flags, int32_t* rank_out,
    int32_t* cand_out, float* score_out, void* scratch, size_t scratch_bytes, void* stream) {
  int rc = draw_check(c, "rank_cells", ct, S, 1, params, eta, scratch);
  if (rc) return rc;
  Tables T;
  RankArgs ra{};
  Arena a(scratch, scratch_bytes);
  stored_layout(a, c, ct->n_rows, S, T, ra.stored, ra.slices);
  if (!a.fits()) return scratch_too_small(c, "rank_cells", a.used, scratch_bytes, rows_S(ct, S));
  if (n_cells < 0) return fail(c, SPMF_E_ARG, "rank_cells: n_cells is negative");
  if (n_cells > 0 && (!cell_row || !cell_col || !rank_out || !cand_out || !score_out)) return fail(c, SPMF_E_ARG,
      "rank_cells: cell_row, cell_col, rank_out, cand_out and score_out must be set for a non-empty list");
  if (flags & ~1u) return fail(c, SPMF_E_ARG, "rank_cells: unknown flag (bit 0: exclude stored cells)");
  if (n_cells == 0 || ct->n_rows == 0) return SPMF_OK;   // (no row: no valid cell; the Python surface lists none)
  hipStream_t st = (hipStream_t)stream;
  rc = draw_stage(c, "rank_cells", ct, S, params, eta, T, st, ra.t);
  if (rc) return rc;
  ra.nnz = ct->nnz;
  ra.row_ptr = ct->row_ptr; ra.col = ct->col_idx;
  rc = stored_bits(c, flags, ct->n_rows, st, ra.stored);
  if (rc) return rc;
  ra.n_cells = n_cells; ra.cell_row = cell_row; ra.cell_col = cell_col;
  ra.rank = rank_out; ra.cand = cand_out; ra.score = score_out;
  return launched(c, launch_rank(ra, st), "rank_cells: no kernel for this K / likelihood");
}

// ---- predictions of a panel of columns (panel.hip) ---------------------------------------------
// The compacted tables of a panel of C listed columns for S draws (V' rows, phi, the column types), three
// regions, into the Vc / phic / ctc of PanelArgs, GroupArgs or SetArgs.
static void panel_tables(Arena& a, const spmf_ctx* c, int S, size_t C, float*& Vc, float*& phic, uint8_t*& ctc) {
  const size_t KP = c->KP, nS = S;
  Vc = a.take<float>(nS * C * KP);
  phic = a.take<float>(nS * C);
  ctc = a.take<uint8_t>(C);
}
// Scratch of one call: the draw tables and, behind them, the compacted tables in a region of their own (the draw
// tables' Ap is not reused), sized for n_cols = D: the size does not depend on the list.
static void predict_layout(Arena& a, const spmf_ctx* c, int64_t rows, int S, Tables& T, PanelArgs& pa) {
  draw_tables(a, c, rows, S, T);
  panel_tables(a, c, S, c->D, pa.Vc, pa.phic, pa.ctc);
}
// The column list of a call `fn`: n_cols in 0..D, and no list is all D columns.
static int check_column_list(spmf_ctx* c, const char* fn, int32_t n_cols, const int32_t* cols) {
  const std::string f = std::string(fn) + ": ";
  if (n_cols < 0 || n_cols > c->D) return fail(c, SPMF_E_ARG, f + "n_cols must be in 0..D");
  if (!cols && n_cols != c->D) return fail(c, SPMF_E_ARG, f + "cols == NULL is all columns: n_cols must be D");
  return SPMF_OK;
}

size_t spmf_predict_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int S) {
  if (!c || n_rows < 0 || S < 1) return 0;
  Arena a;
  Tables T;
  PanelArgs pa{};
  predict_layout(a, c, n_rows, S, T, pa);
  return a.used;
}

int spmf_predict_columns(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS],
    const float* eta, int32_t n_cols, const int32_t* cols, float* mean_out, float* sd_out, float* pnz_out,
    void* scratch, size_t scratch_bytes, void* stream) {
  int rc = draw_check(c, "predict_columns", ct, S, 1, params, eta, scratch);
  if (rc) return rc;
  Tables T;
  PanelArgs pa{};
  Arena a(scratch, scratch_bytes);
  predict_layout(a, c, ct->n_rows, S, T, pa);
  if (!a.fits()) return scratch_too_small(c, "predict_columns", a.used, scratch_bytes, rows_S(ct, S));
  rc = check_column_list(c, "predict_columns", n_cols, cols);
  if (rc) return rc;
  if (sd_out && S < 2) return fail(c, SPMF_E_ARG, "predict_columns: sd_out needs S >= 2 (the deviation over the "
      "draws)");
  const bool work = n_cols > 0 && ct->n_rows > 0;
  if (work && !mean_out) return fail(c, SPMF_E_ARG, "predict_columns: mean_out must be set");
  if (((int64_t)n_cols + 63) / 64 > 65535) return fail(c, SPMF_E_UNSUPPORTED, "predict_columns: n_cols above "
      "65535 * 64");
  if (!work) return SPMF_OK;
  hipStream_t st = (hipStream_t)stream;
  rc = draw_stage(c, "predict_columns", ct, S, params, eta, T, st, pa.t);
  if (rc) return rc;
  pa.n_cols = n_cols; pa.cols = cols;
  pa.mean = mean_out; pa.sd = sd_out; pa.pnz = pnz_out;
  return launched(c, launch_panel(pa, st), "predict_columns: no kernel for this K / likelihood");
}

// ---- streaming per-column top-k rows of the posterior predictive mean (toprows.hip) -------------
// Scratch of one call: stored_layout (the draw tables and the bitmap, whatever the flags), the compacted tables of
// a listed panel sized for n_cols (panel_tables), and the row slices' results (sized for k = kTopkMaxK: the size
// does not depend on the call's k or flags).  The slices are topk_slices with the roles swapped, as in knn_layout:
// the keys are the column blocks of the panel, the candidates the row blocks.
static void toprows_layout(Arena& a, const spmf_ctx* c, int64_t rows, int S, int n_cols, Tables& T, TopRowsArgs& ra) {
  int topk_own;   // (the column slices of a top-k launch over these rows: not this call's)
  stored_layout(a, c, rows, S, T, ra.stored, topk_own);
  panel_tables(a, c, S, (size_t)n_cols, ra.Vc, ra.phic, ra.ctc);
  const int64_t cand_rows = rows < 0x7fffffffLL - 63 ? rows : 0x7fffffffLL - 63;   // (draw_check's bound)
  ra.slices = rows > 0 && n_cols > 0 ? topk_slices(n_cols, (int)cand_rows, device_cus(c)) : 1;
  const size_t part = ra.slices > 1 ? (size_t)ra.slices * n_cols * kTopkMaxK : 0;
  ra.part_rows = a.take<int32_t>(part);
  ra.part_scores = a.take<float>(part);
}

size_t spmf_toprows_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int S, int32_t n_cols) {
  if (!c || n_rows < 0 || S < 1 || n_cols < 0 || n_cols > c->D) return 0;
  Arena a;
  Tables T;
  TopRowsArgs ra{};
  toprows_layout(a, c, n_rows, S, n_cols, T, ra);
  return a.used;
}

int spmf_toprows_columns(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS],
    const float* eta, int32_t n_cols, const int32_t* cols, int k, unsigned flags, int32_t* rows_out,
    float* scores_out, void* scratch, size_t scratch_bytes, void* stream) {
  int rc = draw_check(c, "toprows_columns", ct, S, 1, params, eta, scratch);
  if (rc) return rc;
  // (the scratch's size depends on n_cols: it is checked behind the list)
  rc = check_column_list(c, "toprows_columns", n_cols, cols);
  if (rc) return rc;
  Tables T;
  TopRowsArgs ra{};
  Arena a(scratch, scratch_bytes);
  toprows_layout(a, c, ct->n_rows, S, n_cols, T, ra);
  if (!a.fits()) return scratch_too_small(c, "toprows_columns", a.used, scratch_bytes,
      rows_S(ct, S) + " cols=" + std::to_string(n_cols));
  if (k < 1 || k > kTopkMaxK) return fail(c, SPMF_E_ARG, "toprows_columns: k must be in 1..64");
  if (flags & ~1u) return fail(c, SPMF_E_ARG, "toprows_columns: unknown flag (bit 0: exclude stored cells)");
  if (n_cols > 0 && (!rows_out || !scores_out)) return fail(c, SPMF_E_ARG, "toprows_columns: rows_out and "
      "scores_out must be set for a non-empty list");
  if (n_cols == 0) return SPMF_OK;
  hipStream_t st = (hipStream_t)stream;
  if (ct->n_rows == 0) {   // no row: every column is padding (-1 is all bits set, -inf is 0xff800000)
    const size_t n = (size_t)n_cols * k;
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)rows_out, -1, n, st));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)scores_out, (int)0xff800000u, n, st));
    return SPMF_OK;
  }
  rc = draw_stage(c, "toprows_columns", ct, S, params, eta, T, st, ra.t);
  if (rc) return rc;
  ra.nnz = ct->nnz; ra.n_cols = n_cols; ra.k = k; ra.cols = cols;
  ra.row_ptr = ct->row_ptr; ra.col = ct->col_idx;
  rc = stored_bits(c, flags, ct->n_rows, st, ra.stored);
  if (rc) return rc;
  ra.rows = rows_out; ra.scores = scores_out;
  return launched(c, launch_toprows(ra, st), "toprows_columns: no kernel for this K / likelihood");
}

// ---- per-group sums of the predictions over the rows (groups.hip) ------------------------------
// Scratch of one call: the draw tables and, behind them, the ordering (chunk table, ranks, counts, offsets, block
// records, the padded row order), the rows z in that order, the compacted tables of a listed panel sized for
// n_cols (panel_tables), and the partial sums of one column range (kernels.h group_geom bounds them).
constexpr int32_t kGroupMaxGroups = 1 << 24;
static void groups_layout(Arena& a, const spmf_ctx* c, int64_t rows, int S, int G, int C, Tables& T, GroupArgs& ga) {
  const GroupGeom q = group_geom(rows, S, G, C);
  const size_t KP = c->KP, nS = S, nG = G, NB = (size_t)q.NB;
  draw_tables(a, c, rows, S, T);
  ga.tbl = a.take<int32_t>((size_t)q.chunks * nG);
  ga.lrank = a.take<int32_t>((size_t)rows);
  ga.cnt = a.take<int32_t>(nG);
  ga.boff = a.take<int32_t>(nG + 1);
  ga.fincl = a.take<int32_t>(nG);
  ga.rec = a.take<int4>(NB);
  ga.perm = a.take<int32_t>(NB * 64);
  ga.zs = a.take<float>(nS * NB * 64 * KP);
  panel_tables(a, c, S, C, ga.Vc, ga.phic, ga.ctc);
  ga.part = a.take<double>(q.part_bytes / sizeof(double));   // (whole doubles: group_geom)
}

size_t spmf_groups_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int S, int32_t n_groups, int32_t n_cols) {
  if (!c || n_rows < 0 || S < 1 || n_groups < 1 || n_groups > kGroupMaxGroups || n_cols < 0 || n_cols > c->D)
    return 0;
  Arena a;
  Tables T;
  GroupArgs ga{};
  groups_layout(a, c, n_rows, S, n_groups, n_cols, T, ga);
  return a.used;
}

int spmf_group_sums(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS],
    const float* eta, const int32_t* labels, int32_t n_groups, int32_t n_cols, const int32_t* cols,
    double* sum_out, double* nonzero_out, void* scratch, size_t scratch_bytes, void* stream) {
  int rc = draw_check(c, "group_sums", ct, S, 1, params, eta, scratch);
  if (rc) return rc;
  // (the scratch's size depends on n_groups and n_cols: it is checked behind them)
  if (n_groups < 1) return fail(c, SPMF_E_ARG, "group_sums: n_groups must be at least 1");
  rc = check_column_list(c, "group_sums", n_cols, cols);
  if (rc) return rc;
  if (n_groups > kGroupMaxGroups) return fail(c, SPMF_E_UNSUPPORTED, "group_sums: n_groups above 2^24");
  Tables T;
  GroupArgs ga{};
  Arena a(scratch, scratch_bytes);
  groups_layout(a, c, ct->n_rows, S, n_groups, n_cols, T, ga);
  if (!a.fits()) return scratch_too_small(c, "group_sums", a.used, scratch_bytes,
      rows_S(ct, S) + " groups=" + std::to_string(n_groups) + " cols=" + std::to_string(n_cols));
  const bool work = n_cols > 0 && ct->n_rows > 0;
  if (work && (!labels || !sum_out)) return fail(c, SPMF_E_ARG, "group_sums: labels and sum_out must be set");
  if (!work) return SPMF_OK;
  hipStream_t st = (hipStream_t)stream;
  rc = draw_stage(c, "group_sums", ct, S, params, eta, T, st, ga.t);
  if (rc) return rc;
  ga.n_groups = n_groups; ga.n_cols = n_cols; ga.labels = labels; ga.cols = cols;
  ga.sum = sum_out; ga.nonzero = nonzero_out;
  return launched(c, launch_groups(ga, st), "group_sums: no kernel for this K / likelihood");
}

// ---- per-row sums of the predictions over column sets (sets.hip) -------------------------------
// The padded columns of the host array set_ptr[0 .. n_sets]: every set in whole 64-column blocks.  -1: set_ptr is
// not 0 = set_ptr[0] <= set_ptr[1] <= ..; -2: the padded total is beyond the int32 column blocks of a launch.
static int64_t set_padded_cols(int32_t n_sets, const int64_t* set_ptr) {
  if (n_sets == 0) return 0;
  if (!set_ptr || set_ptr[0] != 0) return -1;
  int64_t blocks = 0;
  for (int32_t g = 0; g < n_sets; ++g) {
    const int64_t n = set_ptr[g + 1] - set_ptr[g];
    if (n < 0) return -1;
    if (n > ((int64_t)1 << 31)) return -2;
    blocks += (n + 63) / 64;
    if (blocks > (((int64_t)1 << 31) - 64) / 64) return -2;
  }
  return blocks * 64;
}
// Scratch of one call: the draw tables and, behind them, the compacted tables of the padded list (panel_tables),
// the padded list itself, its weights and the sets' records.
static void sets_layout(Arena& a, const spmf_ctx* c, int64_t rows, int S, int32_t n_sets, int64_t padded, Tables& T,
    SetArgs& sa) {
  draw_tables(a, c, rows, S, T);
  panel_tables(a, c, S, (size_t)padded, sa.Vc, sa.phic, sa.ctc);
  sa.colsp = a.take<int32_t>((size_t)padded);
  sa.wp = a.take<float>((size_t)padded);
  sa.srec = a.take<int2>((size_t)n_sets);
}

size_t spmf_sets_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int S, int32_t n_sets, const int64_t* set_ptr) {
  if (!c || n_rows < 0 || S < 1 || n_sets < 0) return 0;
  const int64_t padded = set_padded_cols(n_sets, set_ptr);
  if (padded < 0) return 0;
  Arena a;
  Tables T;
  SetArgs sa{};
  sets_layout(a, c, n_rows, S, n_sets, padded, T, sa);
  return a.used;
}

int spmf_set_scores(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS],
    const float* eta, int32_t n_sets, const int64_t* set_ptr, const int32_t* set_cols, const float* set_weights,
    int64_t ld, double* mean_out, double* sd_out, void* scratch, size_t scratch_bytes, void* stream) {
  int rc = draw_check(c, "set_scores", ct, S, 1, params, eta, scratch);
  if (rc) return rc;
  // (the scratch's size depends on the sets: it is checked behind them)
  if (n_sets < 0) return fail(c, SPMF_E_ARG, "set_scores: n_sets must be >= 0");
  if (n_sets > 0 && !set_ptr) return fail(c, SPMF_E_ARG, "set_scores: set_ptr (host, n_sets + 1) must be set");
  const int64_t padded = set_padded_cols(n_sets, set_ptr);
  if (padded == -1) return fail(c, SPMF_E_ARG, "set_scores: set_ptr must start at 0 and be non-decreasing");
  if (padded < 0) return fail(c, SPMF_E_UNSUPPORTED, "set_scores: the padded list is beyond 2^31 columns");
  if (ld < n_sets) return fail(c, SPMF_E_ARG, "set_scores: ld must be at least n_sets");
  if (sd_out && S < 2) return fail(c, SPMF_E_ARG, "set_scores: sd_out needs S >= 2 (the deviation over the draws)");
  Tables T;
  SetArgs sa{};
  Arena a(scratch, scratch_bytes);
  sets_layout(a, c, ct->n_rows, S, n_sets, padded, T, sa);
  if (!a.fits()) return scratch_too_small(c, "set_scores", a.used, scratch_bytes,
      rows_S(ct, S) + " sets=" + std::to_string(n_sets) + " padded columns=" + std::to_string((long long)padded));
  const bool work = n_sets > 0 && ct->n_rows > 0;
  if (work && !mean_out) return fail(c, SPMF_E_ARG, "set_scores: mean_out must be set");
  if (work && padded > 0 && !set_cols) return fail(c, SPMF_E_ARG, "set_scores: set_cols must be set");
  if (!work) return SPMF_OK;
  hipStream_t st = (hipStream_t)stream;
  sa.t = DrawTables{ct->n_rows, c->D, c->KP, S, likelihood_code(c), nullptr, nullptr, nullptr, c->ctype};
  if (padded > 0) {   // (all sets empty: the zero fill alone)
    rc = draw_stage(c, "set_scores", ct, S, params, eta, T, st, sa.t);
    if (rc) return rc;
  }
  sa.n_sets = n_sets; sa.set_ptr = set_ptr; sa.cols = set_cols; sa.weights = set_weights;
  sa.padded_cols = padded; sa.ld = ld; sa.mean = mean_out; sa.sd = sd_out;
  return launched(c, launch_sets(sa, st), "set_scores: no kernel for this K / likelihood");
}

// ---- posterior mean encoding of a batch (knn.hip) ---------------------------------------------
// Scratch of one call: the draw tables alone.
size_t spmf_embed_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int S) {
  if (!c || n_rows < 0 || S < 1) return 0;
  return draw_tables_bytes(c, n_rows, S);
}

int spmf_embed_rows(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS], const float* eta,
    float* mean_out, float* sd_out, void* scratch, size_t scratch_bytes, void* stream) {
  Tables T;
  int rc = draw_only_check(c, "embed_rows", ct, S, 1, params, eta, scratch, scratch_bytes, T);
  if (rc) return rc;
  if (!mean_out) return fail(c, SPMF_E_ARG, "embed_rows: null argument");
  if (sd_out && S < 2) return fail(c, SPMF_E_ARG, "embed_rows: sd_out needs S >= 2 (the deviation over the draws)");
  if (ct->n_rows == 0) return SPMF_OK;
  hipStream_t st = (hipStream_t)stream;
  DrawTables dt;
  rc = draw_stage(c, "embed_rows", ct, S, params, eta, T, st, dt);
  if (rc) return rc;
  launch_embed(dt, c->K, mean_out, sd_out, st);   // (one kernel for every K)
  return launched(c, true, "");
}

// ---- exact k nearest rows (knn.hip) -----------------------------------------------------------
// Scratch of one call: the working rows of the reference set and of the queries (sized for both, whether or not
// the call passes one array as both), the biases, the centre and its per-block partial sums, and the slices'
// results (sized for k = kTopkMaxK: the size does not depend on the call's k).
static int knn_padded(int row_len) {
  int kp = 4;
  while (kp < row_len) kp *= 2;
  return kp;
}
// The shape (the padded row length; the reference slices of the select launch, where the queries take the place
// of top-k's rows and the reference rows that of its columns) and the scratch of a call, all into ka
// (part_slots >= 0: the slots of the slices' results to carve instead of knn's own count -- kmeans_layout)
static void knn_layout(Arena& a, const spmf_ctx* c, int64_t n_query, int64_t n_ref, int row_len, KnnArgs& ka,
    int64_t part_slots = -1) {
  ka.n_query = n_query; ka.n_ref = n_ref; ka.row_len = row_len;
  ka.KP = knn_padded(row_len);
  ka.slices = n_ref > 0 ? topk_slices(n_query, (int)n_ref, device_cus(c)) : 1;
  const size_t nq = n_query, nr = n_ref, KP = ka.KP;
  ka.rw = a.take<float>(nr * KP);
  ka.bias = a.take<float>(nr);
  ka.qw = a.take<float>(nq * KP);
  ka.cpart = a.take<float>(kKnnCentreBlocks * KP);
  ka.ccnt = a.take<int32_t>(kKnnCentreBlocks);
  ka.centre = a.take<float>(KP);
  const size_t part = part_slots >= 0 ? (size_t)part_slots : ka.slices > 1 ? (size_t)ka.slices * nq * kTopkMaxK : 0;
  ka.part_idx = a.take<int32_t>(part);
  ka.part_score = a.take<float>(part);
}

size_t spmf_knn_scratch_bytes(const spmf_ctx* c, int64_t n_query, int64_t n_ref, int row_len) {
  if (!c || n_query < 0 || n_ref < 0 || n_ref > 0x7fffffffLL || row_len < 1 || row_len > 256) return 0;
  Arena a;
  KnnArgs ka{};
  knn_layout(a, c, n_query, n_ref, row_len, ka);
  return a.used;
}

// SPMF_KNN_TILE = 0 | 1 picks the tile function of the select kernel (knn.hip); both give the same bits
static int knn_tile() {
  const char* e = getenv("SPMF_KNN_TILE");
  return e && e[0] == '1' ? 1 : (e && e[0] == '0' ? 0 : kKnnDefaultTile);
}

int spmf_knn(spmf_ctx* c, const float* q, int64_t n_query, const float* r, int64_t n_ref, int row_len, int k,
    unsigned flags, int64_t self_offset, int32_t* idx_out, float* dist_out, void* scratch, size_t scratch_bytes,
    void* stream) {
  if (!c) return SPMF_E_ARG;
  if (n_query < 0 || n_ref < 0) return fail(c, SPMF_E_ARG, "knn: n_query and n_ref must not be negative");
  if (n_ref > 0x7fffffffLL) return fail(c, SPMF_E_ARG, "knn: n_ref above 2^31 - 1 (the indices are int32)");
  if (n_query > ((int64_t)1 << 31) - 64) return fail(c, SPMF_E_ARG, "knn: too many queries in one call");
  if (row_len < 1 || row_len > 256) return fail(c, SPMF_E_ARG, "knn: row_len must be in 1..256");
  if (k < 1 || k > kTopkMaxK) return fail(c, SPMF_E_ARG, "knn: k must be in 1..64");
  if (flags & ~1u) return fail(c, SPMF_E_ARG, "knn: unknown flag (bit 0: cosine)");
  if (self_offset < -1) return fail(c, SPMF_E_ARG, "knn: self_offset must be -1 (none) or the reference row of "
      "query 0");
  if (!scratch) return fail(c, SPMF_E_ARG, "knn: null argument");
  if ((n_query > 0 && (!q || !idx_out || !dist_out)) || (n_ref > 0 && !r)) return fail(c, SPMF_E_ARG,
      "knn: null argument");
  if ((uintptr_t)scratch & 255) return fail(c, SPMF_E_ARG, "knn: scratch must be 256-byte aligned");
  KnnArgs ka{};
  Arena a(scratch, scratch_bytes);
  knn_layout(a, c, n_query, n_ref, row_len, ka);
  if (!a.fits()) return scratch_too_small(c, "knn", a.used, scratch_bytes,
      "n_query=" + std::to_string((long long)n_query) + " n_ref=" + std::to_string((long long)n_ref) + " row_len=" +
      std::to_string(row_len));
  if (n_query == 0) return SPMF_OK;
  ka.k = k;
  ka.cosine = (flags & 1u) != 0; ka.tile = knn_tile(); ka.self_offset = self_offset;
  ka.q = q; ka.r = r;
  if (q == r && n_query == n_ref) ka.qw = ka.rw;
  ka.idx = idx_out; ka.dist = dist_out;
  return launched(c, launch_knn(ka, (hipStream_t)stream), "knn: no kernel for this row_len / k");
}

// ---- one Lloyd step of k-means (kmeans.hip behind knn.hip and groups.hip's ordering) -----------
// Scratch of one call: knn's carve for the rows as queries and the centroids as reference set, the refined
// candidates [rows][4], the ordering of the rows by label (launch_group_order), the segments' partial sums and the
// statistics' partial sums (kernels.h kmeans_geom bounds them).  knn's slices drop to one as the rows grow, and
// their results with them; here they are carved at their bound over all row counts, slices * rows <= 64 * (2 CUs +
// row blocks) with at most 4 candidates each, so that the size is non-decreasing in the rows.
constexpr int32_t kKmeansMaxClusters = 65536;
constexpr int kKmeansCand = 4;
static void kmeans_layout(Arena& a, const spmf_ctx* c, int64_t rows, int G, int row_len, KnnArgs& ka, KmeansArgs& ma) {
  const KmeansGeom q = kmeans_geom(rows, G);
  const size_t nr = rows, nG = G, NB = (size_t)q.NB;
  knn_layout(a, c, rows, G, row_len, ka, 64 * (2 * (int64_t)device_cus(c) + (rows + 63) / 64) * kKmeansCand);
  ka.k = ma.kc = G < kKmeansCand ? G : kKmeansCand;
  ka.idx = a.take<int32_t>(nr * kKmeansCand);
  ka.dist = a.take<float>(nr * kKmeansCand);
  ma.tbl = a.take<int32_t>((size_t)q.chunks * nG);
  ma.lrank = a.take<int32_t>(nr);
  ma.cnt = a.take<int32_t>(nG);
  ma.boff = a.take<int32_t>(nG + 1);
  ma.fincl = a.take<int32_t>(nG);
  ma.rec = a.take<int4>(NB);
  ma.perm = a.take<int32_t>(NB * 64);
  ma.part = a.take<double>((size_t)q.nseg * row_len);
  ma.spart = a.take<double>((size_t)q.sblocks * 3);
}
static bool kmeans_shape_ok(int64_t n_rows, int32_t G, int row_len) {
  return n_rows >= 0 && n_rows <= ((int64_t)1 << 31) - 64 && G >= 1 && G <= kKmeansMaxClusters && row_len >= 1 &&
      row_len <= 256;
}

size_t spmf_kmeans_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int32_t n_clusters, int row_len) {
  if (!c || !kmeans_shape_ok(n_rows, n_clusters, row_len)) return 0;
  Arena a;
  KnnArgs ka{};
  KmeansArgs ma{};
  kmeans_layout(a, c, n_rows, n_clusters, row_len, ka, ma);
  return a.used;
}

int spmf_kmeans_step(spmf_ctx* c, const float* x, int64_t n_rows, int row_len, const float* centroids,
    int32_t n_clusters, const int32_t* prev_labels, int32_t* labels_out, float* dist_out, double* sums_out,
    int64_t* counts_out, double* stats_out, void* scratch, size_t scratch_bytes, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "kmeans_step: ";
  if (n_clusters < 1 || n_clusters > kKmeansMaxClusters) return fail(c, SPMF_E_ARG, f + "n_clusters must be in "
      "1..65536");
  if (row_len < 1 || row_len > 256) return fail(c, SPMF_E_ARG, f + "row_len must be in 1..256");
  if (n_rows < 0 || n_rows > ((int64_t)1 << 31) - 64) return fail(c, SPMF_E_ARG, f + "n_rows must be in "
      "0..2^31 - 64");
  if (prev_labels && prev_labels == labels_out) return fail(c, SPMF_E_ARG, f + "prev_labels must not be labels_out");
  if (!scratch) return fail(c, SPMF_E_ARG, f + "null argument");
  if (!sums_out || !counts_out || !stats_out || (n_rows > 0 && (!x || !centroids || !labels_out))) return fail(c,
      SPMF_E_ARG, f + "null argument");
  if ((uintptr_t)scratch & 255) return fail(c, SPMF_E_ARG, f + "scratch must be 256-byte aligned");
  KnnArgs ka{};
  KmeansArgs ma{};
  Arena a(scratch, scratch_bytes);
  kmeans_layout(a, c, n_rows, n_clusters, row_len, ka, ma);
  if (!a.fits()) return scratch_too_small(c, "kmeans_step", a.used, scratch_bytes,
      "n_rows=" + std::to_string((long long)n_rows) + " n_clusters=" + std::to_string(n_clusters) + " row_len=" +
      std::to_string(row_len));
  hipStream_t st = (hipStream_t)stream;
  if (n_rows == 0) {
    HIPCHK(c, hipMemsetAsync(sums_out, 0, (size_t)n_clusters * row_len * sizeof(double), st));
    HIPCHK(c, hipMemsetAsync(counts_out, 0, (size_t)n_clusters * sizeof(int64_t), st));
    HIPCHK(c, hipMemsetAsync(stats_out, 0, 3 * sizeof(double), st));
    return SPMF_OK;
  }
  // the assignment: spmf_knn's launches with q = x, r = centroids, k = min(4, G), Euclidean, no self
  ka.cosine = false; ka.tile = knn_tile(); ka.self_offset = -1;
  ka.q = x; ka.r = centroids;
  if (!launch_knn(ka, st)) return fail(c, SPMF_E_UNSUPPORTED, f + "no kernel for this row_len");
  ma.n_rows = n_rows; ma.row_len = row_len; ma.n_clusters = n_clusters;
  ma.x = x; ma.cand_idx = ka.idx; ma.cand_dist = ka.dist; ma.prev = prev_labels;
  ma.labels = labels_out; ma.dist = dist_out; ma.sums = sums_out; ma.counts = counts_out; ma.stats = stats_out;
  launch_kmeans(ma, st);
  return launched(c, true, "");
}

// ---- the silhouette of labelled rows (silhouette.hip behind groups.hip's ordering) -------------
// Scratch of one call: the effective labels, the ordering of the members by label (launch_group_order), the
// working rows and biases in that order, the centre with its partial sums, and the blocks' sums of s (kernels.h
// silhouette_geom bounds the blocks).  Every region grows with the rows.
static void silhouette_layout(Arena& a, int64_t rows, int G, int row_len, SilhouetteArgs& sa) {
  const SilhouetteGeom q = silhouette_geom(rows, G);
  sa.n_rows = rows; sa.row_len = row_len; sa.n_clusters = G;
  sa.KP = knn_padded(row_len);
  const size_t nr = rows, nG = G, NB = (size_t)q.NB, KP = sa.KP;
  sa.eff = a.take<int32_t>(nr);
  sa.tbl = a.take<int32_t>((size_t)q.chunks * nG);
  sa.lrank = a.take<int32_t>(nr);
  sa.cnt = a.take<int32_t>(nG);
  sa.boff = a.take<int32_t>(nG + 1);
  sa.fincl = a.take<int32_t>(nG);
  sa.rec = a.take<int4>(NB);
  sa.perm = a.take<int32_t>(NB * 64);
  sa.w = a.take<float>(NB * 64 * KP);
  sa.bias = a.take<float>(NB * 64);
  sa.cpart = a.take<double>((size_t)kSilCentreBlocks * KP);
  sa.ccnt = a.take<int32_t>(kSilCentreBlocks);
  sa.centre = a.take<float>(KP);
  sa.spart = a.take<double>(NB);
}

size_t spmf_silhouette_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int32_t n_clusters, int row_len) {
  if (!c || !kmeans_shape_ok(n_rows, n_clusters, row_len)) return 0;
  Arena a;
  SilhouetteArgs sa{};
  silhouette_layout(a, n_rows, n_clusters, row_len, sa);
  return a.used;
}

int spmf_silhouette(spmf_ctx* c, const float* x, int64_t n_rows, int row_len, const int32_t* labels,
    int32_t n_clusters, unsigned flags, float* sil_out, float* a_out, float* b_out, int32_t* nearest_out,
    double* cluster_sum_out, int64_t* counts_out, void* scratch, size_t scratch_bytes, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "silhouette: ";
  if (n_clusters < 1 || n_clusters > kKmeansMaxClusters) return fail(c, SPMF_E_ARG, f + "n_clusters must be in "
      "1..65536");
  if (row_len < 1 || row_len > 256) return fail(c, SPMF_E_ARG, f + "row_len must be in 1..256");
  if (n_rows < 0 || n_rows > ((int64_t)1 << 31) - 64) return fail(c, SPMF_E_ARG, f + "n_rows must be in "
      "0..2^31 - 64");
  if (flags & ~1u) return fail(c, SPMF_E_ARG, f + "unknown flag (bit 0: cosine)");
  if (!scratch) return fail(c, SPMF_E_ARG, f + "null argument");
  if (!cluster_sum_out || !counts_out || (n_rows > 0 && (!x || !labels || !sil_out))) return fail(c, SPMF_E_ARG,
      f + "null argument");
  if ((uintptr_t)scratch & 255) return fail(c, SPMF_E_ARG, f + "scratch must be 256-byte aligned");
  SilhouetteArgs sa{};
  Arena a(scratch, scratch_bytes);
  silhouette_layout(a, n_rows, n_clusters, row_len, sa);
  if (!a.fits()) return scratch_too_small(c, "silhouette", a.used, scratch_bytes,
      "n_rows=" + std::to_string((long long)n_rows) + " n_clusters=" + std::to_string(n_clusters) + " row_len=" +
      std::to_string(row_len));
  hipStream_t st = (hipStream_t)stream;
  if (n_rows == 0) {
    HIPCHK(c, hipMemsetAsync(cluster_sum_out, 0, (size_t)n_clusters * sizeof(double), st));
    HIPCHK(c, hipMemsetAsync(counts_out, 0, (size_t)n_clusters * sizeof(int64_t), st));
    return SPMF_OK;
  }
  sa.cosine = (flags & 1u) != 0;
  sa.x = x; sa.labels = labels;
  sa.sil = sil_out; sa.a = a_out; sa.b = b_out; sa.nearest = nearest_out;
  sa.cluster_sum = cluster_sum_out; sa.counts = counts_out;
  return launched(c, launch_silhouette(sa, st), "silhouette: no kernel for this row_len");
}

// ---- the epochs of a 2-D graph layout (graph_layout.hip) ---------------------------------------
// Scratch of one call: the two position buffers the epochs alternate between; the first takes the start.
static bool graph_layout_rows_ok(int64_t n_rows) { return n_rows >= 0 && n_rows <= ((int64_t)1 << 31) - 64; }
static void graph_layout_carve(Arena& a, int64_t rows, GraphLayoutArgs& ga) {
  const size_t n = rows > 0 ? (size_t)rows : 1;
  ga.buf[0] = a.take<float2>(n);
  ga.buf[1] = a.take<float2>(n);
}

size_t spmf_graph_layout_scratch_bytes(const spmf_ctx* c, int64_t n_rows) {
  if (!c || !graph_layout_rows_ok(n_rows)) return 0;
  Arena a;
  GraphLayoutArgs ga{};
  graph_layout_carve(a, n_rows, ga);
  return a.used;
}

int spmf_graph_layout(spmf_ctx* c, int64_t n_rows, int64_t nnz, const int64_t* indptr, const int32_t* indices,
    const float* weights, const float* y_in, float* y_out, int epoch0, int n_epochs, int total_epochs, double lr,
    double a, double b, double repulsion, double negative_rate, int n_negatives, uint64_t seed, void* scratch,
    size_t scratch_bytes, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "graph_layout: ";
  auto weight_ok = [](double v) { return v >= 0.0 && v <= 3.0e38; };          // finite, not negative, an fp32
  if (!graph_layout_rows_ok(n_rows)) return fail(c, SPMF_E_ARG, f + "n_rows must be in 0..2^31 - 64");
  if (nnz < 0) return fail(c, SPMF_E_ARG, f + "nnz is negative");
  if (n_negatives < 1 || n_negatives > 64) return fail(c, SPMF_E_ARG, f + "n_negatives must be in 1..64");
  if (epoch0 < 0 || n_epochs < 0 || (int64_t)epoch0 + n_epochs > (int64_t)total_epochs) return fail(c, SPMF_E_ARG,
      f + "epochs: epoch0 >= 0, n_epochs >= 0 and epoch0 + n_epochs <= total_epochs must hold");
  if (!(a > 0.0) || !(b > 0.0) || !(a <= 3.0e38) || !(b <= 3.0e38)) return fail(c, SPMF_E_ARG, f + "a and b must be "
      "positive and finite");
  if (!weight_ok(lr) || !weight_ok(repulsion) || !weight_ok(negative_rate)) return fail(c, SPMF_E_ARG, f + "lr, "
      "repulsion and negative_rate must be finite and not negative");
  if (n_rows > 0 && (!indptr || !y_in || !y_out || (nnz > 0 && (!indices || !weights)))) return fail(c, SPMF_E_ARG,
      f + "null argument");
  if (!scratch) return fail(c, SPMF_E_ARG, f + "null argument");
  if ((uintptr_t)scratch & 255) return fail(c, SPMF_E_ARG, f + "scratch must be 256-byte aligned");
  GraphLayoutArgs ga{};
  Arena ar(scratch, scratch_bytes);
  graph_layout_carve(ar, n_rows, ga);
  if (!ar.fits()) return scratch_too_small(c, "graph_layout", ar.used, scratch_bytes,
      "n_rows=" + std::to_string((long long)n_rows));
  if (n_rows == 0) return SPMF_OK;
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = (size_t)n_rows * sizeof(float2);
  if (n_epochs == 0) {
    if (y_out != y_in) HIPCHK(c, hipMemcpyAsync(y_out, y_in, bytes, hipMemcpyDeviceToDevice, st));
    return SPMF_OK;
  }
  // the prologue: the start goes into the first buffer, so no epoch reads y_in or y_out (they may be one)
  HIPCHK(c, hipMemcpyAsync(ga.buf[0], y_in, bytes, hipMemcpyDeviceToDevice, st));
  ga.n_rows = n_rows; ga.nnz = nnz;
  ga.indptr = indptr; ga.indices = indices; ga.weights = weights;
  ga.y_out = (float2*)y_out;
  ga.epoch0 = epoch0; ga.n_epochs = n_epochs; ga.total_epochs = total_epochs; ga.n_negatives = n_negatives;
  ga.lr = lr;
  ga.a = (float)a; ga.b = (float)b;
  ga.neg2b = (float)(-2.0 * b);
  ga.two_gamma_b = (float)(2.0 * repulsion * b);
  ga.rate_over_m = (float)(negative_rate / (double)n_negatives);
  ga.seed_lo = (uint32_t)seed; ga.seed_hi = (uint32_t)(seed >> 32);
  launch_graph_layout(ga, st);
  return launched(c, true, "");
}

// ---- new rows on a fitted 2-D layout (graph_transform.hip) --------------------------------------
// No scratch: the one launch keeps a row's state in registers.
int spmf_graph_transform(spmf_ctx* c, int64_t n_query, int k, const int32_t* idx, const float* w,
    const float* y_ref, int64_t n_ref, const float* y_in, float* y_out, int64_t row0, int epoch0, int n_epochs,
    int total_epochs, double lr, double a, double b, double repulsion, double negative_rate, int n_negatives,
    uint64_t seed, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "graph_transform: ";
  auto weight_ok = [](double v) { return v >= 0.0 && v <= 3.0e38; };          // finite, not negative, an fp32
  if (k < 1 || k > 64) return fail(c, SPMF_E_ARG, f + "k must be in 1..64");
  if (n_negatives < 1 || n_negatives > 64) return fail(c, SPMF_E_ARG, f + "n_negatives must be in 1..64");
  if (n_query < 0) return fail(c, SPMF_E_ARG, f + "n_query is negative");
  if (n_ref < 0 || n_ref > ((int64_t)1 << 31) - 1) return fail(c, SPMF_E_ARG, f + "n_ref must be in 0..2^31 - 1");
  if (row0 < 0 || row0 > ((int64_t)1 << 32) || n_query > ((int64_t)1 << 32) - row0) return fail(c, SPMF_E_ARG,
      f + "row0 >= 0 and row0 + n_query <= 2^32 must hold");
  if (epoch0 < 0 || n_epochs < 0 || (int64_t)epoch0 + n_epochs > (int64_t)total_epochs) return fail(c, SPMF_E_ARG,
      f + "epochs: epoch0 >= 0, n_epochs >= 0 and epoch0 + n_epochs <= total_epochs must hold");
  if (!(a > 0.0) || !(b > 0.0) || !(a <= 3.0e38) || !(b <= 3.0e38)) return fail(c, SPMF_E_ARG, f + "a and b must be "
      "positive and finite");
  if (!weight_ok(lr) || !weight_ok(repulsion) || !weight_ok(negative_rate)) return fail(c, SPMF_E_ARG, f + "lr, "
      "repulsion and negative_rate must be finite and not negative");
  if ((n_query > 0 && (!idx || !w || !y_out)) || (n_ref > 0 && !y_ref)) return fail(c, SPMF_E_ARG,
      f + "null argument");
  if (!y_in && epoch0 > 0) return fail(c, SPMF_E_ARG, f + "y_in is null with epoch0 > 0: a continued schedule needs "
      "its positions");
  if (n_query == 0) return SPMF_OK;
  hipStream_t st = (hipStream_t)stream;
  if (n_epochs == 0 && y_in) {
    if (y_out != y_in) HIPCHK(c, hipMemcpyAsync(y_out, y_in, (size_t)n_query * sizeof(float2),
                                                hipMemcpyDeviceToDevice, st));
    return SPMF_OK;
  }
  GraphTransformArgs ga{};
  ga.n_query = n_query; ga.n_ref = n_ref; ga.row0 = row0; ga.k = k;
  ga.idx = idx; ga.w = w;
  ga.y_ref = (const float2*)y_ref; ga.y_in = (const float2*)y_in; ga.y_out = (float2*)y_out;
  ga.epoch0 = epoch0; ga.n_epochs = n_epochs; ga.total_epochs = total_epochs; ga.n_negatives = n_negatives;
  ga.lr = lr;
  ga.a = (float)a; ga.b = (float)b;
  ga.neg2b = (float)(-2.0 * b);
  ga.two_gamma_b = (float)(2.0 * repulsion * b);
  ga.rate_over_m = (float)(negative_rate / (double)n_negatives);
  ga.seed_lo = (uint32_t)seed; ga.seed_hi = (uint32_t)(seed >> 32);
  launch_graph_transform(ga, st);
  return launched(c, true, "");
}

// ---- multiplying by the graph (spectral.hip) ----------------------------------------------------
// The graph's checks of the two graph entries, graph_layout's; on SPMF_OK `g` is fit to launch on.
static int graph_csr_check(spmf_ctx* c, const std::string& f, int64_t n_rows, int64_t nnz, const int64_t* indptr,
    const int32_t* indices, const float* weights, GraphCsr& g) {
  if (!graph_layout_rows_ok(n_rows)) return fail(c, SPMF_E_ARG, f + "n_rows must be in 0..2^31 - 64");
  if (nnz < 0) return fail(c, SPMF_E_ARG, f + "nnz is negative");
  if (n_rows > 0 && (!indptr || (nnz > 0 && (!indices || !weights)))) return fail(c, SPMF_E_ARG, f + "null argument");
  g.n_rows = n_rows; g.nnz = nnz; g.indptr = indptr; g.indices = indices; g.weights = weights;
  return SPMF_OK;
}
static bool coef_ok(double v) { return v >= -3.0e38 && v <= 3.0e38; }        // finite, an fp32

int spmf_graph_scale(spmf_ctx* c, int64_t n_rows, int64_t nnz, const int64_t* indptr, const int32_t* indices,
    const float* weights, float* scale, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "graph_scale: ";
  GraphCsr g{};
  const int rc = graph_csr_check(c, f, n_rows, nnz, indptr, indices, weights, g);
  if (rc) return rc;
  if (n_rows > 0 && !scale) return fail(c, SPMF_E_ARG, f + "null argument");
  if (n_rows == 0) return SPMF_OK;
  launch_graph_scale(g, scale, (hipStream_t)stream);
  return launched(c, true, "");
}

int spmf_graph_spmm(spmf_ctx* c, int64_t n_rows, int64_t nnz, const int64_t* indptr, const int32_t* indices,
    const float* weights, const float* scale, const float* x, const float* z, float* y, double c_s,
    const double* c_x, double c_z, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "graph_spmm: ";
  GraphCsr g{};
  const int rc = graph_csr_check(c, f, n_rows, nnz, indptr, indices, weights, g);
  if (rc) return rc;
  if (!c_x || (n_rows > 0 && (!x || !y))) return fail(c, SPMF_E_ARG, f + "null argument");
  if (!coef_ok(c_s) || !coef_ok(c_z)) return fail(c, SPMF_E_ARG, f + "c_s and c_z must be finite");
  BlockCoef cx;
  for (int k = 0; k < kBlockCols; ++k) {
    if (!coef_ok(c_x[k])) return fail(c, SPMF_E_ARG, f + "c_x must be finite");
    cx.cx[k] = (float)c_x[k];
  }
  if (n_rows > 0 && !z && c_z != 0.0) return fail(c, SPMF_E_ARG, f + "null argument: z with c_z != 0");
  if (n_rows > 0 && y == x) return fail(c, SPMF_E_ARG, f + "y aliases x: other rows gather x (y may be z)");
  if (n_rows == 0) return SPMF_OK;
  launch_graph_spmm(g, scale, x, c_z != 0.0 ? z : nullptr, y, (float)c_s, cx, (float)c_z, (hipStream_t)stream);
  return launched(c, true, "");
}

// ---- modularity moves on the graph (graph_move.hip) ----------------------------------------------
int spmf_graph_move(spmf_ctx* c, int64_t n_rows, int64_t nnz, const int64_t* indptr, const int32_t* indices,
    const int64_t* wq, const int32_t* labels_in, const int64_t* tot, const int32_t* long_rows, int64_t n_long,
    double gamma, int64_t m2, int direction, int32_t* labels_out, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "graph_move: ";
  if (!graph_layout_rows_ok(n_rows)) return fail(c, SPMF_E_ARG, f + "n_rows must be in 0..2^31 - 64");
  if (nnz < 0) return fail(c, SPMF_E_ARG, f + "nnz is negative");
  if (!graph_layout_rows_ok(n_long)) return fail(c, SPMF_E_ARG, f + "n_long must be in 0..2^31 - 64");
  if (n_rows > 0 && (!indptr || !labels_in || !tot || !labels_out || (nnz > 0 && (!indices || !wq))))
    return fail(c, SPMF_E_ARG, f + "null argument");
  if (n_long > 0 && !long_rows) return fail(c, SPMF_E_ARG, f + "null argument: long_rows with n_long > 0");
  if (!(gamma > 0.0 && gamma <= 1.7e308)) return fail(c, SPMF_E_ARG, f + "gamma must be finite and > 0");
  if (m2 <= 0) return fail(c, SPMF_E_ARG, f + "m2 must be > 0");
  if (direction != 0 && direction != 1) return fail(c, SPMF_E_ARG, f + "direction must be 0 (up) or 1 (down)");
  if (n_rows > 0 && labels_out == labels_in)
    return fail(c, SPMF_E_ARG, f + "labels_out aliases labels_in: other rows read labels_in");
  if (n_rows == 0) return SPMF_OK;
  MoveArgs ma{};
  ma.n_rows = n_rows; ma.nnz = nnz; ma.indptr = indptr; ma.indices = indices; ma.wq = wq;
  ma.labels_in = labels_in; ma.tot = tot; ma.long_rows = long_rows; ma.n_long = n_long;
  ma.gamma = gamma; ma.m2 = (double)m2; ma.direction = direction; ma.labels_out = labels_out;
  launch_graph_move(ma, (hipStream_t)stream);
  return launched(c, true, "");
}

// Scratch of one block_gram: the chunks' partial sums.
static double* block_gram_carve(Arena& a, int64_t rows) {
  return a.take<double>((size_t)(rows > 0 ? gram_chunks(rows) : 1) * kBlockCols * kBlockCols);
}

size_t spmf_block_gram_scratch_bytes(const spmf_ctx* c, int64_t n_rows) {
  if (!c || !graph_layout_rows_ok(n_rows)) return 0;
  Arena a;
  block_gram_carve(a, n_rows);
  return a.used;
}

int spmf_block_gram(spmf_ctx* c, int64_t n_rows, const float* x, const float* y, double* g, void* scratch,
    size_t scratch_bytes, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "block_gram: ";
  if (!graph_layout_rows_ok(n_rows)) return fail(c, SPMF_E_ARG, f + "n_rows must be in 0..2^31 - 64");
  if (!g || !scratch || (n_rows > 0 && (!x || !y))) return fail(c, SPMF_E_ARG, f + "null argument");
  if ((uintptr_t)scratch & 255) return fail(c, SPMF_E_ARG, f + "scratch must be 256-byte aligned");
  Arena a(scratch, scratch_bytes);
  double* partial = block_gram_carve(a, n_rows);
  if (!a.fits()) return scratch_too_small(c, "block_gram", a.used, scratch_bytes,
      "n_rows=" + std::to_string((long long)n_rows));
  hipStream_t st = (hipStream_t)stream;
  if (n_rows == 0) {
    HIPCHK(c, hipMemsetAsync(g, 0, (size_t)kBlockCols * kBlockCols * sizeof(double), st));
    return SPMF_OK;
  }
  launch_block_gram(n_rows, x, y, partial, g, st);
  return launched(c, true, "");
}

int spmf_block_rotate(spmf_ctx* c, int64_t n_rows, const float* x, const double* r, float* y, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "block_rotate: ";
  if (!graph_layout_rows_ok(n_rows)) return fail(c, SPMF_E_ARG, f + "n_rows must be in 0..2^31 - 64");
  if (!r || (n_rows > 0 && (!x || !y))) return fail(c, SPMF_E_ARG, f + "null argument");
  BlockRot rot;
  for (int k = 0; k < kBlockCols * kBlockCols; ++k) {
    if (!(r[k] >= -1.7e308 && r[k] <= 1.7e308)) return fail(c, SPMF_E_ARG, f + "r must be finite");
    rot.r[k] = r[k];
  }
  if (n_rows == 0) return SPMF_OK;
  launch_block_rotate(n_rows, x, rot, y, (hipStream_t)stream);
  return launched(c, true, "");
}

}  // extern "C"
