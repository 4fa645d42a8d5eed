// api_stream.hip -- the streaming calls behind the C-ABI (include/spmf_hip.h): the draw stage and its consumers'
// entries, spmf_embed_rows included.  The calls on rows and graphs as given are api_points.hip and api_graph.hip;
// the scratch and launch helpers they share with the entries here are defined first.  Host-side orchestration
// only (ctx.h).
#include "ctx.h"

using namespace spmf;

namespace spmf {

int scratch_too_small(spmf_ctx* c, const char* fn, size_t need, size_t have, const std::string& detail) {
  return fail(c, SPMF_E_WORKSPACE, std::string(fn) + ": scratch too small: need " + std::to_string(need) +
      " bytes for " + detail + ", have " + std::to_string(have));
}

int launched(spmf_ctx* c, bool ok, const char* no_kernel) {
  if (!ok) return fail(c, SPMF_E_UNSUPPORTED, no_kernel);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int device_cus(const spmf_ctx* c) {
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
int topk_slices(int64_t n_rows, int D, int cus) {
  const int64_t rb = (n_rows + 63) / 64, cb = ((int64_t)D + 63) / 64;
  if (rb < 1 || rb >= 2 * (int64_t)cus) return 1;
  int64_t nsl = (2 * (int64_t)cus + rb - 1) / rb;
  if (nsl > kTopkMaxSlices) nsl = kTopkMaxSlices;
  if (nsl > cb) nsl = cb;
  const int64_t per = (cb + nsl - 1) / nsl;
  return (int)((cb + per - 1) / per);
}

void group_order_carve(Arena& a, int64_t rows, int G, int64_t chunks, int64_t NB, GroupOrder& o) {
  const size_t nG = G;
  o.tbl = a.take<int32_t>((size_t)chunks * nG);
  o.lrank = a.take<int32_t>((size_t)rows);
  o.cnt = a.take<int32_t>(nG);
  o.boff = a.take<int32_t>(nG + 1);
  o.fincl = a.take<int32_t>(nG);
  o.rec = a.take<int4>((size_t)NB);
  o.perm = a.take<int32_t>((size_t)NB * 64);
}

}  // namespace spmf

extern "C" {

// ---- the draw stage of the streaming calls ---------------------------------------------------
// spmf_waic_accumulate (and its _cols form), spmf_topk_rows, spmf_score_cells, spmf_rank_cells, spmf_predict_columns,
// spmf_toprows_columns, spmf_group_sums, spmf_set_scores and spmf_embed_rows are one stage and a consumer each.
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

static std::string rows_S(const spmf_counts* ct, int S) {
  return "rows=" + std::to_string((long long)ct->n_rows) + " S=" + std::to_string(S);
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
// does not depend on the call's k or flags).  The slices are topk_slices with the roles swapped, as in knn_layout
// (api_points.hip): the keys are the column blocks of the panel, the candidates the row blocks.
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
  const size_t KP = c->KP, nS = S, NB = (size_t)q.NB;
  draw_tables(a, c, rows, S, T);
  group_order_carve(a, rows, G, q.chunks, q.NB, ga.ord);
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

}  // extern "C"
