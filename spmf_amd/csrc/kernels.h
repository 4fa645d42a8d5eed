// kernels.h -- host-side launch interface of the libspmf_hip kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "spmf_hip.h"   // SPMF_BLOCK_COLS, SPMF_GRAM_CHUNK_ROWS

namespace spmf {

// The latent widths the kernels are built for, MINKP, 2 MINKP, .., MAXKP: calls f with KP as a
// std::integral_constant.  false: KP is not one of them (f is not called, nothing is launched).
template <int MAXKP, int MINKP = 4, class F>
inline bool with_kp(int KP, F&& f) {
  if (KP == MINKP) {
    f(std::integral_constant<int, MINKP>{});
    return true;
  }
  if constexpr (MINKP < MAXKP) return with_kp<MAXKP, 2 * MINKP>(KP, f);
  return false;
}

// The streaming kernels' K chunk, the floats of the K axis per LDS tile (score_block.h): calls f with KC as a
// std::integral_constant for KP = 4, 8, .., 256.  false: KP is not one of them (f is not called).
template <class F>
inline bool with_kc(int KP, F&& f) {
  switch (KP) {
    case 4: case 8: f(std::integral_constant<int, 8>{}); return true;
    case 16: f(std::integral_constant<int, 16>{}); return true;
    case 32: case 64: case 128: case 256: f(std::integral_constant<int, 32>{}); return true;
    default: return false;
  }
}

// The likelihood codes 0 .. 4 (common.h): calls f with the code as a std::integral_constant.  false: lik is
// none of them (f is not called).
template <int LIK = 0, class F>
inline bool with_lik(int lik, F&& f) {
  if (lik == LIK) {
    f(std::integral_constant<int, LIK>{});
    return true;
  }
  if constexpr (LIK < 4) return with_lik<LIK + 1>(lik, f);
  return false;
}

struct PrepArgs {
  int D, K;
  const float *u, *v, *w, *s, *eta;
  float *Ap, *Vp, *phi;
  double* dprep;  // [kPrepSeg][KP+1]: partial sums of veta[KP], phisum (written, not accumulated;
                  // readers fold the segments: common.h prep_sum)
  int logt;       // log_transform: A' = w1*u (g(x) is data side), V' = eta*v^T
  const uint8_t* ctype;  // mixed likelihood: 1 = Bernoulli column (may be null)
  float* dbias;          // mixed likelihood: dense-kernel logit bias per column (may be null)
  // S > 1: the launch covers S draws (gridDim.y); pointers are those of draw 0, draw s adds
  // s * D*K to u / v, s * D to w, s * 2D to s, s * D*KP to Ap / Vp, s * D to phi, s * kPrepSeg*(KP+1) to dprep
  int S;
  // optional zero fill folded into the launch (the step's acc | dacc): 16-byte multiple, or null
  void* zero_p = nullptr;
  size_t zero_bytes = 0;
};
void launch_prep(int KP, const PrepArgs& a, hipStream_t st);

struct RowArgs {
  int64_t B;
  const int32_t* row_ptr;
  const int32_t* col;
  const float* val;
  const float* row_scale;  // may be null
  const float *Ap, *Vp, *phi;
  const double* dprep;
  float *z, *gzs;
  double* dacc;  // [kDaccHead+KP] (zeroed by the caller)
  int mode;            // 0 full (linear decoder), 1 sweep 1 only (encode), 2 sweep 2 only, 3 full with the dense
                       // row term left to the dense kernel's epilogue (launch_sigdot3 p_scale / accumulate)
  int logt;            // log_transform rate r = exp(<z,V'>) - 1 + phi
  const float* gzd;    // mode 2: per-row dense term sum_d E_bd V'_d  [B,KP]
  const uint8_t* ctype;  // likelihood code 3 (mixed): column types
  // S > 1 (mode 0 only): S draws per launch (gridDim.y); draw s adds s * D*KP to Ap / Vp, s * D to
  // phi, s * kPrepSeg*(KP+1) to dprep, s * B*KP to z / gzs, s * dacc_stride to dacc
  int S, D;
  int64_t dacc_stride;
  const uint32_t* ent = nullptr;   // packed col << 16 | count copy of (col, val), or null (spmf_counts.ent)
  // deterministic mode: the workgroups' scalar sums go to their own slots (kDetMeta + kDetMaxBlocks *
  // (kDaccHead + KP) doubles per draw, stride det_stride) instead of the fp64 atomics on dacc
  double* det_slots = nullptr;
  int64_t det_stride = 0;
  // 1: the last eighth of every wave's rows is handed out by counters (slot kDaccDynSlot of the kDaccRep replicas
  // of `dacc`, zeroed by the caller with the rest of it; the fold into the accumulator tail skips it, so tail
  // pair 10 / 11 is always zero) instead of by the fixed stride; only for the ONE
  // full row launch of a step (modes 0 and 3), ignored in the deterministic mode
  int dyn_tail = 0;
};
bool launch_row_pass(int KP, const RowArgs& a, hipStream_t st);   // false: KP is not built (nothing launched)
bool launch_row_widek(int KP, const RowArgs& a, hipStream_t st);  // KP = 128, 256 (widek.hip): Poisson / linear decoder, modes 0 and 1

struct ColArgs {
  int D, n_panels, row_base;
  int max_items_per_panel;
  const int32_t* item_ptr;  // [n_panels+1]
  const int32_t* items;     // [n_items][4] = {start, len, column, 0}
  const int32_t* pc_row;
  const float* pc_val;
  const float *Vp, *phi, *z, *gzs;
  float *gAp, *gVp, *gphi;  // accumulated with float atomics (zeroed by the caller)
  int logt;
  const float* pc_gval;     // log_transform: g(x) per panel-CSC entry
  const uint8_t* ctype;     // likelihood code 3 (mixed): column types
  const int32_t* item_mid;  // [n_panels] first item of the upper column half, or null
  int half_sel;             // 0 all items; 1 / 2: lower / upper column half only (needs item_mid)
  // S > 1: S draws per launch (gridDim.y); draw s adds s * D*KP to Vp, s * D to phi, s * B*KP to
  // z / gzs and s * acc_stride to gAp / gVp / gphi
  int S;
  int64_t B, acc_stride;
  int pc_pad = 0;           // readable entries behind the last list of pc_row / pc_val / pc_gval
  const uint32_t* pc_ent = nullptr;   // packed (row in panel << 16 | count) copy of pc_row / pc_val, or null
  int panel_rows = 0;
  // optional: one extra block folds the row pass's fp64 scalar block (kDaccRep replicas) into
  // the accumulator tail as (hi, lo) float pairs -- what pack_kernel does as its own launch
  const double* pack_dacc = nullptr;
  float* pack_tail = nullptr;
  int64_t dacc_stride = 0;
  // deterministic mode: per-item partial sums (det_part_len(KP) floats per item of the batch, item index
  // relative to item_ptr[0]; stride det_part_stride floats per draw) instead of the float atomics, and the
  // pack block reads the row pass's per-workgroup slots
  float* det_part = nullptr;
  int64_t det_part_stride = 0;
  const double* det_slots = nullptr;
  int64_t det_stride = 0;
};
// deterministic mode: adds the per-item partials up column by column in (panel, segment) order
struct DetReduceArgs {
  int D, KP, n_panels, S;
  const int32_t* list_first;   // [n_panels * D + 1], offset to the batch's first panel
  const int32_t* item_pos;
  const int32_t* item_ptr;     // [0] = first item of the batch
  const float* part;
  int64_t part_stride;
  float *gAp, *gVp, *gphi;
  int64_t acc_stride;
};
void launch_det_reduce(const DetReduceArgs& a, hipStream_t st);

struct ExpdotArgs {
  int NP = 0, NQ = 0;
  const float *P = nullptr, *Q = nullptr;  // [NP,KD], [NQ,KD]
  float* out = nullptr;      // [NP,KD]
  float sign = 1.f;
  double* esum = nullptr;    // may be null
  int q_chunks = 1;          // gridDim.y; >1 needs atomic_out
  int atomic_out = 0;
  int act = 0;               // 0 exp (Poisson log_transform), 1 sigmoid/softplus (Bernoulli)
  const float *bias_p = nullptr, *bias_q = nullptr;  // act 1: logit bias per P row / per Q row (one of them)
  float* out2 = nullptr;     // act 1: out2[p] += sign * sum_q sigmoid (may be null)
  const int32_t* out_rows = nullptr;   // P is a compacted row subset: out / out2 rows to write (may be null)
  float* est = nullptr;      // keep E (exp or sigmoid) for launch_estdot (layout: dense.hip), ldE = its P extent
  int64_t ldE = 0;
  int e_planes = 2;          // launch_sigdot3: bf16 planes of E in the second product (3 where the Q rows have mixed signs)
  // launch_sigdot3: out[p] += sign * p_scale[p] * result instead of out[p] = sign * result (p_scale may be
  // null = 1; plain read-modify-write unless atomic_out): the fused row pass leaves xi_b (gz_b - z_b) in
  // gzs and this launch subtracts xi_b * sum_d E_bd V'_d from it
  int accumulate = 0;
  const float* p_scale = nullptr;
};
void launch_expdot(int KD, const ExpdotArgs& a, hipStream_t st);
// dense3.hip: the same operator (act 0, KD = 64, no biases / E store) on the bf16 matrix cores with
// three-way split operands; false = this shape is not covered (use launch_expdot)
bool launch_expdot3(int KD, const ExpdotArgs& a, hipStream_t st);
// dense3.hip: the sigmoid / softplus operator (act 1: Bernoulli and mixed columns, KD = 32 or 64 (64: the step's two launch shapes only), one of
// bias_p / bias_q, out2, out_rows; no E store) on the same bf16x3 operands; false = not covered
bool launch_sigdot3(int KD, const ExpdotArgs& a, hipStream_t st);
int expdot3_rows_per_wg();
int expdot3_wgs_per_cu();
int sigdot3_rows_per_wg(int KD);
int sigdot3_wgs_per_cu(int KD);
void launch_estdot(int KD, int NQ, int NP, int64_t ldE, const float* est, const float* P, float* out, float sign,
                   float* out2, const int32_t* out_rows, hipStream_t st);
void launch_compact_rows(int n, int KD, const int32_t* cols, const float* Vp, const float* phi, float* Vb,
                         float* bb, hipStream_t st);

struct DenseLLArgs {
  int64_t B;
  int D, logt;       // logt = likelihood code 0..3
  const float *z, *Vp, *phi;
  const uint8_t* ctype;
  const int32_t* row_ptr;
  const int32_t* col;
  const float* val;
  float *rate, *ll;  // [B,D] each
};
void launch_dense_ll(int KP, const DenseLLArgs& a, hipStream_t st);
// pass 0: io[0] = min(io[0], finite ll); pass 1: io[1] += clipped/replaced sum, io[2] += #non-finite
void launch_nonfinite(int64_t n, const float* ll, int pass, double* io, hipStream_t st);
void launch_nonfinite_argmin(int64_t n, const float* ll, double index_base, double* io, hipStream_t st);
struct NfPatchArgs {
  int D, K, logt;
  const int32_t* row_ptr;
  const int32_t* col;
  const float* val;
  const float* row_scale;          // may be null
  const float *u, *v, *w, *s;      // draw 0; draw q adds q * D*K / K*D / D / 2D
  const float* eta;
  const uint8_t* ctype;
  float* acc;                      // packed accumulators of draw 0
  int64_t acc_stride;
  int Dh;                          // column split of the accumulator layout (D = none)
  const double* io;                // [0] global minimum, [3] linear index of its cell
  const double* nlg;               // [S] sum of lgamma(x+1) over each draw's replaced cells
  int64_t rows_batch;
  int S;
};
void launch_nonfinite_patch(int KP, const NfPatchArgs& a, hipStream_t st);
void launch_nonfinite_lgamma(const DenseLLArgs& a, double* out, hipStream_t st);   // uses B, D, logt, ctype, CSR, rate
// What the consumer kernel of a streaming call reads: the draw stage's output for S draws over B rows (api_stream.hip
// draw_stage).
struct DrawTables {
  int64_t B;
  int D, KP, S, lik;               // lik = likelihood code 0..4 (common.h)
  const float *z, *Vp, *phi;       // [S,B,KP], [S,D,KP], [S,D]
  const uint8_t* ctype;
};
// waic.hip: per-cell lppd / pwaic over S draws, summed over the cells of the batch (sums6: [0] cells counted,
// [1] sum lppd, [2] sum pwaic, [3] sum elpd^2, [4] excluded cells; accumulated).  false: KP / lik not built.
struct WaicArgs {
  DrawTables t;
  int64_t nnz;
  const int32_t* row_ptr;
  const int32_t* col;
  const float* val;
  double* sums;                    // [6]
  double* row_out;                 // [B][2] (sum_d lppd, sum_d pwaic), accumulated; may be null
  double* col_out;                 // [D][5] (slots 0..4 of sums over the column's cells), accumulated; may be null
};
bool launch_waic(const WaicArgs& a, hipStream_t st);
// topk.hip: per row the k cells with the largest posterior predictive mean over S draws (mean of the rate on a
// Poisson column, of sigmoid(logit) on a Bernoulli one), ordered by (score descending, column ascending) and
// padded with column -1 / score -inf.  false: KP / lik / k / slices not built (nothing launched).
constexpr int kTopkMaxK = 64;
constexpr int kTopkMaxSlices = 16;   // column slices of one launch (the merge kernel's LDS holds their candidates)
struct TopkArgs {
  DrawTables t;
  int64_t nnz;
  int k;
  int slices;                      // gridDim.y of the select launch, 1 .. min(kTopkMaxSlices, column blocks)
  const int32_t* row_ptr;
  const int32_t* col;
  uint32_t* stored;                // zeroed bitmap [B][ceil(D/32)] of the cells to exclude (filled here), or null
  int32_t* part_cols;              // slices > 1: [slices][B][k] each
  float* part_scores;
  int32_t* cols;                   // [B][k]
  float* scores;                   // [B][k]
};
bool launch_topk(const TopkArgs& a, hipStream_t st);
// topk.hip: ORs a bit per CSR entry of the B rows into the zeroed bitmap bits[B][ceil(D/32)] (launch_topk runs it
// itself; rank.hip reads the same bitmap)
void launch_topk_mark(int64_t B, int D, const int32_t* row_ptr, const int32_t* col, uint32_t* bits, hipStream_t st);
// topk.hip: one wave per row ranks the candidates pc / ps [nsl][B][k] of nsl slices (padding: column -1) into
// cols / scores [B][k] (launch_topk runs it itself; knn.hip merges its reference slices with it)
void launch_topk_merge(int64_t B, int k, int nsl, const int32_t* pc, const float* ps, int32_t* cols, float* scores,
                       hipStream_t st);
// toprows.hip: per listed column the k rows with the largest posterior predictive mean over S draws (the score of
// launch_topk and launch_panel, the same bits), ordered by (score descending, row ascending) and padded with row
// -1 / score -inf.  cols as in PanelArgs (null: the tables' own columns, n_cols == t.D); the bitmap is indexed by
// the columns of the draw tables, not of the list.  false: KP / lik / k / slices not built (nothing launched).
struct TopRowsArgs {
  DrawTables t;
  int64_t nnz;
  int n_cols, k;
  int slices;                      // gridDim.y of the select launch: row slices, 1 .. min(kTopkMaxSlices, row blocks)
  const int32_t* cols;             // [n_cols] or null
  const int32_t* row_ptr;
  const int32_t* col;
  uint32_t* stored;                // as TopkArgs.stored
  float *Vc, *phic;                // as PanelArgs (cols set)
  uint8_t* ctc;
  int32_t* part_rows;              // slices > 1: [slices][n_cols][k] each
  float* part_scores;
  int32_t* rows;                   // [n_cols][k], relative to the first row of t.z
  float* scores;                   // [n_cols][k]
};
bool launch_toprows(const TopRowsArgs& a, hipStream_t st);
// knn.hip: the mean (and, with sd, the unbiased standard deviation) over the S draws of the encoded rows
// t.z[S,B,KP], unpadded: mean / sd [B][K].  Nothing is launched for B == 0.
void launch_embed(const DrawTables& t, int K, float* mean, float* sd, hipStream_t st);
// knn.hip: exact k nearest rows of r [n_ref][row_len] for every row of q [n_query][row_len] (include/spmf_hip.h
// spmf_knn has the definition).  The scratch pointers are api_points.hip's carve; qw == rw when q == r.  false: KP / k /
// slices not built (nothing launched).
constexpr int kKnnCentreBlocks = 512;   // most per-block partial sums of the centre
constexpr int kKnnDefaultTile = 1;      // the tile function without SPMF_KNN_TILE: the faster one
struct KnnArgs {
  int64_t n_query, n_ref;
  int row_len, KP, k, slices;
  bool cosine;
  int tile;                        // 0: score_block, 1: the query-resident tile (KP <= 64)
  int64_t self_offset;             // query i is reference row self_offset + i (no candidate of its own); -1: none
  const float *q, *r;              // the caller's rows
  float *qw, *rw, *bias;           // working rows [n][KP], bias [n_ref]
  float* cpart;                    // [kKnnCentreBlocks][KP] partial sums of the finite reference rows
  int32_t* ccnt;                   // [kKnnCentreBlocks] their counts
  float* centre;                   // [KP]
  int32_t* part_idx;               // slices > 1: [slices][n_query][k] each
  float* part_score;
  int32_t* idx;                    // [n_query][k]
  float* dist;                     // [n_query][k]
};
bool launch_knn(const KnnArgs& a, hipStream_t st);
// rank.hip: for a list of cells sorted by row, the rank of each among its row's candidates under the order of
// launch_topk (score descending, equal scores by ascending column), the number of candidates beside it, and its
// score with the bits of launch_topk.  rank / cand / score are initialised here; a cell outside [0,B) x [0,D)
// gets rank -1, 0 candidates, score NaN.  false: KP / lik / slices not built, or no cells or rows (nothing launched).
constexpr int kRankMaxPerRow = 32;   // listed cells of one row that one round of the kernel takes (T)
struct RankArgs {
  DrawTables t;
  int64_t nnz;
  int slices;                      // gridDim.y, as TopkArgs.slices
  const int32_t* row_ptr;
  const int32_t* col;
  uint32_t* stored;                // as TopkArgs.stored
  int64_t n_cells;
  const int32_t* cell_row;         // [n_cells] non-decreasing, relative to the first row of t.z
  const int32_t* cell_col;         // [n_cells]
  int32_t* rank;                   // [n_cells]
  int32_t* cand;                   // [n_cells]
  float* score;                    // [n_cells]
};
bool launch_rank(const RankArgs& a, hipStream_t st);
// cells.hip: posterior predictive mean (and, with values, lppd) of a list of cells over S draws; an index
// outside [0,B) x [0,D) reads nothing and gets NaN.  false: KP / lik not built or too many cells (nothing launched).
struct CellsArgs {
  DrawTables t;
  int64_t n_cells;
  const int32_t* row;              // [n_cells], relative to the first row of t.z
  const int32_t* col;              // [n_cells]
  const float* val;                // [n_cells] or null (mean only)
  float* mean;                     // [n_cells]
  float* lppd;                     // [n_cells]; null iff val is null
};
bool launch_cells(const CellsArgs& a, hipStream_t st);
// panel.hip: posterior predictive mean and, where asked for, standard deviation and P(x > 0) over S draws of
// every cell of B rows x n_cols columns, as dense [B][n_cols] arrays.  cols: the listed columns of the draw
// tables t (any order, repeats allowed; one outside [0, t.D) gives NaN), compacted into Vc / phic / ctc first;
// null: the tables' own columns, n_cols == t.D, no gather.  false: KP / lik not built (nothing launched).
struct PanelArgs {
  DrawTables t;
  int n_cols;
  const int32_t* cols;             // [n_cols] or null
  float *Vc, *phic;                // [S][n_cols][KP], [S][n_cols] (cols set)
  uint8_t* ctc;                    // [n_cols] (cols set, mixed contexts)
  float *mean, *sd, *pnz;          // [B][n_cols]; sd (S >= 2) and pnz may be null
};
bool launch_panel(const PanelArgs& a, hipStream_t st);
// panel.hip: the gather of a listed panel alone, for all t.S draws: Vc[s][j] = t.Vp[s][cols[j]], phic likewise
// (NaN for a column outside [0, t.D)), ctc[j] = t.ctype[cols[j]] (ctc may be null)
void launch_panel_gather(const DrawTables& t, int C, const int32_t* cols, float* Vc, float* phic, uint8_t* ctc,
                         hipStream_t st);
// groups.hip: per draw, group and column the fp64 sum over the group's rows of the posterior predictive mean m_s
// and, where asked for, of P(x > 0), added onto sum / nonzero [S][n_groups][n_cols].  labels [B]: a value outside
// [0, n_groups) is no group.  cols as in PanelArgs.  The scratch pointers are api_stream.hip's carve, sized from
// group_geom, a pure function of (B, S, G, C): the order of every sum depends on the call's arguments alone.
// false: KP / lik not built (nothing launched).
constexpr int kGroupRowChunk = 1024;     // rows per workgroup of the ordering's rank kernel
constexpr int kGroupDrawChunk = 8;       // draws per workgroup of group_kernel
constexpr int kGroupTargetBlocks = 4096; // runs x column blocks aimed at (a constant: not the device's CU count)
// bytes of the partial sums when not all columns fit: a range then has about budget / (16 * 8 * 64) = 2048
// workgroups per 8 draws, enough for the device, and a test can reach the walk over ranges
constexpr size_t kGroupPartBudget = (size_t)16 << 20;
struct GroupGeom {
  int64_t NB, chunks, nseg;        // row blocks (bound: ceil(B / 64) + G), rank chunks, segments (bound: min(run
                                   // target, NB) + G >= runs + G, non-decreasing in B)
  int runs, RB, CR;                // runs of RB row blocks; columns per range (a multiple of 64)
  size_t part_bytes;
};
GroupGeom group_geom(int64_t B, int S, int G, int C);
struct GroupOrder {                // the ordering of B rows by label (launch_group_order), in the carve's order
  int32_t *tbl, *lrank, *cnt, *boff, *fincl;   // [chunks][G], [B], [G], [G + 1], [G]
  int4* rec; int32_t* perm;        // [NB], [64 NB]
};
struct GroupArgs {
  DrawTables t;
  int n_groups, n_cols;
  const int32_t* labels;           // [B]
  const int32_t* cols;             // [n_cols] or null
  double *sum, *nonzero;           // [S][n_groups][n_cols], accumulated; nonzero may be null
  GroupOrder ord;
  float* zs;                       // [S][64 NB][KP]
  float *Vc, *phic;                // as PanelArgs (cols set)
  uint8_t* ctc;
  double* part;                    // part_bytes
};
bool launch_groups(const GroupArgs& a, hipStream_t st);
// groups.hip: the ordering of launch_groups alone (group_rank .. group_scatter): the B rows in label order,
// stable in the row index, every group padded to whole 64-row blocks.  perm [64 NB] (row, -1 in a pad slot), rec
// [NB] (group, valid rows, segment, 0; group -1 for a surplus block), cnt [G], boff [G + 1] (first block of a
// group, boff[G] = blocks in use), with NB = ceil(B / 64) + G; tbl [ceil(B / kGroupRowChunk)][G], lrank [B] and
// fincl [G] are its working arrays.  A segment is the blocks of one group inside one run of RB blocks.  B > 0.
void launch_group_order(int64_t B, int G, int RB, const int32_t* labels, const GroupOrder& o, hipStream_t st);
// kmeans.hip: one Lloyd step behind launch_knn (include/spmf_hip.h spmf_kmeans_step has the definition).  cand_idx /
// cand_dist [n_rows][kc] are launch_knn's refined result for q = x, r = centroids, k = kc = min(4, G).  The
// scratch pointers are api_points.hip's carve, sized from kmeans_geom, a pure function of (n_rows, G): the order
// of every sum depends on (n_rows, the labels) alone.  n_rows > 0.
constexpr int kKmeansTargetRuns = 2048;  // runs of row blocks aimed at (a constant: not the device's CU count)
constexpr int kKmeansStatRows = 256;     // rows per partial sum of the statistics
struct KmeansGeom {
  int64_t NB, chunks, nseg, sblocks;   // as GroupGeom; sblocks = ceil(n_rows / kKmeansStatRows)
  int runs, RB;
};
KmeansGeom kmeans_geom(int64_t n_rows, int G);
struct KmeansArgs {
  int64_t n_rows;
  int row_len, n_clusters, kc;
  const float* x;                  // [n_rows][row_len]
  const int32_t* cand_idx;         // [n_rows][kc]
  const float* cand_dist;
  const int32_t* prev;             // [n_rows] or null
  int32_t* labels;                 // [n_rows]
  float* dist;                     // [n_rows] or null
  double* sums;                    // [G][row_len]
  int64_t* counts;                 // [G]
  double* stats;                   // [3]
  GroupOrder ord;
  double* part;                    // [nseg][row_len]
  double* spart;                   // [sblocks][3]
};
void launch_kmeans(const KmeansArgs& a, hipStream_t st);
// silhouette.hip: the silhouette of labelled rows over all pairs (include/spmf_hip.h spmf_silhouette has the
// definition).  The scratch pointers are api_points.hip's carve, sized from silhouette_geom; every order of
// additions depends on the members' labels alone.  false: KP not built or no row (nothing launched).
constexpr int kSilCentreBlocks = 512;    // runs of blocks whose partial sums make the centre
struct SilhouetteGeom {
  int64_t NB, chunks;              // row blocks (bound: ceil(n_rows / 64) + G), rank chunks
};
SilhouetteGeom silhouette_geom(int64_t n_rows, int G);
struct SilhouetteArgs {
  int64_t n_rows;
  int row_len, KP, n_clusters;
  bool cosine;
  const float* x;                  // [n_rows][row_len]
  const int32_t* labels;           // [n_rows]
  float *sil, *a, *b;              // [n_rows]; a and b may be null
  int32_t* nearest;                // [n_rows] or null
  double* cluster_sum;             // [G]
  int64_t* counts;                 // [G]
  int32_t* eff;                    // [n_rows]: the effective labels
  GroupOrder ord;
  float *w, *bias;                 // working rows [64 NB][KP] in group order, bias [64 NB]
  double* cpart;                   // [kSilCentreBlocks][KP]
  int32_t* ccnt;                   // [kSilCentreBlocks]
  float* centre;                   // [KP]
  double* spart;                   // [NB]: the blocks' sums of s
};
bool launch_silhouette(const SilhouetteArgs& a, hipStream_t st);
// graph_layout.hip: the epochs of a 2-D layout of a CSR graph (include/spmf_hip.h spmf_graph_layout has the
// definition).  One launch per epoch: epoch k reads every position of `from` and writes every row's position to
// `to`, the last epoch into y_out; buf[0] / buf[1] are api_graph.hip's two scratch buffers and buf[0] holds the
// start.  The step of epoch e is lr * (1 - e / total_epochs), formed in fp64 here and passed as fp32.  The graph is
// read as it stands: every index, weight and indptr value is checked in the kernel.
struct LayoutSchedule {            // of both layout kernels: the call's epochs in the run, the force, the seed
  int epoch0, n_epochs, total_epochs, n_negatives;
  double lr;
  float a, b, neg2b, two_gamma_b, rate_over_m;    // fp64 on the host, each rounded once
  uint32_t seed_lo, seed_hi;
};
struct GraphLayoutArgs {
  int64_t n_rows, nnz;
  const int64_t* indptr;           // [n_rows + 1]
  const int32_t* indices;          // [nnz]
  const float* weights;            // [nnz]
  float2* buf[2];                  // [n_rows] each
  float2* y_out;                   // [n_rows]
  LayoutSchedule s;
};
void launch_graph_layout(const GraphLayoutArgs& a, hipStream_t st);
// graph_transform.hip: the epochs of new rows on a fitted layout, the reference positions held fixed
// (include/spmf_hip.h spmf_graph_transform has the definition).  One launch for all epochs of the call: a row keeps
// its neighbours in registers and reads only y_ref.  The struct is the kernel's argument: the step of epoch e is
// formed in the kernel from lr and total_epochs in fp64.  idx, w, y_ref and y_in are read as they stand: every
// index, weight and position is checked in the kernel.
struct GraphTransformArgs {
  int64_t n_query, n_ref, row0;
  int k;
  const int32_t* idx;              // [n_query][k]
  const float* w;                  // [n_query][k]
  const float2* y_ref;             // [n_ref]
  const float2* y_in;              // [n_query], or null: the weighted mean of the neighbours
  float2* y_out;                   // [n_query]; may be y_in
  LayoutSchedule s;
};
void launch_graph_transform(const GraphTransformArgs& a, hipStream_t st);
// spectral.hip: multiplying by the graph (include/spmf_hip.h spmf_graph_scale .. spmf_block_rotate have the
// definitions).  A block is fp32 [n_rows][SPMF_BLOCK_COLS] row-major: a row is one 64-byte segment.  The graph is
// read as it stands, under graph_layout's rules: every index, weight and indptr value is checked in the kernel.
constexpr int kBlockCols = SPMF_BLOCK_COLS;
constexpr int kGramChunk = SPMF_GRAM_CHUNK_ROWS;   // rows per partial of block_gram: a constant, never the grid's
struct GraphCsr {
  int64_t n_rows, nnz;
  const int64_t* indptr;           // [n_rows + 1]
  const int32_t* indices;          // [nnz]
  const float* weights;            // [nnz]
};
struct BlockCoef {
  float cx[kBlockCols];            // fp64 on the host, each rounded once
};
struct BlockRot {
  double r[kBlockCols * kBlockCols];   // row-major: the kernel's argument (2 KiB)
};
void launch_graph_scale(const GraphCsr& g, float* scale, hipStream_t st);
// y = c_s s_i sum_j w_ij s_j x_j + x_i o cx + c_z z_i; scale and z may be null; y may be z, never x
void launch_graph_spmm(const GraphCsr& g, const float* scale, const float* x, const float* z, float* y, float cs,
                       const BlockCoef& cx, float cz, hipStream_t st);
inline int64_t gram_chunks(int64_t n_rows) { return (n_rows + kGramChunk - 1) / kGramChunk; }
// g[256] = x^T y in fp64: partial [gram_chunks(n_rows)][256], then their sum in ascending chunk order
void launch_block_gram(int64_t n_rows, const float* x, const float* y, double* partial, double* g, hipStream_t st);
void launch_block_rotate(int64_t n_rows, const float* x, const BlockRot& r, float* y, hipStream_t st);
// graph_paths.hip: n_sweeps >= 1 sweeps of Y_il = min(X_il, min_j fl(X_jl + w_ij)) on fp32 [n_rows][16] blocks
// (include/spmf_hip.h spmf_graph_relax has the definition), one launch each, graph_spmm's access pattern.  buf[0]
// holds the start; the sweeps alternate between the two buffers and the last writes x_out, pred_out and
// changed_out (zeroed on the stream in front of it); the last two may be null.  n_rows > 0.
struct GraphRelaxArgs {
  int64_t n_rows, nnz;
  const int64_t* indptr;           // [n_rows + 1]
  const int32_t* indices;          // [nnz]
  const float* lengths;            // [nnz]; an entry counts with a finite length > 0
  float* buf[2];                   // [n_rows][16] each
  float* x_out;                    // [n_rows][16]
  int32_t* pred_out;               // [n_rows][16], or null
  int32_t* changed_out;            // one word, or null
  int n_sweeps;
};
void launch_graph_relax(const GraphRelaxArgs& a, hipStream_t st);
// graph_move.hip: one Jacobi sweep of modularity moves (include/spmf_hip.h spmf_graph_move has the definition).
// Weights are int64 fixed point, so every sum is exact; the score is four fp64 operations, each rounded once.
// Rows of at most kMoveGroupLen entries are moved by a 16-lane group each, the rows of long_rows by a workgroup
// each (O(d^2 / 256) per row of d entries); every other row keeps its label.
constexpr int kMoveGroupLen = SPMF_MOVE_GROUP_LEN;
struct MoveArgs {
  int64_t n_rows, nnz;
  const int64_t* indptr;           // [n_rows + 1]
  const int32_t* indices;          // [nnz]
  const int64_t* wq;               // [nnz]; an entry counts with wq >= 1
  const int32_t* labels_in;        // [n_rows]
  const int64_t* tot;              // [n_rows], by label
  const int32_t* long_rows;        // [n_long], or null
  int64_t n_long;
  double gamma, m2;                // m2 rounded once on the host
  int direction;                   // 0: only c > a is admitted, 1: only c < a
  int32_t* labels_out;             // [n_rows]; never labels_in
};
void launch_graph_move(const MoveArgs& a, hipStream_t st);
// graph_groups.hip: the graph's entries summed by (label of row, label of column) into dense [G][G] tables
// (include/spmf_hip.h spmf_graph_group_edges has the definition).  Integers only: LDS and global integer atomics,
// exact in any order.  ord is api_graph.hip's carve, sized from group_edges_geom, a pure function of (n_rows, G).
// n_rows > 0.
constexpr int kGroupEdgesMaxGroups = SPMF_GROUP_EDGES_MAX_GROUPS;
constexpr int kGroupEdgesTargetRuns = 2048;   // runs of row blocks aimed at (a constant: not the device's CU count)
struct GroupEdgesGeom {
  int64_t NB, chunks;              // as GroupGeom
  int runs, RB;
};
GroupEdgesGeom group_edges_geom(int64_t n_rows, int G);
struct GroupEdgesArgs {
  int64_t n_rows, nnz;
  const int64_t* indptr;           // [n_rows + 1]
  const int32_t* indices;          // [nnz]
  const int64_t* wq;               // [nnz]; an entry counts with wq >= 1
  const int32_t* labels;           // [n_rows]; outside [0, n_groups): no group
  int n_groups;
  int64_t *count_out, *weight_out; // [G][G]
  int64_t* size_out;               // [G]
  GroupOrder ord;
};
void launch_group_edges(const GroupEdgesArgs& a, hipStream_t st);
// sets.hip: per row and column set the fp64 weighted sum over the set's listed columns of the posterior
// predictive mean m_s, reduced over the draws: mean [B][ld] (column g = set g) and, where asked for, the unbiased
// standard deviation over the draws (S >= 2).  set_ptr: HOST, [n_sets + 1], set g lists cols[set_ptr[g] ..
// set_ptr[g + 1]) (device; any order, repeats allowed, one outside [0, t.D) makes its set NaN) with the weights
// beside them (device, null = 1).  The scratch pointers are api_stream.hip's carve for padded_cols = 64 * sum_g
// ceil(n_g / 64) columns.  false: KP / lik not built (nothing launched).
constexpr int kSetDrawChunk = 8;         // draws per pass of set_kernel over the set's column blocks
constexpr int kSetFillChunk = 128;       // sets whose offsets one launch of the fill kernel takes as arguments
struct SetFill {
  int64_t ptr[kSetFillChunk + 1];        // set_ptr of the chunk's sets
  int32_t boff[kSetFillChunk + 1];       // their first 64-column blocks in the padded list
};
struct SetArgs {
  DrawTables t;
  int n_sets;
  const int64_t* set_ptr;          // host
  const int32_t* cols;             // [set_ptr[n_sets]]
  const float* weights;            // [set_ptr[n_sets]] or null
  int64_t padded_cols;             // 0: every set is empty (the outputs are zero-filled)
  int32_t* colsp;                  // [padded_cols]: the padded list, -1 in a pad slot
  float* wp;                       // [padded_cols]: the padded weights
  int2* srec;                      // [n_sets]: (first block, columns)
  float *Vc, *phic;                // as PanelArgs, for padded_cols columns
  uint8_t* ctc;
  int64_t ld;                      // row stride of mean / sd, >= n_sets
  double *mean, *sd;               // sd may be null
};
bool launch_sets(const SetArgs& a, hipStream_t st);
bool launch_col_pass(int KP, const ColArgs& a, hipStream_t st);   // true: launched, with the pack block if asked
bool launch_col_widek(int KP, const ColArgs& a, hipStream_t st);  // KP = 128, 256 (widek.hip)

struct PackArgs {
  int KP;
  const double* dacc;
  float* tail;  // acc tail: 2*(kDaccHead+KP) floats
  int S;        // draws (gridDim.y): draw s adds s * dacc_stride / s * acc_stride
  int64_t dacc_stride, acc_stride;
};
void launch_pack(const PackArgs& a, hipStream_t st);
void launch_zero(void* p, size_t bytes, hipStream_t st);   // zero fill as a kernel (see stats.hip)

struct FinishArgs {
  int D, K;
  int64_t B_global;
  double lgamma_sum;
  double u_tau_scale, s_tau_scale, decay, prior_weight;
  const float* acc;     // this draw's accumulators (after any all-reduce)
  const double* dprep;  // this draw's veta/phisum
  const float* const* params;  // 12 device pointers (this draw)
  const float* eta;
  float* const* grads;  // 12 device pointers (this draw)
  double* parts;        // [14] (zeroed by the caller)
  double* n_nonfinite;  // [1] or null
  int logt;
  const uint8_t* ctype;  // likelihood code 3 (mixed): column types
  int Dh;                // column split of the accumulator layout (0 / D = none; multiple of 32)
  // S > 1: S draws per launch (gridDim.y); draw s adds s * vstride[i] to params[i] / grads[i],
  // s * acc_stride to acc, s * kPrepSeg*(KP+1) to dprep, s * 14 to parts, s to n_nonfinite
  int S;
  int64_t acc_stride;
  int64_t vstride[12];
  int abs_horseshoe;     // horshoe_plus=False: only params/grads 0, 1, 2, 7 are used
  double* ppart;         // [S][ceil(D/32)][12] per-block prior-part sums (workspace)
  float* putau;          // [S][ceil(D/32)][KP] per-block u_tau gradient sums (workspace)
};
void launch_finish(int KP, const FinishArgs& a, int phase, hipStream_t st);
// The step as spmf_step_begin / spmf_step_end run it (ABI 6): the prior half of the finish inside the prep
// launch (prep.hip begin_kernel; f.acc / f.dprep / f.n_nonfinite unused, f.S == a.S), and the data half with
// the fold of the prior half's per-block sums as the step's last launch (finish.hip end_kernel).
void launch_step_begin(int KP, const PrepArgs& a, const FinishArgs& f, hipStream_t st);
void launch_step_end(int KP, const FinishArgs& a, hipStream_t st);

// ---- surrogate posterior / optimiser (surrogate.hip) ----------------------
struct SurVar {
  const float* t0;      // loc            | raw concentration
  const float* t1;      // raw scale      | raw scale
  const float* noise;   // [S,n] eps ~ N(0,1) | g ~ Gamma(softplus(t0), 1)
  const float* dgda;    // [S,n] d g / d a (kind 2 only)
  float* theta;         // [S,n] out (fwd)
  const float* gtheta;  // [S,n] dE/dtheta (bwd)
  float *g0, *g1;       // [n] out (bwd)
  int n, kind;          // kind 0 softplus-normal, 1 identity-normal, 2 softplus-invgamma
  const uint8_t* ident; // optional per-element kind-1 override of kind 0
  int64_t ld;           // stride between draws in noise / dgda
};
struct SurTable {
  SurVar v[12];
};
struct AdamVar {
  float *p, *m, *v;
  const float* g;
  int n;
};
struct AdamTable {
  AdamVar v[24];
};
void launch_surrogate_fwd(const SurTable& T, int nvars, int max_n, int S, double* logq, double* scratch,
                          size_t scratch_doubles, hipStream_t st);
void launch_sample_noise(const SurTable& T, int nvars, int max_n, int S, uint64_t seed, uint64_t counter,
                         const double* state, hipStream_t st);
// sample + transform in one launch + the fold of the log q block sums; false: scratch too small for S * blocks
// partial sums (nothing launched)
bool launch_sample_fwd(const SurTable& T, int nvars, int max_n, int S, uint64_t seed, uint64_t counter,
                       const double* state, double* logq, double* scratch, size_t scratch_doubles, hipStream_t st);
void launch_surrogate_bwd(const SurTable& T, int nvars, int max_n, int S, float inv_sb, float c, hipStream_t st);
void launch_surrogate_bwd_adam(const SurTable& T, const AdamTable& A, int nvars, int max_n, int S, float inv_sb,
                               float c, const double* state, hipStream_t st);
void launch_vi_gate(const double* parts, const double* logq, const double* nnf, int S, double c, double rows, double* state, hipStream_t st);
void launch_adam_dev(const AdamTable& T, int ntensors, int max_n, const double* state, hipStream_t st);
void launch_adam(const AdamTable& T, int ntensors, int max_n, double lr, double b1, double b2, double eps, double c1, double c2, double clip, hipStream_t st);

// ---- the step's collective over peer pointers (p2p.hip) ---------------------------------
constexpr int kP2PMaxWorld = 16;    // ranks of one node
constexpr int kP2PMaxChunks = 256;  // workgroups of the collective's kernel
struct P2PLaunch {
  float* buf;
  int64_t n;
  int rank, world, nchunk;
  int64_t slice_cap;
  float *rs, *ag;
  uint64_t *flags, *seq;
  float* peer_rs[kP2PMaxWorld];
  float* peer_ag[kP2PMaxWorld];
  uint64_t* peer_flags[kP2PMaxWorld];
};
void launch_p2p_allreduce(const P2PLaunch& L, hipStream_t st);

struct StatsArgs {
  int64_t B;
  const int32_t* row_ptr;
  const int32_t* col;
  const float* val;
  double *colsum, *colnnz;
  float* row_sum;
  double* row_lgamma;
};
void launch_stats(const StatsArgs& a, hipStream_t st);
void launch_gvals(int64_t nnz, int n_panels, int D, const int32_t* row_ptr, const int32_t* col, const float* val,
                  const int32_t* pc_ptr, const float* pc_val, const float* eta, float* gval, float* pc_gval,
                  hipStream_t st);
void launch_colstats(int n_panels, int D, const int32_t* pc_ptr, const float* pc_val, double* colsum,
                     double* colnnz, hipStream_t st);

}  // namespace spmf
