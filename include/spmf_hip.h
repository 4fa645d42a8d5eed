/* spmf_hip.h -- C-ABI of libspmf_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE path of mederrata/spmf: the per-batch energy
 * (ELBO integrand) of PoissonFactorization and its gradient through the
 * factor matrices.  The reference has no FFI; the seam this library sits
 * behind is the Python method
 *     PoissonFactorization.unormalized_log_prob_parts(data, **params)
 *         mederrata_spmf/poisson.py:582-621
 * (called once per optimiser step by bayesianquilts' fit/calibrate_advi,
 * tests/spmf_test.py:35-43, bin/factorize_csv.py:121-124) and the helpers it
 * calls: encode :623-650, encoding_matrix :652-666, intercept_matrix
 * :680-701, log_likelihood_components :156-184, compute_scales :113-154 and
 * the prior of create_distributions :212-401.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (torch tensors on
 *    the Python side) unless marked "host"; the caller supplies the workspace
 *    (spmf_workspace_bytes); the library's only own device allocation is an
 *    8 MiB scratch for the fixed-order reductions of the surrogate kernels.
 *  - all calls are asynchronous on the hipStream_t passed as `stream`
 *    (void* so the header needs no HIP include); one ctx per (process,
 *    device); calls on one ctx are stream-ordered and not re-entrant.
 *  - return value: 0 = ok, <0 = error (SPMF_E_*); spmf_last_error() gives
 *    the message.  Nothing throws across this boundary.
 *  - arithmetic: fp32 storage and fp32 FMA, fp64 accumulation of every
 *    scalar reduction ("dtype": "f32" in bench.py).
 *  - S = number of Monte-Carlo draws = leading axis of every parameter.
 *
 * Variable order everywhere (= the reference's surrogate var_list,
 * poisson.py:403-539,572):
 *   0 v[K,D] 1 w[1,D] 2 u[D,K] 3 u_eta[D,K] 4 u_tau[1,K] 5 s_eta[2,D]
 *   6 s_tau[1,D] 7 s[2,D] 8 u_eta_a[D,K] 9 u_tau_a[1,K] 10 s_eta_a[2,D]
 *   11 s_tau_a[1,D]
 * Energy parts order: the 12 prior parts in that order, then 12 = 'z',
 * 13 = 'x' (poisson.py:604,619).
 */
#ifndef SPMF_HIP_H
#define SPMF_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Every function below is exported; nothing else is (the library is built with
 * -fvisibility=hidden). */
#if defined(SPMF_BUILD)
#pragma GCC visibility push(default)
#endif

#define SPMF_NVARS 12
#define SPMF_NPARTS 14
#define SPMF_PART_Z 12
#define SPMF_PART_X 13

#define SPMF_OK 0
#define SPMF_E_ARG (-1)       /* bad argument (null pointer, bad size, K unsupported) */
#define SPMF_E_HIP (-2)       /* a HIP runtime call failed */
#define SPMF_E_WORKSPACE (-3) /* caller's workspace too small */
#define SPMF_E_UNSUPPORTED (-4)

/* flags for spmf_ctx_create */
#define SPMF_FLAG_SCALE_ROWS 1u     /* poisson.py:61,644-649 */
#define SPMF_FLAG_BERNOULLI 4u      /* BernoulliFactorization (mederrata_spmf/bernoulli.py): Bernoulli(logits=rate)
                                     * likelihood :147-155, Normal priors on v,w :187-216; with SPMF_FLAG_LOG_TRANSFORM
                                     * the logit is exp(<z, eta v>) - 1 + phi (:60-61) */
#define SPMF_FLAG_MIXED 8u          /* build-defined (mederrata_spmf/mixed.py is an empty file): per-column likelihood,
                                     * Bernoulli(logits) on the columns flagged by spmf_ctx_set_column_types, Poisson
                                     * on the others; linear decoder only */
#define SPMF_FLAG_LOG_TRANSFORM 2u  /* poisson.py:41-42,52-53: sparse stored-cell terms + dense f32-MFMA exp sums */
#define SPMF_FLAG_ABS_HORSESHOE 16u /* horshoe_plus=False (poisson.py:378-398): AbsHorseshoe priors on u (scale
                                     * u_tau_scale*decay^k) and s (scale s_tau_scale); only the variables v, w, u, s
                                     * (indices 0, 1, 2, 7) exist: the other params / grads pointers are ignored
                                     * (may be NULL) and their energy parts are 0 */

typedef struct spmf_ctx spmf_ctx;

/* One batch (or one row shard) of the count matrix, device resident.
 * Row-major CSR for the row pass and a row-panel CSC ("panel-CSC": for each
 * panel of `panel_rows` consecutive rows, a CSC of that panel) for the
 * column pass; the column pass walks the panels of residue class blockIdx % 8
 * on one XCD, so a panel's z and xi*gz rows (panel_rows * 2 * KP floats) should
 * fit that XCD's L2 and n_panels should be a multiple of 8 for big batches:
 * spmf_amd/sparse.py balanced_panel_rows).  Replaces the dense [B,D] tensor data[count_key] the
 * reference feeds to encode/log_likelihood_components (poisson.py:170,182).
 */
typedef struct spmf_counts {
  int64_t n_rows;           /* B: rows of this batch */
  int64_t nnz;              /* stored entries of this batch */
  int32_t n_cols;           /* D */
  int32_t n_panels;         /* row panels covering the batch */
  int32_t panel_rows;       /* rows per panel (last one may be short) */
  int32_t row_base;         /* row id stored in pc_row for batch row 0 */
  const int32_t* row_ptr;   /* [B+1] absolute offsets into col_idx/val */
  const int32_t* col_idx;   /* base pointer (not offset) */
  const float* val;         /* base pointer: raw counts x_bd */
  const float* row_scale;   /* [B] xi_b = rowsum_b / xi_u_global, or NULL => 1 */
  const int32_t* pc_ptr;    /* [n_panels*(D+1)] absolute offsets into pc_row/pc_val */
  const int32_t* pc_row;    /* base pointer: row id (row_base + batch row) */
  const float* pc_val;      /* base pointer */
  double lgamma_sum;        /* sum over the batch of lgamma(x+1) (parameter free) */
  /* log_transform only (poisson.py:41-42): g(x) = log(x/eta + 1) per stored
   * entry, in CSR and in panel-CSC order (base pointers); NULL otherwise. */
  const float* gval;
  const float* pc_gval;
  /* Column-pass work items: every non-empty (panel, column) list cut into
   * segments of bounded length, sorted by length inside a panel.
   *   items[i] = {start, len, column, 0} (int32 x 4, start absolute into
   *   pc_row/pc_val); item_ptr[p], item_ptr[p+1] bound panel p's items
   *   (absolute item indices; pointer already offset to the batch's first
   *   panel); max_items_per_panel sizes the launch. */
  const int32_t* item_ptr;
  const int32_t* items;
  int32_t max_items_per_panel;
  /* Readable int32/float entries behind the END of the last list in pc_row, pc_val, pc_ent
   * AND pc_gval (every list array the context's decoder reads must carry the same padding:
   * with log_transform that includes pc_gval).  With pc_pad >= 4*ceil(K/4) - 1 (K padded to 4,
   * 8, 16, 32, 64) the column pass fetches list entries four or eight at a time (16-B loads that
   * may run past a list's end); 0 selects the entry-at-a-time fetch, which never reads behind a list.
   * Negative values are rejected.  (Until version 2 this slot was a reserved field: a caller
   * that left it uninitialised is caught by struct_size below.) */
  int32_t pc_pad;
  /* Optional column split of the work items (multi-GPU overlap): inside a panel
   * the items are sorted by column half first (columns < col_split, then the
   * rest), then by length; item_mid[p] is the first item of panel p's upper
   * half (absolute item index, pointer offset like item_ptr) and
   * max_items_half[h] sizes a launch over one half.  NULL / 0 when unused. */
  const int32_t* item_mid;
  int32_t col_split;
  int32_t max_items_half[2];
  /* ABI guard (spmf_version() >= 3): sizeof(spmf_counts) as the CALLER was compiled.  Every entry
   * point that takes a spmf_counts rejects a struct whose struct_size differs from the library's
   * own sizeof (SPMF_E_ARG, "built against another spmf_hip.h"): a caller compiled against an older,
   * shorter layout can no longer have the fields appended since (ent, pc_ent) read from whatever
   * follows its struct.  Zero-initialise the struct, then set this first. */
  int32_t struct_size;
  /* Optional packed copy of the CSR entries for the row pass: ent[i] = col_idx[i] << 16 | count,
   * valid when D <= 65536 and every stored value is an integer in [0, 65535] (counts are:
   * tests/spmf_test.py:19); NULL otherwise.  Halves the entry stream of the sweeps that read the
   * raw counts (4 instead of 8 bytes per stored entry); col_idx / val stay the canonical arrays. */
  const uint32_t* ent;
  /* The same for the column pass's lists: pc_ent[i] = (row - first row of its panel) << 16 | count,
   * in the order (and with the pc_pad) of pc_row / pc_val; needs panel_rows <= 65536 as well
   * (rejected otherwise).  Used by the four-per-lane fetch only; NULL otherwise. */
  const uint32_t* pc_ent;
  /* Optional, for the deterministic mode (spmf_ctx_set_deterministic): the work items in their
   * GENERATION order -- (panel, column, segment) -- so that the per-item partial sums of the column
   * pass can be added up column by column in a fixed order:
   *   list_first[p * D + d] .. list_first[p * D + d + 1]   raw indices of the items cut from list
   *                       (p, d) (pointer already offset to the batch's first panel, like pc_ptr with
   *                       stride D; n_panels * D + 1 entries are read)
   *   item_pos[r]         position of raw item r in `items` (absolute item index, base pointer)
   *   n_items             items of THIS batch: item_ptr[n_panels] - item_ptr[0]
   * spmf_layout_build fills them; NULL / 0 when unused. */
  const int32_t* list_first;
  const int32_t* item_pos;
  int64_t n_items;
} spmf_counts;

/* ABI version of this header: 6.  (2 -> 3: spmf_counts.struct_size replaces a reserved slot
 * and is verified; pc_pad / ent / pc_ent are validated.  3 -> 4: the device layout builder
 * spmf_layout_* added.  4 -> 5: spmf_counts grows by list_first / item_pos / n_items for the
 * deterministic mode -- a caller built against 4 is refused by the struct_size check, not
 * misread.  5 -> 6: spmf_step_begin / spmf_step_end added -- the step with its outputs handed over
 * up front -- and spmf_p2p_*, the step's collective as a hand-written kernel over peer pointers; no
 * struct changed, every version-5 entry point keeps its meaning.)  A binding checks it
 * at load time. */
#define SPMF_ABI_VERSION 6
int spmf_version(void);

/* sizeof(spmf_counts) / sizeof(spmf_sur_var) / sizeof(spmf_adam_var) as this
 * library was built: a binding (ctypes, cgo, JNI ...) asserts its own mirror of
 * the struct against it before the first call. */
size_t spmf_sizeof_counts(void);
size_t spmf_sizeof_sur_var(void);
size_t spmf_sizeof_adam_var(void);

/* K = latent_dim, D = feature_dim (poisson.py:58,102-104).  1 <= K <= 256 for the Poisson likelihood with
 * the linear decoder (K <= 64: the lane-group sparse passes; above: one wave per factor row,
 * csrc/widek.hip); 1 <= K <= 64 with SPMF_FLAG_LOG_TRANSFORM / BERNOULLI / MIXED (SPMF_E_UNSUPPORTED above)
 * and for the deterministic mode. */
int spmf_ctx_create(int device, int K, int D, unsigned flags, spmf_ctx** out);
void spmf_ctx_destroy(spmf_ctx* ctx);
const char* spmf_last_error(const spmf_ctx* ctx); /* host string */

/* Hyper-parameters of the prior (poisson.py:59,106-107,225-226). */
int spmf_ctx_set_prior(spmf_ctx* ctx, double u_tau_scale, double s_tau_scale,
                       double symmetry_breaking_decay);

/* SPMF_FLAG_MIXED only: column_is_bernoulli[D] (uint8, device, caller-owned,
 * must outlive the ctx calls). */
int spmf_ctx_set_column_types(spmf_ctx* ctx, const uint8_t* column_is_bernoulli);
/* Optional with SPMF_FLAG_MIXED: the ascending indices of the Bernoulli columns (int32,
 * device, caller-owned, must outlive the ctx calls).  With it the dense softplus /
 * sigmoid sums run over those n columns only (compacted rows of V'); without it over
 * all D columns with the Poisson ones masked by a -1e30 logit bias. */
int spmf_ctx_set_bernoulli_columns(spmf_ctx* ctx, const int32_t* cols, int n);

/* Upper bound in bytes of the buffer that keeps E between the two dense contractions
 * (log_transform / Bernoulli / mixed contexts; default 8 GiB).  The rows of a batch are
 * processed in equal chunks that fit it; fewer, larger chunks fill the chip better (at
 * C4, 500k x 30k: 8 chunks at 8 GiB, one at 64 GiB).  Call before
 * spmf_workspace_bytes / spmf_ctx_set_workspace: it changes the workspace size. */
int spmf_ctx_set_e_cap(spmf_ctx* ctx, size_t bytes);

/* Deterministic mode (Poisson likelihood, linear decoder, no column split): the step's float and
 * fp64 atomics are replaced by single-writer partial sums added up in a fixed order -- per-item
 * partials of the column pass summed column by column in (panel, segment) order, per-workgroup
 * scalar sums of the row pass summed in workgroup order -- so the 14 parts and all 12 gradients of
 * a step are bit-identical from run to run (and replicas of a row-sharded job cannot drift apart
 * through rounding order).  Costs the column pass its atomics' bandwidth twice (write + read of
 * n_items * (2*KP + 4) floats): C3 2.81 -> 2.87 ms per step.  `scratch`: caller-owned device buffer of
 * spmf_det_scratch_bytes(ctx, n_items, S) bytes for the largest batch (n_items = spmf_counts.n_items),
 * 256-byte aligned; NULL switches the mode off.  The counts must carry list_first / item_pos.
 * (Covers the step as spmf_data_pass + spmf_finish run it; the replacement rule for non-finite cells,
 * spmf_nonfinite_patch, adds its correction with atomics and is outside the guarantee.) */
size_t spmf_det_scratch_bytes(const spmf_ctx* ctx, int64_t n_items, int S);
int spmf_ctx_set_deterministic(spmf_ctx* ctx, void* scratch, size_t bytes);

/* Bytes of caller-owned device workspace needed for batches of up to
 * max_rows rows and S draws.  With SPMF_FLAG_LOG_TRANSFORM / BERNOULLI / MIXED this
 * includes the buffer that keeps E = exp(<z_b, eta_d v_d>) (or the sigmoid of the
 * Bernoulli logits) between the two dense contractions
 * (min(max_rows, chunk) * D floats, chunk chosen so that it stays within
 * spmf_ctx_set_e_cap; the
 * environment variable SPMF_DENSE_E_ONCE=0, read at spmf_ctx_create, selects the
 * form that recomputes E instead and needs no such buffer). */
size_t spmf_workspace_bytes(const spmf_ctx* ctx, int64_t max_rows, int S);
int spmf_ctx_set_workspace(spmf_ctx* ctx, void* workspace, size_t bytes);

/* ---- dataset pre-pass ------------------------------------------------- */
/* compute_scales (poisson.py:113-154): column sums and per-column counts of
 * x>0 of a CSR block, ACCUMULATED into colsum[D] (fp64) / colnnz[D] (fp64),
 * plus per-row sums row_sum[B] (fp32) and per-row sums of lgamma(x+1)
 * row_lgamma[B] (fp64).  Any output pointer may be NULL. */
int spmf_counts_stats(spmf_ctx* ctx, int64_t n_rows, const int32_t* row_ptr,
                      const int32_t* col_idx, const float* val, double* colsum,
                      double* colnnz, float* row_sum, double* row_lgamma,
                      void* stream);

/* The column half of the same statistics from a built layout: colsum[D] / colnnz[D] (fp64,
 * ACCUMULATED, either may be NULL) from the panel-CSC lists of `counts` -- one atomic per
 * (panel, column) list instead of one per stored entry (C3: 6.7 -> 0.3 ms).  Sums of integer
 * counts are exact in fp64, so both forms give the same numbers. */
int spmf_counts_colstats(spmf_ctx* ctx, const spmf_counts* counts, double* colsum,
                         double* colnnz, void* stream);

/* log_transform contexts: the encoder side g(x) = log(x / eta_d + 1) (encoder_function,
 * poisson.py:41-42) of every stored entry of `counts`, in CSR order into gval (base pointer,
 * indexed like col_idx / val) and in list order into pc_gval (base pointer, indexed like pc_val);
 * either may be NULL.  eta[D] fp32.  The pc_pad entries behind the last list of the shard are the
 * caller's (zero-filled): only list entries are written.  Depends on the counts and the column
 * scales only: once per (shard, eta), then set spmf_counts.gval / pc_gval. */
int spmf_counts_gvals(spmf_ctx* ctx, const spmf_counts* counts, const float* eta, float* gval,
                      float* pc_gval, void* stream);

/* ---- device layout builder ------------------------------------------- */
/* Builds everything of a spmf_counts that is derived from the CSR arrays of one row shard
 * (the reference hands its model a dense [B,D] batch, poisson.py:170,182; a caller of this
 * library hands it CSR and gets the row-panel CSC, the column-pass work items and the packed
 * entry streams back): on the device, stream-ordered, deterministic (the same input gives the
 * same bytes), into ONE caller-owned buffer.
 *
 *   spmf_layout_sizes   bytes of the layout buffer (kept as long as the spmf_counts is used)
 *                       and of the scratch buffer (free after the call returns)
 *   spmf_layout_build   fills `layout`, then *out (zero-initialised by the callee; row_ptr /
 *                       col_idx / val are the caller's arrays, lgamma_sum / row_scale / gval /
 *                       pc_gval stay 0 / NULL: spmf_counts_stats and the model supply them) and
 *                       *info.  Synchronises `stream` once, at the end, to read back the item
 *                       count and the input checks.
 *
 * Input: canonical CSR of the shard -- row_ptr[0] == 0, row_ptr[n_rows] == nnz, non-decreasing,
 * 0 <= col_idx < n_cols, no (row, column) pair stored twice (columns need not be sorted inside
 * a row).  The first four are verified on the device (SPMF_E_ARG, nothing usable in *out).
 * panel_rows >= 1 (spmf_amd/sparse.py balanced_panel_rows chooses it from K); col_split = 0 or
 * the column split of spmf_ctx_set_column_split.  nnz < 2^31, n_rows < 2^31 and n_panels * n_cols < 2^32
 * (SPMF_E_UNSUPPORTED otherwise: choose larger panels).
 *
 * Layout produced (what spmf_amd/sparse.py built with torch sorts until version 3 of
 * this header; the two are compared array by array in tests/test_gpu_layout.py):
 *   lists     entries ordered by (panel, column, row): pc_ptr, pc_row, pc_val with pc_pad = 64
 *   items     every non-empty list cut into segments of <= info->segment entries (16 ... 256,
 *             so that a panel offers a few thousand items), inside a panel ordered by column
 *             half (col_split), then by descending length, ties in (column, segment) order
 *   ent / pc_ent  when every stored value is an integer count in [0, 65535] and n_cols
 *             (resp. panel_rows) <= 65536; NULL in *out otherwise
 */
typedef struct spmf_layout_info {
  int32_t struct_size;            /* in: sizeof(spmf_layout_info) of the caller */
  int32_t n_panels;
  int32_t panel_rows;
  int32_t segment;                /* longest work item */
  int64_t n_items;
  int32_t packed_ent;             /* 1: out->ent is set */
  int32_t packed_pc_ent;          /* 1: out->pc_ent is set */
  const int32_t* items_per_panel; /* [n_panels] device, inside `layout`: for max_items_per_panel of a panel range */
  const int32_t* items_lower;     /* [n_panels] items of the lower column half (all of them without a split) */
} spmf_layout_info;
size_t spmf_sizeof_layout_info(void);
int spmf_layout_sizes(int device, int64_t n_rows, int64_t nnz, int32_t n_cols, int32_t panel_rows,
                      size_t* layout_bytes, size_t* scratch_bytes);
int spmf_layout_build(int device, int64_t n_rows, int64_t nnz, int32_t n_cols,
                      const int32_t* row_ptr, const int32_t* col_idx, const float* val,
                      int32_t panel_rows, int32_t col_split, void* layout, size_t layout_bytes,
                      void* scratch, size_t scratch_bytes, spmf_counts* out,
                      spmf_layout_info* info, void* stream);
/* The same with the model's latent dimension as a hint (ABI 6; 0 = unknown = the two calls above): a work item
 * is one lane group of the column pass, K padded / 4 lanes, so at K <= 8 a wave carries 32 or 64 items and the
 * lists are cut into proportionally more, shorter items (16 384 / 32 768 per panel instead of 4096) -- the
 * reference CLI's default K = 2 ran its column pass on a few dozen waves otherwise.  Sizes and build must get
 * the same hint. */
int spmf_layout_sizes_k(int device, int64_t n_rows, int64_t nnz, int32_t n_cols, int32_t panel_rows,
                        int32_t latent_dim, size_t* layout_bytes, size_t* scratch_bytes);
int spmf_layout_build_k(int device, int64_t n_rows, int64_t nnz, int32_t n_cols,
                        const int32_t* row_ptr, const int32_t* col_idx, const float* val,
                        int32_t panel_rows, int32_t col_split, int32_t latent_dim, void* layout,
                        size_t layout_bytes, void* scratch, size_t scratch_bytes, spmf_counts* out,
                        spmf_layout_info* info, void* stream);
/* Message of the last failed spmf_layout_* call of the calling thread (host string). */
const char* spmf_layout_last_error(void);

/* Dense batches -- the reference's own input, data[count_key] as a [B,D] array
 * (poisson.py:170,182; tests/spmf_test.py:17-22) -- to the CSR arrays above, on the device:
 *   spmf_dense_row_ptr   row_ptr[n_rows+1] = offsets of the rows' stored cells (x != 0, so NaN cells
 *                        are stored); scratch: spmf_dense_scratch_bytes(n_rows), 8-byte aligned;
 *                        the total is row_ptr[n_rows] (saturating at 2^31-1: a shard must stay below)
 *   spmf_dense_fill_csr  col_idx / val (sized by that total) in row-major, ascending-column order
 * dense: fp32, row-major with leading dimension ld >= n_cols.  Both are stream-ordered and do not
 * synchronise; the caller reads row_ptr[n_rows] between the two to size col_idx / val. */
size_t spmf_dense_scratch_bytes(int64_t n_rows);
int spmf_dense_row_ptr(int device, int64_t n_rows, int32_t n_cols, const float* dense, int64_t ld,
                       int32_t* row_ptr, void* scratch, size_t scratch_bytes, void* stream);
int spmf_dense_fill_csr(int device, int64_t n_rows, int32_t n_cols, const float* dense, int64_t ld,
                        const int32_t* row_ptr, int32_t* col_idx, float* val, void* stream);

/* ---- the hot path ------------------------------------------------------ */
/* Phase 1: sparse data term for S draws.  Reads u,v,w,s (params[2,0,1,7])
 * and eta[D] (eta_i, poisson.py:88-91,142-149; ones when unscaled).  Leaves
 * per-draw accumulators in the workspace:
 *   acc[S][acc_len] fp32 = [ gA'(D*KP) | gV'(D*KP) | gphi(D) | tail ]
 * where the tail carries the fp64 scalars (sum x log r, sum z^2, non-finite
 * count, dense sum, saturated count, one spare, sum_b z_b[KP]) as (hi,lo)
 * float pairs so ONE fp32 sum-all-reduce of
 * acc over row shards finishes the reduction. */
int spmf_data_pass(spmf_ctx* ctx, const spmf_counts* counts, int S,
                   const float* const params[SPMF_NVARS], const float* eta,
                   void* stream);
float* spmf_acc_ptr(const spmf_ctx* ctx);      /* device pointer into the workspace */
int64_t spmf_acc_len(const spmf_ctx* ctx, int S); /* floats, all S draws */

/* Optional overlap for the multi-GPU step: launch the prior half of
 * spmf_finish (all twelve prior log-densities and prior_weight * d prior /
 * d theta; it reads no accumulator) on the context's side stream, forked from
 * `stream`.  Meant to be called between spmf_data_pass and the all-reduce, so
 * it runs while the collective leaves the GPU mostly idle (beside the sparse
 * passes it costs them more than it hides: 3.60 -> 3.80 ms on C3).
 * spmf_finish with the same S, parts and grads then joins the side stream and
 * adds the data half only; without this call it does both halves itself.
 * Order: it writes per-workgroup partial sums into the workspace a data pass has
 * bound, so it must FOLLOW a spmf_data_pass on the current workspace;
 * spmf_ctx_set_workspace / spmf_ctx_set_e_cap forget that binding, and until the next
 * data pass spmf_prior_async, spmf_finish and spmf_nonfinite_patch return
 * SPMF_E_WORKSPACE / SPMF_E_ARG (spmf_acc_ptr: NULL) instead of touching the old buffer. */
int spmf_prior_async(spmf_ctx* ctx, int S, double prior_weight,
                     const float* const params[SPMF_NVARS], const float* eta, double* parts,
                     float* const grads[SPMF_NVARS], void* stream);

/* Optional marker inside the data pass (ABI 6): `event` (a hipEvent_t of the caller, NULL = none) is recorded
 * on the pass's stream right behind its row stage -- after the row pass of the last draw has been issued,
 * before the column pass.  Work of the caller that does not feed the data pass (the VI step's draws and
 * transform of the scale hierarchy, the prior half of the finish: spmf_amd/vi.py) waits for it on another
 * stream and so runs beside the column pass -- many short workgroups that share the chip gracefully -- and
 * not beside the row pass, whose launch is exactly the resident set and is delayed as a whole by any
 * workgroup that holds a slot when it starts. */
int spmf_ctx_set_rows_event(spmf_ctx* ctx, void* event);

/* Column split of the packed accumulators (multi-GPU: all-reduce one half while
 * the column pass still produces the other).  With Dh set (a multiple of 32 in
 * (0, D); 0 or D = none; linear Poisson decoder only) the accumulators of a
 * draw are laid out [cols < Dh: gA'|gV'|gphi][cols >= Dh: gA'|gV'|gphi][tail];
 * spmf_acc_split returns the two contiguous element ranges (the second one
 * includes the fp64 tail) relative to spmf_acc_ptr.  spmf_data_pass_split runs
 * part 0 (everything up to and including the lower half's column pass) or
 * part 1 (upper half + pack) of one draw's data pass; the counts must carry
 * item_mid for the same split.  Order per step:
 *   data_pass_split(0) -> all-reduce range 0 (async) -> data_pass_split(1)
 *   -> all-reduce range 1 -> spmf_finish. */
int spmf_ctx_set_column_split(spmf_ctx* ctx, int Dh);
int spmf_acc_split(const spmf_ctx* ctx, int64_t off[2], int64_t len[2]);
int spmf_data_pass_split(spmf_ctx* ctx, const spmf_counts* counts, int S,
                         const float* const params[SPMF_NVARS], const float* eta, int part,
                         void* stream);

/* ---- the step's one collective, inside the library (RCCL over xGMI) ---------
 * Row shards of the count matrix live on different GPUs, one process per GPU
 * (the reference has no counterpart: only the `strategy` pass-through,
 * poisson.py:60,72).  Between spmf_data_pass and spmf_finish every rank sums the
 * packed accumulators:  spmf_allreduce(ctx, spmf_acc_ptr(ctx), spmf_acc_len(ctx,S),
 * stream) -- ncclAllReduce(float, sum) on the caller's stream, so the collective is
 * stream-ordered with the kernels around it and needs no host synchronisation.
 * librccl is bound at run time (dlopen); without it these return SPMF_E_UNSUPPORTED
 * and single-GPU use is unaffected.  Set-up: rank 0 calls spmf_comm_unique_id, the
 * 128 bytes travel to the other ranks by any channel the host has (the Python
 * mirror uses a torch.distributed broadcast), every rank calls spmf_comm_init. */
int spmf_comm_unique_id(void* out128);
int spmf_comm_init(spmf_ctx* ctx, const void* id128, int rank, int world);
int spmf_allreduce(spmf_ctx* ctx, float* buf, int64_t n, void* stream);
int spmf_comm_destroy(spmf_ctx* ctx);

/* ---- the same collective as a hand-written kernel over peer pointers (ABI 6) -----
 * SURVEY 5 (last row) / 8e ask for a direct reduce-scatter + all-gather over the xGMI mesh instead of a
 * ring: csrc/p2p.hip.  Every rank pushes slice q of its buffer straight into rank q's inbox (N-1 links at
 * once), rank q adds the N contributions IN RANK ORDER and pushes the reduced slice to every peer, every
 * rank copies the N-1 reduced slices home: ONE kernel launch per rank on the caller's stream (capturable
 * in a hipGraph: the call counter lives on the device), flags with system-scope release / acquire, and all
 * ranks end with the SAME bits (each slice is reduced once, by its owner, in a fixed order).  The memory
 * the peers write is a fine-grained region this library allocates and exports with hipIpcGetMemHandle; the
 * peers may be other GPUs of the node (xGMI) or other processes on the same GPU (how the one-GPU tests run
 * it at world 2 and 4) -- the kernel is the same.
 *   spmf_p2p_init     allocates this rank's region for buffers of up to n_max floats and returns its 64-byte
 *                     IPC handle; nchunk = workgroups of the kernel (0: default 32; <= 256)
 *   [ the host exchanges the handles: the Python mirror uses a torch.distributed all_gather ]
 *   spmf_p2p_connect  handles = world x 64 bytes in rank order; opens the peers' regions
 *   spmf_allreduce    then runs this kernel instead of ncclAllReduce (n <= n_max, buf 16-byte aligned)
 *   spmf_p2p_enable   a context may hold both transports (bench.py times them against each other): which one
 *                     spmf_allreduce uses; spmf_p2p_connect leaves the kernel selected
 *   spmf_p2p_status   SYNCHRONISES; out3 = {calls completed, 0, first call in which a workgroup gave up
 *                     waiting for a peer (0 = none)}: every spin is bounded, a lost peer cannot hang the GPU
 *   spmf_p2p_disconnect / spmf_p2p_destroy   an orderly shutdown frees no region a peer still has mapped: every rank
 *                     disconnects (unmaps the peers), the host synchronises the ranks, every rank destroys (unmaps
 *                     what is left and frees; also done by spmf_ctx_destroy)
 * All ranks must call spmf_allreduce with the same n, the same number of times. */
int spmf_p2p_init(spmf_ctx* ctx, int rank, int world, int64_t n_max, int nchunk, void* handle_out64);
int spmf_p2p_connect(spmf_ctx* ctx, const void* handles);
int spmf_p2p_enable(spmf_ctx* ctx, int on);   /* 0: spmf_allreduce goes back to RCCL (if spmf_comm_init was called); 1: the kernel again */
int spmf_p2p_status(spmf_ctx* ctx, uint64_t out3[3]);
int spmf_p2p_disconnect(spmf_ctx* ctx);   /* unmap the peers' regions, keep the own one (first half of an orderly shutdown) */
int spmf_p2p_destroy(spmf_ctx* ctx);

/* Phase 2: chain the accumulators to d/d(u,v,w,s), add the prior's parts and
 * gradients -- the horseshoe-plus hierarchy over all 12 variables (poisson.py:228-377)
 * or, for a context created with SPMF_FLAG_ABS_HORSESHOE, the AbsHorseshoe priors on u
 * and s with v, w as before (poisson.py:378-398; variables 0, 1, 2, 7 only) -- and
 * finish the 14 energy parts.  n_rows_global / lgamma_sum_global are the
 * batch totals over all shards (= this shard's when single GPU).
 *   parts[S][14] fp64 (unweighted), grads[i] has the shape of params[i]
 *   (fp32) and holds d(x + z + prior_weight * sum of prior parts)/d(param):
 *   prior_weight = 1 is the reference's energy (poisson.py:577 passes the
 *   literal 1.); a minibatch driver passes B/N.
 *   n_nonfinite[2*S] (fp64, may be NULL): [s] = stored cells of draw s whose
 *   log-pmf was not finite; the sparse fast path assumes 0 (poisson.py:606-616
 *   is then the identity).  [S+s] = saturation events of draw s: the number of
 *   workgroups of the dense exp kernel (128 rows x all columns each) in which a
 *   log_transform exponent exceeded 70 and was saturated there: fp32 cannot
 *   hold exp(y) beyond y ~ 88 where the fp64 reference still can, so the decoder
 *   is evaluated as exp(min(y,70)) - 1; 0 means the decoder was exact.
 * Input domain (also of spmf_prior_async / spmf_step_begin): positive, finite fp32 parameters (v, w of
 *   Bernoulli columns: any sign).  Every gradient entry whose yardstick -- the sum of the absolute additive
 *   pieces of that entry, |d piece / d entry| over the prior's terms and the data term -- is below 1e37 is
 *   returned finite and to 1e-5 of that yardstick: no intermediate of the prior's gradients exceeds the result
 *   it goes into.  An entry whose yardstick is above has left fp32 (+-inf / NaN; d/d u_tau[k] sums over d, so
 *   one such (d, k) takes the entry).  The twelve prior parts are accurate to 1e-12 of the sum of their
 *   absolute terms (fp64 throughout, u_tau_scale / s_tau_scale / 0.1 as doubles); 'z' and 'x' likewise given
 *   the accumulators.  Tested at the edge: tests/test_gpu_finish_edges.py, DESIGN.md 7a. */
int spmf_finish(spmf_ctx* ctx, int S, int64_t n_rows_global,
                double lgamma_sum_global, double prior_weight,
                const float* const params[SPMF_NVARS], const float* eta,
                double* parts, float* const grads[SPMF_NVARS],
                double* n_nonfinite, void* stream);

/* ---- the step with its outputs known up front (ABI 6) ------------------------
 * poisson.py:582-621 is ONE call; spmf_data_pass + spmf_finish split it in two so that the row-shard
 * all-reduce fits between them, but handed the gradient outputs over only at the second call, which
 * forced the prior's twelve log-densities and their gradients (poisson.py:590-591: parameters only, no
 * accumulator) into the step's LAST launch, behind the collective.  This pair is the same step with
 * parts / grads / n_nonfinite known from the first call on:
 *   spmf_step_begin  = spmf_data_pass, and the prior half of the finish runs INSIDE the data pass's
 *                      first launch, beside the A' / V' / phi tiles (O(D*K) work on the parameters, both);
 *   [ the caller's all-reduce of spmf_acc_ptr / spmf_acc_len, row shards only ]
 *   spmf_step_end    = the data half of spmf_finish (chain rule from the accumulators ADDED to what
 *                      the prior half left in grads, parts 'z' and 'x', the fold of the prior half's
 *                      per-workgroup sums) in ONE launch.
 * Four launches per step instead of five, none of them on a side stream, and what is independent of
 * the batch size shrinks to the prep launch + a 7 us data half (C3 sizes).  Arguments as
 * spmf_data_pass / spmf_finish; params, eta, parts, grads, n_nonfinite must stay valid until
 * spmf_step_end returns (the pointer ARRAYS are copied, the caller's may go).  Results are those of
 * spmf_data_pass + spmf_finish.  When the S draws of a large batch run in turn (S > 1 beyond the
 * batched-draw size) spmf_step_end falls back to the whole finish.  A spmf_data_pass, or anything that
 * re-binds the workspace, between the two calls cancels the step (spmf_step_end: SPMF_E_ARG). */
int spmf_step_begin(spmf_ctx* ctx, const spmf_counts* counts, int S, double prior_weight,
                    const float* const params[SPMF_NVARS], const float* eta, double* parts,
                    float* const grads[SPMF_NVARS], double* n_nonfinite, void* stream);
int spmf_step_end(spmf_ctx* ctx, int64_t n_rows_global, double lgamma_sum_global, void* stream);

/* spmf_step_begin + spmf_step_end back to back (single shard). */
int spmf_elbo_fwd_bwd(spmf_ctx* ctx, const spmf_counts* counts, int S,
                      double prior_weight,
                      const float* const params[SPMF_NVARS], const float* eta,
                      double* parts, float* const grads[SPMF_NVARS],
                      double* n_nonfinite, void* stream);

/* encode (poisson.py:623-650) for one (u,s) draw: z[B,K] row-major fp32. */
int spmf_encode(spmf_ctx* ctx, const spmf_counts* counts, const float* u,
                const float* s, const float* eta, float* z_out, void* stream);

/* log_likelihood_components (poisson.py:156-184, bernoulli.py:126-155) for ONE
 * draw, dense like the reference: rate[B,D] and the log-pmf ll[B,D] of every
 * cell (fp32, row-major): Poisson(rate), or for a Bernoulli context / the
 * Bernoulli columns of a mixed one rate = the logit and ll = x*logit -
 * softplus(logit).  Output bound (8 B per cell); not on the hot path.  Serves
 * the class surface and the non-finite replacement rule. */
int spmf_dense_ll(spmf_ctx* ctx, const spmf_counts* counts, const float* u,
                  const float* v, const float* w, const float* s,
                  const float* eta, float* rate_out, float* ll_out, void* stream);

/* ---- streaming WAIC (added within ABI 6: two new entry points, no struct changed) ----
 * The pointwise criterion over the cells (b, d) of `counts` for S >= 2 draws, without a
 * [S,B,D] or [B,D] tensor (csrc/waic.hip).  With ll_s = log p(x_bd | theta_s), by the per-cell
 * formulas of spmf_dense_ll:
 *   lppd_i = logsumexp_s(ll_s) - log S,  pwaic_i = unbiased var_s(ll_s),  elpd_i = lppd_i - pwaic_i
 * ADDED to the caller's sums6 = double[6] (zero it before the first call; batches and row shards
 * add up):  [0] cells counted  [1] sum lppd_i  [2] sum pwaic_i  [3] sum elpd_i^2
 *           [4] cells excluded  [5] spare.
 * A cell is excluded, and counted in [4] instead of [0..3], when any of its S values is not
 * finite (a NaN count, a rate of 0 under a positive count).  row_out (NULL = skip) = double
 * [n_rows][2], ADDED to: (sum_d lppd_i, sum_d pwaic_i) of every row over its counted cells.
 * params: only u, v, w, s (slots 2, 0, 1, 7) are read, each with the leading axis S.
 * scratch: 256-byte aligned, at least spmf_waic_scratch_bytes(ctx, counts->n_rows, S) bytes
 * (the S draws' tables, 2 * S * D * KP floats, and encoded rows, S * n_rows * KP floats: call it
 * over row chunks to bound it); SPMF_E_WORKSPACE when short.  SPMF_E_ARG for S < 2, NULL pointers
 * or a struct_size mismatch.  The context's workspace is not touched: the call may sit between
 * other calls on the context, a spmf_step_begin .. spmf_step_end pair included.  Stream-ordered,
 * synchronises nowhere; the fp64 sums, the row and the column sums (spmf_waic_accumulate_cols)
 * included, are atomics (not bit-reproducible). */
size_t spmf_waic_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows, int S);
int spmf_waic_accumulate(spmf_ctx* ctx, const spmf_counts* counts, int S,
                         const float* const params[SPMF_NVARS], const float* eta,
                         double* sums6, double* row_out, void* scratch,
                         size_t scratch_bytes, void* stream);
/* The same call with the column reduction (added within ABI 6: one new entry point, no struct
 * changed).  col_out (NULL = skip: then exactly spmf_waic_accumulate) = double [D][5], ADDED to
 * (zero it before the first call; batches and row chunks add up): slot j of column d is sums6[j]
 * restricted to the cells of that column --
 *   [0] cells counted  [1] sum lppd_i  [2] sum pwaic_i  [3] sum elpd_i^2  [4] cells excluded --
 * so that  sum_d col_out[d][j] = the call's contribution to sums6[j].  A column nothing is stored
 * in is scored like any other (all x = 0); a NaN count excludes its whole row, one cell of every
 * column.  Arguments, scratch (spmf_waic_scratch_bytes), checks and their order, and the empty
 * batch are those of spmf_waic_accumulate; this entry's name stands in front of its messages.
 * The fp64 column sums are atomics too (not bit-reproducible): one per (column, slot) and
 * 64 x 64 block of cells, and three to five per stored entry. */
int spmf_waic_accumulate_cols(spmf_ctx* ctx, const spmf_counts* counts, int S,
                              const float* const params[SPMF_NVARS], const float* eta,
                              double* sums6, double* row_out, double* col_out, void* scratch,
                              size_t scratch_bytes, void* stream);

/* ---- streaming per-row top-k (added within ABI 6: two new entry points, no struct changed) ----
 * For every row of `counts` the k cells with the largest posterior predictive mean over S >= 1
 * draws, without a [B,D] array (csrc/topk.hip):
 *   score_bd = (1/S) sum_s m_s,  m_s = rate_s on a Poisson column, sigmoid(logit_s) on a Bernoulli
 *   column (a Bernoulli context, the Bernoulli columns of a mixed one),
 * rate_s / logit_s being what spmf_dense_ll writes as `rate` for draw s.  A cell is a candidate
 * when its score is finite (a NaN count makes its whole row's z NaN: that row has none) and, with
 * bit 0 of `flags` (exclude stored cells), when `counts` holds no entry for it.  cols_out / score_out
 * = [n_rows][k] int32 / fp32: the row's best k candidates, score descending, equal scores by
 * ascending column; a row with fewer candidates is padded with column -1 / score -inf.  The result
 * is the exact top k under that order of the fp32 scores (the mean is taken in draw order), so two
 * calls on the same inputs return the same bits.
 * params: only u, v, w, s (slots 2, 0, 1, 7) are read, each with the leading axis S.
 * scratch: 256-byte aligned, at least spmf_topk_scratch_bytes(ctx, counts->n_rows, S) bytes (the
 * scratch of the WAIC call, a bitmap of the stored cells, n_rows * ceil(D/32) words, and for a
 * batch too small to fill the device the partial results of its column slices: call it over row
 * chunks to bound it); SPMF_E_WORKSPACE when short.  SPMF_E_ARG for S outside 1..65535, k outside
 * 1..64, unknown flag bits, NULL pointers, a misaligned scratch, a mixed context without column
 * types or a struct_size mismatch.  n_rows == 0 returns SPMF_OK.  The context's workspace is not
 * touched: the call may sit between other calls on the context, a spmf_step_begin .. spmf_step_end
 * pair included.  Stream-ordered, synchronises nowhere.  K as for spmf_waic_accumulate. */
size_t spmf_topk_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows, int S);
int spmf_topk_rows(spmf_ctx* ctx, const spmf_counts* counts, int S,
                   const float* const params[SPMF_NVARS], const float* eta, int k,
                   unsigned flags, int32_t* cols_out, float* score_out, void* scratch,
                   size_t scratch_bytes, void* stream);

/* ---- scores of listed cells (added within ABI 6: two new entry points, no struct changed) ----
 * Held-out evaluation: for n_cells cells (cell_row[i], cell_col[i]) of the batch `counts`, over
 * S >= 1 draws, without a [S,B,D] tensor (csrc/cells.hip):
 *   mean_out[i] = (1/S) sum_s m_s, m_s as spmf_topk_rows defines its score (rate_s on a Poisson
 *                 column, sigmoid(logit_s) on a Bernoulli one), added in draw order;
 *   lppd_out[i] = logsumexp_s(ll_s) - log S,  ll_s = log p(cell_val[i] | theta_s) by the per-cell
 *                 formulas of spmf_dense_ll (0 * log 0 := 0), lgamma(x+1) subtracted once.
 * `counts` conditions the scores: its stored entries encode the rows (z of every row under each
 * draw), as in every other call; the listed values are never stored by this call.  cell_row is
 * relative to the first row of `counts`.  The list may be in any order, may repeat cells and may
 * list cells that `counts` stores or does not store (zeros included).  cell_val == NULL and
 * lppd_out == NULL together: the mean only.  lppd_out[i] is NaN when any ll_s is not finite (a NaN
 * value, a rate of 0 under a positive value: the exclusion rule of spmf_waic_accumulate); a NaN
 * count in `counts` makes its row's z NaN and with it both outputs of the row's cells.  An index
 * outside [0, n_rows) x [0, D) reads no memory; both outputs of that cell are NaN.  A cell's
 * outputs depend on the cell alone: not on its place in the list, on the other cells or on how the
 * rows are cut into calls (no atomics, one summation order), so equal cells get equal bits.
 * params: only u, v, w, s (slots 2, 0, 1, 7) are read, each with the leading axis S.
 * scratch: 256-byte aligned, at least spmf_cells_scratch_bytes(ctx, counts->n_rows, S) bytes (the
 * scratch of the WAIC call: call it over row chunks, each with its own cells, to bound it);
 * SPMF_E_WORKSPACE when short.  SPMF_E_ARG for S outside 1..65535, a negative n_cells, NULL
 * params / eta / scratch, NULL cell_row / cell_col / mean_out with n_cells > 0, cell_val and
 * lppd_out not both NULL or both set, a misaligned scratch, a mixed context without column types or
 * a struct_size mismatch; every error returns before any launch.  n_cells == 0 or n_rows == 0
 * returns SPMF_OK without work.  The context's workspace is not touched: the call may sit between
 * other calls on the context, a spmf_step_begin .. spmf_step_end pair included.  Stream-ordered,
 * synchronises nowhere.  K as for spmf_waic_accumulate. */
size_t spmf_cells_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows, int S);
int spmf_score_cells(spmf_ctx* ctx, const spmf_counts* counts, int S,
                     const float* const params[SPMF_NVARS], const float* eta, int64_t n_cells,
                     const int32_t* cell_row, const int32_t* cell_col, const float* cell_val,
                     float* mean_out, float* lppd_out, void* scratch, size_t scratch_bytes,
                     void* stream);

/* ---- rank of listed cells (added within ABI 6: two new entry points, no struct changed) ----
 * Where held-out cells land in the ranking of spmf_topk_rows: for n_cells cells (cell_row[i],
 * cell_col[i]) of the batch `counts`, over S >= 1 draws, without a [B,D] array (csrc/rank.hip).
 * Score, order and candidates are those of spmf_topk_rows: the fp32 mean over the draws of the rate
 * (Poisson column) or sigmoid(logit) (Bernoulli column); score descending, equal scores by ascending
 * column; a candidate of a row is a column with a finite score that, with bit 0 of `flags` (exclude
 * stored cells), `counts` does not store.  For cell i = (b, d), a candidate itself or not:
 *   score_out[i] = score_bd, bit for bit what spmf_topk_rows reports for that cell;
 *   cand_out[i]  = the number of candidates d' != d of row b;
 *   rank_out[i]  = the number of them that precede (b, d) in the order (0 = best), -1 when the
 *                  score is not finite (a NaN count makes its whole row NaN: 0 candidates there).
 * So for a cell that is not stored and has a finite score: rank_out[i] < k <=> entry rank_out[i]
 * of the row's spmf_topk_rows result is column d.  cell_row is relative to the first row of
 * `counts` and must be non-decreasing (the kernel finds a row block's cells by binary search; an
 * unsorted list gives wrong ranks but no access outside the list); cells may repeat.  An index
 * outside [0, n_rows) x [0, D) reads nothing: rank -1, 0 candidates, score NaN.  A row may list any
 * number of cells; the kernel serves 32 per row and round, so a row with n listed cells costs its block
 * of 64 rows ceil(n/32) double sweeps of the columns (about two spmf_topk_rows sweeps up to 32 per row).  All counts are integers added by
 * integer atomics: a cell's outputs do not depend on the list's other cells, on duplicates, on how
 * the rows are cut into calls or on the column slices of the launch; two calls return the same bits.
 * params: only u, v, w, s (slots 2, 0, 1, 7) are read, each with the leading axis S.
 * scratch: 256-byte aligned, at least spmf_rank_scratch_bytes(ctx, counts->n_rows, S) bytes (the
 * scratch of the WAIC call and the bitmap of the stored cells, n_rows * ceil(D/32) words);
 * SPMF_E_WORKSPACE when short.  SPMF_E_ARG for S outside 1..65535, a negative n_cells, NULL params /
 * eta / scratch, a NULL list or output with n_cells > 0, unknown flag bits, a misaligned scratch, a
 * mixed context without column types or a struct_size mismatch; every error returns before any
 * launch.  n_cells == 0 or n_rows == 0 returns SPMF_OK without work.  The context's workspace is not
 * touched.  Stream-ordered, synchronises nowhere.  K as for spmf_waic_accumulate. */
size_t spmf_rank_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows, int S);
int spmf_rank_cells(spmf_ctx* ctx, const spmf_counts* counts, int S,
                    const float* const params[SPMF_NVARS], const float* eta, int64_t n_cells,
                    const int32_t* cell_row, const int32_t* cell_col, unsigned flags,
                    int32_t* rank_out, int32_t* cand_out, float* score_out, void* scratch,
                    size_t scratch_bytes, void* stream);

/* ---- predictions of a column panel (added within ABI 6: two new entry points, no struct changed) ----
 * The reconstruction as a dense block: for every row of the batch `counts` and every column of a panel,
 * over S >= 1 draws, without a [S,B,D] tensor (csrc/panel.hip).  With r_s what spmf_dense_ll writes as
 * `rate` for draw s (the rate of a Poisson column, the logit of a Bernoulli one) and m_s = r_s |
 * sigmoid(r_s):
 *   mean_out[b][j] = (1/S) sum_s m_s, added in draw order: bit for bit the score of spmf_topk_rows and
 *                    spmf_rank_cells for that cell;
 *   sd_out[b][j]   = the unbiased standard deviation of m_s over the draws (Welford in draw order),
 *                    which needs S >= 2;
 *   pnz_out[b][j]  = P(x > 0) under the predictive mixture: (1/S) sum_s -expm1(-r_s) on a Poisson column
 *                    (no cancellation at small rates), the mean itself, the same bits, on a Bernoulli one.
 * Each output is [n_rows][n_cols] fp32, row-major; sd_out and pnz_out may be NULL; nothing outside
 * [n_rows][n_cols] is written.  cols == NULL: all columns, n_cols must be D.  Otherwise cols lists
 * 0 <= n_cols <= D columns (int32, device) in any order, repeats allowed; output column j is column
 * cols[j].  A listed column outside [0, D) reads nothing: its output column is NaN in every output.  A
 * NaN count makes its row NaN in all outputs.  An element depends on its cell alone: not on the list,
 * on the other outputs asked for or on how the rows are cut into calls (no atomics, one summation
 * order); two calls return the same bits.
 * params: only u, v, w, s (slots 2, 0, 1, 7) are read, each with the leading axis S.
 * scratch: 256-byte aligned, at least spmf_predict_scratch_bytes(ctx, counts->n_rows, S) bytes: the
 * scratch of the WAIC call and, in a region of their own behind it (the draw stage's A' region is not
 * reused), the compacted tables of a listed panel sized for n_cols = D, S * D * (KP + 1) floats and D
 * bytes -- the size does not depend on the list; SPMF_E_WORKSPACE when short.  SPMF_E_ARG for S outside
 * 1..65535, NULL params / eta / scratch, a misaligned scratch, a mixed context without column types, a
 * struct_size mismatch, n_cols outside 0..D, cols == NULL with n_cols != D, sd_out with S < 2, a NULL
 * mean_out with n_rows > 0 and n_cols > 0; SPMF_E_UNSUPPORTED for ceil(n_cols / 64) > 65535; every
 * error returns before any launch.  n_cols == 0 or n_rows == 0 returns SPMF_OK without work.  The
 * context's workspace is not touched: the call may sit between other calls on the context, a
 * spmf_step_begin .. spmf_step_end pair included.  Stream-ordered, synchronises nowhere.  K as for
 * spmf_waic_accumulate. */
size_t spmf_predict_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows, int S);
int spmf_predict_columns(spmf_ctx* ctx, const spmf_counts* counts, int S,
                         const float* const params[SPMF_NVARS], const float* eta,
                         int32_t n_cols, const int32_t* cols,
                         float* mean_out, float* sd_out, float* pnz_out,
                         void* scratch, size_t scratch_bytes, void* stream);

/* ---- streaming per-column top-k rows (added within ABI 6: two new entry points, no struct changed) ----
 * The selection of spmf_topk_rows along the other axis: for every column of a panel the k rows of the batch
 * `counts` with the largest posterior predictive mean over S >= 1 draws, without a [n_rows][n_cols] array
 * (csrc/toprows.hip).  The score of a cell is mean_out of spmf_predict_columns, bit for bit (and so the score of
 * spmf_topk_rows and spmf_rank_cells).  A row is a candidate of a column when the cell's score is finite (a NaN
 * count makes its whole row's z NaN: that row is a candidate of no column) and, with bit 0 of `flags` (exclude
 * stored cells), when `counts` holds no entry for the cell.  The panel is that of spmf_predict_columns: cols ==
 * NULL is all columns and n_cols must be D; otherwise cols lists 0 <= n_cols <= D columns (int32, device) in any
 * order, repeats allowed, and output row j belongs to column cols[j]; a listed column outside [0, D) reads nothing
 * and has no candidates.  rows_out / scores_out = [n_cols][k] int32 / fp32: the column's best k candidates, score
 * descending, equal scores by ascending row, the rows relative to the first row of `counts`; a column with fewer
 * candidates is padded with row -1 / score -inf.  The result is the exact top k under that order of the fp32
 * scores: it does not depend on the other listed columns or on the row slices of the launch, and two calls on the
 * same inputs return the same bits.  Row chunks are combined by the caller: concatenate the chunks' results per
 * column in ascending row order and keep the best k under a stable sort by score.
 * params: only u, v, w, s (slots 2, 0, 1, 7) are read, each with the leading axis S.
 * scratch: 256-byte aligned, at least spmf_toprows_scratch_bytes(ctx, counts->n_rows, S, n_cols) bytes: the
 * scratch of spmf_rank_cells (the WAIC call's and the bitmap of the stored cells, n_rows * ceil(D/32) words), the
 * compacted tables of the panel, S * n_cols * (KP + 1) floats and n_cols bytes, and, for a panel too narrow to
 * fill the device with its column blocks, the partial results of its row slices; SPMF_E_WORKSPACE when short
 * (the size function returns 0 for n_cols outside 0..D).  SPMF_E_ARG for S outside 1..65535, NULL params / eta /
 * scratch, a misaligned scratch, a mixed context without column types, a struct_size mismatch, n_cols outside
 * 0..D, cols == NULL with n_cols != D, k outside 1..64, unknown flag bits, a NULL output with n_cols > 0; every
 * error returns before any launch.  n_cols == 0 returns SPMF_OK: nothing is launched or written.  n_rows == 0
 * returns SPMF_OK: nothing is launched but the fill of both outputs with the padding, on the stream.  The
 * context's workspace is not touched: the call may sit between other calls on the context, a spmf_step_begin ..
 * spmf_step_end pair included.  Stream-ordered, synchronises nowhere.  K as for spmf_waic_accumulate. */
size_t spmf_toprows_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows, int S, int32_t n_cols);
int spmf_toprows_columns(spmf_ctx* ctx, const spmf_counts* counts, int S,
                         const float* const params[SPMF_NVARS], const float* eta,
                         int32_t n_cols, const int32_t* cols, int k, unsigned flags,
                         int32_t* rows_out, float* scores_out,
                         void* scratch, size_t scratch_bytes, void* stream);

/* ---- per-group sums of the predictions (added within ABI 6: two new entry points, no struct changed) ----
 * The posterior predictive reduced over the rows of the batch `counts`, per draw: with r_s and m_s as for
 * spmf_predict_columns, for every draw s < S, group g < n_groups and listed column j
 *   sum_out[s][g][j]     += sum over the rows b with labels[b] == g of m_s(b, cols[j]);
 *   nonzero_out[s][g][j] += the same sum of -expm1(-r_s) on a Poisson column (the expected number of rows
 *                           with x > 0), of m_s on a Bernoulli one
 * without a [n_rows][n_cols] block (csrc/groups.hip).  Both are [S][n_groups][n_cols] fp64, device, and are
 * ADDED to: the caller zeroes them, and batches and row chunks accumulate (as sums6 of
 * spmf_waic_accumulate); nonzero_out may be NULL.  All additions are fp64: every fp32 m_s is converted
 * before its first addition, no fp32 partial sums and no floating-point atomics.  The order of the
 * additions is a function of (n_rows, S, n_groups, n_cols) and the labels alone: rows in ascending order
 * inside 64-row blocks of a group, blocks in ascending order; two calls return the same bits.
 * labels: [n_rows] int32, device; a value outside [0, n_groups) is "no group": the row is in no sum.  A
 * row with a NaN count makes the sums of ITS group NaN in every draw and column and touches no other
 * group; in no group it changes nothing.  cols == NULL: all columns, n_cols must be D.  Otherwise cols
 * lists 0 <= n_cols <= D columns as for spmf_predict_columns; a listed column outside [0, D) makes its
 * output column NaN (of the groups that have rows).
 * params: only u, v, w, s (slots 2, 0, 1, 7) are read, each with the leading axis S.
 * scratch: 256-byte aligned, at least spmf_groups_scratch_bytes(ctx, counts->n_rows, S, n_groups, n_cols)
 * bytes: the draw stage's scratch, the row order (about n_rows / 1024 * n_groups + n_rows + 80 * n_groups
 * int32), the encoded rows once more in group order (S * (n_rows + 64 * n_groups) * KP floats), the
 * compacted tables of the list and the partial sums of a column range, at most 16 MiB unless a single
 * 64-column block needs more: the entry walks column ranges.  The size is 0 for bad arguments.
 * SPMF_E_ARG for the draw stage's errors (S outside 1..65535, NULL params / eta / scratch, a misaligned
 * scratch, a mixed context without column types, a struct_size mismatch), n_groups < 1, n_cols outside
 * 0..D, cols == NULL with n_cols != D, NULL labels or sum_out with work to do; SPMF_E_UNSUPPORTED for
 * n_groups > 2^24; then SPMF_E_WORKSPACE for a short scratch, naming the need; every error returns before
 * any launch or write.  n_cols == 0 or n_rows == 0 returns SPMF_OK without work.  The context's workspace
 * is not touched.  Stream-ordered, synchronises nowhere.  K as for spmf_waic_accumulate. */
size_t spmf_groups_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows, int S, int32_t n_groups,
                                 int32_t n_cols);
int spmf_group_sums(spmf_ctx* ctx, const spmf_counts* counts, int S,
                    const float* const params[SPMF_NVARS], const float* eta,
                    const int32_t* labels, int32_t n_groups, int32_t n_cols, const int32_t* cols,
                    double* sum_out, double* nonzero_out,
                    void* scratch, size_t scratch_bytes, void* stream);

/* ---- per-row sums of the predictions over column sets (added within ABI 6: two new entry points, no struct changed) ----
 * The posterior predictive reduced over columns: a gene-set or signature score per row, with its posterior
 * standard deviation, without a [n_rows][columns] block (csrc/sets.hip).  With m_s as for spmf_predict_columns,
 * for every row b of the batch `counts` and every set g < n_sets, whose list is set_cols[set_ptr[g] ..
 * set_ptr[g+1]) with the weights set_weights[..] beside it (j runs over the list: a column listed twice counts
 * twice):
 *   score_s(b, g)   = sum_j (double)w_j * (double)m_s(b, c_j)            per draw s
 *   mean[b*ld + g]  = (1/S) sum_s score_s(b, g), fp64, added in draw order;
 *   sd[b*ld + g]    = the unbiased standard deviation of score_s over the draws (fp64 Welford in draw order),
 *                     which needs S >= 2; sd may be NULL.
 * Both are fp64, device, row stride ld >= n_sets; columns n_sets .. ld-1 of a row are not written, so several
 * calls may fill column ranges of one array.  All additions are fp64: w_j * m_s is formed from the two converted
 * operands (exact), no fp32 partial sums and no atomics.  The order of the additions of a set is a function of
 * that set's own list, S and K alone: a set's output has the same bits whatever the other sets of the call, its
 * position among them, or how the rows are cut into calls; two calls return the same bits.  Sets may overlap;
 * signed weights give a contrast of two signatures its own posterior sd.
 * set_ptr: HOST array of n_sets + 1 offsets, set_ptr[0] == 0, non-decreasing; it is read during the call only.
 * set_cols: int32, device; set_weights: fp32, device, or NULL for weight 1.  An empty set scores 0 (sd 0) in
 * every row.  A listed column outside [0, D) reads nothing and makes its set NaN in every row.  A row with a NaN
 * count is NaN in every non-empty set; a non-finite cell makes its set NaN for that row.
 * params: only u, v, w, s (slots 2, 0, 1, 7) are read, each with the leading axis S.
 * scratch: 256-byte aligned, at least spmf_sets_scratch_bytes(ctx, counts->n_rows, S, n_sets, set_ptr) bytes:
 * the draw stage's scratch and the compacted tables of the padded list (every set in whole 64-column blocks:
 * P = 64 * sum_g ceil(n_g / 64) columns, S * P * (KP + 1) floats and 9 P bytes) -- bound it by calling over
 * runs of sets.  The size is 0 for bad arguments (a bad set_ptr included).
 * SPMF_E_ARG for the draw stage's errors (S outside 1..65535, NULL params / eta / scratch, a misaligned
 * scratch, a mixed context without column types, a struct_size mismatch), n_sets < 0, a set_ptr that is NULL
 * (n_sets > 0), does not start at 0 or decreases, ld < n_sets, sd with S < 2; SPMF_E_UNSUPPORTED for P >= 2^31;
 * then SPMF_E_WORKSPACE for a short scratch, naming the need; then SPMF_E_ARG for a NULL mean with work to do
 * or a NULL set_cols with listed columns; every error returns before any launch or write.  n_sets == 0 or
 * n_rows == 0 returns SPMF_OK without work; when every set is empty the outputs are zero-filled and the draw
 * stage does not run.  The context's workspace is not touched.  Stream-ordered, synchronises nowhere.  K as for
 * spmf_waic_accumulate. */
size_t spmf_sets_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows, int S, int32_t n_sets,
                               const int64_t* set_ptr);
int spmf_set_scores(spmf_ctx* ctx, const spmf_counts* counts, int S,
                    const float* const params[SPMF_NVARS], const float* eta,
                    int32_t n_sets, const int64_t* set_ptr, const int32_t* set_cols,
                    const float* set_weights, int64_t ld, double* mean, double* sd,
                    void* scratch, size_t scratch_bytes, void* stream);

/* ---- posterior mean encoding (added within ABI 6: two new entry points, no struct changed) ----
 * The rows of the batch `counts` in the latent space: mean_out[b][k] = (1/S) sum_s z_sb[k], k < K,
 * where z_sb is the encode sweep of draw s (what spmf_encode computes from u_s, s_s), fp32, the sum in
 * draw order times 1/S; with sd_out the unbiased standard deviation over the draws (Welford in draw
 * order), which needs S >= 2.  mean_out / sd_out: [n_rows][K], unpadded.  A NaN count makes its whole
 * row NaN.  (csrc/knn.hip)
 * params: only u, v, w, s (slots 2, 0, 1, 7) are read, each with the leading axis S.
 * scratch: 256-byte aligned, at least spmf_embed_scratch_bytes(ctx, counts->n_rows, S) bytes (the
 * draw stage's scratch alone); SPMF_E_WORKSPACE when short.  SPMF_E_ARG for S outside 1..65535, NULL
 * params / eta / scratch / mean_out, sd_out with S < 2, a misaligned scratch, a mixed context without
 * column types or a struct_size mismatch; every error returns before any launch.  The context's
 * workspace is not touched.  Stream-ordered, synchronises nowhere.  Bit-reproducible, and a row's
 * result does not depend on how the rows are cut into calls. */
size_t spmf_embed_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows, int S);
int spmf_embed_rows(spmf_ctx* ctx, const spmf_counts* counts, int S,
                    const float* const params[SPMF_NVARS], const float* eta, float* mean_out,
                    float* sd_out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- exact k nearest rows (added within ABI 6: two new entry points, no struct changed) ----
 * For every row of q [n_query][row_len] the k nearest rows of r [n_ref][row_len] (fp32, device,
 * 1 <= row_len <= 256 whatever the context's K, 1 <= k <= 64), without an array of size
 * n_query * n_ref (csrc/knn.hip).  The context serves the error message and the device only.
 * flags bit 0: cosine distance 1 - cos instead of the Euclidean distance.  self_offset >= 0: query i
 * IS reference row self_offset + i and is no candidate of its own; -1: no exclusion.
 *   Working rows: Euclidean q' = q - c, r' = r - c with c the mean of the finite reference rows
 * (fixed-order sums, no float atomics; distances do not depend on c, it removes the cancellation
 * of the expansion below for clouds far from the origin); cosine q' = q/|q|, r' = r/|r|.  They are
 * zero-padded to KP = 4 .. 256 in the scratch; q == r with n_query == n_ref is prepared once.
 *   Selection score s_ij = <q'_i, r'_j> - 1/2 |r'_j|^2 on the exact-f32 matrix cores: the larger
 * score is the nearer row, equal scores go to the smaller index.  A candidate has a finite score
 * and is not the excluded self: a non-finite reference row is none, a non-finite query row (or a
 * zero row under cosine) has none.  The best k candidates are then refined from the caller's rows:
 * Euclidean dist = sqrt(sum_k (q_ik - r_jk)^2) by fmaf in ascending k, cosine
 * dist = 1/2 sum_k (q'_ik - r'_jk)^2 = 1 - cos, and ordered by (dist ascending, index ascending).
 * The expansion only decides membership at near-ties; the distances carry no cancellation.
 *   idx_out int32 [n_query][k], dist_out fp32 [n_query][k]; fewer than k candidates are padded
 * with -1 / +inf at the tail.  Bit-reproducible; a query's result does not depend on the other
 * queries or on its position in the list.
 * scratch: 256-byte aligned, at least spmf_knn_scratch_bytes(ctx, n_query, n_ref, row_len) bytes
 * (it does not depend on k); SPMF_E_WORKSPACE when short, naming the need.  SPMF_E_ARG for
 * n_ref > 2^31 - 1, a negative count, k outside 1..64, row_len outside 1..256, unknown flag bits,
 * self_offset < -1, NULL q / idx_out / dist_out with n_query > 0, NULL r with n_ref > 0, a NULL or
 * misaligned scratch; every error returns before any launch with "knn: " in front of the message.
 * n_query == 0 returns SPMF_OK without work; n_ref == 0 fills the padding.  Stream-ordered,
 * synchronises nowhere. */
size_t spmf_knn_scratch_bytes(const spmf_ctx* ctx, int64_t n_query, int64_t n_ref, int row_len);
int spmf_knn(spmf_ctx* ctx, const float* q, int64_t n_query, const float* r, int64_t n_ref,
             int row_len, int k, unsigned flags, int64_t self_offset, int32_t* idx_out,
             float* dist_out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- one Lloyd step of k-means (added within ABI 6: two new entry points, no struct changed) ----
 * For the rows x [n_rows][row_len] and the centroids [n_clusters][row_len] (fp32, device,
 * 1 <= row_len <= 256 whatever the context's K, 1 <= n_clusters <= 65536): every row's nearest
 * centroid, and per cluster the fp64 sums of its rows from which the caller forms the next
 * centroids (csrc/kmeans.hip behind csrc/knn.hip).  Like spmf_knn the call takes rows as given: the
 * context serves the error message and the device only.
 *   Assignment: labels_out[i] and dist_out[i] are, bit for bit, idx_out[i][0] and dist_out[i][0]
 * of spmf_knn(q = x, r = centroids, k = min(4, n_clusters), flags = 0, self_offset = -1) -- the
 * same launches: the centre is the mean of the finite centroids, the score <x', c'> - 1/2 |c'|^2 on
 * the exact-f32 matrix cores, and the best min(4, G) candidates are refined by the fmaf chain of
 * squared differences in ascending k and ordered by (distance, index).  Four candidates, not one:
 * the expansion decides membership only at near-ties, the label is the exact-distance minimum among
 * them.  A non-finite row of x gets label -1 and distance +inf; a non-finite centroid is nobody's
 * label; of equal centroids the smaller index wins.  labels_out int32 [n_rows]; dist_out fp32
 * [n_rows], may be NULL.  A row's label and distance do not depend on the other rows or on its
 * position.
 *   Accumulation: sums_out[g][k], fp64 [n_clusters][row_len], = the sum of (double)x[i][k] over the
 * rows labelled g; counts_out[g], int64, their number; stats_out[0] = the sum of (double)dist_i^2
 * over the labelled rows, stats_out[1] = the rows with labels_out[i] != prev_labels[i] (n_rows when
 * prev_labels is NULL), stats_out[2] = the rows with label -1 (fp64 [3]).  All outputs are
 * overwritten, not added to.  Every addition is fp64 from the first one on: no fp32 partial sums, no
 * floating-point atomics.
 *   Orders: the rows are put in label order, stable in the row index, every cluster in whole 64-row
 * blocks (the ordering of spmf_group_sums).  With KP = row_len rounded up to 4, 8, .., 256, the rows
 * at positions rr, rr + 256 / KP, .. of a cluster's blocks are added in ascending order, blocks
 * ascending, per run of blocks; the 256 / KP partial sums are added in ascending rr, and a cluster's
 * runs in ascending order.  The statistics add 256 rows by a fixed tree and those sums in a fixed
 * order.  All of it is a function of (n_rows, n_clusters, row_len, the labels) alone: two calls
 * return the same bits.
 * scratch: 256-byte aligned, at least spmf_kmeans_scratch_bytes(ctx, n_rows, n_clusters, row_len)
 * bytes, non-decreasing in n_rows; the size is 0 for bad arguments.
 * SPMF_E_ARG for n_clusters outside 1..65536, row_len outside 1..256, n_rows outside 0..2^31 - 64,
 * prev_labels == labels_out, NULL sums_out / counts_out / stats_out, NULL x / centroids /
 * labels_out with n_rows > 0, a NULL or misaligned scratch; then SPMF_E_WORKSPACE for a short
 * scratch, naming the need; every error returns before any launch or write with "kmeans_step: " in
 * front of the message.  n_rows == 0 returns SPMF_OK after zero fills of sums_out, counts_out and
 * stats_out on the stream.  The context's workspace is not touched: the call may sit between
 * spmf_step_begin and spmf_step_end.  Stream-ordered, synchronises nowhere. */
size_t spmf_kmeans_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows, int32_t n_clusters,
                                 int row_len);
int spmf_kmeans_step(spmf_ctx* ctx, const float* x, int64_t n_rows, int row_len,
                     const float* centroids, int32_t n_clusters, const int32_t* prev_labels,
                     int32_t* labels_out, float* dist_out, double* sums_out, int64_t* counts_out,
                     double* stats_out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- silhouette of labelled rows (added within ABI 6: two new entry points, no struct changed) ----
 * For the rows x [n_rows][row_len] (fp32, device, 1 <= row_len <= 256 whatever the context's K) with
 * labels int32 [n_rows] into 1 <= n_clusters <= 65536 clusters: every member's mean distance to its
 * own cluster and to the nearest other one over ALL pairs, and the silhouette from the two, without an
 * array of size n_rows * n_rows or n_rows * n_clusters (csrc/silhouette.hip).  The cost is n_rows^2
 * distances.  The context serves the error message and the device only.  flags bit 0: cosine distance
 * 1 - cos instead of the Euclidean distance.
 *   Members: row i is a member of cluster g = labels[i] when 0 <= g < n_clusters and all its values
 * are finite (under cosine its norm, the fp32 fmaf chain of knn's working rows, must also be positive
 * and finite).  Every other row -- label -1 or any label outside [0, n_clusters), a non-finite row --
 * is a non-member: it belongs to no cluster, gets sil = a = b = NaN and nearest = -1, and has no
 * influence on any member's result, bit for bit.  n_g is the number of members of g.
 *   Distances: working rows as spmf_knn's, Euclidean x' = x - c with c the mean of the member rows
 * (fp64 sums in a fixed order, no float atomics, rounded to fp32), cosine x' = x/|x|; zero-padded to
 * KP = 4 .. 256 and laid out in label order, stable in the row index, every cluster in whole 64-row
 * blocks (the ordering of spmf_group_sums); bias_j = -1/2 |x'_j|^2 (fmaf chain, fp32).  The tile value
 * t_ij = <x'_i, x'_j> + bias_j comes from the exact-f32 matrix cores (the tile loop of spmf_knn's
 * selection), u_ij = -(bias_i + t_ij) = 1/2 |x'_i - x'_j|^2 in fp32, and
 *   Euclidean d_ij = sqrtf(max(0, 2 u_ij)),   cosine d_ij = max(0, u_ij)   (= 1 - cos for unit rows).
 * d_ii is not added; pad positions of a block are not added.  The absolute error of one d^2 is about
 * 2^-24 KP (|x'_i|^2 + |x'_j|^2): distances far below the rows' norms are coarse.
 *   Per member i of cluster g, all in fp64 (each fp32 d_ij is converted before its first addition):
 * a_i = sum_{j in g, j != i} d_ij / (n_g - 1), 0 when n_g = 1;  b_i = the smallest over the clusters
 * h != g with n_h > 0 of sum_{j in h} d_ij / n_h, nearest_i that h, equal means going to the smaller
 * index;  s_i = 0 when n_g = 1 or max(a_i, b_i) = 0, else (b_i - a_i) / max(a_i, b_i), in [-1, 1].
 * With fewer than two non-empty clusters b = +inf, nearest = -1 and s = NaN for every member.
 * sil_out, a_out, b_out: fp32 [n_rows] in the caller's row order (the fp64 values rounded); a_out and
 * b_out may be NULL.  nearest_out: int32 [n_rows], may be NULL.
 *   Per cluster: cluster_sum_out[g], fp64 [n_clusters], = the sum of the fp64 s_i over the members of
 * g (per 64-row block by a fixed tree, the blocks in ascending order; 0 for an empty cluster);
 * counts_out[g], int64, = n_g.  Both are overwritten, not added to.  The caller forms the clusters'
 * means and the overall score sum_g cluster_sum[g] / sum_g n_g.
 *   Orders: a row's sum over a cluster adds, per position of a 64-row block, the blocks in ascending
 * order, then the 64 positions by a fixed tree.  Everything is a function of (G, row_len, the
 * members and their labels) alone: two calls return the same bits, and dropping the non-members from
 * the input changes no bit of a member's results.
 * scratch: 256-byte aligned, at least spmf_silhouette_scratch_bytes(ctx, n_rows, n_clusters, row_len)
 * bytes, a multiple of 256, non-decreasing in n_rows; the size is 0 for bad arguments.
 * SPMF_E_ARG for n_clusters outside 1..65536, row_len outside 1..256, n_rows outside 0..2^31 - 64,
 * unknown flag bits, NULL cluster_sum_out / counts_out, NULL x / labels / sil_out with n_rows > 0, a
 * NULL or misaligned scratch; then SPMF_E_WORKSPACE for a short scratch, naming the need; every error
 * returns before any launch or write with "silhouette: " in front of the message.  n_rows == 0
 * returns SPMF_OK after zero fills of cluster_sum_out and counts_out on the stream.  The context's
 * workspace is not touched.  Stream-ordered, synchronises nowhere. */
size_t spmf_silhouette_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows, int32_t n_clusters,
                                     int row_len);
int spmf_silhouette(spmf_ctx* ctx, const float* x, int64_t n_rows, int row_len,
                    const int32_t* labels, int32_t n_clusters, unsigned flags, float* sil_out,
                    float* a_out, float* b_out, int32_t* nearest_out, double* cluster_sum_out,
                    int64_t* counts_out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- epochs of a 2-D graph layout (added within ABI 6: two new entry points, no struct changed) ----
 * The full-batch form of UMAP's layout objective on a weighted graph in CSR form (csrc/graph_layout.hip):
 * indptr int64 [n_rows + 1], indices int32 [nnz], weights fp32 [nnz], positions y_in / y_out fp32
 * [n_rows][2], all on the device; y_out may be y_in (they may not overlap otherwise).  The call runs the
 * epochs e = epoch0 .. epoch0 + n_epochs - 1 of a schedule of total_epochs, one launch per epoch behind a
 * copy of y_in into the scratch.  The context serves the error message and the device only.
 *   One epoch reads the positions y of the epoch before it and writes every row's new position into
 * the other buffer (Jacobi, alternating between the two halves of the scratch, the last epoch into
 * y_out): no row writes another row's position, so there are no atomics and no races.  For row i with
 * its valid entries (j, w_ij), W_i = sum_j w_ij, D = y_i - y_j, d2 = |D|^2, clip4 = the clamp of each
 * component to [-4, 4], q = a d2^b (through exp2f(b log2f(d2))):
 *   attraction  F_i  = sum_j w_ij clip4(c_a D),  c_a = -2ab d2^(b-1) / (1 + q) = -2b q / (d2 (1 + q));
 *               the term is 0 when d2 = 0;
 *   repulsion   F_i += (negative_rate W_i / M) sum_{m < M} clip4(c_r (y_i - y_r)),
 *               c_r = 2 repulsion b / ((0.001 + d2)(1 + q)),  r = r(i, e, m),  M = n_negatives;
 *               the term is 0 when r = i, when d2 = 0 or when y_r is not finite; the scale keeps M;
 *   update      y_i <- y_i + alpha_e F_i / max(1, W_i),  alpha_e = lr (1 - e / total_epochs), formed in
 *               fp64 on the host and passed as fp32.
 * An entry of weight w is what UMAP's sampler visits w times an epoch, each visit with negative_rate
 * negatives, and both endpoints pull themselves.  The division by max(1, W_i) makes the simultaneous
 * step a convex combination of clipped per-entry steps.  a, b, -2b, 2 repulsion b and
 * negative_rate / M are rounded to fp32 once; all arithmetic of an epoch is fp32.
 *   Negatives: Philox4x32-10 with key = (seed's low word, seed's high word) and counter =
 * (i, m >> 2, e, 0x554D4150); word m & 3 of the block in x, y, z, w order; r = the high 32 bits of
 * word * n_rows.  A draw is a function of (seed, i, e, m, n_rows): epochs split over several calls
 * give the bits of one call.
 *   Robustness: an entry whose index lies outside [0, n_rows), whose weight is not finite and
 * positive or whose neighbour's position is not finite is skipped (it is no part of W_i); indptr
 * values are clamped to [0, nnz]; no argument values make a kernel read outside its arrays.  A row
 * with a non-finite position keeps its bits, and so does a row with W_i = 0, which is still a
 * possible negative of others.
 *   Order: a row's additions run in an order fixed by its own list length and M alone (16 lanes
 * striding the list, then a fixed tree); two calls return the same bits.
 * scratch: 256-byte aligned, at least spmf_graph_layout_scratch_bytes(ctx, n_rows) bytes, a multiple
 * of 256, non-decreasing in n_rows; the size is 0 for bad arguments.
 * SPMF_E_ARG for n_rows outside 0..2^31 - 64 or nnz < 0, n_negatives outside 1..64, epoch0 < 0,
 * n_epochs < 0 or epoch0 + n_epochs > total_epochs, a <= 0, b <= 0, a non-finite or negative lr /
 * repulsion / negative_rate, NULL indptr / y_in / y_out with n_rows > 0 (indices / weights with
 * nnz > 0 too), a NULL or misaligned scratch; then SPMF_E_WORKSPACE for a short scratch, naming the
 * need; every error returns before any launch or write with "graph_layout: " in front of the
 * message.  n_rows == 0 or n_epochs == 0 returns SPMF_OK; with n_epochs == 0 and y_out != y_in, y_in
 * is copied.  The context's workspace is not touched.  Stream-ordered, synchronises nowhere. */
size_t spmf_graph_layout_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows);
int spmf_graph_layout(spmf_ctx* ctx, int64_t n_rows, int64_t nnz, const int64_t* indptr,
                      const int32_t* indices, const float* weights, const float* y_in, float* y_out,
                      int epoch0, int n_epochs, int total_epochs, double lr, double a, double b,
                      double repulsion, double negative_rate, int n_negatives, uint64_t seed,
                      void* scratch, size_t scratch_bytes, void* stream);

/* ---- new rows on a fitted 2-D layout (added within ABI 6: one new entry point, no scratch) ----
 * umap-learn's transform (csrc/graph_transform.hip): n_query new rows are laid out among n_ref reference
 * rows whose positions y_ref fp32 [n_ref][2] stay fixed.  idx int32 and w fp32 [n_query][k] hold every
 * query row's k neighbours among the reference rows and their memberships (a bipartite graph in dense
 * form); y_in / y_out fp32 [n_query][2]; all on the device.  y_out may be y_in (they may not overlap
 * otherwise); y_in may be NULL.  The call runs the epochs e = epoch0 .. epoch0 + n_epochs - 1 of a
 * schedule of total_epochs in ONE launch: no query row reads another query row, so a row's 16 lanes load
 * its neighbours once, keep them in registers and write y_out once.  The context serves the error message
 * and the device only.
 *   Query row i has the global number g = row0 + i.  Its valid entries are the (j, w_ij) with
 * 0 <= j < n_ref, w_ij finite and > 0 and y_ref[j] finite; W_i = the sum of the valid weights.
 *   Start: with y_in == NULL, y_i = sum_j w_ij y_j / W_i, (NaN, NaN) when W_i = 0; else y_in[i].
 *   One epoch e, with D = y_i - y_j, d2 = |D|^2, clip4 and q = a d2^b as in spmf_graph_layout:
 *   attraction  F_i  = sum_j w_ij clip4(c_a D),  c_a = -2b q / (d2 (1 + q)); the term is 0 when d2 = 0;
 *   repulsion   F_i += (negative_rate W_i / M) sum_{m < M} clip4(c_r (y_i - y_ref[r])),
 *               c_r = 2 repulsion b / ((0.001 + d2)(1 + q)),  r = r(g, e, m),  M = n_negatives;
 *               the term is 0 when d2 = 0 or when y_ref[r] is not finite (there is no r = i rule: the
 *               two row sets differ); the scale keeps M;
 *   update      y_i <- y_i + alpha_e F_i / max(1, W_i),  alpha_e = (float)(lr (1 - e / total_epochs)),
 *               formed in fp64 in the kernel: the bits spmf_graph_layout forms on the host.
 * a, b, -2b, 2 repulsion b and negative_rate / M are rounded to fp32 once; all other arithmetic of an
 * epoch is fp32.
 *   Negatives: Philox4x32-10 with key = (seed's low word, seed's high word) and counter =
 * ((uint32)g, m >> 2, e, 0x554D5854); word m & 3 of the block in x, y, z, w order; r = the high 32 bits
 * of word * n_ref.  With n_ref == 0 no negative is drawn and nothing of y_ref is read.
 *   Rows that keep their bits: a row whose position is not finite (from y_in, or after an epoch), and a
 * row with W_i = 0 -- from a NULL y_in it is NaN.
 *   Order: a row's additions run in an order fixed by k and M alone (lane l of 16 takes the entries
 * l, l + 16, .. and the negatives l, l + 16, .., then a fixed tree).  A row's result is a function of
 * its own entries, y_ref, g and the arguments: rows may be mapped in chunks of any size, with row0 the
 * chunk's first global number, and epochs split over several calls (through epoch0 and y_in) give the
 * bits of one call.  No argument values make the kernel read outside its arrays.
 * SPMF_E_ARG for k outside 1..64, n_negatives outside 1..64, n_query < 0, n_ref outside 0..2^31 - 1,
 * row0 < 0 or row0 + n_query > 2^32, epoch0 < 0, n_epochs < 0 or epoch0 + n_epochs > total_epochs,
 * a <= 0, b <= 0, a non-finite or negative lr / repulsion / negative_rate, NULL idx / w / y_out with
 * n_query > 0, NULL y_ref with n_ref > 0, NULL y_in with epoch0 > 0 (a continued schedule needs its
 * positions); every error returns before any launch or write with "graph_transform: " in front of the
 * message.  n_query == 0 returns SPMF_OK; with n_epochs == 0 the start is written, or y_in is copied
 * when y_out differs.  The context's workspace is not touched.  Stream-ordered, synchronises nowhere. */
int spmf_graph_transform(spmf_ctx* ctx, int64_t n_query, int k, const int32_t* idx, const float* w,
                         const float* y_ref, int64_t n_ref, const float* y_in, float* y_out,
                         int64_t row0, int epoch0, int n_epochs, int total_epochs, double lr, double a,
                         double b, double repulsion, double negative_rate, int n_negatives,
                         uint64_t seed, void* stream);

/* ---- multiplying by the graph (added within ABI 6: five new entry points, no struct changed) ----
 * What a deterministic eigensolver of S = D^-1/2 A D^-1/2 needs of the graph spmf_graph_layout takes
 * (csrc/spectral.hip; spmf_amd/spectral.py is the solver): the scaling, the product with a tall block,
 * and two small fp64 reductions over tall blocks.  A block is fp32 [n_rows][SPMF_BLOCK_COLS], row-major, on
 * the device, 16-byte aligned: one row is one 64-byte segment; a caller with fewer columns leaves the rest zero.  The graph
 * is read under spmf_graph_layout's rules: an indptr value is clamped to [0, nnz], a falling indptr is an
 * empty row, an entry counts only if its index lies in [0, n_rows) and its weight is finite and > 0;
 * n_rows <= 2^31 - 64.  No argument values make a kernel read outside its arrays.  None of the calls has
 * an atomic: two calls return the same bits.  The context serves the error message and the device only.
 *
 * spmf_graph_scale: scale[i] = 1 / sqrt(d_i) with d_i the fp64 sum of row i's valid weights, rounded
 *   once to fp32; 0 for a row without a valid entry.  Lane l of the row's 16 takes the entries l, l + 16,
 *   .. in ascending order, then a fixed tree: the order is a function of the row's list length alone.
 * spmf_graph_spmm: Y_i = c_s s_i sum_j w_ij s_j X_j + X_i o c_x + c_z Z_i over the valid entries of row
 *   i in list order, s = 1 with scale == NULL.  c_x: HOST, SPMF_BLOCK_COLS doubles, read before the return
 *   (one per column: with c_s = 1, c_x = -lambda the call forms the residual block S V - V Lambda).  c_s,
 *   c_x and c_z are rounded to fp32 once on the host; everything else is fp32: t = w_ij s_j, acc =
 *   fmaf(t, X_jl, acc) from 0, Y_il = fmaf(c_z, Z_il, fmaf(c_x[l], X_il, (c_s s_i) acc)).  A lane owns a
 *   column, so an entry of Y is a function of its row's list alone.  z may be NULL when c_z = 0.  y may
 *   be z (a row reads Z_i and writes Y_i itself); y == x is refused: other rows gather X.  Values of X
 *   and Z are taken as given: a NaN reaches the rows that list it and no further.
 * spmf_block_gram: g[a * 16 + b] = sum_r x_ra y_rb in fp64 (device, 256 doubles).  Rows are cut into chunks
 *   of SPMF_GRAM_CHUNK_ROWS; a chunk's sum runs in ascending r, then the chunks' sums are added in ascending
 *   order: the bits are a function of (x, y, n_rows).  x may be y.  scratch: 256-byte aligned, at least
 *   spmf_block_gram_scratch_bytes(ctx, n_rows) bytes (a multiple of 256, non-decreasing in n_rows; 0 for
 *   bad arguments).
 * spmf_block_rotate: Y = X R, r HOST, 256 doubles row-major, read before the return: Y_ib = the fp64 sum
 *   of X_ik r[k * 16 + b] in ascending k from 0, rounded once to fp32.  y may be x (a row is read whole
 *   before it is written).
 *
 * SPMF_E_ARG for n_rows outside 0..2^31 - 64, nnz < 0, a NULL pointer where one is needed (indptr, the
 * blocks and outputs with n_rows > 0; indices / weights with nnz > 0; c_x, r, g and the scratch always; z
 * with c_z != 0), a non-finite coefficient (or one beyond fp32), y == x in spmf_graph_spmm ("aliases"), a
 * misaligned scratch; then SPMF_E_WORKSPACE for a short one, naming the need; every error returns before
 * any launch or copy with the entry's name ("graph_scale: ", "graph_spmm: ", "block_gram: ",
 * "block_rotate: ") in front of the message.  n_rows == 0 returns SPMF_OK behind the checks (spmf_block_gram
 * zero-fills g on the stream).  The context's workspace is not touched.  Stream-ordered, synchronises
 * nowhere. */
#define SPMF_BLOCK_COLS 16
#define SPMF_GRAM_CHUNK_ROWS 512
int spmf_graph_scale(spmf_ctx* ctx, int64_t n_rows, int64_t nnz, const int64_t* indptr,
                     const int32_t* indices, const float* weights, float* scale, void* stream);
int spmf_graph_spmm(spmf_ctx* ctx, int64_t n_rows, int64_t nnz, const int64_t* indptr,
                    const int32_t* indices, const float* weights, const float* scale, const float* x,
                    const float* z, float* y, double c_s, const double* c_x, double c_z, void* stream);
size_t spmf_block_gram_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows);
int spmf_block_gram(spmf_ctx* ctx, int64_t n_rows, const float* x, const float* y, double* g,
                    void* scratch, size_t scratch_bytes, void* stream);
int spmf_block_rotate(spmf_ctx* ctx, int64_t n_rows, const float* x, const double* r, float* y,
                      void* stream);

/* ---- shortest-path sweeps on the graph (added within ABI 6: two new entry points, no struct changed) ----
 * Single- and multi-source shortest paths on a CSR graph of edge lengths, as spmf_graph_spmm in the (min, +)
 * semiring (csrc/graph_paths.hip; spmf_amd/geodesic.py is the driver that repeats the call to the fixed point).
 * A block is fp32 [n_rows][SPMF_BLOCK_COLS] as above, a column per source or set of sources: the start holds 0 on
 * a column's sources and +inf elsewhere.  The graph is read under spmf_graph_spmm's rules: an indptr value is
 * clamped to [0, nnz], a falling indptr is an empty row, an entry counts only if its index lies in [0, n_rows)
 * and its length is finite and > 0; n_rows <= 2^31 - 64.  No argument values make a kernel read outside its
 * arrays.  No atomic: two calls return the same bits.
 *
 * One sweep X -> Y.  For row i and column l, with best = +inf and arg = -1, the counting entries (j, w_ij) of
 *   the row are walked in list order: t = X_jl + w_ij, one fp32 addition; if t < best then best = t, arg = j.
 *   Then Y_il = best < X_il ? best : X_il.  A lane owns a column, so Y_il is a function of row i's list and of
 *   column l of X alone.  Values are taken as given: a NaN never wins a <, so it stays where it is and reaches
 *   nobody.  fl(a + w) is monotone in a and a minimum does not depend on the order, so the fixed point of the
 *   sweep is unique: bit for bit what an fp32 Dijkstra making the same left-to-right additions returns.
 * n_sweeps >= 0 sweeps run as that many launches, alternating between the two blocks of the scratch; x_in is
 *   copied into the first, so x_out may be x_in.  n_sweeps == 0 copies x_in to x_out.
 * changed_out (device, one int32, may be NULL): zero-filled on the stream before the last sweep, then set to 1
 *   by every lane whose Y_il differs from its X_il in that last sweep (a plain store; all writers store the
 *   same word): 0 tells that x_out is the fixed point.  With n_sweeps == 0 it is zero-filled.
 * pred_out (device, int32 [n_rows][SPMF_BLOCK_COLS], may be NULL): written by the last sweep only (not at all
 *   with n_sweeps == 0): arg where best == Y_il, Y_il is finite and X_{arg,l} < Y_il; else -1.  On a converged
 *   block that is the first entry in list order that attains the row's distance from a strictly nearer row:
 *   the chain of predecessors strictly decreases in distance, so it is acyclic and ends at a source (which has
 *   -1, all lengths being positive) or at -1.  A reached row that is no source gets -1 only where the addition
 *   was absorbed -- w below half an ulp of the distance, fl(X_jl + w) == X_jl: such a row has the distance of
 *   its neighbour and no strictly nearer one.
 *
 * scratch: 256-byte aligned, at least spmf_graph_relax_scratch_bytes(ctx, n_rows) bytes, a multiple of 256 and
 * non-decreasing in n_rows (0 for n_rows outside the range).
 *
 * SPMF_E_ARG for n_rows outside 0..2^31 - 64, nnz < 0, n_sweeps < 0, a NULL pointer where one is needed (indptr,
 * x_in, x_out with n_rows > 0; indices / lengths with nnz > 0; the scratch always), an output (x_out, pred_out,
 * changed_out) that is one of indptr, indices, lengths or another output, or pred_out / changed_out == x_in
 * ("aliases"), a misaligned scratch; then SPMF_E_WORKSPACE for a short one, naming the need; every error returns
 * before any launch or write with "graph_relax: " in front of the message.  n_rows == 0 returns SPMF_OK behind
 * the checks.  The context's workspace is not touched.  Stream-ordered, synchronises nowhere. */
size_t spmf_graph_relax_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows);
int spmf_graph_relax(spmf_ctx* ctx, int64_t n_rows, int64_t nnz, const int64_t* indptr,
                     const int32_t* indices, const float* lengths, const float* x_in, float* x_out,
                     int32_t* pred_out, int32_t* changed_out, int n_sweeps, void* scratch,
                     size_t scratch_bytes, void* stream);

/* ---- modularity moves on the graph (added within ABI 6: one new entry point, no struct changed) ----
 * One Jacobi sweep of Louvain's local moving on a graph in CSR whose weights are int64 fixed point
 * (csrc/graph_move.hip; spmf_amd/communities.py is the driver and has the whole algorithm).  Every sum is an
 * int64 sum, exact and the same in any order; the score is four fp64 operations, each rounded on its own.
 * No atomic, no scratch: two calls return the same bits, and a row's new label is a function of that row's
 * list, labels_in and tot alone.
 *
 * indptr is read under spmf_graph_spmm's rules (clamped to [0, nnz], a falling indptr is an empty row).  An
 * entry counts when its column lies in [0, n_rows) and wq >= 1.  For row i with a = labels_in[i]:
 *   k_i   = the sum of the row's counting wq (a self entry (i, i) included),
 *   e_ic  = the sum of wq over the counting entries j != i with labels_in[j] == c,
 *   score(c) = double(e_ic) - ((gamma * double(k_i)) * double(tot'[c])) / double(m2),
 *   tot'[a] = tot[a] - k_i, tot'[c] = tot[c] otherwise.
 * Candidates are the labels c of the row's counting non-self entries with c in [0, n_rows); direction 0
 * admits only c > a, direction 1 only c < a.  labels_out[i] is the admitted candidate of largest score, the
 * smaller c on equal scores, if that score is strictly greater than score(a); else a.  A row with k_i = 0,
 * and a row whose own label lies outside [0, n_rows), keeps its label.
 *
 * Two tilings of one method.  A row of at most SPMF_MOVE_GROUP_LEN entries is moved by a group of 16 lanes,
 * four rows to a wave: the entries in registers, one broadcast step per entry.  A longer row is moved only if
 * long_rows (device, int32 [n_long], any order, NULL with n_long == 0) lists it: one 256-thread workgroup per
 * listed row, a thread per candidate of a 256-entry tile, the row streamed through LDS tiles of 256 for every
 * candidate tile -- any length, no table, no capacity, at a cost of O(d^2 / 256) per row of d entries.  A
 * long row left off the list keeps its label; a short row on it gets the value the group path writes; an
 * entry of long_rows outside [0, n_rows) is skipped.
 *
 * SPMF_E_ARG for n_rows outside 0..2^31 - 64, nnz < 0, n_long outside 0..2^31 - 64, a NULL pointer where one
 * is needed (indptr, labels_in, tot, labels_out with n_rows > 0; indices / wq with nnz > 0; long_rows with
 * n_long > 0), gamma not finite and > 0, m2 <= 0, direction not 0 or 1, labels_out == labels_in ("aliases":
 * other rows read labels_in); every error returns before any launch with "graph_move: " in front of the
 * message.  n_rows == 0 returns SPMF_OK behind the checks.  The context's workspace is not touched.
 * Stream-ordered, synchronises nowhere. */
#define SPMF_MOVE_GROUP_LEN 64
int spmf_graph_move(spmf_ctx* ctx, int64_t n_rows, int64_t nnz, const int64_t* indptr,
                    const int32_t* indices, const int64_t* wq, const int32_t* labels_in,
                    const int64_t* tot, const int32_t* long_rows, int64_t n_long, double gamma,
                    int64_t m2, int direction, int32_t* labels_out, void* stream);

/* ---- the entries summed by the groups of their two ends (added within ABI 6: two new entry points, no struct
 * changed) ----
 * The dense group-to-group tables of a labelled graph in CSR whose weights are int64 fixed point
 * (csrc/graph_groups.hip; spmf_amd/paga.py is the driver and turns the integers into PAGA's connectivities).
 * Every sum is an integer sum, exact and the same in any order: the kernel uses integer atomics in LDS and, per
 * segment of one group's rows, at most n_groups 64-bit global atomics -- never one per entry -- and two calls
 * return the same bits.  No floating-point arithmetic anywhere.
 *
 * indptr is read under spmf_graph_spmm's rules (clamped to [0, nnz], a falling indptr is an empty row).  With
 * G = n_groups, take row i with a = labels[i].  Entry p of that row counts when all of these hold:
 *   a lies in [0, G);  j = indices[p] lies in [0, n_rows);  wq[p] >= 1;  b = labels[j] lies in [0, G).
 * Self entries and repeated columns count as listed.  Then
 *   count_out[a * G + b]  = the number of counting entries,
 *   weight_out[a * G + b] = the int64 sum of their wq,
 *   size_out[a]           = the number of rows with label a, with or without entries.
 * All three outputs (int64 [G][G], [G][G], [G]) are overwritten in full.  A label outside [0, G) is "no
 * group": such a row is skipped as a source and as a target and counts in no size.
 *
 * The rows are ordered by label first (the ordering of spmf_group_sums, in the scratch); a workgroup then takes
 * blocks of one group's rows and keeps that group's row of the two tables in LDS, 16 KB at
 * SPMF_GROUP_EDGES_MAX_GROUPS; a row of any length is walked by 16 lanes, and entries inside the row's own
 * group are summed in registers.
 *
 * scratch: 256-byte aligned, at least spmf_graph_group_edges_scratch_bytes(ctx, n_rows, n_groups) bytes (a
 * multiple of 256, non-decreasing in n_rows; 0 for arguments the call refuses).
 *
 * SPMF_E_ARG for n_rows outside 0..2^31 - 64, nnz < 0, n_groups outside 1..SPMF_GROUP_EDGES_MAX_GROUPS, a NULL
 * pointer where one is needed (the three outputs and the scratch always; indptr and labels with n_rows > 0;
 * indices / wq with nnz > 0), an output that is one of indptr, indices, wq, labels or another output
 * ("aliases"), a misaligned scratch; then SPMF_E_WORKSPACE for a short one, naming the need; every error
 * returns before any launch or fill with "graph_group_edges: " in front of the message.  n_rows == 0 zero-fills
 * the outputs on the stream and returns SPMF_OK behind the checks.  The context's workspace is not touched.
 * Stream-ordered, synchronises nowhere. */
#define SPMF_GROUP_EDGES_MAX_GROUPS 1024
size_t spmf_graph_group_edges_scratch_bytes(const spmf_ctx* ctx, int64_t n_rows, int32_t n_groups);
int spmf_graph_group_edges(spmf_ctx* ctx, int64_t n_rows, int64_t nnz, const int64_t* indptr,
                           const int32_t* indices, const int64_t* wq, const int32_t* labels,
                           int32_t n_groups, int64_t* count_out, int64_t* weight_out, int64_t* size_out,
                           void* scratch, size_t scratch_bytes, void* stream);

/* Reductions of the non-finite rule (poisson.py:606-616) over a dense ll
 * buffer of n cells; io = double[3] on the device.
 *   pass 0: io[0] = min(io[0], min over finite cells)  (initialise io[0]=0:
 *           the reference's where(finite, ll, 0) puts 0 into the minimum)
 *   pass 1: io[1] += sum where(finite, clip(ll, io[0]-10, 0), io[0]-10),
 *           io[2] += number of non-finite cells. */
int spmf_nonfinite_reduce(spmf_ctx* ctx, int64_t n, const float* ll, int pass,
                          double* io, void* stream);

/* Third reduction of the rule: io[3] = min(io[3], index_base + i) over the
 * cells i of ll[0..n) whose value equals the global minimum io[0] (initialise
 * io[3] = +inf): the linear index (draw * B*D + row * D + column, built by the
 * caller through index_base) of the minimum's cell, where d(min_val) flows. */
int spmf_nonfinite_argmin(spmf_ctx* ctx, int64_t n, const float* ll, double index_base,
                          double* io, void* stream);

/* out[0] += sum of lgamma(x+1) over the stored Poisson cells of `counts` whose entry
 * in rate[n_rows, D] (spmf_dense_ll's output for the same counts) is not a positive
 * finite number: the cells the rule replaces.  Their lgamma is part of the batch's
 * pre-summed constant (counts.lgamma_sum) and spmf_nonfinite_patch takes it back out. */
int spmf_nonfinite_lgamma(spmf_ctx* ctx, const spmf_counts* counts, const float* rate,
                          double* out, void* stream);

/* Apply the rule (poisson.py:606-616) to the packed accumulators that
 * spmf_data_pass left for S draws of `counts`, VALUE AND GRADIENT, so that a
 * following spmf_finish returns the energy the reference computes when stored
 * cells have a non-finite log-pmf (rate 0 under a positive count):
 *   'x'_s  += nnf_s * (io[0] - 10) + sum over those cells of lgamma(x+1)
 *   draw s* (the draw of the minimum's cell io[3]): gA' / gV' / gphi gain
 *   (sum_s nnf_s) * d ll(cell) / d theta   -- clip is the identity on finite
 *   cells, replaced cells are worth min_val, whose derivative is that of the
 *   minimum's cell (tf.reduce_min).
 * io = double[4]: [0] global minimum over all S*B*D cells (spmf_nonfinite_reduce
 * pass 0 over spmf_dense_ll output), [3] its cell (spmf_nonfinite_argmin);
 * nlg = double[S]: spmf_nonfinite_lgamma per draw.
 * Row shards: call it on the shard's OWN (not yet summed) accumulators with
 * io[0] = the minimum over the shard minima, io[2] = sum_s nnf_s over ALL shards
 * (0: taken from the accumulators, the single-shard case) and io[3] = +inf on
 * every shard but the one that holds the minimum's cell; the value terms are
 * per shard and add up in the all-reduce that follows. */
int spmf_nonfinite_patch(spmf_ctx* ctx, const spmf_counts* counts, int S,
                         const float* const params[SPMF_NVARS], const float* eta,
                         const double* io, const double* nlg, void* stream);

/* ---- VI step around the energy: surrogate posterior and optimiser ------- */
/* One latent variable of the mean-field surrogate (poisson.py:403-569).
 * kind 0: theta = softplus(t0 + softplus(t1)*eps)      (tfb.Softplus(Normal))
 * kind 1: theta = t0 + softplus(t1)*eps                (tfb.Identity(Normal), bernoulli.py:187-193)
 * kind 2: theta = softplus(softplus(t1) / g), g ~ Gamma(softplus(t0), 1)
 *                                                      (tfb.Softplus(InverseGamma))
 * noise = eps or g, [S,n]; dgda = d g / d concentration [S,n] (kind 2). */
typedef struct spmf_sur_var {
  const float* t0;
  const float* t1;
  const float* noise;
  const float* dgda;
  float* theta;        /* [S,n] written by spmf_surrogate_fwd */
  const float* gtheta; /* [S,n] dE/dtheta, read by spmf_surrogate_bwd */
  float* g0;           /* [n] d loss / d t0, written by spmf_surrogate_bwd */
  float* g1;           /* [n] d loss / d t1 */
  int32_t n;
  int32_t kind;
  /* optional per-element override for kind 0 (mixed likelihood): ident[i] != 0
   * means element i has the Identity bijector (kind 1). NULL otherwise. */
  const uint8_t* ident;
  /* elements between consecutive draws in noise / dgda (they may be slices of
   * one [S, total] buffer drawn for all variables at once); 0 means n. */
  int64_t noise_ld;
} spmf_sur_var;

/* (spmf_sample_noise and spmf_surrogate_fwd skip a variable whose n is 0: nothing is read or written for it,
 * the other variables keep their indices -- the Philox counter of a draw and the order of the log q sum do
 * not depend on which variables a call covers, so a caller may draw / transform the variables in two calls.) */
/* Base noise for every variable, drawn on the device into the caller's noise
 * (and, kind 2, dgda) buffers: eps ~ N(0,1), or g ~ Gamma(softplus(t0), 1) with
 * its implicit-reparameterisation derivative d g / d concentration.  Counter-based
 * (Philox4x32-10): the draw is a pure function of (seed, counter [+ state[13]],
 * variable index, draw, element), so replicas on different ranks that pass the
 * same seed draw the same noise, and a step replayed from a hipGraph gets fresh
 * noise through the device-resident step counter state[13] (spmf_vi_gate advances
 * it; pass state = NULL to use `counter` alone).
 * Domain of dgda: its series runs to the first term past g and stops after 4000 terms, so the
 * derivative is valid for draws g < 3998, which a concentration softplus(t0) <= 3500 keeps
 * (g <= a + 8 sqrt(a)); above that the series is cut short and dgda is wrong.  g itself is
 * clamped below at 1e-30. */
int spmf_sample_noise(spmf_ctx* ctx, const spmf_sur_var* vars, int nvars, int S, uint64_t seed,
                      uint64_t counter, const double* state, void* stream);

/* spmf_sample_noise + spmf_surrogate_fwd with the draw and the transform in ONE launch (ABI 6; the VI step's path): a
 * thread draws its element's base noise, transforms it while it is in registers, writes noise / dgda
 * (spmf_surrogate_bwd needs them), theta and its share of log q; a second small launch adds the per-workgroup sums up
 * in a fixed order.  Same draws and same theta bits as the two calls, logq equal to fp64 rounding (other partial-sum
 * groups); three launches become two. */
int spmf_sample_transform(spmf_ctx* ctx, const spmf_sur_var* vars, int nvars, int S, uint64_t seed,
                          uint64_t counter, const double* state, double* logq, void* stream);

/* theta for every variable and logq[S] (fp64) = sum over variables and
 * elements of log q(theta). */
int spmf_surrogate_fwd(spmf_ctx* ctx, const spmf_sur_var* vars, int nvars, int S,
                       double* logq, void* stream);
/* Gradient of  loss = -(1/(S*B)) sum_s [E_s - c*logq_s]  wrt the trainables,
 * given gtheta = dE/dtheta; inv_sb = 1/(S*B).  (E = x + z +
 * c*prior, c = B/N.) */
int spmf_surrogate_bwd(spmf_ctx* ctx, const spmf_sur_var* vars, int nvars, int S,
                       double inv_sb, double c, void* stream);

typedef struct spmf_adam_var {
  float* p;
  float* m;
  float* v;
  const float* g;
  int32_t n;
  int32_t reserved_;
} spmf_adam_var;
/* tf.keras-style Adam (bias-corrected, eps outside the sqrt) over up to 24
 * tensors in one launch; clip > 0 clips each gradient element to [-clip, clip]
 * first (clip_value, bin/factorize_csv.py:44-47); step is 1-based. */
int spmf_adam_step(spmf_ctx* ctx, const spmf_adam_var* tensors, int ntensors, double lr,
                   double beta1, double beta2, double eps, int step, double clip,
                   void* stream);

/* spmf_surrogate_bwd and spmf_adam_step_dev in ONE pass over the trainables (the
 * gradient of a trainable never goes to memory): tensors[2i], tensors[2i+1] are the
 * Adam records (p, m, v, n; g unused) of vars[i].t0 / vars[i].t1, p pointing at the
 * same memory; vars[i].g0 / g1 are not written.  Gated by state[9] like
 * spmf_adam_step_dev.  The training loop's step path; the two separate calls remain
 * for callers that want the gradient. */
int spmf_surrogate_bwd_adam_dev(spmf_ctx* ctx, const spmf_sur_var* vars, int nvars, int S,
                                double inv_sb, double c, const spmf_adam_var* tensors,
                                const double* state, void* stream);

/* Device-resident optimiser state, so that a whole VI step (noise, surrogate,
 * energy + gradient, chain rule, Adam) is a fixed launch sequence with no host
 * read-back and can be captured in a hipGraph and replayed.  state is a device
 * array of SPMF_VI_STATE_LEN doubles:
 *   [0] lr  [1] beta1  [2] beta2  [3] eps  [4] clip (0 = off)     (host-written)
 *   [5] beta1^t  [6] beta2^t  [7] t                               (init 1, 1, 0)
 *   [8] loss of the last step  [9] 1 if it was applied, 0 if skipped
 *   [10] sum of applied losses  [11] applied steps  [12] skipped steps
 *   [13] steps gated so far, applied or not (the RNG step counter of spmf_sample_noise)
 *   [14] saturation events (log_transform decoder: exp evaluated at min(y, 70); counted per
 *        workgroup) summed over the steps gated since the caller last zeroed it
 * spmf_vi_gate computes loss = -mean_s[x + z + c*(prior - log q)]/rows from the
 * [S,14] parts of spmf_finish and log q of spmf_surrogate_fwd (SURVEY 8a row
 * 14), marks the step skipped when the loss is not finite or a stored cell's
 * log-pmf was not ("Batch loss NaN, skipping",
 * notebooks/factorizing_random_noise.ipynb:122-420), and advances [5..7],
 * [10..12], [14].  n_nonfinite is the [2*S] array spmf_finish wrote ([0:S] non-finite stored
 * cells, [S:2S] saturation events) or NULL.  spmf_adam_step_dev is spmf_adam_step reading
 * every scalar from state; it does nothing when [9] == 0. */
#define SPMF_VI_STATE_LEN 16
int spmf_vi_gate(spmf_ctx* ctx, const double* parts, const double* logq,
                 const double* n_nonfinite, int S, double c, double rows, double* state,
                 void* stream);
int spmf_adam_step_dev(spmf_ctx* ctx, const spmf_adam_var* tensors, int ntensors,
                       const double* state, void* stream);

/* Test/diagnostic taps: per-row z and d/dz of the LAST draw processed by
 * spmf_data_pass, [B,KP] fp32 with KP = spmf_padded_k(). */
int spmf_padded_k(const spmf_ctx* ctx);
const float* spmf_z_ptr(const spmf_ctx* ctx);
const float* spmf_gz_ptr(const spmf_ctx* ctx);

/* Per-kernel device time, averaged over the (up to 64) most recent
 * spmf_data_pass + spmf_finish pairs issued since timing was enabled
 * (hipEvents recorded on `stream` between the kernels of the last draw; the
 * query synchronises, the hot path does not): ms[6] = prep, row pass (sparse
 * launches), column pass, finish, sum of all, dense exp kernels
 * (log_transform only, else 0).  For bench.py's roofline. */
int spmf_ctx_enable_timing(spmf_ctx* ctx, int on);
int spmf_last_timing(spmf_ctx* ctx, float* ms6);

#if defined(SPMF_BUILD)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* SPMF_HIP_H */
