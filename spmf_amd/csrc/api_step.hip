// api_step.hip -- the step behind the C-ABI (include/spmf_hip.h): which dense form a context runs, the layout
// and binding of its workspace, the launches' argument blocks, the data pass, the prior half and the finish,
// spmf_step_begin .. spmf_step_end, the encode sweep with spmf_encode / spmf_dense_ll, the spmf_nonfinite_* entries.
// Host-side orchestration only (ctx.h).
#include <stdio.h>

#include "ctx.h"

using namespace spmf;

// Small batches run all S draws in ONE launch per kernel (gridDim.y = S): the per-draw tables and
// row outputs then exist S times.  Only for the linear Poisson decoder.  Two cases:
//   * the S table pairs stay L2 sized (<= 3 MB): any batch up to 256 MB of row outputs -- beyond that size a
//     draw is gather-bound, its tables want the L2 to themselves, and draws run in turn;
//   * the batch is launch-bound whatever the tables weigh (<= kSmallBatchRows rows: the reference's own
//     harness trains on batches of 10 rows with sample_size = 20, tests/spmf_test.py:35-43, where D = 350,
//     K = 50 gives 3.58 MB of tables -- just over the cut above -- and 20 launch sequences per step): a
//     draw's tables are only touched by that draw's few rows, residency is moot, and S x 4 launches
//     become 4.  Bounded by 512 MB of tables.
constexpr int64_t kSmallBatchRows = 2048;
static bool batched_draws(const spmf_ctx* c, int64_t rows, int S) {
  if (S < 2 || c->Dh > 0) return false;
  if (c->flags & (SPMF_FLAG_LOG_TRANSFORM | SPMF_FLAG_BERNOULLI | SPMF_FLAG_MIXED)) return false;
  const size_t tables = (size_t)S * 2 * c->D * c->KP * sizeof(float);
  const size_t rowbuf = (size_t)S * 2 * (size_t)rows * c->KP * sizeof(float);
  if (rows <= kSmallBatchRows && tables <= ((size_t)512 << 20)) return true;
  return tables <= (3u << 20) && rowbuf <= (256u << 20);
}

// a bf16x3 dense launcher answered "shape not covered": the dense term of the step would be missing from
// gzs / gV' / the softplus sum -- fail instead (dense_form below is meant to make this unreachable)
static int dense3_uncovered(spmf_ctx* c) {
  return fail(c, SPMF_E_UNSUPPORTED, "data_pass: the bf16x3 dense kernels do not cover this launch shape "
      "(set SPMF_DENSE_BF16X3=0 for the exact-f32 kernels)");
}

// rows of one E chunk: whole 128-row workgroups of the exp kernel, at most kEstCapBytes
static int64_t est_chunk_rows(const spmf_ctx* c, int64_t rows) {
  const size_t per_row = (size_t)((c->D + 31) / 32) * 32 * sizeof(float);
  int64_t cap = (int64_t)(c->est_cap_bytes / per_row) / 128 * 128;
  if (cap < 128) cap = 128;
  return rows < cap ? rows : cap;
}

// Which dense form a context runs: the workspace layout (the E buffer) and the launch sequence of the row stage
// (data_pass_impl, dense_rows) both follow this one answer.
enum DenseForm {
  kDenseNone,       // Poisson / linear decoder: closed-form dense term, one row pass
  kDenseSig3Fused,  // Bernoulli / mixed with the linear decoder (dense3.hip sigdot3, ACT 1): ONE fused row pass,
                    // the (Z, W) launch subtracts the dense row term from gzs in its epilogue
  kDenseExp3,       // Poisson log_transform at KP = 64 on the bf16x3 exp kernels (dense3.hip expdot3)
  kDenseSig3,       // KP = 32 on the sigdot3 family: Poisson log_transform (ACT 0, bin/factorize_scrnaseq_counts.py
                    // runs P = 3) or Bernoulli + log_transform (ACT 2: exp accumulators as ACT 0, sigmoid / softplus
                    // epilogue as ACT 1, E = sigmoid * exp)
  kDenseEKept,      // exact-f32 MFMA kernels (dense.hip) keeping E in HBM between their two contractions
  kDenseRecompute,  // exact-f32 MFMA kernels recomputing E in the second launch
};
// The bf16x3 forms recompute E (or the sigmoid) in their second launch.  The fused row pass is the sigmoid
// forms' only (C5 row launches 0.97 -> 0.84 ms); the exp decoder keeps sweep 1 -> dense -> sweep 2, where the
// fused two-stream row pass (20 spilled registers at four waves per SIMD) ran 13.9 ms against 12.8 for the two
// launches on C4 (profiles/r04_fused_rows_c4.txt).  Bernoulli + log_transform (code 4: E would have to carry
// exp(X) too) never keeps E.
static DenseForm dense_form(const spmf_ctx* c) {
  const int lik = likelihood_code(c);
  if (lik == 0) return kDenseNone;
  if (c->dense3) {
    if ((lik == 2 || lik == 3) && (c->KP == 32 || c->KP == 64)) return kDenseSig3Fused;
    if (lik == 1 && c->KP == 64) return kDenseExp3;
    if ((lik == 1 || lik == 4) && c->KP == 32) return kDenseSig3;
  }
  return c->e_once && lik != 4 ? kDenseEKept : kDenseRecompute;
}

// Q chunks (gridDim.y) of a P-stationary dense launch of nbx workgroup columns over ntiles Q tiles on
// `slots` resident workgroups: the count that fills whole rounds of the chip best, charging every
// workgroup a fixed prologue (P fragments, first tile) of about 0.7 tile-times.
static int pick_chunks(int nbx, int ntiles, int slots, int max_chunks) {
  int best = 1;
  double best_eff = -1.0;
  for (int c = 1; c <= ntiles && c <= max_chunks; ++c) {
    const int tpc = (ntiles + c - 1) / c;
    if ((ntiles + tpc - 1) / tpc != c) continue;          // some chunk would get no tile
    const long n = (long)nbx * c;
    const long rounds = (n + slots - 1) / slots;
    const double eff = ((double)n / (double)(rounds * slots)) * ((double)ntiles / ((double)c * tpc)) *
                       ((double)tpc / (tpc + 0.7));
    if (eff > best_eff + 1e-9) {
      best_eff = eff;
      best = c;
    }
  }
  return best;
}

// The workspace of a batch of `rows` rows under S draws.  acc | dacc are contiguous: the step's first prep launch
// zeroes them as one range.
static void ws_layout(Arena& a, const spmf_ctx* c, int64_t rows, int S, WsBuffers& w) {
  const size_t KP = c->KP, D = c->D, nS = S, B = rows;
  const unsigned dense_flags = SPMF_FLAG_LOG_TRANSFORM | SPMF_FLAG_BERNOULLI | SPMF_FLAG_MIXED;
  w.batched = batched_draws(c, rows, S) ? 1 : 0;
  const size_t nd = w.batched ? nS : 1;   // per-draw copies
  w.acc = a.take<float>(nS * acc_len(c->D, c->KP));
  w.dacc = a.take<double>(nS * kDaccRep * (kDaccHead + KP));
  w.dprep = a.take<double>(nS * kPrepSeg * (KP + 1));
  const size_t fnb = (D + kFinishCols - 1) / kFinishCols;   // workgroups of the finish kernel
  w.fpart = a.take<double>(nS * fnb * 12);
  w.futau = a.take<float>(nS * fnb * KP);
  w.Ap = a.take<float>(nd * D * KP);
  w.Vp = a.take<float>(nd * D * KP);
  w.phi = a.take<float>(nd * D);
  w.dbias = a.take<float>(D);
  const bool mixed = (c->flags & SPMF_FLAG_MIXED) != 0;
  w.Vb = mixed ? a.take<float>(D * KP) : nullptr;
  w.bb = mixed ? a.take<float>(D) : nullptr;
  w.z = a.take<float>(nd * B * KP);
  w.gzs = a.take<float>(nd * B * KP);
  w.gzd = (c->flags & dense_flags) ? a.take<float>(B * KP) : nullptr;
  w.est_rows = est_chunk_rows(c, rows);
  w.est = dense_form(c) == kDenseEKept ? a.take<float>((D + 31) / 32 * 32 * (size_t)w.est_rows) : nullptr;
}
static size_t ws_bytes_for(const spmf_ctx* c, int64_t rows, int S) {
  Arena a;
  WsBuffers w;
  ws_layout(a, c, rows, S, w);
  return a.used;
}

static int bind_ws(spmf_ctx* c, int64_t rows, int S) {
  if (!c->ws) return fail(c, SPMF_E_WORKSPACE, "no workspace set (spmf_ctx_set_workspace)");
  Arena a(c->ws, c->ws_bytes);
  WsBuffers w;
  ws_layout(a, c, rows, S, w);
  if (!a.fits()) {   // (what is bound stays bound)
    char b[160];
    snprintf(b, sizeof b, "workspace too small: need %zu bytes for rows=%lld S=%d, have %zu", a.used,
        (long long)rows, S, c->ws_bytes);
    return fail(c, SPMF_E_WORKSPACE, b);
  }
  static_cast<WsBuffers&>(*c) = w;
  c->ws_rows = rows;
  c->ws_S = S;
  return SPMF_OK;
}

// ---- the launches' argument blocks, each built in one place and by name ----------------------
static const float* row_scale_of(const spmf_ctx* c, const spmf_counts* ct) {
  return (c->flags & SPMF_FLAG_SCALE_ROWS) ? ct->row_scale : nullptr;
}

// S draws per launch; u, v, w, s are those of the launch's first draw.  (The mixed likelihood's ctype / dbias
// and the zero fill are the data pass's own.)
static PrepArgs prep_args(const spmf_ctx* c, int S, const Tables& T, const float* u, const float* v, const float* w,
    const float* s, const float* eta) {
  PrepArgs pa{};
  pa.D = c->D; pa.K = c->K; pa.S = S;
  pa.u = u; pa.v = v; pa.w = w; pa.s = s; pa.eta = eta;
  pa.Ap = T.Ap; pa.Vp = T.Vp; pa.phi = T.phi; pa.dprep = T.dprep;
  pa.logt = lik_exp(likelihood_code(c)) ? 1 : 0;
  return pa;
}

// The full row launch (mode 0) over the counts; `lik` is the likelihood code the kernel is built for.
static RowArgs row_args(const spmf_ctx* c, const spmf_counts* ct, int S, const Tables& T, int lik,
    int64_t dacc_stride) {
  RowArgs ra{};
  ra.B = ct->n_rows; ra.D = c->D; ra.S = S;
  ra.row_ptr = ct->row_ptr; ra.col = ct->col_idx; ra.val = ct->val; ra.ent = ct->ent;
  ra.row_scale = row_scale_of(c, ct);
  ra.Ap = T.Ap; ra.Vp = T.Vp; ra.phi = T.phi; ra.dprep = T.dprep;
  ra.z = T.z; ra.gzs = T.gzs; ra.dacc = T.dacc; ra.dacc_stride = dacc_stride;
  ra.mode = 0; ra.logt = lik; ra.ctype = lik == 3 ? c->ctype : nullptr;
  return ra;
}
// The encode-only sweep (mode 1) of `ra`: z from g(x) under the exp decoders (g has no packed stream), and
// never the dynamic tail -- its counters are the full launch's alone.
static RowArgs encode_sweep(RowArgs ra, const spmf_counts* ct) {
  ra.mode = 1;
  ra.dyn_tail = 0;
  if (lik_exp(ra.logt)) {
    ra.val = ct->gval;
    ra.ent = nullptr;
  }
  return ra;
}

// The column pass over column half hf of the accumulators `acc` (hf = 0 without a split: all columns); the
// pack block and the deterministic scratch are the data pass's own.
static ColArgs col_args(const spmf_ctx* c, const spmf_counts* ct, int S, const Tables& T, float* acc,
    const AccLayout& L, int hf) {
  const bool split = c->Dh > 0;
  ColArgs ca{};
  ca.D = c->D; ca.B = ct->n_rows; ca.S = S;
  ca.n_panels = ct->n_panels; ca.row_base = ct->row_base; ca.panel_rows = ct->panel_rows;
  ca.item_ptr = ct->item_ptr; ca.items = ct->items;
  ca.max_items_per_panel = split ? ct->max_items_half[hf] : ct->max_items_per_panel;
  ca.item_mid = split ? ct->item_mid : nullptr; ca.half_sel = split ? hf + 1 : 0;
  ca.pc_row = ct->pc_row; ca.pc_val = ct->pc_val; ca.pc_gval = ct->pc_gval; ca.pc_ent = ct->pc_ent;
  ca.pc_pad = ct->pc_pad;
  ca.Vp = T.Vp; ca.phi = T.phi; ca.z = T.z; ca.gzs = T.gzs;
  ca.gAp = acc + L.gA_off(hf); ca.gVp = acc + L.gV_off(hf); ca.gphi = acc + L.gphi_off(hf);
  ca.acc_stride = acc_len(c->D, c->KP);
  ca.logt = likelihood_code(c); ca.ctype = c->ctype;
  return ca;
}

// spmf_prior_async, spmf_finish and the step: the finish kernels' arguments without the data half's
// (finish_data_half sets them)
static FinishArgs finish_args(const spmf_ctx* c, int S, double prior_weight, const float* const* params,
    const float* eta, float* const* grads, double* parts) {
  FinishArgs fa{};
  fa.D = c->D; fa.K = c->K; fa.Dh = c->Dh; fa.S = S;
  fa.u_tau_scale = c->u_tau_scale; fa.s_tau_scale = c->s_tau_scale; fa.decay = c->decay;
  fa.prior_weight = prior_weight;
  fa.params = params; fa.eta = eta; fa.grads = grads; fa.parts = parts;
  fa.logt = likelihood_code(c); fa.ctype = c->ctype;
  fa.abs_horseshoe = (c->flags & SPMF_FLAG_ABS_HORSESHOE) ? 1 : 0;
  for (int i = 0; i < SPMF_NVARS; ++i) fa.vstride[i] = (int64_t)var_size(c, i);
  fa.ppart = c->fpart; fa.putau = c->futau;
  return fa;
}

namespace spmf {

// The checks, the prep launch and the encode sweep: z of every row under each of S draws into T->z.
// T == nullptr (spmf_encode, spmf_dense_ll): the tables of the workspace, bound here (one draw); otherwise
// those of the draw stage.
// Nothing is launched for an empty batch.
int encode_rows(spmf_ctx* c, const char* fn, const spmf_counts* ct, int S, const Tables* T, const float* u,
    const float* v, const float* w, const float* s, const float* eta, hipStream_t st) {
  const int logt = lik_exp(likelihood_code(c)) ? 1 : 0;
  int rc = check_counts(c, ct);
  if (!rc && logt && ct->nnz > 0 && !ct->gval) rc = fail(c, SPMF_E_ARG,
      std::string(fn) + ": log_transform needs counts.gval");
  if (rc || ct->n_rows == 0) return rc;
  Tables ws;
  if (!T) {
    rc = bind_ws(c, ct->n_rows, S);
    if (rc) return rc;
    ws = ws_tables(c);
    T = &ws;
  }
  launch_prep(c->KP, prep_args(c, S, *T, u, v, w, s, eta), st);
  // (sweep 1 does not depend on the likelihood; it writes z and nothing else: one scalar block for all draws)
  if (!launch_row_pass(c->KP, encode_sweep(row_args(c, ct, S, *T, logt, 0), ct), st)) return fail(c,
      SPMF_E_UNSUPPORTED, std::string(fn) + ": no encode kernel for this K");
  return SPMF_OK;
}

}  // namespace spmf

extern "C" {

size_t spmf_workspace_bytes(const spmf_ctx* c, int64_t max_rows, int S) {
  if (!c || max_rows < 0 || S < 1) return 0;
  size_t need = ws_bytes_for(c, max_rows, S);
  // (a batch of at most kSmallBatchRows rows keeps S table pairs: cover it too, so that every batch of up
  //  to max_rows rows fits the workspace this sizes)
  if (max_rows > kSmallBatchRows) {
    const size_t small = ws_bytes_for(c, kSmallBatchRows, S);
    if (small > need) need = small;
  }
  return need;
}

// The row stage of one draw of a context with a dense term (form != kDenseNone): the row pass(es) and the two
// dense launches.  `ra` holds what the row launches share (mode 0, the packed stream, the dynamic tail).
static int dense_rows(spmf_ctx* c, const spmf_counts* ct, DenseForm form, RowArgs ra, float* acc, const AccLayout& L,
    bool tm, hipStream_t st) {
  const int KP = c->KP, lik = ra.logt, B = (int)ct->n_rows;
  double* dacc = ra.dacc;
  const bool fused = form == kDenseSig3Fused;
  // fused: both sweeps read the same counts: ONE row pass (mode 3 leaves xi_b (gz_b - [veta] - z_b) in gzs) and the
  // (Z, W) launch subtracts the dense row term in its epilogue, gzs_b -= xi_b sum_d sigmoid(l_bd) V'_d, instead
  // of encode-only sweep -> dense -> stored-cell sweep (two row launches re-stream the entries and pass z
  // through HBM: DESIGN section 4).  Else z from g(x) (exp decoders) or the counts (sweep 1); the stored-cell
  // terms with the dense row term follow the dense launches (sweep 2)
  RowArgs r1 = fused ? ra : encode_sweep(ra, ct);
  if (fused) r1.mode = 3;
  launch_row_pass(KP, r1, st);
  if (tm) HIPCHK(c, hipEventRecord(c->ev[6], st));
  const int act = lik == 4 ? 2 : (lik >= 2 ? 1 : 0);   // dense.hip / dense3.hip ACT
  const float* lbias = lik == 3 ? c->dbias : c->phi;   // mixed: -1e30 masks the Poisson columns
  float* gVp = acc + L.gV_off(0);
  float* gphi_acc = acc + L.gphi_off(0);
  // mixed likelihood with the Bernoulli column list set: the dense sums run over those
  // columns only (compacted V' rows), instead of over all D with the Poisson half masked
  const float* Wd = c->Vp;
  int Dd = c->D;
  const int32_t* orows = nullptr;
  if (lik == 3 && c->bcols && c->n_bcols > 0) {
    launch_compact_rows(c->n_bcols, KP, c->bcols, c->Vp, c->phi, c->Vb, c->bb, st);
    Wd = c->Vb;
    Dd = c->n_bcols;
    lbias = c->bb;
    orows = c->bcols;
  }
  // The two products every form runs.  (Z, W): rows b against columns d, the bias on the Q rows:
  // gzd_b = sum_d E_bd V'_d for sweep 2, dacc[3] = sum E (ACT 0) or sum softplus(l) (ACT 1, 2); E = exp, sigmoid,
  // or sigmoid * exp.  (W, Z): the bias on the P rows: gV'_d -= sum_b E_bd z_b ; gphi_d -= sum_b sigmoid(l_bd)
  // (ACT 1, 2), added with float atomics.
  ExpdotArgs ez, ew;
  ez.NP = B; ez.P = c->z; ez.NQ = Dd; ez.Q = Wd;
  ez.out = c->gzd; ez.sign = 1.f; ez.esum = dacc + 3;
  ez.act = act; ez.bias_q = act ? lbias : nullptr;
  ew.NP = Dd; ew.P = Wd; ew.NQ = B; ew.Q = c->z;
  ew.out = gVp; ew.sign = -1.f; ew.atomic_out = 1;
  ew.act = act; ew.bias_p = act ? lbias : nullptr;
  ew.out2 = act ? gphi_acc : nullptr; ew.out_rows = orows;
  switch (form) {
    case kDenseExp3: {
      // E is recomputed by the second launch (at this matrix rate a B*D*4-byte round trip through HBM would be
      // the bound)
      if (!launch_expdot3(KP, ez, st)) return dense3_uncovered(c);
      // Q chunks of the W-stationary launch: whole rounds of the resident workgroups (one 110 KB
      // workgroup per CU: 118 column blocks x 13 chunks = 6 rounds of 256 on C4; 5 chunks = 590
      // workgroups ran 2.3 rounds, the last one a third full)
      ew.q_chunks = pick_chunks((Dd + expdot3_rows_per_wg() - 1) / expdot3_rows_per_wg(), (B + 127) / 128,
                                256 * expdot3_wgs_per_cu(), 64);
      if (!launch_expdot3(KP, ew, st)) return dense3_uncovered(c);
      break;
    }
    case kDenseSig3Fused:
    case kDenseSig3: {
      // Two waves per SIMD by registers: chunk counts that fill whole rounds of the resident workgroups.
      const int zt = (Dd + 127) / 128, wt = (B + 127) / 128;
      const int rpw = sigdot3_rows_per_wg(KP), slots = 256 * sigdot3_wgs_per_cu(KP);
      ez.q_chunks = pick_chunks((B + rpw - 1) / rpw, zt, slots, 16);
      ew.q_chunks = pick_chunks((Dd + rpw - 1) / rpw, wt, slots, 256);
      ez.atomic_out = ez.q_chunks > 1 ? 1 : 0;
      if (act) ez.e_planes = 3;   // V' rows have mixed signs under the Normal priors: third plane of E
      if (fused) {
        // gzs_b -= xi_b sum_d E_bd V'_d in the launch's epilogue
        ez.out = c->gzs; ez.sign = -1.f;
        ez.accumulate = 1; ez.p_scale = ra.row_scale;
      } else if (ez.q_chunks > 1) {
        launch_zero(c->gzd, (size_t)B * KP * sizeof(float), st);
      }
      if (!launch_sigdot3(KP, ez, st)) return dense3_uncovered(c);
      if (!launch_sigdot3(KP, ew, st)) return dense3_uncovered(c);
      break;
    }
    case kDenseEKept: {
      // E once: per row chunk, the Z-stationary kernel keeps E (exp, or the sigmoid of the
      // Bernoulli logits) and the second contraction (gV'_d -= sum_b E_bd z_b; Bernoulli:
      // gphi_d -= sum_b E_bd too) reads it back instead of recomputing it
      // (chunks of equal size, whole 128-row workgroups: a short last chunk would run the
      //  chip half empty)
      const int64_t nch = (ct->n_rows + c->est_rows - 1) / c->est_rows;
      int64_t step = ((ct->n_rows + nch - 1) / nch + 127) / 128 * 128;
      if (step > c->est_rows) step = c->est_rows;
      ez.est = c->est;
      for (int64_t r0 = 0; r0 < ct->n_rows; r0 += step) {
        const int nr = (int)((ct->n_rows - r0) < step ? (ct->n_rows - r0) : step);
        ez.NP = nr; ez.ldE = nr;
        ez.P = c->z + (size_t)r0 * KP; ez.out = c->gzd + (size_t)r0 * KP;
        launch_expdot(KP, ez, st);
        launch_estdot(KP, Dd, nr, ez.ldE, c->est, ez.P, ew.out, ew.sign, ew.out2, ew.out_rows, st);
      }
      break;
    }
    case kDenseRecompute: {
      launch_expdot(KP, ez, st);
      // W-stationary launch has only D/128 workgroups: split the row (Q) range
      // into chunks until ~4 workgroups per CU are in flight
      const int nbx = (Dd + 127) / 128;
      const int qtiles = (B + 127) / 128;
      int chunks = (1024 + nbx - 1) / nbx;
      if (chunks > qtiles) chunks = qtiles;
      if (chunks < 1) chunks = 1;
      ew.q_chunks = chunks;
      launch_expdot(KP, ew, st);
      break;
    }
    case kDenseNone:
      break;
  }
  if (tm) HIPCHK(c, hipEventRecord(c->ev[7], st));
  if (!fused) {
    ra.mode = 2;
    ra.gzd = c->gzd;
    launch_row_pass(KP, ra, st);
  }
  return SPMF_OK;
}

// parts: bit 0 = zero, prep, row pass and the column pass of the lower column half (all columns
// without a split); bit 1 = column pass of the upper half and the fp64 pack
static int data_pass_impl(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS],
    const float* eta, int parts_mask, void* stream, spmf_ctx::StepOut* so = nullptr) {
  if (!c || !params || !eta || S < 1) return fail(c, SPMF_E_ARG, "data_pass: bad arguments");
  if (!so) c->step.active = 0;   // a plain data pass ends a step begun earlier
  // likelihood / decoder code of the kernels: 0 Poisson linear, 1 Poisson log_transform, 2 Bernoulli
  const int logt = likelihood_code(c);
  const DenseForm form = dense_form(c);
  int rc = check_counts(c, ct);
  if (!rc && logt == 3 && !c->ctype) rc = fail(c, SPMF_E_ARG,
      "mixed likelihood: spmf_ctx_set_column_types was not called");
  if (!rc && lik_exp(logt) && ct->nnz > 0 && (!ct->gval || !ct->pc_gval)) rc = fail(c, SPMF_E_ARG,
      "counts: log_transform needs gval / pc_gval");
  if (rc) return rc;
  if (ct->n_rows > 0 && ct->nnz > 0 && (!ct->pc_row || !ct->pc_val || !ct->item_ptr || !ct->items || ct->n_panels < 1)) return fail(c, SPMF_E_ARG, "counts: panel-CSC arrays / work items missing");
  for (int i : {0, 1, 2, 7})
    if (!params[i]) return fail(c, SPMF_E_ARG, "data_pass: params v,w,u,s must be non-null");
  const bool det = c->det_buf != nullptr;
  if (det) {
    if (logt != 0 || c->Dh > 0 || parts_mask != 3) return fail(c, SPMF_E_UNSUPPORTED,
        "deterministic mode: Poisson / linear decoder without the column split only");
    if (ct->nnz > 0 && ct->n_rows > 0 && (!ct->list_first || !ct->item_pos || ct->n_items < 0)) return fail(c,
        SPMF_E_ARG, "deterministic mode: counts.list_first / item_pos / n_items missing (spmf_layout_build fills them)");
    if (spmf_det_scratch_bytes(c, ct->n_items, S) > c->det_bytes) return fail(c, SPMF_E_WORKSPACE,
        "deterministic mode: scratch smaller than spmf_det_scratch_bytes for this batch");
  }
  rc = bind_ws(c, ct->n_rows, S);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int KP = c->KP, D = c->D;
  const size_t al_ = acc_len(D, KP);
  const bool split = c->Dh > 0;
  const AccLayout L{D, KP, split ? c->Dh : D};
  if (split && ct->n_rows > 0 && ct->nnz > 0 && (!ct->item_mid || ct->col_split != c->Dh))
    return fail(c, SPMF_E_ARG, "counts: work items are not sorted for this context's column split");
  if (!split && parts_mask != 3) return fail(c, SPMF_E_ARG, "data_pass_split needs spmf_ctx_set_column_split");
  if (parts_mask != 3 && S != 1) return fail(c, SPMF_E_UNSUPPORTED, "data_pass_split: one draw per step only");
  const bool first = parts_mask & 1, second = parts_mask & 2;
  const DetDraw dd = det ? det_layout(c->det_buf, c->det_bytes, KP, ct->n_items) : DetDraw{};
  // acc | dacc (contiguous in the workspace) are zeroed by the first prep launch of the step,
  // slice by slice in its tile blocks; dprep is written, not accumulated (prep.hip)
  if (c->timing && first) {
    c->ev_set = (c->ev_set + 1) % spmf_ctx::kSets;
    c->ev = c->evs[c->ev_set];
    c->ev_valid = 0;
  }
  // batched: one pass of the loop launches every kernel once for all S draws (gridDim.y)
  const int nbat = c->batched ? S : 1;
  const int64_t dacc_stride = (int64_t)kDaccRep * (kDaccHead + KP);
  for (int s = 0; s < S; s += nbat) {
    const bool tm = c->timing && s + nbat == S;
    float* acc = c->acc + (size_t)s * al_;
    Tables T = ws_tables(c);   // (the scalar blocks are draw s's)
    T.dacc += (size_t)s * dacc_stride;
    T.dprep += (size_t)s * kPrepSeg * (KP + 1);
    double* det_slots = det ? dd.slots + s * dd.dstride : nullptr;
    float* det_part = det ? dd.part + s * dd.fstride : nullptr;
    bool packed = false;
    if (first) {
      if (tm) HIPCHK(c, hipEventRecord(c->ev[0], st));
      PrepArgs pa = prep_args(c, nbat, T, params[2] + s * var_size(c, 2), params[0] + s * var_size(c, 0),
          params[1] + s * var_size(c, 1), params[7] + s * var_size(c, 7), eta);
      if (logt == 3) {
        pa.ctype = c->ctype;
        pa.dbias = c->dbias;
      }
      if (s == 0) {
        pa.zero_p = c->acc;
        pa.zero_bytes = (size_t)((char*)c->dprep - (char*)c->acc);
      }
      if (so && nbat == S) {
        // spmf_step_begin with every draw in this launch: the prior half of the finish (all twelve prior
        // log-densities and prior_weight * d prior / d theta: parameters only) runs in the prep launch
        launch_step_begin(KP, pa, finish_args(c, S, so->prior_weight, so->params, so->eta, so->grads, so->parts), st);
        so->fused = 1;
      } else {
        launch_prep(KP, pa, st);
      }
      if (tm) HIPCHK(c, hipEventRecord(c->ev[1], st));
      if (ct->n_rows > 0) {
        RowArgs ra = row_args(c, ct, nbat, T, logt, dacc_stride);
        ra.dyn_tail = 1;   // the step's ONE full row launch hands its last rows out dynamically (row_pass.hip)
        if (form != kDenseNone) {
          rc = dense_rows(c, ct, form, ra, acc, L, tm, st);
          if (rc) return rc;
        } else {
          if (det) {
            ra.det_slots = det_slots;
            ra.det_stride = dd.dstride;
          }
          launch_row_pass(KP, ra, st);
        }
      }
      if (tm) HIPCHK(c, hipEventRecord(c->ev[2], st));
      // the caller's marker "the row stage of the last draw has been issued": what it makes wait for this event
      // runs beside the column pass instead of beside the resident-set row launch (spmf_ctx_set_rows_event)
      if (c->rows_event && s + nbat == S) HIPCHK(c, hipEventRecord(c->rows_event, st));
    }
    if (ct->n_rows > 0 && ct->nnz > 0) {
      for (int hf = 0; hf < 2; ++hf) {
        if (!(hf == 0 ? first : second)) continue;
        if (!split && hf == 1) continue;
        ColArgs ca = col_args(c, ct, nbat, T, acc, L, hf);
        if (det) {
          ca.det_slots = det_slots;
          ca.det_stride = dd.dstride;
          ca.det_part = det_part;
          ca.det_part_stride = dd.fstride;
        }
        if (hf == (split ? 1 : 0)) {
          // the fp64 scalars of the row pass are complete before this launch starts: its
          // extra first block folds them into the accumulator tail (the former pack launch)
          ca.pack_dacc = T.dacc;
          ca.pack_tail = acc + L.tail_off();
          ca.dacc_stride = dacc_stride;
          packed = launch_col_pass(KP, ca, st);
        } else {
          launch_col_pass(KP, ca, st);
        }
      }
    }
    if (det && ct->n_rows > 0 && ct->nnz > 0) {
      // the per-item partial sums, column by column in (panel, segment) order, into the zeroed accumulators
      DetReduceArgs dr{D, KP, ct->n_panels, nbat, ct->list_first, ct->item_pos, ct->item_ptr,
          det_part, dd.fstride,
          acc + L.gA_off(0), acc + L.gV_off(0), acc + L.gphi_off(0), (int64_t)al_};
      launch_det_reduce(dr, st);
    }
    if (second) {
      if (!packed) {
        PackArgs pk{KP, T.dacc, acc + L.tail_off(), nbat, dacc_stride, (int64_t)al_};
        launch_pack(pk, st);
      }
      if (tm) {
        HIPCHK(c, hipEventRecord(c->ev[3], st));
        c->ev_valid = 1;
      }
    }
  }
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_data_pass(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS],
    const float* eta, void* stream) {
  return data_pass_impl(c, ct, S, params, eta, 3, stream);
}

int spmf_data_pass_split(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS],
    const float* eta, int part, void* stream) {
  if (part != 0 && part != 1) return fail(c, SPMF_E_ARG, "data_pass_split: part must be 0 or 1");
  return data_pass_impl(c, ct, S, params, eta, part == 0 ? 1 : 2, stream);
}

int spmf_ctx_set_rows_event(spmf_ctx* c, void* event) {
  if (!c) return SPMF_E_ARG;
  c->rows_event = (hipEvent_t)event;
  return SPMF_OK;
}

int spmf_ctx_set_column_split(spmf_ctx* c, int Dh) {
  if (!c) return SPMF_E_ARG;
  if (Dh == 0 || Dh == c->D) {
    c->Dh = 0;
    return SPMF_OK;
  }
  if (Dh < 0 || Dh > c->D || (Dh % 32) != 0) return fail(c, SPMF_E_ARG,
      "column split must be a multiple of 32 inside (0, D)");
  if (c->flags & (SPMF_FLAG_LOG_TRANSFORM | SPMF_FLAG_BERNOULLI | SPMF_FLAG_MIXED))
    return fail(c, SPMF_E_UNSUPPORTED, "column split: linear Poisson decoder only");
  c->Dh = Dh;
  return SPMF_OK;
}

int spmf_acc_split(const spmf_ctx* c, int64_t off[2], int64_t len[2]) {
  if (!c || !off || !len) return SPMF_E_ARG;
  const AccLayout L{c->D, c->KP, c->Dh > 0 ? c->Dh : c->D};
  off[0] = 0;
  len[0] = L.half_len(0);
  off[1] = len[0];
  len[1] = acc_len(c->D, c->KP) - len[0];
  return SPMF_OK;
}


// all twelve params / grads non-null; with ABS_HORSESHOE only v, w, u, s (0, 1, 2, 7) are used
static int check_params_grads(spmf_ctx* c, const char* fn, const float* const params[SPMF_NVARS],
    float* const grads[SPMF_NVARS]) {
  const bool hsf = (c->flags & SPMF_FLAG_ABS_HORSESHOE) != 0;
  for (int i = 0; i < SPMF_NVARS; ++i)
    if ((!params[i] || !grads[i]) && !(hsf && i != 0 && i != 1 && i != 2 && i != 7))
      return fail(c, SPMF_E_ARG, std::string(fn) +
          ": params/grads must be non-null (all 12; v,w,u,s with ABS_HORSESHOE)");
  return SPMF_OK;
}

// the timing tap behind the step's last launch: the event set is complete once the data pass recorded its part
static int timing_close(spmf_ctx* c, hipStream_t st) {
  if (!c->timing) return SPMF_OK;
  HIPCHK(c, hipEventRecord(c->ev[5], st));
  if (c->ev_valid == 1) {
    c->ev_valid = 3;
    c->ev_count++;
  }
  return SPMF_OK;
}

// The data half of the finish over the bound accumulators: the step's last launch.  phase 0 / 2: launch_finish
// (whole finish / data half behind a prior half that ran on the side stream); kStepEnd: launch_step_end (data half
// + the fold of the per-block sums the prep launch's prior half left).
// (no zero fill: the fold writes the twelve prior parts and the u_tau gradient whole, the data half stores
//  parts 12 and 13 -- single writers)
constexpr int kStepEnd = -1;
static int finish_data_half(spmf_ctx* c, FinishArgs fa, int64_t n_rows_global, double lgamma_sum_global,
    double* n_nonfinite, int phase, hipStream_t st) {
  fa.B_global = n_rows_global; fa.lgamma_sum = lgamma_sum_global; fa.n_nonfinite = n_nonfinite;
  fa.acc = c->acc; fa.acc_stride = (int64_t)acc_len(c->D, c->KP); fa.dprep = c->dprep;
  if (c->timing) HIPCHK(c, hipEventRecord(c->ev[4], st));
  if (phase == kStepEnd) launch_step_end(c->KP, fa, st);
  else launch_finish(c->KP, fa, phase, st);
  const int rc = timing_close(c, st);
  if (rc) return rc;
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_prior_async(spmf_ctx* c, int S, double prior_weight, const float* const params[SPMF_NVARS],
    const float* eta, double* parts, float* const grads[SPMF_NVARS], void* stream) {
  if (!c || !params || !grads || !eta || !parts || S < 1) return fail(c, SPMF_E_ARG, "prior_async: bad arguments");
  int rc = check_params_grads(c, "prior_async", params, grads);
  if (rc) return rc;
  if (!c->fpart) return fail(c, SPMF_E_WORKSPACE, "prior_async: no data pass has bound the workspace yet");
  hipStream_t st = (hipStream_t)stream;
  if (!c->side) {
    HIPCHK(c, hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  }
  // the side stream forks off `stream` (outputs need no zero fill: single writers)
  HIPCHK(c, hipEventRecord(c->ev_fork, st));
  HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
  // one launch for all S draws (gridDim.y)
  launch_finish(c->KP, finish_args(c, S, prior_weight, params, eta, grads, parts), 1, c->side);
  HIPCHK(c, hipEventRecord(c->ev_join, c->side));
  HIPCHK(c, hipGetLastError());
  c->prior_pending = S;
  c->prior_parts = parts;
  return SPMF_OK;
}

int spmf_finish(spmf_ctx* c, int S, int64_t n_rows_global, double lgamma_sum_global, double prior_weight,
    const float* const params[SPMF_NVARS], const float* eta, double* parts, float* const grads[SPMF_NVARS],
    double* n_nonfinite, void* stream) {
  if (!c || !params || !grads || !eta || !parts || S < 1) return fail(c, SPMF_E_ARG, "finish: bad arguments");
  if (!c->acc || c->ws_S < S) return fail(c, SPMF_E_ARG, "finish: no data pass precedes it for this S");
  int rc = check_params_grads(c, "finish", params, grads);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the prior half may already be running on the side stream (spmf_prior_async
  // with these outputs): join it and add the data half only
  const bool joined = c->prior_pending == S && c->prior_parts == parts;
  c->prior_pending = 0;
  c->prior_parts = nullptr;
  if (joined) {
    HIPCHK(c, hipStreamWaitEvent(st, c->ev_join, 0));
  }
  // one launch for all S draws (gridDim.y)
  return finish_data_half(c, finish_args(c, S, prior_weight, params, eta, grads, parts), n_rows_global,
                          lgamma_sum_global, n_nonfinite, joined ? 2 : 0, st);
}

// ---- the step with its outputs known up front (ABI 6) -------------------------
int spmf_step_begin(spmf_ctx* c, const spmf_counts* ct, int S, double prior_weight,
    const float* const params[SPMF_NVARS], const float* eta, double* parts, float* const grads[SPMF_NVARS],
    double* n_nonfinite, void* stream) {
  if (!c || !params || !grads || !eta || !parts || S < 1) return fail(c, SPMF_E_ARG, "step_begin: bad arguments");
  int rc = check_params_grads(c, "step_begin", params, grads);
  if (rc) return rc;
  spmf_ctx::StepOut so;
  so.S = S;
  so.prior_weight = prior_weight;
  for (int i = 0; i < SPMF_NVARS; ++i) {
    so.params[i] = params[i];
    so.grads[i] = grads[i];
  }
  so.eta = eta;
  so.parts = parts;
  so.nnf = n_nonfinite;
  c->step.active = 0;
  rc = data_pass_impl(c, ct, S, params, eta, 3, stream, &so);
  if (rc) return rc;
  so.active = 1;
  c->step = so;
  return SPMF_OK;
}

int spmf_step_end(spmf_ctx* c, int64_t n_rows_global, double lgamma_sum_global, void* stream) {
  if (!c) return SPMF_E_ARG;
  if (!c->step.active || !c->acc) return fail(c, SPMF_E_ARG, "step_end: no spmf_step_begin precedes it");
  spmf_ctx::StepOut& so = c->step;
  so.active = 0;
  if (!so.fused)   // the draws ran in turn (S > 1 on a large batch): the whole finish, as spmf_finish runs it
    return spmf_finish(c, so.S, n_rows_global, lgamma_sum_global, so.prior_weight, so.params, so.eta, so.parts,
                       so.grads, so.nnf, stream);
  return finish_data_half(c, finish_args(c, so.S, so.prior_weight, so.params, so.eta, so.grads, so.parts),
                          n_rows_global, lgamma_sum_global, so.nnf, kStepEnd, (hipStream_t)stream);
}

int spmf_elbo_fwd_bwd(spmf_ctx* c, const spmf_counts* ct, int S, double prior_weight,
    const float* const params[SPMF_NVARS], const float* eta, double* parts, float* const grads[SPMF_NVARS],
    double* n_nonfinite, void* stream) {
  int rc = spmf_step_begin(c, ct, S, prior_weight, params, eta, parts, grads, n_nonfinite, stream);
  if (rc) return rc;
  return spmf_step_end(c, ct->n_rows, ct->lgamma_sum, stream);
}

int spmf_encode(spmf_ctx* c, const spmf_counts* ct, const float* u, const float* s, const float* eta, float* z_out,
    void* stream) {
  if (!c || !u || !s || !eta || !z_out) return fail(c, SPMF_E_ARG, "encode: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int rc = encode_rows(c, "encode", ct, 1, nullptr, u, nullptr, nullptr, s, eta, st);
  if (rc || ct->n_rows == 0) return rc;
  HIPCHK(c, hipMemcpy2DAsync(z_out, (size_t)c->K * sizeof(float), c->z, (size_t)c->KP * sizeof(float),
      (size_t)c->K * sizeof(float), (size_t)ct->n_rows, hipMemcpyDeviceToDevice, st));
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_dense_ll(spmf_ctx* c, const spmf_counts* ct, const float* u, const float* v, const float* w,
    const float* s, const float* eta, float* rate_out, float* ll_out, void* stream) {
  if (!c || !u || !v || !w || !s || !eta || !rate_out || !ll_out) return fail(c, SPMF_E_ARG,
      "dense_ll: bad arguments");
  const int lik = likelihood_code(c);
  if (lik == 3 && !c->ctype) return fail(c, SPMF_E_ARG, "dense_ll: spmf_ctx_set_column_types was not called");
  hipStream_t st = (hipStream_t)stream;
  const int rc = encode_rows(c, "dense_ll", ct, 1, nullptr, u, v, w, s, eta, st);
  if (rc || ct->n_rows == 0) return rc;
  DenseLLArgs da{ct->n_rows, c->D, lik, c->z, c->Vp, c->phi, c->ctype, ct->row_ptr, ct->col_idx, ct->val, rate_out,
      ll_out};
  launch_dense_ll(c->KP, da, st);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_nonfinite_reduce(spmf_ctx* c, int64_t n, const float* ll, int pass, double* io, void* stream) {
  if (!c || !ll || !io || n < 0 || (pass != 0 && pass != 1)) return fail(c, SPMF_E_ARG,
      "nonfinite_reduce: bad arguments");
  if (n == 0) return SPMF_OK;
  launch_nonfinite(n, ll, pass, io, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_nonfinite_argmin(spmf_ctx* c, int64_t n, const float* ll, double index_base, double* io, void* stream) {
  if (!c || !ll || !io || n < 0 || !(index_base >= 0.0)) return fail(c, SPMF_E_ARG, "nonfinite_argmin: bad arguments");
  if (n == 0) return SPMF_OK;
  launch_nonfinite_argmin(n, ll, index_base, io, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_nonfinite_lgamma(spmf_ctx* c, const spmf_counts* ct, const float* rate, double* out, void* stream) {
  if (!c || !rate || !out) return fail(c, SPMF_E_ARG, "nonfinite_lgamma: bad arguments");
  int rc = check_counts(c, ct);
  if (rc) return rc;
  if (ct->n_rows == 0 || ct->nnz == 0) return SPMF_OK;
  DenseLLArgs da{ct->n_rows, c->D, likelihood_code(c), nullptr, nullptr, nullptr, c->ctype, ct->row_ptr, ct->col_idx,
      ct->val, const_cast<float*>(rate), nullptr};
  launch_nonfinite_lgamma(da, out, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_nonfinite_patch(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS],
    const float* eta, const double* io, const double* nlg, void* stream) {
  if (!c || !params || !eta || !io || !nlg || S < 1) return fail(c, SPMF_E_ARG, "nonfinite_patch: bad arguments");
  int rc = check_counts(c, ct);
  if (rc) return rc;
  if (!c->acc || c->ws_S < S || c->ws_rows != ct->n_rows) return fail(c, SPMF_E_ARG,
      "nonfinite_patch: no data pass over this batch and S precedes it");
  for (int i : {0, 1, 2, 7})
    if (!params[i]) return fail(c, SPMF_E_ARG, "nonfinite_patch: params v,w,u,s must be non-null");
  const int logt = likelihood_code(c);
  if (lik_exp(logt) && ct->nnz > 0 && !ct->gval) return fail(c, SPMF_E_ARG, "nonfinite_patch: log_transform needs counts.gval");
  NfPatchArgs a{c->D, c->K, logt, ct->row_ptr, ct->col_idx, ct->val, row_scale_of(c, ct), params[2], params[0], params[1], params[7], eta,
      c->ctype, c->acc, (int64_t)acc_len(c->D, c->KP), c->Dh > 0 ? c->Dh : c->D, io, nlg, ct->n_rows, S};
  launch_nonfinite_patch(c->KP, a, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

}  // extern "C"
