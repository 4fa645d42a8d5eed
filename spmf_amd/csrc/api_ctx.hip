// api_ctx.hip -- the C-ABI of libspmf_hip.so (see include/spmf_hip.h): the context's life cycle and settings,
// the workspace it is given, the timing taps, the counts' checks and statistics, the deterministic scratch.
// Host-side orchestration only: argument checks, workspace carving, stream
// ordered launches.  No device allocation, no host<->device copies, no
// synchronisation on the hot path (timing taps excepted, off by default).
// The step is api_step.hip, the streaming calls api_stream.hip, the calls on rows and graphs as given api_points.hip
// and api_graph.hip, the collectives api_comm.hip, the VI kernels' entries api_vi.hip; ctx.h is what they share.
#include <stdio.h>
#include <stdlib.h>

#include "ctx.h"

using namespace spmf;

namespace spmf {

int check_counts(spmf_ctx* c, const spmf_counts* ct) {
  if (!ct) return fail(c, SPMF_E_ARG, "counts is null");
  if (ct->struct_size != (int32_t)sizeof(spmf_counts)) {
    char b[200];
    snprintf(b, sizeof b, "counts.struct_size is %d, this library's spmf_counts has %zu bytes: the caller was "
        "built against another spmf_hip.h (ABI version %d)", (int)ct->struct_size, sizeof(spmf_counts),
        SPMF_ABI_VERSION);
    return fail(c, SPMF_E_ARG, b);
  }
  if (ct->pc_pad < 0) return fail(c, SPMF_E_ARG, "counts.pc_pad must be >= 0");
  if (ct->pc_ent && ct->panel_rows > 65536) return fail(c, SPMF_E_ARG,
      "counts.pc_ent packs the row inside its panel into 16 bits: panel_rows must be <= 65536");
  if (ct->n_cols != c->D) return fail(c, SPMF_E_ARG, "counts.n_cols != ctx D");
  if (ct->n_rows < 0 || ct->nnz < 0 || ct->nnz > 2147483647LL) return fail(c, SPMF_E_ARG,
      "counts: bad n_rows/nnz (nnz must fit int32)");
  // the kernels gather factor rows with 32-bit byte offsets: B*KP*4 must stay below 4 GiB
  if (ct->n_rows * (int64_t)c->KP * 4 >= (1LL << 32) - c->KP * 4) return fail(c, SPMF_E_ARG,
      "counts: too many rows in one batch for this K (B*KP*4 must be < 4 GiB)");
  if (!ct->row_ptr || (ct->nnz > 0 && (!ct->col_idx || !ct->val))) return fail(c, SPMF_E_ARG,
      "counts: null CSR arrays");
  if (ct->ent && c->D > 65536) return fail(c, SPMF_E_ARG,
      "counts.ent packs the column into 16 bits: D must be <= 65536");
  return SPMF_OK;
}

DetDraw det_layout(void* buf, size_t bytes, int KP, int64_t n_items) {
  Arena a(buf, bytes);
  DetDraw d;
  d.slots = a.take<double>((size_t)kDetMeta + (size_t)kDetMaxBlocks * (kDaccHead + KP));
  d.part = a.take<float>((size_t)(n_items > 0 ? n_items : 0) * det_part_len(KP));
  d.bytes = a.used;
  d.dstride = (int64_t)(a.used / sizeof(double));
  d.fstride = (int64_t)(a.used / sizeof(float));
  return d;
}

}  // namespace spmf

extern "C" {

int spmf_version(void) { return SPMF_ABI_VERSION; }
size_t spmf_sizeof_counts(void) { return sizeof(spmf_counts); }
size_t spmf_sizeof_sur_var(void) { return sizeof(spmf_sur_var); }
size_t spmf_sizeof_adam_var(void) { return sizeof(spmf_adam_var); }

int spmf_ctx_create(int device, int K, int D, unsigned flags, spmf_ctx** out) {
  if (!out) return SPMF_E_ARG;
  *out = nullptr;
  if (K < 1 || K > 256 || D < 1) return SPMF_E_ARG;
  // K above 64: the whole-wave passes of widek.hip -- Poisson likelihood with the linear decoder only (the
  // dense exp / sigmoid operators of the other contexts are built for K padded to 32 or 64)
  if (K > 64 && (flags & (SPMF_FLAG_LOG_TRANSFORM | SPMF_FLAG_BERNOULLI | SPMF_FLAG_MIXED))) return SPMF_E_UNSUPPORTED;
  if ((int64_t)D * 64 * 4 >= (1LL << 32) - 256) return SPMF_E_ARG;   // 32-bit gather offsets into [D,KP]; the last KP*4 bytes below 4 GiB are the padded slots' (common.h kPadRow)
  spmf_ctx* c = new spmf_ctx();
  c->device = device;
  c->K = K;
  c->D = D;
  c->KP = padded_k(K);
  // the dense exp kernels of the log_transform decoder work on 32-feature MFMA tiles
  if ((flags & (SPMF_FLAG_LOG_TRANSFORM | SPMF_FLAG_BERNOULLI | SPMF_FLAG_MIXED)) && c->KP < 32) c->KP = 32;
  if ((flags & SPMF_FLAG_LOG_TRANSFORM) && (flags & SPMF_FLAG_MIXED)) {
    delete c;
    return SPMF_E_UNSUPPORTED;   // the per-column mix with the exp decoder is not built
  }
  c->flags = flags;
  if (const char* e = getenv("SPMF_DENSE_E_ONCE")) c->e_once = e[0] != '0';
  if (const char* e = getenv("SPMF_DENSE_BF16X3")) c->dense3 = e[0] != '0';
  *out = c;
  return SPMF_OK;
}

void spmf_ctx_destroy(spmf_ctx* c) {
  if (!c) return;
  for (auto& set : c->evs)
    for (auto& e : set)
      if (e) (void)hipEventDestroy(e);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->side) (void)hipStreamDestroy(c->side);
  if (c->scratch) (void)hipFree(c->scratch);
  if (c->comm) comm_release(c);
  p2p_release(c);
  delete c;
}

const char* spmf_last_error(const spmf_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int spmf_ctx_set_prior(spmf_ctx* c, double u_tau_scale, double s_tau_scale, double decay) {
  if (!c || !(u_tau_scale > 0) || !(s_tau_scale > 0) || !(decay > 0)) return fail(c, SPMF_E_ARG,
      "set_prior: scales must be > 0");
  c->u_tau_scale = u_tau_scale;
  c->s_tau_scale = s_tau_scale;
  c->decay = decay;
  return SPMF_OK;
}

int spmf_padded_k(const spmf_ctx* c) { return c ? c->KP : 0; }

int spmf_ctx_set_column_types(spmf_ctx* c, const uint8_t* column_is_bernoulli) {
  if (!c || !(c->flags & SPMF_FLAG_MIXED) || !column_is_bernoulli) return fail(c, SPMF_E_ARG,
      "set_column_types: needs a ctx created with SPMF_FLAG_MIXED and a [D] device array");
  c->ctype = column_is_bernoulli;
  return SPMF_OK;
}

int spmf_ctx_set_bernoulli_columns(spmf_ctx* c, const int32_t* cols, int n) {
  if (!c || !(c->flags & SPMF_FLAG_MIXED) || n < 0 || n > c->D || (n > 0 && !cols)) return fail(c, SPMF_E_ARG,
      "set_bernoulli_columns: needs a SPMF_FLAG_MIXED ctx and n indices in [0, D)");
  c->bcols = n > 0 ? cols : nullptr;
  c->n_bcols = n;
  return SPMF_OK;
}

// Forget the buffers bound in the previous workspace: until the next data pass binds the new one the
// entry points that only READ a bound workspace (spmf_prior_async, spmf_finish,
// spmf_nonfinite_patch, spmf_acc_ptr) fail with SPMF_E_WORKSPACE / return NULL instead of
// touching memory the caller may have freed.
static void unbind_ws(spmf_ctx* c) {
  // a prior half still running on the side stream writes per-workgroup partials into the OLD
  // workspace and the caller's gradients: let it finish before the caller may free / reuse that
  // memory (torch's caching allocator does not synchronise on free)
  if (c->prior_pending && c->ev_join) (void)hipEventSynchronize(c->ev_join);
  c->ws_rows = -1;
  c->ws_S = 0;
  c->acc = nullptr;
  c->dacc = nullptr;
  c->dprep = nullptr;
  c->fpart = nullptr;
  c->futau = nullptr;
  c->prior_pending = 0;
  c->step.active = 0;
}

int spmf_ctx_set_e_cap(spmf_ctx* c, size_t bytes) {
  if (!c || bytes < ((size_t)1 << 20)) return fail(c, SPMF_E_ARG, "set_e_cap: at least 1 MiB");
  c->est_cap_bytes = bytes;
  unbind_ws(c);               // the layout changes: the next data pass re-binds (and re-checks) the workspace
  return SPMF_OK;
}

int spmf_ctx_set_workspace(spmf_ctx* c, void* workspace, size_t bytes) {
  if (!c) return SPMF_E_ARG;
  if (!workspace || ((uintptr_t)workspace & 255)) return fail(c, SPMF_E_ARG,
      "workspace must be 256-byte aligned and non-null");
  c->ws = (char*)workspace;
  c->ws_bytes = bytes;
  unbind_ws(c);
  return SPMF_OK;
}

float* spmf_acc_ptr(const spmf_ctx* c) { return c ? c->acc : nullptr; }
int64_t spmf_acc_len(const spmf_ctx* c, int S) { return c ? (int64_t)S * acc_len(c->D, c->KP) : 0; }
const float* spmf_z_ptr(const spmf_ctx* c) {
  return c ? c->z + (c->batched ? (size_t)(c->ws_S - 1) * c->ws_rows * c->KP : 0) : nullptr;
}
const float* spmf_gz_ptr(const spmf_ctx* c) {
  return c ? c->gzs + (c->batched ? (size_t)(c->ws_S - 1) * c->ws_rows * c->KP : 0) : nullptr;
}

int spmf_ctx_enable_timing(spmf_ctx* c, int on) {
  if (!c) return SPMF_E_ARG;
  if (on && !c->evs[0][0])
    for (auto& set : c->evs)
      for (auto& e : set) HIPCHK(c, hipEventCreate(&e));
  c->timing = on;
  c->ev_valid = 0;
  c->ev_set = -1;
  c->ev_count = 0;
  return SPMF_OK;
}

int spmf_last_timing(spmf_ctx* c, float* ms5) {
  if (!c || !ms5) return SPMF_E_ARG;
  const bool logt = (c->flags & (SPMF_FLAG_LOG_TRANSFORM | SPMF_FLAG_BERNOULLI | SPMF_FLAG_MIXED)) != 0;
  if (!c->timing || c->ev_count < 1) return fail(c, SPMF_E_ARG,
      "no timing recorded (enable timing, run data_pass + finish)");
  // average over the (up to kSets) most recent complete steps
  const int n = c->ev_count < spmf_ctx::kSets ? c->ev_count : spmf_ctx::kSets;
  double acc[4] = {0, 0, 0, 0};
  for (int k = 0; k < n; ++k) {
    hipEvent_t* e = c->evs[((c->ev_set - k) % spmf_ctx::kSets + spmf_ctx::kSets) % spmf_ctx::kSets];
    HIPCHK(c, hipEventSynchronize(e[5]));
    float t;
    for (int i = 0; i < 3; ++i) {
      HIPCHK(c, hipEventElapsedTime(&t, e[i], e[i + 1]));
      acc[i] += t;
    }
    HIPCHK(c, hipEventElapsedTime(&t, e[4], e[5]));
    acc[3] += t;
  }
  for (int i = 0; i < 4; ++i) ms5[i] = (float)(acc[i] / n);
  ms5[4] = ms5[0] + ms5[1] + ms5[2] + ms5[3];
  ms5[5] = 0.f;
  if (logt) {   // the two dense launches sit inside the row interval: report them apart
    double d = 0;
    for (int k = 0; k < n; ++k) {
      hipEvent_t* e = c->evs[((c->ev_set - k) % spmf_ctx::kSets + spmf_ctx::kSets) % spmf_ctx::kSets];
      float t;
      HIPCHK(c, hipEventElapsedTime(&t, e[6], e[7]));
      d += t;
    }
    ms5[5] = (float)(d / n);
    ms5[1] -= ms5[5];
  }
  return SPMF_OK;
}

int spmf_counts_stats(spmf_ctx* c, int64_t n_rows, const int32_t* row_ptr, const int32_t* col_idx, const float* val,
    double* colsum, double* colnnz, float* row_sum, double* row_lgamma, void* stream) {
  if (!c || !row_ptr || n_rows < 0) return fail(c, SPMF_E_ARG, "counts_stats: bad arguments");
  if (n_rows == 0) return SPMF_OK;
  StatsArgs a{n_rows, row_ptr, col_idx, val, colsum, colnnz, row_sum, row_lgamma};
  launch_stats(a, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_counts_colstats(spmf_ctx* c, const spmf_counts* ct, double* colsum, double* colnnz, void* stream) {
  if (!c || !ct) return fail(c, SPMF_E_ARG, "counts_colstats: bad arguments");
  int rc = check_counts(c, ct);
  if (rc) return rc;
  if (ct->nnz == 0 || ct->n_rows == 0 || (!colsum && !colnnz)) return SPMF_OK;
  if (!ct->pc_ptr || !ct->pc_val || ct->n_panels < 1)
    return fail(c, SPMF_E_ARG, "counts_colstats: panel-CSC arrays missing");
  launch_colstats(ct->n_panels, ct->n_cols, ct->pc_ptr, ct->pc_val, colsum, colnnz, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_counts_gvals(spmf_ctx* c, const spmf_counts* ct, const float* eta, float* gval, float* pc_gval,
    void* stream) {
  if (!c || !ct || !eta) return fail(c, SPMF_E_ARG, "counts_gvals: bad arguments");
  int rc = check_counts(c, ct);
  if (rc) return rc;
  if (ct->nnz == 0 || ct->n_rows == 0) return SPMF_OK;
  if (pc_gval && (!ct->pc_ptr || !ct->pc_val || ct->n_panels < 1))
    return fail(c, SPMF_E_ARG, "counts_gvals: panel-CSC arrays missing");
  launch_gvals(ct->nnz, ct->n_panels, ct->n_cols, ct->row_ptr, ct->col_idx, ct->val, ct->pc_ptr, ct->pc_val, eta,
               gval, pc_gval, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

size_t spmf_det_scratch_bytes(const spmf_ctx* c, int64_t n_items, int S) {
  if (!c || S < 1) return 0;
  return (size_t)S * det_layout(nullptr, 0, c->KP, n_items).bytes;
}
int spmf_ctx_set_deterministic(spmf_ctx* c, void* scratch, size_t bytes) {
  if (!c) return SPMF_E_ARG;
  if (!scratch) {
    c->det_buf = nullptr;
    c->det_bytes = 0;
    return SPMF_OK;
  }
  if (likelihood_code(c) != 0) return fail(c, SPMF_E_UNSUPPORTED,
      "set_deterministic: Poisson likelihood with the linear decoder only (the dense sums of the other contexts "
      "accumulate with float atomics)");
  if (c->Dh > 0) return fail(c, SPMF_E_UNSUPPORTED, "set_deterministic: not together with the column split");
  if (c->KP > 64) return fail(c, SPMF_E_UNSUPPORTED, "set_deterministic: latent dimensions up to 64 only");
  if ((uintptr_t)scratch & 255) return fail(c, SPMF_E_ARG, "set_deterministic: scratch must be 256-byte aligned");
  if (bytes < det_layout(nullptr, 0, c->KP, 0).bytes) return fail(c, SPMF_E_WORKSPACE, "set_deterministic: scratch too small");
  c->det_buf = (char*)scratch;
  c->det_bytes = bytes;
  return SPMF_OK;
}

}  // extern "C"
