// api.hip -- the C-ABI of libspmf_hip.so (see include/spmf_hip.h).
// Host-side orchestration only: argument checks, workspace carving, stream
// ordered launches.  No device allocation, no host<->device copies, no
// synchronisation on the hot path (timing taps excepted, off by default).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../include/spmf_hip.h"
#include "arena.h"
#include "common.h"
#include "kernels.h"

using namespace spmf;

// What a data pass binds inside the caller's workspace (ws_layout), in the order of the memory
struct WsBuffers {
  float* acc = nullptr;
  double* dacc = nullptr;
  double* dprep = nullptr;
  double* fpart = nullptr;   // finish kernel: per-block prior-part sums
  float* futau = nullptr;    //                per-block u_tau gradient sums
  float *Ap = nullptr, *Vp = nullptr, *phi = nullptr, *dbias = nullptr;
  float *Vb = nullptr, *bb = nullptr;   // mixed likelihood only: compacted V' rows / logit biases of the Bernoulli columns
  float *z = nullptr, *gzs = nullptr;
  float* gzd = nullptr;      // contexts with a dense term only
  // log_transform: E = exp(<z_b, W_d>) is computed once and kept for the second contraction
  // (dense.hip, estdot_kernel), in row chunks of at most est_cap_bytes; kDenseEKept only
  float* est = nullptr;
  int64_t est_rows = 0;      // rows per chunk of E
  int batched = 0;           // the tables and row outputs exist per draw (S draws per launch)
};

struct spmf_ctx : WsBuffers {
  int device = 0, K = 0, D = 0, KP = 0;
  unsigned flags = 0;
  double u_tau_scale = 0.01, s_tau_scale = 1.0, decay = 0.99;  // poisson.py:59
  // the workspace and the batch it is bound for
  char* ws = nullptr;
  size_t ws_bytes = 0;
  int64_t ws_rows = 0;
  int ws_S = 0;
  // deterministic mode (spmf_ctx_set_deterministic): caller-owned scratch for the row pass's per-workgroup
  // scalar slots and the column pass's per-item partial sums; null = off
  char* det_buf = nullptr;
  size_t det_bytes = 0;
  const uint8_t* ctype = nullptr;   // mixed likelihood: 1 = Bernoulli column (device, caller-owned)
  const int32_t* bcols = nullptr;   // mixed likelihood: ascending indices of the Bernoulli columns (optional)
  int n_bcols = 0;
  // timing taps
  int timing = 0;
  static constexpr int kSets = 64;  // ring of event sets: no sync inside a timed loop
  hipEvent_t evs[kSets][8] = {};   // 0..3 data pass, 4..5 finish, 6..7 dense exp kernels
  hipEvent_t* ev = evs[0];
  int ev_set = -1;      // set used by the call in flight
  int ev_count = 0;     // complete sets recorded since enable
  int ev_valid = 0;
  // prior half of the finish on a side stream (spmf_prior_async)
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int Dh = 0;                     // column split of the accumulator layout (0 = none)
  int prior_pending = 0;          // S of the launched prior half, 0 = none
  const double* prior_parts = nullptr;
  // the library's only device allocation: a small scratch for per-block partial sums of the
  // O(D*K) surrogate kernels (fixed-order reductions instead of same-address atomics)
  int e_once = 1;                 // SPMF_DENSE_E_ONCE=0: recompute E in a second launch instead
  int dense3 = 1;                 // exp sums on the bf16 matrix cores with three-way split operands
                                  // (dense3.hip; Poisson log_transform at KP = 64 only);
                                  // SPMF_DENSE_BF16X3=0 selects the exact-f32 MFMA kernels (dense.hip)
  size_t est_cap_bytes = (size_t)8 << 30;   // spmf_ctx_set_e_cap
  double* scratch = nullptr;
  static constexpr size_t kScratchDoubles = 1u << 20;   // 8 MiB
  void* comm = nullptr;           // ncclComm_t of the row-shard collective (spmf_comm_init)
  hipEvent_t rows_event = nullptr; // caller's event recorded behind the row stage of a data pass (spmf_ctx_set_rows_event)
  // spmf_step_begin .. spmf_step_end (ABI 6): the step's outputs are known from its first call on, so the
  // prior half of the finish rides in the prep launch (fused = 1) and spmf_step_end launches the data half only
  struct StepOut {
    int active = 0, fused = 0, S = 0;
    double prior_weight = 1.0;
    const float* params[SPMF_NVARS] = {};
    float* grads[SPMF_NVARS] = {};
    const float* eta = nullptr;
    double* parts = nullptr;
    double* nnf = nullptr;
  } step;
  int comm_rank = 0, comm_world = 1;
  // the hand-written collective over peer pointers (spmf_p2p_*; p2p.hip): this rank's fine-grained region
  // and the peers' regions as mapped into this process
  struct P2P {
    char* region = nullptr;          // own allocation: [rs | ag | flags | seq]
    size_t bytes = 0, alloc_bytes = 0, off_ag = 0, off_flags = 0, off_seq = 0;
    int64_t n_max = 0, slice_cap = 0;
    int rank = 0, world = 0, nchunk = 0, connected = 0;
    char* peer[kP2PMaxWorld] = {};   // peer regions (own rank: own region); opened with hipIpcOpenMemHandle
  } p2p;
  std::string err;
};

// ---- RCCL, bound at run time ------------------------------------------------
// The library does not link librccl: single-GPU users never need it.  spmf_comm_*
// dlopen it on first use; the few entry points used are declared here with the
// ABI of <rccl/rccl.h> (ncclUniqueId = 128 opaque bytes, passed by value).
namespace {
struct RcclId { char internal[128]; };
typedef int (*fn_get_id)(RcclId*);
typedef int (*fn_init_rank)(void**, int, RcclId, int);
typedef int (*fn_allreduce)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*fn_destroy)(void*);
typedef const char* (*fn_errstr)(int);
struct Rccl {
  void* h = nullptr;
  fn_get_id get_id = nullptr;
  fn_init_rank init_rank = nullptr;
  fn_allreduce allreduce = nullptr;
  fn_destroy destroy = nullptr;
  fn_errstr errstr = nullptr;
};
Rccl* rccl() {
  static Rccl r;
  static bool tried = false;
  if (!tried) {
    tried = true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      r.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (r.h) break;
    }
    if (r.h) {
      r.get_id = (fn_get_id)dlsym(r.h, "ncclGetUniqueId");
      r.init_rank = (fn_init_rank)dlsym(r.h, "ncclCommInitRank");
      r.allreduce = (fn_allreduce)dlsym(r.h, "ncclAllReduce");
      r.destroy = (fn_destroy)dlsym(r.h, "ncclCommDestroy");
      r.errstr = (fn_errstr)dlsym(r.h, "ncclGetErrorString");
      if (!r.get_id || !r.init_rank || !r.allreduce || !r.destroy) r.h = nullptr;
    }
  }
  return r.h ? &r : nullptr;
}
constexpr int kNcclFloat = 7, kNcclSum = 0;   // ncclFloat32, ncclSum (rccl.h enums)
}  // namespace

static int fail(spmf_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}
#define HIPCHK(c, call)                                                            \
  do {                                                                             \
    hipError_t e_ = (call);                                                        \
    if (e_ != hipSuccess)                                                          \
      return fail((c), SPMF_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

static int padded_k(int K) {
  int kp = 4;
  while (kp < K) kp <<= 1;
  return kp;
}
static size_t var_size(const spmf_ctx* c, int i) {
  const size_t D = c->D, K = c->K;
  switch (i) {
    case 0: case 2: case 3: case 8: return D * K;
    case 4: case 9: return K;
    case 1: case 6: case 11: return D;
    default: return 2 * D;  // 5 s_eta, 7 s, 10 s_eta_a
  }
}

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

static int fail(spmf_ctx* c, int code, const std::string& msg);
// a bf16x3 dense launcher answered "shape not covered": the dense term of the step would be missing from
// gzs / gV' / the softplus sum -- fail instead (dense_form below is meant to make this unreachable)
static int dense3_uncovered(spmf_ctx* c) {
  return fail(c, SPMF_E_UNSUPPORTED, "data_pass: the bf16x3 dense kernels do not cover this launch shape "
      "(set SPMF_DENSE_BF16X3=0 for the exact-f32 kernels)");
}

static int likelihood_code(const spmf_ctx* c) {   // common.h: lik_exp / lik_bern
  const bool lt = (c->flags & SPMF_FLAG_LOG_TRANSFORM) != 0;
  if (c->flags & SPMF_FLAG_BERNOULLI) return lt ? 4 : 2;
  if (c->flags & SPMF_FLAG_MIXED) return 3;
  return lt ? 1 : 0;
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

extern "C" {

int spmf_version(void) { return SPMF_ABI_VERSION; }
size_t spmf_sizeof_counts(void) { return sizeof(spmf_counts); }
size_t spmf_sizeof_sur_var(void) { return sizeof(spmf_sur_var); }
size_t spmf_sizeof_adam_var(void) { return sizeof(spmf_adam_var); }

static void p2p_release(spmf_ctx* c);

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
  if (c->comm) {
    Rccl* r = rccl();
    if (r) (void)r->destroy(c->comm);
  }
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

int spmf_ctx_set_workspace(spmf_ctx* c, void* workspace, size_t bytes) {
  if (!c) return SPMF_E_ARG;
  if (!workspace || ((uintptr_t)workspace & 255)) return fail(c, SPMF_E_ARG,
      "workspace must be 256-byte aligned and non-null");
  c->ws = (char*)workspace;
  c->ws_bytes = bytes;
  unbind_ws(c);
  return SPMF_OK;
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

static int check_counts(spmf_ctx* c, const spmf_counts* ct) {
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

// deterministic-mode scratch: per draw the row pass's slots, then the column pass's per-item partial sums.
// Draw 0's two buffers inside the `bytes` of `buf` (null: sizes only); draw s lies s * dstride doubles = s * fstride
// floats behind (the data pass checks all S draws against spmf_det_scratch_bytes first).
struct DetDraw {
  double* slots;                // [kDetMeta + kDetMaxBlocks * (kDaccHead + KP)]
  float* part;                  // [n_items][det_part_len]
  int64_t dstride, fstride;
  size_t bytes;                 // of one draw
};
static DetDraw det_layout(void* buf, size_t bytes, int KP, int64_t n_items) {
  Arena a(buf, bytes);
  DetDraw d;
  d.slots = a.take<double>((size_t)kDetMeta + (size_t)kDetMaxBlocks * (kDaccHead + KP));
  d.part = a.take<float>((size_t)(n_items > 0 ? n_items : 0) * det_part_len(KP));
  d.bytes = a.used;
  d.dstride = (int64_t)(a.used / sizeof(double));
  d.fstride = (int64_t)(a.used / sizeof(float));
  return d;
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

// ---- the launches' argument blocks, each built in one place and by name ----------------------
// The per-draw tables and row outputs a launch sequence works on: those of the bound workspace (draw 0), or
// those of the draw stage inside a streaming call's scratch (draw_stage)
struct Tables {
  float *Ap, *Vp, *phi;
  double *dprep, *dacc;
  float *z, *gzs;
};
static Tables ws_tables(const spmf_ctx* c) { return Tables{c->Ap, c->Vp, c->phi, c->dprep, c->dacc, c->z, c->gzs}; }

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

// The checks, the prep launch and the encode sweep: z of every row under each of S draws into T->z.
// T == nullptr (spmf_encode, spmf_dense_ll): the tables of the workspace, bound here (one draw); otherwise
// those of the draw stage.
// Nothing is launched for an empty batch.
static int encode_rows(spmf_ctx* c, const char* fn, const spmf_counts* ct, int S, const Tables* T, const float* u,
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

// ---- the draw stage of the streaming calls ---------------------------------------------------
// spmf_waic_accumulate, spmf_topk_rows, spmf_score_cells, spmf_rank_cells, spmf_predict_columns,
// spmf_group_sums, spmf_set_scores and spmf_embed_rows are one stage and a consumer each (spmf_knn, at the end of the section,
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

int spmf_waic_accumulate(spmf_ctx* c, const spmf_counts* ct, int S, const float* const params[SPMF_NVARS],
    const float* eta, double* sums6, double* row_out, void* scratch, size_t scratch_bytes, void* stream) {
  Tables T;
  int rc = draw_only_check(c, "waic_accumulate", ct, S, 2, params, eta, scratch, scratch_bytes, T);
  if (rc) return rc;
  if (!sums6) return fail(c, SPMF_E_ARG, "waic_accumulate: null argument");
  if ((int64_t)(c->D + 63) / 64 > 65535) return fail(c, SPMF_E_UNSUPPORTED, "waic_accumulate: D above 65535 * 64");
  hipStream_t st = (hipStream_t)stream;
  DrawTables dt;
  rc = draw_stage(c, "waic_accumulate", ct, S, params, eta, T, st, dt);
  if (rc || ct->n_rows == 0) return rc;
  WaicArgs wa{dt, ct->nnz, ct->row_ptr, ct->col_idx, ct->val, sums6, row_out};
  return launched(c, launch_waic(wa, st), "waic_accumulate: no kernel for this K / likelihood");
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
static void knn_layout(Arena& a, const spmf_ctx* c, int64_t n_query, int64_t n_ref, int row_len, KnnArgs& ka) {
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
  const size_t part = ka.slices > 1 ? (size_t)ka.slices * nq * kTopkMaxK : 0;
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

int spmf_nonfinite_reduce(spmf_ctx* c, int64_t n, const float* ll, int pass, double* io, void* stream) {
  if (!c || !ll || !io || n < 0 || (pass != 0 && pass != 1)) return fail(c, SPMF_E_ARG,
      "nonfinite_reduce: bad arguments");
  if (n == 0) return SPMF_OK;
  launch_nonfinite(n, ll, pass, io, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

// ---- row-shard collective inside the library (spmf_allreduce) ---------
// (1) hand-written, over peer pointers: p2p.hip.  Region layout of a rank:
//     rs[2][kP2PMaxWorld][slice_cap] | ag[2][kP2PMaxWorld][slice_cap] | flags[2][2][kP2PMaxWorld][kP2PMaxChunks] | seq[8]
static void p2p_unmap(spmf_ctx* c) {
  spmf_ctx::P2P& p = c->p2p;
  for (int i = 0; i < p.world; ++i) {
    if (p.peer[i] && p.peer[i] != p.region) (void)hipIpcCloseMemHandle(p.peer[i]);
    p.peer[i] = nullptr;
  }
  p.connected = 0;
}
static void p2p_release(spmf_ctx* c) {
  spmf_ctx::P2P& p = c->p2p;
  p2p_unmap(c);
  if (p.region) (void)hipFree(p.region);
  p = spmf_ctx::P2P();
}

static int p2p_allreduce(spmf_ctx* c, float* buf, int64_t n, hipStream_t st) {
  spmf_ctx::P2P& p = c->p2p;
  if (n > p.n_max) {
    char b[160];
    snprintf(b, sizeof b, "allreduce: %lld floats, the peer regions were sized for %lld (spmf_p2p_init n_max)",
        (long long)n, (long long)p.n_max);
    return fail(c, SPMF_E_WORKSPACE, b);
  }
  if (((uintptr_t)buf & 15) != 0) return fail(c, SPMF_E_ARG, "allreduce: buffer must be 16-byte aligned");
  if (n == 0 || p.world == 1) return SPMF_OK;
  P2PLaunch L{};
  L.buf = buf;
  L.n = n;
  L.rank = p.rank;
  L.world = p.world;
  L.nchunk = p.nchunk;
  L.slice_cap = p.slice_cap;
  L.rs = (float*)p.region;
  L.ag = (float*)(p.region + p.off_ag);
  L.flags = (uint64_t*)(p.region + p.off_flags);
  L.seq = (uint64_t*)(p.region + p.off_seq);
  for (int i = 0; i < p.world; ++i) {
    L.peer_rs[i] = (float*)p.peer[i];
    L.peer_ag[i] = (float*)(p.peer[i] + p.off_ag);
    L.peer_flags[i] = (uint64_t*)(p.peer[i] + p.off_flags);
  }
  launch_p2p_allreduce(L, st);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_p2p_init(spmf_ctx* c, int rank, int world, int64_t n_max, int nchunk, void* handle_out64) {
  if (!c || !handle_out64 || world < 1 || world > kP2PMaxWorld || rank < 0 || rank >= world || n_max < 1)
    return fail(c, SPMF_E_ARG, "p2p_init: bad arguments (world <= 16)");
  if (nchunk <= 0) nchunk = 32;
  if (nchunk > kP2PMaxChunks) nchunk = kP2PMaxChunks;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  spmf_ctx::P2P& p = c->p2p;
  const int64_t per = ((n_max + world - 1) / world + 3) & ~(int64_t)3;
  const int64_t slice_cap = (per + 63) & ~(int64_t)63;           // 256-byte slots
  const size_t box = (size_t)2 * kP2PMaxWorld * slice_cap * sizeof(float);
  const size_t off_flags = 2 * box;
  const size_t off_seq = off_flags + (size_t)2 * 2 * kP2PMaxWorld * kP2PMaxChunks * sizeof(uint64_t);
  const size_t bytes = off_seq + 64;
  // A context's region is allocated ONCE and re-used while it is large enough: freeing a region and exporting a
  // new allocation inside one process is what the runtime's IPC bookkeeping did not survive (round 5, world 4:
  // "hipIpcGetMemHandle: invalid argument", or peers that mapped something stale and never saw a flag).
  p2p_unmap(c);
  char* keep = (p.region && p.alloc_bytes >= bytes) ? p.region : nullptr;
  const size_t keep_bytes = keep ? p.alloc_bytes : 0;
  if (p.region && !keep) (void)hipFree(p.region);
  p = spmf_ctx::P2P();
  p.rank = rank;
  p.world = world;
  p.nchunk = nchunk;
  p.n_max = n_max;
  p.slice_cap = slice_cap;
  p.off_ag = box;
  p.off_flags = off_flags;
  p.off_seq = off_seq;
  p.bytes = bytes;
  hipError_t e = hipSuccess;
  if (keep) {
    p.region = keep;
    p.alloc_bytes = keep_bytes;
  } else {
    // fine-grained: coherent across agents INSIDE a kernel (a coarse-grained allocation is only
    // coherent at kernel boundaries); what RCCL allocates for its own buffers
    void* reg = nullptr;
    e = hipExtMallocWithFlags(&reg, p.bytes, hipDeviceMallocFinegrained);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, SPMF_E_HIP, std::string("p2p_init: hipExtMallocWithFlags(fine-grained): ") + hipGetErrorString(e));
    }
    p.region = (char*)reg;
    p.alloc_bytes = p.bytes;
  }
  HIPCHK(c, hipMemset(p.region + p.off_flags, 0, p.bytes - p.off_flags));
  HIPCHK(c, hipDeviceSynchronize());
  hipIpcMemHandle_t hnd;
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "spmf_p2p_init hands out 64-byte handles");
  e = hipIpcGetMemHandle(&hnd, p.region);
  if (e != hipSuccess) {
    // seen once (round 5, world 4, a region re-created in a process whose earlier region a peer had still mapped
    // when it was freed): the runtime refused to export the new allocation.  One more try at another address.
    (void)hipGetLastError();
    void* again = nullptr;
    if (hipExtMallocWithFlags(&again, p.bytes, hipDeviceMallocFinegrained) == hipSuccess) {
      (void)hipFree(p.region);
      p.region = (char*)again;
      p.alloc_bytes = p.bytes;
      (void)hipMemset(p.region + p.off_flags, 0, p.bytes - p.off_flags);
      (void)hipDeviceSynchronize();
      e = hipIpcGetMemHandle(&hnd, p.region);
    }
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    p2p_release(c);
    return fail(c, SPMF_E_HIP, std::string("p2p_init: hipIpcGetMemHandle: ") + hipGetErrorString(e));
  }
  memcpy(handle_out64, &hnd, 64);
  return SPMF_OK;
}

int spmf_p2p_connect(spmf_ctx* c, const void* handles) {
  if (!c || !handles) return fail(c, SPMF_E_ARG, "p2p_connect: bad arguments");
  spmf_ctx::P2P& p = c->p2p;
  if (!p.region) return fail(c, SPMF_E_ARG, "p2p_connect: spmf_p2p_init was not called");
  HIPCHK(c, hipSetDevice(c->device));
  for (int i = 0; i < p.world; ++i) {
    if (i == p.rank) {
      p.peer[i] = p.region;
      continue;
    }
    hipIpcMemHandle_t hnd;
    memcpy(&hnd, (const char*)handles + (size_t)i * 64, 64);
    void* ptr = nullptr;
    const hipError_t e = hipIpcOpenMemHandle(&ptr, hnd, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      char b[200];
      snprintf(b, sizeof b, "p2p_connect: hipIpcOpenMemHandle(rank %d): %s", i, hipGetErrorString(e));
      return fail(c, SPMF_E_HIP, b);
    }
    p.peer[i] = (char*)ptr;
    // a region that lives on ANOTHER device of this process's view (ranks = GPUs of one node): kernels here will
    // store into it, so the link must be there -- an inaccessible peer is refused now (the caller falls back to
    // RCCL: dist.PeerComm agrees on the failure over all ranks) instead of faulting in the first launch.
    // Same device (ranks = processes on one GPU: the one-GPU tests) or attributes unavailable: nothing to check.
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptr) == hipSuccess) {
      if (at.device >= 0 && at.device != c->device) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, c->device, at.device) == hipSuccess && !can) {
          char b[200];
          snprintf(b, sizeof b, "p2p_connect: device %d has no peer access to device %d (rank %d)", c->device,
                   at.device, i);
          return fail(c, SPMF_E_UNSUPPORTED, b);
        }
      }
    } else {
      (void)hipGetLastError();
    }
  }
  p.connected = 1;
  return SPMF_OK;
}

int spmf_p2p_enable(spmf_ctx* c, int on) {
  if (!c) return SPMF_E_ARG;
  if (on && (!c->p2p.region || !c->p2p.peer[c->p2p.world > 0 ? c->p2p.world - 1 : 0]))
    return fail(c, SPMF_E_ARG, "p2p_enable: spmf_p2p_connect has not connected the peers");
  c->p2p.connected = on ? 1 : 0;
  return SPMF_OK;
}

int spmf_p2p_status(spmf_ctx* c, uint64_t out3[3]) {
  if (!c || !out3) return SPMF_E_ARG;
  if (!c->p2p.region) return fail(c, SPMF_E_ARG, "p2p_status: spmf_p2p_init was not called");
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(out3, c->p2p.region + c->p2p.off_seq, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return SPMF_OK;
}

int spmf_p2p_disconnect(spmf_ctx* c) {
  if (!c) return SPMF_E_ARG;
  (void)hipDeviceSynchronize();
  p2p_unmap(c);
  return SPMF_OK;
}

int spmf_p2p_destroy(spmf_ctx* c) {
  if (!c) return SPMF_E_ARG;
  (void)hipDeviceSynchronize();
  p2p_release(c);
  return SPMF_OK;
}

// (2) RCCL, bound at run time
int spmf_comm_unique_id(void* out128) {
  if (!out128) return SPMF_E_ARG;
  Rccl* r = rccl();
  if (!r) return SPMF_E_UNSUPPORTED;
  RcclId id;
  const int rc = r->get_id(&id);
  if (rc != 0) return SPMF_E_HIP;
  memcpy(out128, &id, sizeof id);
  return SPMF_OK;
}

int spmf_comm_init(spmf_ctx* c, const void* id128, int rank, int world) {
  if (!c || !id128 || world < 1 || rank < 0 || rank >= world) return fail(c, SPMF_E_ARG, "comm_init: bad arguments");
  Rccl* r = rccl();
  if (!r) return fail(c, SPMF_E_UNSUPPORTED, "comm_init: librccl.so.1 could not be loaded");
  if (c->comm) {
    (void)r->destroy(c->comm);
    c->comm = nullptr;
  }
  HIPCHK(c, hipSetDevice(c->device));
  RcclId id;
  memcpy(&id, id128, sizeof id);
  void* comm = nullptr;
  const int rc = r->init_rank(&comm, world, id, rank);
  if (rc != 0) return fail(c, SPMF_E_HIP, std::string("ncclCommInitRank: ") + (r->errstr ? r->errstr(rc) : "?"));
  c->comm = comm;
  c->comm_rank = rank;
  c->comm_world = world;
  return SPMF_OK;
}

int spmf_allreduce(spmf_ctx* c, float* buf, int64_t n, void* stream) {
  if (!c || !buf || n < 0) return fail(c, SPMF_E_ARG, "allreduce: bad arguments");
  if (c->p2p.connected) return p2p_allreduce(c, buf, n, (hipStream_t)stream);
  if (!c->comm) return fail(c, SPMF_E_ARG, "allreduce: neither spmf_comm_init nor spmf_p2p_connect was called");
  if (n == 0) return SPMF_OK;
  Rccl* r = rccl();
  const int rc = r->allreduce(buf, buf, (size_t)n, kNcclFloat, kNcclSum, c->comm, (hipStream_t)stream);
  if (rc != 0) return fail(c, SPMF_E_HIP, std::string("ncclAllReduce: ") + (r->errstr ? r->errstr(rc) : "?"));
  return SPMF_OK;
}

int spmf_comm_destroy(spmf_ctx* c) {
  if (!c) return SPMF_E_ARG;
  if (c->comm) {
    Rccl* r = rccl();
    if (r) (void)r->destroy(c->comm);
    c->comm = nullptr;
    c->comm_world = 1;
    c->comm_rank = 0;
  }
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

// the library's one device allocation, at its first use (never inside a stream capture: a step is run eagerly
// before it is captured); zero-filled: its last word is the arrival ticket of sample_fwd_kernel.  Without it the
// surrogate kernels fall back (atomics / two launches).
static void ensure_scratch(spmf_ctx* c, hipStream_t st) {
  if (c->scratch) return;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cap);
  if (cap != hipStreamCaptureStatusNone) return;
  if (hipMalloc((void**)&c->scratch, spmf_ctx::kScratchDoubles * sizeof(double)) != hipSuccess ||
      hipMemset(c->scratch, 0, spmf_ctx::kScratchDoubles * sizeof(double)) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {
    if (c->scratch) (void)hipFree(c->scratch);
    c->scratch = nullptr;
    (void)hipGetLastError();
  }
}

// The buffers of a spmf_sur_var an entry point needs besides t0 and noise (sur_table)
enum : unsigned {
  kSurT1 = 1,      // t1
  kSurTheta = 2,   // theta
  kSurGrad = 4,    // gtheta
  kSurG01 = 8,     // g0, g1
  kSurDgda = 16,   // dgda of the kind-2 variables
  kSurSkip = 32,   // n = 0 skips the variable (its slot keeps its index: the RNG counter, the logq slots)
};
// vars[0, nvars) into T, max_n = the largest n; a variable without a buffer in `need` fails as
// "<fn>: bad variable<detail>"
static int sur_table(spmf_ctx* c, const char* fn, const char* detail, const spmf_sur_var* vars, int nvars,
    unsigned need, SurTable& T, int& max_n) {
  max_n = 0;
  for (int i = 0; i < nvars; ++i) {
    const spmf_sur_var& v = vars[i];
    if (v.n == 0 && (need & kSurSkip)) {
      T.v[i] = SurVar{};
      continue;
    }
    if (!v.t0 || !v.noise || v.n < 1 || v.kind < 0 || v.kind > 2 || ((need & kSurT1) && !v.t1) ||
        ((need & kSurTheta) && !v.theta) || ((need & kSurGrad) && !v.gtheta) ||
        ((need & kSurG01) && (!v.g0 || !v.g1)) || ((need & kSurDgda) && v.kind == 2 && !v.dgda))
      return fail(c, SPMF_E_ARG, std::string(fn) + ": bad variable" + detail);
    if (v.noise_ld != 0 && v.noise_ld < v.n) return fail(c, SPMF_E_ARG, "surrogate: noise_ld < n");
    T.v[i] = SurVar{v.t0, v.t1, v.noise, v.dgda, v.theta, v.gtheta, v.g0, v.g1, v.n, v.kind, v.ident,
        v.noise_ld ? v.noise_ld : (int64_t)v.n};
    if (v.n > max_n) max_n = v.n;
  }
  if ((need & kSurSkip) && max_n < 1)
    return fail(c, SPMF_E_ARG, std::string(fn) + ": every variable is skipped (n = 0)");
  return SPMF_OK;
}

// tensors[0, n) into T, max_n = the largest n
static int adam_table(spmf_ctx* c, const char* fn, const spmf_adam_var* tensors, int n, AdamTable& T, int& max_n) {
  max_n = 0;
  for (int i = 0; i < n; ++i) {
    const spmf_adam_var& a = tensors[i];
    if (!a.p || !a.m || !a.v || !a.g || a.n < 1) return fail(c, SPMF_E_ARG, std::string(fn) + ": bad tensor");
    T.v[i] = AdamVar{a.p, a.m, a.v, a.g, a.n};
    if (a.n > max_n) max_n = a.n;
  }
  return SPMF_OK;
}

int spmf_sample_transform(spmf_ctx* c, const spmf_sur_var* vars, int nvars, int S, uint64_t seed, uint64_t counter,
    const double* state, double* logq, void* stream) {
  if (!c || !vars || nvars < 1 || nvars > 12 || S < 1 || S > 65535 || !logq) return fail(c, SPMF_E_ARG,
      "sample_transform: bad arguments");
  SurTable T;
  int max_n;
  const int rc = sur_table(c, "sample_transform", " (t0 / t1 / noise / dgda / theta buffers)", vars, nvars,
      kSurT1 | kSurTheta | kSurDgda | kSurSkip, T, max_n);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  ensure_scratch(c, st);
  if (!launch_sample_fwd(T, nvars, max_n, S, seed, counter, state, logq, c->scratch, spmf_ctx::kScratchDoubles, st)) {
    // no scratch for the per-block sums: the two separate launches (same numbers)
    launch_sample_noise(T, nvars, max_n, S, seed, counter, state, st);
    launch_surrogate_fwd(T, nvars, max_n, S, logq, c->scratch, spmf_ctx::kScratchDoubles, st);
  }
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_surrogate_fwd(spmf_ctx* c, const spmf_sur_var* vars, int nvars, int S, double* logq, void* stream) {
  if (!c || !vars || nvars < 1 || nvars > 12 || S < 1 || !logq) return fail(c, SPMF_E_ARG,
      "surrogate_fwd: bad arguments");
  SurTable T;
  int max_n;
  const int rc = sur_table(c, "surrogate_fwd", "", vars, nvars, kSurT1 | kSurTheta | kSurSkip, T, max_n);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  ensure_scratch(c, st);
  launch_surrogate_fwd(T, nvars, max_n, S, logq, c->scratch, spmf_ctx::kScratchDoubles, st);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_sample_noise(spmf_ctx* c, const spmf_sur_var* vars, int nvars, int S, uint64_t seed, uint64_t counter,
    const double* state, void* stream) {
  if (!c || !vars || nvars < 1 || nvars > 12 || S < 1 || S > 65535) return fail(c, SPMF_E_ARG,
      "sample_noise: bad arguments");
  SurTable T;
  int max_n;
  const int rc = sur_table(c, "sample_noise", " (t0 / noise / dgda buffers)", vars, nvars, kSurDgda | kSurSkip, T,
      max_n);
  if (rc) return rc;
  launch_sample_noise(T, nvars, max_n, S, seed, counter, state, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_surrogate_bwd(spmf_ctx* c, const spmf_sur_var* vars, int nvars, int S, double inv_sb, double cw,
    void* stream) {
  if (!c || !vars || nvars < 1 || nvars > 12 || S < 1) return fail(c, SPMF_E_ARG, "surrogate_bwd: bad arguments");
  SurTable T;
  int max_n;
  const int rc = sur_table(c, "surrogate_bwd", "", vars, nvars, kSurT1 | kSurGrad | kSurG01 | kSurDgda, T, max_n);
  if (rc) return rc;
  launch_surrogate_bwd(T, nvars, max_n, S, (float)inv_sb, (float)cw, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_adam_step(spmf_ctx* c, const spmf_adam_var* tensors, int ntensors, double lr, double beta1, double beta2,
    double eps, int step, double clip, void* stream) {
  if (!c || !tensors || ntensors < 1 || ntensors > 24 || step < 1) return fail(c, SPMF_E_ARG,
      "adam_step: bad arguments");
  AdamTable T;
  int max_n;
  const int rc = adam_table(c, "adam_step", tensors, ntensors, T, max_n);
  if (rc) return rc;
  const double c1 = 1.0 - pow(beta1, step), c2 = 1.0 - pow(beta2, step);
  launch_adam(T, ntensors, max_n, lr, beta1, beta2, eps, c1, c2, clip, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_vi_gate(spmf_ctx* c, const double* parts, const double* logq, const double* n_nonfinite, int S, double cw,
    double rows, double* state, void* stream) {
  if (!c || !parts || !logq || !state || S < 1 || !(rows > 0.0)) return fail(c, SPMF_E_ARG, "vi_gate: bad arguments");
  launch_vi_gate(parts, logq, n_nonfinite, S, cw, rows, state, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_adam_step_dev(spmf_ctx* c, const spmf_adam_var* tensors, int ntensors, const double* state, void* stream) {
  if (!c || !tensors || ntensors < 1 || ntensors > 24 || !state) return fail(c, SPMF_E_ARG,
      "adam_step_dev: bad arguments");
  AdamTable T;
  int max_n;
  const int rc = adam_table(c, "adam_step_dev", tensors, ntensors, T, max_n);
  if (rc) return rc;
  launch_adam_dev(T, ntensors, max_n, state, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

int spmf_surrogate_bwd_adam_dev(spmf_ctx* c, const spmf_sur_var* vars, int nvars, int S, double inv_sb, double cw,
    const spmf_adam_var* tensors, const double* state, void* stream) {
  if (!c || !vars || !tensors || !state || nvars < 1 || nvars > 12 || S < 1) return fail(c, SPMF_E_ARG,
      "surrogate_bwd_adam_dev: bad arguments");
  SurTable T;
  AdamTable A;
  int max_n;
  const int rc = sur_table(c, "surrogate_bwd_adam_dev", "", vars, nvars, kSurT1 | kSurGrad | kSurDgda, T, max_n);
  if (rc) return rc;
  // tensors[2i], tensors[2i+1]: the Adam records of vars[i].t0 / t1 (the gradients come from the fused kernel)
  for (int i = 0; i < 2 * nvars; ++i) {
    const spmf_adam_var& a = tensors[i];
    const spmf_sur_var& v = vars[i / 2];
    if (!a.p || !a.m || !a.v || a.n != v.n || a.p != (i % 2 ? v.t1 : v.t0)) return fail(c, SPMF_E_ARG,
        "surrogate_bwd_adam_dev: tensors[2i+j] must be the Adam record (p, m, v, n) of vars[i].t{j}");
    A.v[i] = AdamVar{a.p, a.m, a.v, nullptr, a.n};
  }
  launch_surrogate_bwd_adam(T, A, nvars, max_n, S, (float)inv_sb, (float)cw, state, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SPMF_OK;
}

}  // extern "C"
