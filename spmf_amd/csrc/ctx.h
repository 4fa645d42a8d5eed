// ctx.h -- host only: what the seven files behind the C-ABI of libspmf_hip.so (api_ctx.hip, api_step.hip,
// api_stream.hip, api_points.hip, api_graph.hip, api_comm.hip, api_vi.hip; see include/spmf_hip.h) share: the
// context, the error return, the likelihood code, the per-draw tables, the scratch prologue of the calls on rows and
// graphs as given, and the few functions one file defines for another.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/spmf_hip.h"
#include "arena.h"
#include "common.h"
#include "kernels.h"

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

// The members stand by the file that owns them; the first group is everybody's.
struct spmf_ctx : WsBuffers {
  int device = 0, K = 0, D = 0, KP = 0;
  unsigned flags = 0;
  double u_tau_scale = 0.01, s_tau_scale = 1.0, decay = 0.99;  // poisson.py:59
  std::string err;
  // workspace (api_ctx.hip; bound by api_step.hip): the workspace and the batch it is bound for
  char* ws = nullptr;
  size_t ws_bytes = 0;
  int64_t ws_rows = 0;
  int ws_S = 0;
  // deterministic mode (spmf_ctx_set_deterministic): caller-owned scratch for the row pass's per-workgroup
  // scalar slots and the column pass's per-item partial sums; null = off
  char* det_buf = nullptr;
  size_t det_bytes = 0;
  // likelihood tables (api_ctx.hip)
  const uint8_t* ctype = nullptr;   // mixed likelihood: 1 = Bernoulli column (device, caller-owned)
  const int32_t* bcols = nullptr;   // mixed likelihood: ascending indices of the Bernoulli columns (optional)
  int n_bcols = 0;
  // timing taps (api_ctx.hip; recorded by api_step.hip)
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
  int prior_pending = 0;          // S of the launched prior half, 0 = none
  const double* prior_parts = nullptr;
  // step (api_step.hip)
  int Dh = 0;                     // column split of the accumulator layout (0 = none)
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
  // dense switches (api_step.hip)
  int e_once = 1;                 // SPMF_DENSE_E_ONCE=0: recompute E in a second launch instead
  int dense3 = 1;                 // exp sums on the bf16 matrix cores with three-way split operands
                                  // (dense3.hip; Poisson log_transform at KP = 64 only);
                                  // SPMF_DENSE_BF16X3=0 selects the exact-f32 MFMA kernels (dense.hip)
  size_t est_cap_bytes = (size_t)8 << 30;   // spmf_ctx_set_e_cap
  // VI scratch (api_vi.hip)
  // the library's only device allocation: a small scratch for per-block partial sums of the
  // O(D*K) surrogate kernels (fixed-order reductions instead of same-address atomics)
  double* scratch = nullptr;
  static constexpr size_t kScratchDoubles = 1u << 20;   // 8 MiB
  // RCCL (api_comm.hip)
  void* comm = nullptr;           // ncclComm_t of the row-shard collective (spmf_comm_init)
  int comm_rank = 0, comm_world = 1;
  // P2P (api_comm.hip)
  // the hand-written collective over peer pointers (spmf_p2p_*; p2p.hip): this rank's fine-grained region
  // and the peers' regions as mapped into this process
  struct P2P {
    char* region = nullptr;          // own allocation: [rs | ag | flags | seq]
    size_t bytes = 0, alloc_bytes = 0, off_ag = 0, off_flags = 0, off_seq = 0;
    int64_t n_max = 0, slice_cap = 0;
    int rank = 0, world = 0, nchunk = 0, connected = 0;
    char* peer[spmf::kP2PMaxWorld] = {};   // peer regions (own rank: own region); opened with hipIpcOpenMemHandle
  } p2p;
};

inline int fail(spmf_ctx* c, int code, const std::string& msg) {
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

static int likelihood_code(const spmf_ctx* c) {   // common.h: lik_exp / lik_bern
  const bool lt = (c->flags & SPMF_FLAG_LOG_TRANSFORM) != 0;
  if (c->flags & SPMF_FLAG_BERNOULLI) return lt ? 4 : 2;
  if (c->flags & SPMF_FLAG_MIXED) return 3;
  return lt ? 1 : 0;
}

// The per-draw tables and row outputs a launch sequence works on: those of the bound workspace (draw 0), or
// those of the draw stage inside a streaming call's scratch (draw_stage)
struct Tables {
  float *Ap, *Vp, *phi;
  double *dprep, *dacc;
  float *z, *gzs;
};
static Tables ws_tables(const spmf_ctx* c) { return Tables{c->Ap, c->Vp, c->phi, c->dprep, c->dacc, c->z, c->gzs}; }

// deterministic-mode scratch: per draw the row pass's slots, then the column pass's per-item partial sums.
// Draw 0's two buffers inside the `bytes` of `buf` (null: sizes only); draw s lies s * dstride doubles = s * fstride
// floats behind (the data pass checks all S draws against spmf_det_scratch_bytes first).
struct DetDraw {
  double* slots;                // [kDetMeta + kDetMaxBlocks * (kDaccHead + KP)]
  float* part;                  // [n_items][det_part_len]
  int64_t dstride, fstride;
  size_t bytes;                 // of one draw
};

// ---- what one file defines for another ---------------------------------------------------------
namespace spmf {
// api_ctx.hip
int check_counts(spmf_ctx* c, const spmf_counts* ct);
DetDraw det_layout(void* buf, size_t bytes, int KP, int64_t n_items);
// api_step.hip
int encode_rows(spmf_ctx* c, const char* fn, const spmf_counts* ct, int S, const Tables* T, const float* u,
    const float* v, const float* w, const float* s, const float* eta, hipStream_t st);
// api_stream.hip
// The SPMF_E_WORKSPACE failure of a call `fn` whose scratch holds `have` bytes where its layout takes `need` for
// the shape `detail` ("rows=70 S=2").
int scratch_too_small(spmf_ctx* c, const char* fn, size_t need, size_t have, const std::string& detail);
// The end of every entry: `ok` is what its launcher returned, `no_kernel` the entry's text for false.
int launched(spmf_ctx* c, bool ok, const char* no_kernel);
int device_cus(const spmf_ctx* c);
int topk_slices(int64_t n_rows, int D, int cus);
// The ordering of `rows` rows by one of G labels (launch_group_order): chunks and NB are the call's geometry
void group_order_carve(Arena& a, int64_t rows, int G, int64_t chunks, int64_t NB, GroupOrder& o);
// api_comm.hip (spmf_ctx_destroy)
void comm_release(spmf_ctx* c);
void p2p_release(spmf_ctx* c);

// ---- the calls on rows and graphs as given (api_points.hip, api_graph.hip) -----------------------
// A row count that a launch takes as a 31-bit grid extent of 64-row blocks
inline bool rows_ok(int64_t n) { return n >= 0 && n <= ((int64_t)1 << 31) - 64; }
// The bytes of a layout: `layout(arena)` on an arena without memory
template <class Layout>
size_t layout_bytes(Layout&& layout) {
  Arena a;
  layout(a);
  return a.used;
}
// The scratch of a call `fn`: not NULL, 256-byte aligned, and `layout(arena)` fits into its scratch_bytes;
// `detail()` is the shape in the SPMF_E_WORKSPACE failure.  On SPMF_OK the layout's pointers are fit to launch on.
template <class Layout, class Detail>
int carve_scratch(spmf_ctx* c, const char* fn, void* scratch, size_t scratch_bytes, Layout&& layout,
    Detail&& detail) {
  if (!scratch) return fail(c, SPMF_E_ARG, std::string(fn) + ": null argument");
  if ((uintptr_t)scratch & 255) return fail(c, SPMF_E_ARG, std::string(fn) + ": scratch must be 256-byte aligned");
  Arena a(scratch, scratch_bytes);
  layout(a);
  return a.fits() ? SPMF_OK : scratch_too_small(c, fn, a.used, scratch_bytes, detail());
}
}  // namespace spmf
