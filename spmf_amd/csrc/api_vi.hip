// api_vi.hip -- the VI kernels' entries behind the C-ABI (include/spmf_hip.h; surrogate.hip): the sampler, the
// surrogate posterior forward / backward, Adam and the gate.  Host-side orchestration only (ctx.h).
#include <math.h>

#include "ctx.h"

using namespace spmf;

extern "C" {

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
