// cells.hip -- score_cells: posterior predictive mean and lppd of a LIST of cells over S draws
// (held-out evaluation), without a [S,B,D] tensor.
//
// For a listed cell (b, d) with an optional value x, over the draws s = 0 .. S-1:
//   mean = (1/S) sum_s m_s,   m_s = rate_s (Poisson column) | sigmoid(logit_s) (Bernoulli column)   (topk.hip)
//   lppd = logsumexp_s(ll_s) - log S,   ll_s = log p(x | theta_s)                                    (waic.hip)
// from the per-draw tables z[S,B,KP] (encode sweep), V'[S,D,KP], phi[S,D] (prep).  lgamma(x+1) does not
// depend on the draw and is subtracted once behind the loop.  A cell with a non-finite ll_s in any draw
// has lppd = NaN (the exclusion rule of the WAIC call); mean is whatever the arithmetic gives.
//
// One launch.  A cell owns a group of G = max(1, KP/4) lanes: lane `sub` of the group loads the sub-th
// float4 of V'_s[d] and of z_s[b], so a table row is one contiguous request of the group instead of KP/4
// requests of one lane (the request rate binds gathers on this chip: DESIGN.md section 4), and the partial
// dots are summed over the group by DPP adds (and xor shuffles above 16 lanes).  Every lane of the group
// ends with the same y and carries the same running statistics; lane 0 of the group writes.  The work is
// balanced by cells, not rows: a wave takes kCellsPerWave consecutive cells of the list, 64 / G at a
// time.  No atomics; the FMA order of a lane, the reduction tree of a group and the draw order are fixed
// and do not depend on where in the list, in the wave or in the batch chunk a cell sits, so a cell's
// result is a function of the cell alone.  An index outside [0,B) x [0,D) reads no memory and writes NaN.
#include "common.h"
#include "kernels.h"

namespace spmf {

namespace {

constexpr int kCellsPerWave = 64;

// sum over the aligned group of G lanes (G = 1 .. 64); every lane of the group gets the total
template <int G>
__device__ __forceinline__ float cell_group_sum(float v) {
  v = group_sum<(G < 16 ? G : 16)>(v);
  if constexpr (G >= 32) v += __shfl_xor(v, 16);
  if constexpr (G >= 64) v += __shfl_xor(v, 32);
  return v;
}

}  // namespace

template <int G>
__global__ __launch_bounds__(256) void cells_kernel(int64_t n_cells, int64_t B, int D, int S, int lik,
                                                    const int32_t* __restrict__ cell_row,
                                                    const int32_t* __restrict__ cell_col,
                                                    const float* __restrict__ cell_val,
                                                    const float* __restrict__ z,
                                                    const float* __restrict__ Vp,
                                                    const float* __restrict__ phi,
                                                    const uint8_t* __restrict__ ctype,
                                                    float* __restrict__ mean_out,
                                                    float* __restrict__ lppd_out) {
  constexpr int KP = 4 * G;
  constexpr int CPP = 64 / G;          // cells of one pass of a wave
  const int lane = threadIdx.x & 63;
  const int sub = lane % G, grp = lane / G;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t first = wave * kCellsPerWave;
  const size_t zs = (size_t)B * KP, vs = (size_t)D * KP;   // floats between two draws
  const float inv_s = 1.f / (float)S;
  const double logS = log((double)S);
  const float nan = __int_as_float(0x7fc00000);
  const bool with_val = cell_val != nullptr;               // kernel argument: uniform

  for (int p = 0; p < kCellsPerWave / CPP; ++p) {          // uniform trip count: the shuffles see whole groups
    const int64_t i = first + p * CPP + grp;
    const bool live = i < n_cells;
    const int b = live ? cell_row[i] : -1;
    const int d = live ? cell_col[i] : -1;
    // the same for every lane of a group; nothing below reads a table unless it holds
    const bool ok = live && b >= 0 && (int64_t)b < B && d >= 0 && d < D;
    const float x = ok && with_val ? cell_val[i] : 0.f;
    const bool bern = ok && cell_is_bern(lik, ctype, d);
    const float* zr = z + (size_t)(ok ? b : 0) * KP + 4 * sub;
    const float* vr = Vp + (size_t)(ok ? d : 0) * KP + 4 * sub;
    const float* pr = phi + (ok ? d : 0);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), v = a;
    float ph = 0.f;
    if (ok) {
      a = *reinterpret_cast<const float4*>(zr);
      v = *reinterpret_cast<const float4*>(vr);
      ph = *pr;
    }
    float sm = 0.f, m = -INFINITY, se = 0.f;
    bool fin = true;
    for (int s = 0; s < S; ++s) {
      // the next draw's rows are asked for before this draw's are used
      float4 an = a, vn = v;
      float pn = ph;
      if (ok && s + 1 < S) {
        an = *reinterpret_cast<const float4*>(zr + (size_t)(s + 1) * zs);
        vn = *reinterpret_cast<const float4*>(vr + (size_t)(s + 1) * vs);
        pn = pr[(size_t)(s + 1) * D];
      }
      const float y = cell_group_sum<G>(dot4(a, v));
      float ey;
      const float rt = cell_rate(lik, y, ph, ey);
      sm += cell_mean(bern, rt);
      if (with_val) {
        const float ll = cell_ll<false>(bern, x, rt);
        fin = fin && isfinite(ll);
        lse_update(ll, m, se);
      }
      a = an;
      v = vn;
      ph = pn;
    }
    if (sub == 0 && live) {
      mean_out[i] = ok ? sm * inv_s : nan;
      if (with_val) {
        const double lg = bern ? 0.0 : (double)lgammaf(x + 1.f);
        const float lp = (float)((double)m + (double)logf(se) - logS - lg);
        lppd_out[i] = ok && fin ? lp : nan;
      }
    }
  }
}

bool launch_cells(const CellsArgs& a, hipStream_t st) {
  const DrawTables& t = a.t;
  if (t.lik < 0 || t.lik > 4 || a.n_cells < 1) return false;
  const int64_t per_block = 4 * kCellsPerWave;
  const int64_t nb = (a.n_cells + per_block - 1) / per_block;
  if (nb > 0x7fffffff) return false;
  return with_kp<256>(t.KP, [&](auto kp) {
    hipLaunchKernelGGL((cells_kernel<decltype(kp)::value / 4>), dim3((unsigned)nb), dim3(256), 0, st, a.n_cells, t.B,
                       t.D, t.S, t.lik, a.row, a.col, a.val, t.z, t.Vp, t.phi, t.ctype, a.mean, a.lppd);
  });
}

}  // namespace spmf
