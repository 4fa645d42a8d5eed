// panel.hip -- streaming predictions: the posterior predictive mean, standard deviation and P(x > 0) of every
// cell of a rows x columns panel over S draws, written out as dense [B][C] arrays, without a [S,B,D] tensor.
//
// With r_s = cell_rate(<z_sb, V'_sd>, phi_sd) (the rate of a Poisson column, the logit of a Bernoulli one) and
// m_s = cell_mean(r_s) (r_s | sigmoid(r_s)), s = 0 .. S-1 in draw order:
//   mean = (1/S) sum_s m_s                      -- the score of topk.hip / rank.hip, the same bits
//   sd   = sqrt(q / (S-1)), q by Welford's recurrence over m_s (running mean mu += (m_s - mu) / (s+1),
//          q = fma(m_s - mu_old, m_s - mu_new, q)); mu is never written out
//   pnz  = (1/S) sum_s -expm1f(-r_s) on a Poisson column: P(x > 0) under the predictive mixture, without the
//          cancellation of 1 - mean exp(-r) at small rates; on a Bernoulli column the mean itself
//
// Two kernels over the per-draw tables z[S,B,KP] (encode sweep), V'[S,D,KP], phi[S,D] (prep):
//   panel_gather_kernel : a listed panel.  Vc[s][j][:] = V'[s][cols[j]][:], phic[s][j] = phi[s][cols[j]],
//     ctc[j] = ctype[cols[j]] for all S draws in one launch, so that the main kernel sees C contiguous
//     columns.  A listed column outside [0, D) reads nothing: a zero row and phic = NaN in every draw, which
//     makes every output of that column NaN without a case of its own in the main kernel.
//   panel_kernel<KC, LIK, SD, PNZ> : a workgroup owns a 64 x 64 block of cells, a wave a 32 x 32 tile:
//     y_s = <z_sb, V'_sd> by score_tile_loop (score_block.h), whose per-draw callback updates the statistics
//     asked for.  They stay in registers across the draws, 16 cells per lane; SD and PNZ are template flags, so
//     a mean-only launch is score_block itself and carries neither register set.  Accumulator r of the 32
//     lanes of a wave half is 32 consecutive columns of one row: every store instruction writes 128
//     contiguous bytes per row.
// Every output element depends on its own cell alone: no atomics, one summation order.
#include "common.h"
#include "kernels.h"
#include "score_block.h"

namespace spmf {

// grid (ceil(C * KP / 4 / 256), S): a thread per float4 of a compacted row of one draw
__global__ __launch_bounds__(256) void panel_gather_kernel(int D, int C, int KP, const int32_t* __restrict__ cols,
                                                           const float* __restrict__ Vp,
                                                           const float* __restrict__ phi,
                                                           const uint8_t* __restrict__ ctype,
                                                           float* __restrict__ Vc, float* __restrict__ phic,
                                                           uint8_t* __restrict__ ctc) {
  const int K4 = KP / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)C * K4) return;
  const int s = blockIdx.y;
  const int j = (int)(i / K4), q = (int)(i - (int64_t)j * K4);
  const int c = cols[j];
  const bool in = c >= 0 && c < D;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (in) v = *reinterpret_cast<const float4*>(Vp + ((size_t)s * D + c) * KP + 4 * q);
  *reinterpret_cast<float4*>(Vc + ((size_t)s * C + j) * KP + 4 * q) = v;
  if (q == 0) {
    phic[(size_t)s * C + j] = in ? phi[(size_t)s * D + c] : __builtin_nanf("");
    if (s == 0 && ctc) ctc[j] = in && ctype ? ctype[c] : (uint8_t)0;
  }
}

// KC: floats of the K axis per LDS tile (8, 16, 32); KP > KC runs KP / KC chunks per draw.  C: the columns of
// the tables Vp / phi / ctype (the context's D, or the length of the compacted list) and of the outputs.
template <int KC, int LIK, bool SD, bool PNZ>
__global__ __launch_bounds__(256) void panel_kernel(int64_t B, int C, int KP, int S, const float* __restrict__ z,
                                                    const float* __restrict__ Vp, const float* __restrict__ phi,
                                                    const uint8_t* __restrict__ ctype, float inv_s,
                                                    float* __restrict__ mean, float* __restrict__ sd,
                                                    float* __restrict__ pnz) {
  __shared__ float tiles[2][2][64][KC + 4];
  const int t = threadIdx.x;
  const int h = (t & 63) >> 5, wr = t >> 7;
  const int64_t b0 = (int64_t)blockIdx.x * 64;
  const int d0 = blockIdx.y * 64;
  const int d = score_tile_col(d0);
  const bool bern = score_col_bern<LIK>(ctype, C, d);

  float sc[16];
  float mu[SD ? 16 : 1], q[SD ? 16 : 1], pz[PNZ ? 16 : 1];
  if constexpr (!SD && !PNZ) {
    score_block<KC, LIK>(tiles, B, C, KP, S, b0, d0, z, Vp, phi, ctype, inv_s, sc);
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sc[r] = 0.f;
      if constexpr (SD) mu[r] = q[r] = 0.f;
      if constexpr (PNZ) pz[r] = 0.f;
    }
    // the mean: the statements of score_block's callback
    score_tile_loop<KC>(tiles, B, C, KP, S, b0, d0, z, Vp, phi, [&](int s, const score_f32x16& acc, float ph) {
      const float inv_n = 1.f / (float)(s + 1);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float ey;
        const float rs = cell_rate(LIK, acc[r], ph, ey);
        const float ms = cell_mean(bern, rs);
        sc[r] += ms;
        if constexpr (SD) {
          const float dl = ms - mu[r];                // Welford; a non-finite m_s leaves q non-finite for good
          mu[r] = fmaf(dl, inv_n, mu[r]);
          q[r] = fmaf(dl, ms - mu[r], q[r]);
        }
        if constexpr (PNZ && !lik_bern(LIK)) pz[r] -= expm1f(-rs);   // (a Bernoulli lane's sum is not used)
      }
    });
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[r] *= inv_s;
  }

  if (d >= C) return;
  const float inv_sm1 = 1.f / (float)(S - 1);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t b = b0 + score_tile_row(wr, r, h);
    if (b >= B) continue;
    const size_t o = (size_t)b * C + d;
    mean[o] = sc[r];
    if constexpr (SD) sd[o] = sqrtf(q[r] * inv_sm1);
    if constexpr (PNZ) pnz[o] = bern ? sc[r] : pz[r] * inv_s;
  }
}

void launch_panel_gather(const DrawTables& t, int C, const int32_t* cols, float* Vc, float* phic, uint8_t* ctc,
                         hipStream_t st) {
  const int64_t n4 = (int64_t)C * (t.KP / 4);
  hipLaunchKernelGGL(panel_gather_kernel, dim3((unsigned)((n4 + 255) / 256), (unsigned)t.S), dim3(256), 0, st, t.D,
                     C, t.KP, cols, t.Vp, t.phi, t.ctype, Vc, phic, ctc);
}

bool launch_panel(const PanelArgs& a, hipStream_t st) {
  DrawTables t = a.t;
  const int C = a.n_cols;
  if (!with_kc(t.KP, [](auto) {}) || !with_lik(t.lik, [](auto) {})) return false;
  if (t.B <= 0 || C <= 0) return true;
  if (a.cols) {
    uint8_t* ctc = t.lik == 3 ? a.ctc : nullptr;
    launch_panel_gather(t, C, a.cols, a.Vc, a.phic, ctc, st);
    t.Vp = a.Vc;
    t.phi = a.phic;
    t.ctype = ctc;
  }
  t.D = C;
  const dim3 grid((unsigned)((t.B + 63) / 64), (unsigned)((C + 63) / 64));
  const float inv_s = 1.f / (float)t.S;
  auto flags = [&](auto kc, auto lik, auto sd, auto pz) {
    hipLaunchKernelGGL((panel_kernel<decltype(kc)::value, decltype(lik)::value, decltype(sd)::value,
                                     decltype(pz)::value>),
                       grid, dim3(256), 0, st, t.B, t.D, t.KP, t.S, t.z, t.Vp, t.phi, t.ctype, inv_s, a.mean, a.sd,
                       a.pnz);
  };
  with_kc(t.KP, [&](auto kc) {
    with_lik(t.lik, [&](auto lik) {
      using T = std::true_type;
      using F = std::false_type;
      if (a.sd && a.pnz) flags(kc, lik, T{}, T{});
      else if (a.sd) flags(kc, lik, T{}, F{});
      else if (a.pnz) flags(kc, lik, F{}, T{});
      else flags(kc, lik, F{}, F{});
    });
  });
  return true;
}

}  // namespace spmf
