// waic.hip -- streaming WAIC: per-cell lppd / pwaic over S draws, summed over the cells of a
// batch, without a [S,B,D] (or [B,D]) tensor.
//
// A point is one cell (b, d).  With ll_s = log p(x_bd | theta_s), s = 0 .. S-1:
//   lppd_i  = logsumexp_s(ll_s) - log S
//   pwaic_i = unbiased var_s(ll_s)
//   elpd_i  = lppd_i - pwaic_i
// and the call adds  #cells, sum lppd_i, sum pwaic_i, sum elpd_i^2, #excluded cells  to a
// caller-owned double[6] (a cell with a non-finite ll_s in any draw is excluded and counted).
// Optionally the sums of each row's cells (lppd, pwaic: row_out[B][2]) and the five sums of each
// column's cells (col_out[D][5], the slots of the double[6]) are added to caller-owned arrays.
//
// Two launches over the per-draw tables z[S,B,KP] (encode sweep), V'[S,D,KP], phi[S,D] (prep):
//   waic_dense_kernel : EVERY cell as if x = 0.  A workgroup owns a 64 x 64 block of cells, a
//     wave a 32 x 32 tile: y_s = <z_sb, V'_sd> by score_tile_loop (score_block.h: the one
//     double-buffered MFMA loop over (draw, K chunk) of all streaming kernels), whose per-draw
//     callback here updates the four statistics of a cell -- running maximum, rescaled sum of
//     exp, running mean, sum of squared deviations -- which stay in registers across the loop
//     over draws (16 cells per lane).
//   waic_fix_kernel   : the stored cells, one wave per row, one lane per entry: the same
//     statistics for the x = 0 value and for the true count, both by fp32 FMA from the same
//     tables; the x = 0 contribution is taken out of the sums and the true one put in (the
//     sums are additive over cells).  lgamma(x+1) does not depend on the draw: it cancels in
//     the variance and is subtracted from lppd_i once, behind the loop.
// Column sums: a lane's 16 cells lie in one column, so the dense kernel's share of a column is the
// lane's own five sums, joined across the lane halves by a shuffle and across the two waves of a
// block column through LDS: one fp64 atomic per (column, slot) and workgroup.  The fix kernel adds
// an entry's net change to its column: three atomics, five where a count changes.
// The log-mean-exp carries a running maximum, so a cell whose every ll_s is below -1000 is as
// exact as any other.
#include "common.h"
#include "kernels.h"
#include "score_block.h"

namespace spmf {

namespace {

// running statistics of one cell over the draws
__device__ __forceinline__ void stat_update(float ll, float inv_n, float& m, float& se, float& mu, float& q) {
  lse_update(ll, m, se);
  const float dl = ll - mu;                    // Welford; a non-finite ll leaves q non-finite for good
  mu = fmaf(dl, inv_n, mu);
  q = fmaf(dl, ll - mu, q);
}

__device__ __forceinline__ double half_sum(double v) {   // over the 32 lanes of a wave half
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

}  // namespace

// KC: floats of the K axis per LDS tile (8, 16, 32); KP > KC runs KP / KC chunks per draw
template <int KC, int LIK>
__global__ __launch_bounds__(256) void waic_dense_kernel(int64_t B, int D, int KP, int S,
                                                         const float* __restrict__ z,
                                                         const float* __restrict__ Vp,
                                                         const float* __restrict__ phi,
                                                         const uint8_t* __restrict__ ctype,
                                                         double* __restrict__ sums,
                                                         double* __restrict__ row_out,
                                                         double* __restrict__ col_out) {
  __shared__ __align__(16) float tiles[2][2][64][KC + 4];
  __shared__ double red[16];
  const int t = threadIdx.x;
  const int lane = t & 63, wv = t >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int wr = wv >> 1;
  const int64_t b0 = (int64_t)blockIdx.x * 64;
  const int d0 = blockIdx.y * 64;
  const int d = score_tile_col(d0);
  const bool bern = score_col_bern<LIK>(ctype, D, d);

  float m[16], se[16], mu[16], q[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    m[r] = -INFINITY;
    se[r] = 0.f;
    mu[r] = 0.f;
    q[r] = 0.f;
  }
  score_tile_loop<KC>(tiles, B, D, KP, S, b0, d0, z, Vp, phi, [&](int s, const score_f32x16& acc, float ph) {
    const float inv_n = 1.f / (float)(s + 1);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float ey;
      const float rt = cell_rate(LIK, acc[r], ph, ey);
      stat_update(cell_ll0(bern, rt), inv_n, m[r], se[r], mu[r], q[r]);
    }
  });

  const double logS = log((double)S), inv_sm1 = 1.0 / (double)(S - 1);
  double an = 0.0, aL = 0.0, aP = 0.0, aE = 0.0, ax = 0.0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t b = b0 + score_tile_row(wr, r, h);
    const bool in = b < B && d < D;
    const double lp = (double)m[r] + (double)logf(se[r]) - logS;
    const double pw = (double)q[r] * inv_sm1;
    const bool fin = isfinite(lp) && isfinite(pw);
    if (in && fin) {
      const double e = lp - pw;
      an += 1.0;
      aL += lp;
      aP += pw;
      aE += e * e;
    } else if (in) {
      ax += 1.0;
    }
    if (row_out) {                                        // block-uniform
      const double rl = half_sum(in && fin ? lp : 0.0);
      const double rp = half_sum(in && fin ? pw : 0.0);
      if (i32 == 0 && b < B) {
        atomicAdd(&row_out[2 * b], rl);
        atomicAdd(&row_out[2 * b + 1], rp);
      }
    }
  }
  const double tn = block_sum(an, red);
  const double tL = block_sum(aL, red);
  const double tP = block_sum(aP, red);
  const double tE = block_sum(aE, red);
  const double tx = block_sum(ax, red);
  if (t == 0) {
    atomicAdd(&sums[0], tn);
    atomicAdd(&sums[1], tL);
    atomicAdd(&sums[2], tP);
    atomicAdd(&sums[3], tE);
    if (tx != 0.0) atomicAdd(&sums[4], tx);
  }
  if (col_out) {                                          // block-uniform
    // the lane's five sums are those of its column over 16 of the wave's 32 rows: the other lane half holds
    // the other 16, wave row 1 the block's other 32 rows (through the tile buffers, which the loop's last
    // barrier released: [5][64] doubles of their 12 KB and more)
    double* cs = reinterpret_cast<double*>(&tiles[0][0][0][0]);
    double c[5] = {an, aL, aP, aE, ax};
#pragma unroll
    for (int j = 0; j < 5; ++j) c[j] += __shfl_xor(c[j], 32);
    const int cl = (wv & 1) * 32 + i32;                   // the column inside the block
    if (wr == 1 && h == 0) {
#pragma unroll
      for (int j = 0; j < 5; ++j) cs[j * 64 + cl] = c[j];
    }
    __syncthreads();
    if (wr == 0 && h == 0 && d < D) {
      double* co = col_out + (size_t)d * 5;
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(&co[j], c[j] + cs[j * 64 + cl]);
      const double cx = c[4] + cs[4 * 64 + cl];
      if (cx != 0.0) atomicAdd(&co[4], cx);
    }
  }
}

// stored cells: x = 0 statistics out, true statistics in.  One wave per row, one lane per entry.
__global__ __launch_bounds__(256) void waic_fix_kernel(int64_t B, int D, int KP, int S, int lik,
                                                       const int32_t* __restrict__ row_ptr,
                                                       const int32_t* __restrict__ col,
                                                       const float* __restrict__ val,
                                                       const float* __restrict__ z,
                                                       const float* __restrict__ Vp,
                                                       const float* __restrict__ phi,
                                                       const uint8_t* __restrict__ ctype,
                                                       double* __restrict__ sums,
                                                       double* __restrict__ row_out,
                                                       double* __restrict__ col_out) {
  __shared__ double red[16];
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const double logS = log((double)S), inv_sm1 = 1.0 / (double)(S - 1);
  const int K4 = KP / 4;
  double an = 0.0, aL = 0.0, aP = 0.0, aE = 0.0, ax = 0.0;
  for (int64_t b = wave; b < B; b += nwaves) {
    const int start = row_ptr[b], end = row_ptr[b + 1];
    double rl = 0.0, rp = 0.0;
    for (int i = start + lane; i < end; i += 64) {
      const float x = val[i];
      const int d = col[i];
      const bool bern = cell_is_bern(lik, ctype, d);
      float m0 = -INFINITY, e0 = 0.f, u0 = 0.f, q0 = 0.f;
      float m1 = -INFINITY, e1 = 0.f, u1 = 0.f, q1 = 0.f;
      for (int s = 0; s < S; ++s) {
        const float4* zr = reinterpret_cast<const float4*>(z + ((size_t)s * B + b) * KP);
        const float4* vr = reinterpret_cast<const float4*>(Vp + ((size_t)s * D + d) * KP);
        float y = 0.f;
        for (int k = 0; k < K4; ++k) {
          const float4 a = zr[k], v = vr[k];
          y = fmaf(a.x, v.x, y);
          y = fmaf(a.y, v.y, y);
          y = fmaf(a.z, v.z, y);
          y = fmaf(a.w, v.w, y);
        }
        float ey;
        const float rt = cell_rate(lik, y, phi[(size_t)s * D + d], ey);
        const float inv_n = 1.f / (float)(s + 1);
        // the cell as the dense kernel counted it (x = 0) and as it is, without lgamma(x+1) (once, behind the
        // loop); one branch on the cell's type for both
        float l0, l1;
        if (bern) {
          l0 = cell_ll0(true, rt);
          l1 = cell_ll<false>(true, x, rt);
        } else {
          l0 = cell_ll0(false, rt);
          l1 = cell_ll<false>(false, x, rt);
        }
        stat_update(l0, inv_n, m0, e0, u0, q0);
        stat_update(l1, inv_n, m1, e1, u1, q1);
      }
      const double lg = bern ? 0.0 : (double)lgammaf(x + 1.f);
      const double lp0 = (double)m0 + (double)logf(e0) - logS, pw0 = (double)q0 * inv_sm1;
      const double lp1 = (double)m1 + (double)logf(e1) - logS - lg, pw1 = (double)q1 * inv_sm1;
      const bool fin0 = isfinite(lp0) && isfinite(pw0), fin1 = isfinite(lp1) && isfinite(pw1);
      if (fin0) {
        const double e = lp0 - pw0;
        an -= 1.0; aL -= lp0; aP -= pw0; aE -= e * e;
        rl -= lp0; rp -= pw0;
      } else {
        ax -= 1.0;
      }
      if (fin1) {
        const double e = lp1 - pw1;
        an += 1.0; aL += lp1; aP += pw1; aE += e * e;
        rl += lp1; rp += pw1;
      } else {
        ax += 1.0;
      }
      if (col_out) {                                       // grid-uniform: the entry's net change to its column
        const double e0 = lp0 - pw0, e1 = lp1 - pw1;
        const double dn = (fin1 ? 1.0 : 0.0) - (fin0 ? 1.0 : 0.0);
        double* co = col_out + (size_t)d * 5;
        if (dn != 0.0) {                                   // counted <-> excluded
          atomicAdd(&co[0], dn);
          atomicAdd(&co[4], -dn);
        }
        atomicAdd(&co[1], (fin1 ? lp1 : 0.0) - (fin0 ? lp0 : 0.0));
        atomicAdd(&co[2], (fin1 ? pw1 : 0.0) - (fin0 ? pw0 : 0.0));
        atomicAdd(&co[3], (fin1 ? e1 * e1 : 0.0) - (fin0 ? e0 * e0 : 0.0));
      }
    }
    if (row_out && end > start) {                          // wave-uniform
      rl = wave_sum(rl);
      rp = wave_sum(rp);
      if (lane == 0) {
        atomicAdd(&row_out[2 * b], rl);
        atomicAdd(&row_out[2 * b + 1], rp);
      }
    }
  }
  const double tn = block_sum(an, red);
  const double tL = block_sum(aL, red);
  const double tP = block_sum(aP, red);
  const double tE = block_sum(aE, red);
  const double tx = block_sum(ax, red);
  if (threadIdx.x == 0) {
    if (tn != 0.0) atomicAdd(&sums[0], tn);
    atomicAdd(&sums[1], tL);
    atomicAdd(&sums[2], tP);
    atomicAdd(&sums[3], tE);
    if (tx != 0.0) atomicAdd(&sums[4], tx);
  }
}

bool launch_waic(const WaicArgs& a, hipStream_t st) {
  const DrawTables& t = a.t;
  const dim3 grid((unsigned)((t.B + 63) / 64), (unsigned)((t.D + 63) / 64));
  bool ok = false;
  with_kc(t.KP, [&](auto kc) {
    ok = with_lik(t.lik, [&](auto lik) {
      hipLaunchKernelGGL((waic_dense_kernel<decltype(kc)::value, decltype(lik)::value>), grid, dim3(256), 0, st, t.B,
                         t.D, t.KP, t.S, t.z, t.Vp, t.phi, t.ctype, a.sums, a.row_out, a.col_out);
    });
  });
  if (!ok) return false;
  if (a.nnz > 0) {
    const int64_t want = (t.B + 3) / 4;
    const int nb = (int)(want < 1 ? 1 : (want > 4096 ? 4096 : want));
    hipLaunchKernelGGL(waic_fix_kernel, dim3(nb), dim3(256), 0, st, t.B, t.D, t.KP, t.S, t.lik, a.row_ptr, a.col,
                       a.val, t.z, t.Vp, t.phi, t.ctype, a.sums, a.row_out, a.col_out);
  }
  return true;
}

}  // namespace spmf
