// sets.hip -- streaming per-row sums of the posterior predictive over column sets: for every row b of a batch
// and every set g with listed columns c_j and weights w_j (j over the set's list, a repeated column counts twice)
//   score_s(b, g) = sum_j (double)w_j * (double)m_s(b, c_j)           per draw s
//   mean(b, g)    = (1/S) sum_s score_s(b, g)                         fp64, in draw order
//   sd(b, g)      = sqrt(q / (S-1)), q by Welford's recurrence over score_s in draw order, fp64
// with r_s = cell_rate(<z_sb, V'_sd>, phi_sd) and m_s = cell_mean(r_s) as in panel.hip: the weighted sums of
// predict's cells along the column axis, without the [rows, columns] block of a draw.  All additions are fp64:
// every product w * m_s is formed from two converted operands and is exact; no fp32 partial sums, no atomics.
//
// The layout: the listed columns of all sets of a call are laid out set after set, every set padded to whole
// 64-column blocks (index -1, weight 0), and compacted with launch_panel_gather (panel.hip), which turns a pad
// slot -- and a listed column outside [0, D) -- into a zero row of V' with phi = NaN.  The set offsets reach the
// device as kernel arguments, kSetFillChunk sets per launch of set_fill_kernel: no host-to-device copy.
//
// set_kernel<KC, LIK>: a workgroup owns 64 rows x one set.  It walks the draws in chunks of kSetDrawChunk and,
// per chunk, the set's column blocks with score_tile_loop (score_block.h, unchanged; the padded column count is
// its bound and its row stride).  The callback forms w * m_s of the lane's 16 cells (one column, 16 rows) as
// doubles, columns at or past the set's valid count selected out (not multiplied by 0: a pad column holds NaN),
// and adds them over the 32 columns of the wave by a halving exchange -- lane bit 4, 3, 2, 1 each keep half of the
// rows and add the partner's half, lane bit 0 adds the two remaining columns -- so that lane pair (2r, 2r+1) of
// a wave half holds the sum of accumulator row r.  Behind the block's loop thread (draw, row) adds wave column
// 0 + wave column 1 onto its register accumulator; behind the chunk's last block the accumulators pass through
// LDS to 64 threads that advance the per-row sum and Welford state draw by draw.  One summation order, a pure
// function of the set's own list, S and KP: not of the other sets, the set's place in the call or the rows'.
#include "common.h"
#include "kernels.h"
#include "score_block.h"

namespace spmf {

// grid = the sets of the chunk: the padded list, the padded weights and the record (first block, columns) of set
// g0 + blockIdx.x
__global__ __launch_bounds__(256) void set_fill_kernel(SetFill f, int g0, const int32_t* __restrict__ cols,
                                                       const float* __restrict__ weights,
                                                       int32_t* __restrict__ colsp, float* __restrict__ wp,
                                                       int2* __restrict__ srec) {
  const int g = blockIdx.x;
  const int64_t p0 = f.ptr[g];
  const int n = (int)(f.ptr[g + 1] - p0);
  const int64_t o = (int64_t)f.boff[g] * 64;
  const int np = (n + 63) / 64 * 64;
  for (int i = threadIdx.x; i < np; i += 256) {
    const bool in = i < n;
    colsp[o + i] = in ? cols[p0 + i] : -1;
    wp[o + i] = in ? (weights ? weights[p0 + i] : 1.f) : 0.f;
  }
  if (threadIdx.x == 0) srec[g0 + g] = make_int2(f.boff[g], n);
}

// a thread per (row, set): every set of the call is empty
__global__ __launch_bounds__(256) void set_zero_kernel(int64_t B, int G, int64_t ld, double* __restrict__ mean,
                                                       double* __restrict__ sd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * G) return;
  const size_t o = (size_t)(i / G) * ld + (size_t)(i % G);
  mean[o] = 0.0;
  if (sd) sd[o] = 0.0;
}

// grid (ceil(B / 64), sets of the launch); set g0 + blockIdx.y.  CP: the padded columns of Vc / phic / ctc / wp.
template <int KC, int LIK>
__global__ __launch_bounds__(256) void set_kernel(int64_t B, int CP, int KP, int S, int g0, const float* __restrict__ z,
                                                  const float* __restrict__ Vc, const float* __restrict__ phic,
                                                  const uint8_t* __restrict__ ctc, const float* __restrict__ wp,
                                                  const int2* __restrict__ srec, int64_t ld,
                                                  double* __restrict__ mean, double* __restrict__ sd) {
  constexpr int SC = kSetDrawChunk;
  constexpr int NA = SC * 64 / 256;        // (draw, row) accumulators per thread
  __shared__ float tiles[2][2][64][KC + 4];
  __shared__ double stage[2][SC][64];      // [wave column][draw of the chunk][row]
  __shared__ double fold[SC][64];          // a chunk's score_s per (draw, row)
  const int t = threadIdx.x;
  const int lane = t & 63, h = lane >> 5, i32 = lane & 31;
  const int wr = t >> 7, wc = t >> 6 & 1;
  const int g = g0 + blockIdx.y;
  const int64_t b0 = (int64_t)blockIdx.x * 64;
  const int2 rec = srec[g];                // (first block, columns): the same for every thread
  const int n = rec.y;
  const int nblk = (n + 63) / 64;
  const bool k4 = i32 & 16, k3 = i32 & 8, k2 = i32 & 4, k1 = i32 & 2;

  double sum = 0.0, mu = 0.0, q = 0.0;     // threads 0 .. 63: row b0 + t
  for (int s0 = 0; s0 < S; s0 += SC) {
    const int sc = S - s0 < SC ? S - s0 : SC;
    double a[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) a[i] = 0.0;
    for (int cb = 0; cb < nblk; ++cb) {
      const int d0 = (rec.x + cb) * 64;
      const int d = score_tile_col(d0);
      const bool bern = score_col_bern<LIK>(ctc, CP, d);
      const bool in = cb * 64 + wc * 32 + i32 < n;
      const double w = (double)wp[d];
      score_tile_loop<KC>(tiles, B, CP, KP, sc, b0, d0, z + (size_t)s0 * B * KP, Vc + (size_t)s0 * CP * KP,
                          phic + (size_t)s0 * CP, [&](int s, const score_f32x16& acc, float ph) {
        double v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float ey;
          const float ms = cell_mean(bern, cell_rate(LIK, acc[r], ph, ey));
          v[r] = in ? w * (double)ms : 0.0;
        }
        // the 32 columns of the wave half: lane bit 4 keeps rows 8 k4 .., bit 3 rows 4 k3 .. of those, ...
        double u8[8], u4[4], u2[2];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const double got = __shfl_xor(k4 ? v[r] : v[r + 8], 16);
          u8[r] = (k4 ? v[r + 8] : v[r]) + got;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double got = __shfl_xor(k3 ? u8[r] : u8[r + 4], 8);
          u4[r] = (k3 ? u8[r + 4] : u8[r]) + got;
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const double got = __shfl_xor(k2 ? u4[r] : u4[r + 2], 4);
          u2[r] = (k2 ? u4[r + 2] : u4[r]) + got;
        }
        const double got = __shfl_xor(k1 ? u2[0] : u2[1], 2);
        double u1 = (k1 ? u2[1] : u2[0]) + got;
        u1 += __shfl_xor(u1, 1);           // the same bits in both lanes
        // accumulator row i32 >> 1 of the lane half
        if (!(i32 & 1)) stage[wc][s][score_tile_row(wr, i32 >> 1, h)] = u1;
      });
      // (the loop's last barrier is behind the last callback; the next loop's first one is behind these reads)
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int idx = t + 256 * i;
        const int sl = idx >> 6, row = idx & 63;
        if (sl >= sc) continue;
        a[i] += stage[0][sl][row] + stage[1][sl][row];
      }
    }
    // the chunk's scores to the 64 row threads (the barrier in front: the row threads may still read the last
    // chunk's)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int idx = t + 256 * i;
      fold[idx >> 6][idx & 63] = a[i];
    }
    __syncthreads();
    if (t < 64) {
      for (int sl = 0; sl < sc; ++sl) {
        double x = fold[sl][t];
        if (!(fabs(x) <= 1.7976931348623157e308)) x = __builtin_nan("");   // a non-finite cell: NaN for good
        sum += x;
        const double dl = x - mu;
        mu += dl / (double)(s0 + sl + 1);
        q = fma(dl, x - mu, q);
      }
    }
  }
  if (t >= 64 || b0 + t >= B) return;
  const size_t o = (size_t)(b0 + t) * ld + g;
  mean[o] = sum / (double)S;
  if (sd) sd[o] = sqrt(q / (double)(S - 1));
}

bool launch_sets(const SetArgs& a, hipStream_t st) {
  DrawTables t = a.t;
  const int G = a.n_sets;
  if (!with_kc(t.KP, [](auto) {}) || !with_lik(t.lik, [](auto) {})) return false;
  if (t.B <= 0 || G <= 0) return true;
  if (a.padded_cols <= 0) {
    const int64_t n = t.B * G;
    hipLaunchKernelGGL(set_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t.B, G, a.ld, a.mean,
                       a.sd);
    return true;
  }
  const int CP = (int)a.padded_cols;
  int64_t blocks = 0;
  for (int g0 = 0; g0 < G; g0 += kSetFillChunk) {
    const int ng = G - g0 < kSetFillChunk ? G - g0 : kSetFillChunk;
    SetFill f{};
    for (int i = 0; i <= ng; ++i) {
      f.ptr[i] = a.set_ptr[g0 + i];
      f.boff[i] = (int32_t)blocks;
      if (i < ng) blocks += (a.set_ptr[g0 + i + 1] - a.set_ptr[g0 + i] + 63) / 64;
    }
    hipLaunchKernelGGL(set_fill_kernel, dim3((unsigned)ng), dim3(256), 0, st, f, g0, a.cols, a.weights, a.colsp,
                       a.wp, a.srec);
  }
  uint8_t* ctc = t.lik == 3 ? a.ctc : nullptr;
  launch_panel_gather(t, CP, a.colsp, a.Vc, a.phic, ctc, st);
  const unsigned gx = (unsigned)((t.B + 63) / 64);
  for (int g0 = 0; g0 < G; g0 += 65535) {
    const int ng = G - g0 < 65535 ? G - g0 : 65535;
    with_kc(t.KP, [&](auto kc) {
      with_lik(t.lik, [&](auto lik) {
        hipLaunchKernelGGL((set_kernel<decltype(kc)::value, decltype(lik)::value>), dim3(gx, (unsigned)ng), dim3(256),
                           0, st, t.B, CP, t.KP, t.S, g0, t.z, a.Vc, a.phic, ctc, a.wp, a.srec, a.ld, a.mean, a.sd);
      });
    });
  }
  return true;
}

}  // namespace spmf
