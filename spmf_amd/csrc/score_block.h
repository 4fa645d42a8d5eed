// score_block.h -- the scores of one 64-row x 64-column block, as topk.hip and rank.hip form them.
//
//   score_bd = (1/S) sum_s m_s,   m_s = rate_s (Poisson column) | sigmoid(logit_s) (Bernoulli column)
// with rate_s / logit_s = cell_rate(<z_sb, V'_sd>, phi_sd).  A workgroup of 256 threads = four waves; wave
// (wr, wc) forms the 32 x 32 tile of rows 32 wr .. and columns 32 wc .. of the block on the exact-f32 matrix
// cores (v_mfma_f32_32x32x2_f32), the operand tiles double-buffered in LDS over (draw, K chunk), m_s added in
// draw order.  Both consumers include this one function, so a cell's score has the same bits in either: the
// sums of a lane do not depend on which block, slice, launch or kernel they are formed in.
#pragma once
#include "common.h"

namespace spmf {

typedef float score_f32x16 __attribute__((ext_vector_type(16)));

// the order of the results: score descending, ties by ascending column
__device__ __forceinline__ bool score_precedes(float s, int c, float s2, int c2) {
  return s > s2 || (s == s2 && c < c2);
}

// row (inside the block) of accumulator r of a lane of wave row wr, lane half h = lane >> 5; its column is
// 32 wc + (lane & 31)
__device__ __forceinline__ int score_tile_row(int wr, int r, int h) { return wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * h; }

// KC: floats of the K axis per LDS tile (8, 16, 32); KP > KC runs KP / KC chunks per draw.  tiles: the
// workgroup's [2][2][64][KC + 4] floats of LDS.  Every thread of the workgroup calls it (barriers inside; the
// last one releases both buffers).  sc[r]: the score of row b0 + score_tile_row(wr, r, h), column
// d0 + 32 wc + (lane & 31); rows >= B and columns >= D read zeros and carry no meaning.
template <int KC, int LIK>
__device__ __forceinline__ void score_block(float (*tiles)[2][64][KC + 4], int64_t B, int D, int KP, int S, int64_t b0,
                                            int d0, const float* __restrict__ z, const float* __restrict__ Vp,
                                            const float* __restrict__ phi, const uint8_t* __restrict__ ctype,
                                            float inv_s, float (&sc)[16]) {
  constexpr int NLD = KC / 8;          // float4 per thread and (draw, chunk): 2 tiles x 64 rows x KC floats
  constexpr int TQ = 16 * KC;          // float4 per tile
  const int t = threadIdx.x;
  const int lane = t & 63, wv = t >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int wr = wv >> 1, wc = wv & 1;
  const int NCH = KP > KC ? KP / KC : 1;
  const int NIT = S * NCH;
  const int d = d0 + wc * 32 + i32;
  const bool bern = lik_bern(LIK) || (LIK == 3 && d < D && cell_is_bern(LIK, ctype, d));   // (no type behind D)

  auto fetch = [&](int it, float4* pre) {
    const int s = it / NCH, kc0 = (it % NCH) * KC;
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int idx = t + 256 * j;
      const int tile = idx / TQ, rem = idx % TQ;
      const int row = rem / (KC / 4), kk = kc0 + 4 * (rem % (KC / 4));
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kk < KP) {
        if (tile == 0) {
          if (b0 + row < B) v = *reinterpret_cast<const float4*>(z + ((size_t)s * B + b0 + row) * KP + kk);
        } else {
          if (d0 + row < D) v = *reinterpret_cast<const float4*>(Vp + ((size_t)s * D + d0 + row) * KP + kk);
        }
      }
      pre[j] = v;
    }
  };
  auto stash = [&](int buf, const float4* pre) {
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int idx = t + 256 * j;
      const int tile = idx / TQ, rem = idx % TQ;
      *reinterpret_cast<float4*>(&tiles[buf][tile][rem / (KC / 4)][4 * (rem % (KC / 4))]) = pre[j];
    }
  };

  score_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    sc[r] = 0.f;
    acc[r] = 0.f;
  }
  float4 pre[NLD];
  fetch(0, pre);
  stash(0, pre);   // (the last barrier of the block before released both buffers)
  __syncthreads();
  float ph = 0.f;
  for (int it = 0; it < NIT; ++it) {
    const int buf = it & 1;
    const int s = it / NCH, ch = it % NCH;
    if (it + 1 < NIT) fetch(it + 1, pre);
    if (ch == 0) ph = d < D ? phi[(size_t)s * D + d] : 0.f;
    // lane half h takes k = 8 q + 4 h + e of the chunk for both operands (waic.hip)
    const float* ar = &tiles[buf][0][wr * 32 + i32][4 * h];
    const float* br = &tiles[buf][1][wc * 32 + i32][4 * h];
#pragma unroll
    for (int qk = 0; qk < KC / 8; ++qk) {
      const float4 a = *reinterpret_cast<const float4*>(ar + 8 * qk);
      const float4 b = *reinterpret_cast<const float4*>(br + 8 * qk);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    }
    if (ch == NCH - 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float ey;
        sc[r] += cell_mean(bern, cell_rate(LIK, acc[r], ph, ey));
        acc[r] = 0.f;
      }
    }
    if (it + 1 < NIT) stash(buf ^ 1, pre);
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) sc[r] *= inv_s;
}

}  // namespace spmf
