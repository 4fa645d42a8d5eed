// score_block.h -- the 64-row x 64-column block of <z_sb, V'_sd> over the draws, as every streaming consumer
// forms it: waic.hip (statistics of ll_s), topk.hip and rank.hip (scores), knn.hip (scores of one "draw").
//
// A workgroup of 256 threads = four waves; wave (wr, wc) forms the 32 x 32 tile of rows 32 wr .. and columns
// 32 wc .. of the block on the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32, the accumulator layout of
// dense.hip).  score_tile_loop is the one loop: operand tiles double-buffered in LDS over (draw, K chunk), the
// tiles of the next (draw, chunk) fetched to registers while the current one is multiplied, and a callback per
// draw that takes the 16 dot products of the lane.  score_block is the loop with
//   score_bd = (1/S) sum_s m_s,   m_s = rate_s (Poisson column) | sigmoid(logit_s) (Bernoulli column)
// as its callback, rate_s / logit_s = cell_rate(<z_sb, V'_sd>, phi_sd), m_s added in draw order.  Every consumer
// includes these functions, so a cell's dot products -- and its score -- have the same bits in each: the sums of
// a lane do not depend on which block, slice, launch or kernel they are formed in.
//
// Also here, for the kernels that sweep the column blocks of a slice (topk.hip, rank.hip, knn.hip): the slice
// geometry and the lookup in the bitmap of the stored cells.
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
// the calling lane's column of the block at d0: 32 wc + (lane & 31), wc = the wave's column of the block
__device__ __forceinline__ int score_tile_col(int d0) { return d0 + (threadIdx.x >> 6 & 1) * 32 + (threadIdx.x & 31); }

// 8 floats of K: ar / br are the lane's row of the A / B tile at float 4 h of them, h = lane >> 5.  Lane half h
// takes k = 4 h + e, e = 0 .. 3, for both operands: the pairing of the k values inside a step is free as long
// as A and B agree.
__device__ __forceinline__ void score_mfma8(const float* ar, const float* br, score_f32x16& acc) {
  const float4 a = *reinterpret_cast<const float4*>(ar);
  const float4 b = *reinterpret_cast<const float4*>(br);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
}

// KC: floats of the K axis per LDS tile (8, 16, 32); KP > KC runs KP / KC chunks per draw.  tiles: the
// workgroup's [2][2][64][KC + 4] floats of LDS.  Every thread of the workgroup calls it (barriers inside; the
// last one releases both buffers).  Behind the last chunk of draw s: on_draw(s, acc, ph), acc[r] = <z_sb, V'_sd>
// of row b0 + score_tile_row(wr, r, h), column d = score_tile_col(d0), ph = phi_sd; rows >= B and
// columns >= D read zeros and carry no meaning.
template <int KC, class OnDraw>
__device__ __forceinline__ void score_tile_loop(float (*tiles)[2][64][KC + 4], int64_t B, int D, int KP, int S, int64_t b0,
                                                int d0, const float* __restrict__ z, const float* __restrict__ Vp,
                                                const float* __restrict__ phi, OnDraw on_draw) {
  constexpr int NLD = KC / 8;          // float4 per thread and (draw, chunk): 2 tiles x 64 rows x KC floats
  constexpr int TQ = 16 * KC;          // float4 per tile
  const int t = threadIdx.x;
  const int lane = t & 63, wv = t >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int wr = wv >> 1, wc = wv & 1;
  const int NCH = KP > KC ? KP / KC : 1;
  const int NIT = S * NCH;
  const int d = score_tile_col(d0);

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
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
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
    const float* ar = &tiles[buf][0][wr * 32 + i32][4 * h];
    const float* br = &tiles[buf][1][wc * 32 + i32][4 * h];
#pragma unroll
    for (int qk = 0; qk < KC / 8; ++qk) score_mfma8(ar + 8 * qk, br + 8 * qk, acc);
    if (ch == NCH - 1) {
      on_draw(s, acc, ph);
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
    if (it + 1 < NIT) stash(buf ^ 1, pre);
    __syncthreads();
  }
}

// column d is a Bernoulli one under likelihood code LIK (no type behind D)
template <int LIK>
__device__ __forceinline__ bool score_col_bern(const uint8_t* __restrict__ ctype, int D, int d) {
  return lik_bern(LIK) || (LIK == 3 && d < D && cell_is_bern(LIK, ctype, d));
}

// score_tile_loop's arguments and barrier contract.  sc[r]: the score of row b0 + score_tile_row(wr, r, h),
// column score_tile_col(d0).
template <int KC, int LIK>
__device__ __forceinline__ void score_block(float (*tiles)[2][64][KC + 4], int64_t B, int D, int KP, int S, int64_t b0,
                                            int d0, const float* __restrict__ z, const float* __restrict__ Vp,
                                            const float* __restrict__ phi, const uint8_t* __restrict__ ctype,
                                            float inv_s, float (&sc)[16]) {
  const bool bern = score_col_bern<LIK>(ctype, D, score_tile_col(d0));
#pragma unroll
  for (int r = 0; r < 16; ++r) sc[r] = 0.f;
  score_tile_loop<KC>(tiles, B, D, KP, S, b0, d0, z, Vp, phi, [&](int, const score_f32x16& acc, float ph) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float ey;
      sc[r] += cell_mean(bern, cell_rate(LIK, acc[r], ph, ey));
    }
  });
#pragma unroll
  for (int r = 0; r < 16; ++r) sc[r] *= inv_s;
}

// ---- a sweep over the 64-column blocks of D columns (or reference rows), split over gridDim.y slices -------
struct SliceGeom {
  int slices, CB, per, W;   // gridDim.y (>= 1), column blocks, blocks per slice, 32-bit words of a bitmap row
  SliceGeom(int64_t D, int slices_)
      : slices(slices_), CB((int)((D + 63) / 64)), per((CB + slices - 1) / slices), W((int)((D + 31) / 32)) {}
  dim3 grid(int64_t rows) const { return dim3((unsigned)((rows + 63) / 64), (unsigned)slices); }
};

// the blocks [cb0, cb1) of the workgroup's slice (blockIdx.y), per = SliceGeom.per
template <class Int>   // of D: int64_t where D + 63 may not fit an int
__device__ __forceinline__ void slice_blocks(Int D, int per, int& cb0, int& cb1) {
  const int CB = (int)((D + 63) / 64);
  cb0 = blockIdx.y * per;
  cb1 = cb0 + per < CB ? cb0 + per : CB;
}

// cell (b, d) is not marked in the bitmap stored[rows][W] (topk_mark_kernel); no bitmap: nothing is stored
__device__ __forceinline__ bool not_stored(const uint32_t* __restrict__ stored, int W, int64_t b, int d) {
  return !stored || !((stored[(size_t)b * W + (d >> 5)] >> (d & 31)) & 1u);
}

}  // namespace spmf
