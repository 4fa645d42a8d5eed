// topk.hip -- streaming per-row top-k of the posterior predictive mean, without a [B,D] array.
//
// The score of a cell (b, d) over the draws s = 0 .. S-1 is
//   score_bd = (1/S) sum_s m_s,   m_s = rate_s (Poisson column) | sigmoid(logit_s) (Bernoulli column)
// with rate_s / logit_s = cell_rate(<z_sb, V'_sd>, phi_sd) exactly as dense_ll.hip and waic.hip form it.
// Per row the k candidates with the largest score leave the kernel, ordered by (score descending,
// column ascending); a candidate is a cell with a finite score that is not stored in the batch (when
// stored cells are excluded).  Missing candidates are padded with column -1 / score -inf.
//
// Launches over the per-draw tables z[S,B,KP] (encode sweep), V'[S,D,KP], phi[S,D] (prep):
//   topk_mark_kernel   : (stored cells excluded) one wave per row ORs a bit per CSR entry into a zeroed
//     bitmap [B][ceil(D/32)]: CSR columns are not sorted inside a row, so a block of cells cannot find
//     its stored entries by search.
//   topk_select_kernel : a workgroup owns 64 rows and sweeps the 64-column blocks of its slice.  Per block the
//     scores are formed by score_block (score_block.h: the tile loop that waic.hip, rank.hip and knn.hip run
//     too): 32 x 32 wave tiles of <z, V'> on the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32),
//     double-buffered LDS operand tiles over (draw, K chunk), m_s added in draw order to 16 sums per lane.  Selection
//     (select_rows.h, shared with knn.hip): per row a threshold and a buffer of CAP candidates in LDS; a cell
//     that beats its row's threshold -- and only such a cell looks up its bit -- is appended, a full row is
//     compacted to its best k by rank: the exact top k whatever the order of the appends, bit-reproducible.
//     After the first blocks a cell beats the threshold with probability ~ k / (columns seen).
//   topk_merge_kernel  : with few row blocks the columns are split over gridDim.y slices (api_stream.hip
//     topk_slices), each writing its k per row; one wave per row ranks the slices' candidates.
//
// LDS and occupancy (160 KiB per CU): operand tiles 2 x 2 x 64 x (KC+4) floats = 36 864 B at KC = 32,
// thresholds and counters 768 B, candidates 64 x CAP x 8 B.  CAP = 32 (k <= 16): 54 272 B with alignment,
// CAP = 80 (k <= 64): 78 848 B: two workgroups fit at the widest buffer, three at the narrow one.  The
// registers set the occupancy reached: 171 .. 220 VGPRs + 16 AGPRs at KC = 32, no spills, which is two
// waves per SIMD = two workgroups (8 waves) per CU for every k (three at KC = 8 / 16, k <= 16 on the Poisson
// and mixed codes).
// All arithmetic is fp32 FMA.
#include "common.h"
#include "kernels.h"
#include "score_block.h"
#include "select_rows.h"

namespace spmf {

// one wave per row: a bit per stored cell
__global__ __launch_bounds__(256) void topk_mark_kernel(int64_t B, int D, int W, const int32_t* __restrict__ row_ptr,
                                                        const int32_t* __restrict__ col, uint32_t* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t b = wave; b < B; b += nwaves) {
    const int start = row_ptr[b], end = row_ptr[b + 1];
    for (int i = start + lane; i < end; i += 64) {
      const int d = col[i];
      if ((unsigned)d < (unsigned)D) atomicOr(&bits[(size_t)b * W + (d >> 5)], 1u << (d & 31));
    }
  }
}

// KC: floats of the K axis per LDS tile (8, 16, 32); KP > KC runs KP / KC chunks per draw.  CAP: candidates
// buffered per row (k <= CAP - 16).  Grid (row blocks, column slices); slice y writes cols / scores [y][B][k].
template <int KC, int LIK, int CAP>
__global__ __launch_bounds__(256) void topk_select_kernel(int64_t B, int D, int KP, int S, int k, int cb_per_slice, int W,
                                                          const float* __restrict__ z, const float* __restrict__ Vp,
                                                          const float* __restrict__ phi,
                                                          const uint8_t* __restrict__ ctype,
                                                          const uint32_t* __restrict__ stored,
                                                          int32_t* __restrict__ cols, float* __restrict__ scores) {
  __shared__ float tiles[2][2][64][KC + 4];
  SPMF_SELECT_ROWS_LDS(CAP, sel);
  const int64_t b0 = (int64_t)blockIdx.x * 64;
  int cb0, cb1;
  slice_blocks(D, cb_per_slice, cb0, cb1);
  const float inv_s = 1.f / (float)S;
  // only a cell that beats its row's threshold looks up its bit
  const auto cand = [=](int64_t b, int d) { return not_stored(stored, W, b, d); };
  select_begin(sel);
  for (int cb = cb0; cb < cb1; ++cb) {
    const int d0 = cb * 64;
    float sc[16];
    score_block<KC, LIK>(tiles, B, D, KP, S, b0, d0, z, Vp, phi, ctype, inv_s, sc);
    select_block(sel, sc, B, D, b0, d0, k, cand);
  }
  select_end(sel, B, b0, k, (int)blockIdx.y, cols, scores);
}

constexpr int kMergeMax = kTopkMaxSlices * kTopkMaxK;

// one wave per row: the best k of the slices' candidates pc / ps [nsl][B][k] (padding: column -1)
__global__ __launch_bounds__(64) void topk_merge_kernel(int64_t B, int k, int nsl, const int32_t* __restrict__ pc,
                                                        const float* __restrict__ ps, int32_t* __restrict__ cols,
                                                        float* __restrict__ scores) {
  __shared__ float s[kMergeMax];
  __shared__ int c[kMergeMax];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int n = nsl * k;
  for (int i = lane; i < n; i += 64) {
    const size_t o = ((size_t)(i / k) * B + b) * k + (i % k);
    c[i] = pc[o];
    s[i] = ps[o];
  }
  __syncthreads();
  int nv = 0;
  for (int i = lane; i < n; i += 64) {
    const int ci = c[i];
    if (ci < 0) continue;
    const float si = s[i];
    ++nv;
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (c[j] >= 0 && score_precedes(s[j], c[j], si, ci)) ? 1 : 0;
    if (rank < k) {
      cols[(size_t)b * k + rank] = ci;
      scores[(size_t)b * k + rank] = si;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) nv += __shfl_xor(nv, m);
  if (lane < k && lane >= nv) {
    cols[(size_t)b * k + lane] = -1;
    scores[(size_t)b * k + lane] = -INFINITY;
  }
}

template <int KC, int LIK, int CAP>
static void launch_select(const TopkArgs& a, const SliceGeom& g, int32_t* cols, float* scores, hipStream_t st) {
  const DrawTables& t = a.t;
  hipLaunchKernelGGL((topk_select_kernel<KC, LIK, CAP>), g.grid(t.B), dim3(256), 0, st, t.B, t.D, t.KP, t.S, a.k, g.per,
                     g.W, t.z, t.Vp, t.phi, t.ctype, a.stored, cols, scores);
}

void launch_topk_mark(int64_t B, int D, const int32_t* row_ptr, const int32_t* col, uint32_t* bits, hipStream_t st) {
  const int64_t want = (B + 3) / 4;
  const int nb = (int)(want < 1 ? 1 : (want > 4096 ? 4096 : want));
  hipLaunchKernelGGL(topk_mark_kernel, dim3(nb), dim3(256), 0, st, B, D, SliceGeom(D, 1).W, row_ptr, col, bits);
}

void launch_topk_merge(int64_t B, int k, int nsl, const int32_t* pc, const float* ps, int32_t* cols, float* scores,
                       hipStream_t st) {
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)B), dim3(64), 0, st, B, k, nsl, pc, ps, cols, scores);
}

bool launch_topk(const TopkArgs& a, hipStream_t st) {
  const DrawTables& t = a.t;
  if (a.k < 1 || a.k > kTopkMaxK || a.slices < 1 || a.slices > kTopkMaxSlices) return false;
  const SliceGeom g(t.D, a.slices);
  if (a.slices > g.CB) return false;
  int32_t* cols = a.slices > 1 ? a.part_cols : a.cols;
  float* scores = a.slices > 1 ? a.part_scores : a.scores;
  bool ok = false;
  with_kc(t.KP, [&](auto kc) {
    ok = with_lik(t.lik, [&](auto lik) {
      constexpr int KC = decltype(kc)::value, LIK = decltype(lik)::value;
      if (a.stored && a.nnz > 0) launch_topk_mark(t.B, t.D, a.row_ptr, a.col, a.stored, st);
      if (a.k <= 16) launch_select<KC, LIK, 32>(a, g, cols, scores, st);
      else launch_select<KC, LIK, 80>(a, g, cols, scores, st);
      if (a.slices > 1) launch_topk_merge(t.B, a.k, a.slices, a.part_cols, a.part_scores, a.cols, a.scores, st);
    });
  });
  return ok;
}

}  // namespace spmf
