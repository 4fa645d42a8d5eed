// select_rows.h -- the exact best k per row of a stream of 64 x 64 score blocks, as topk.hip and knn.hip select.
//
// A workgroup of 256 threads owns 64 rows and feeds the blocks of score_block (score_block.h) one after the
// other.  LDS holds per row the k-th best candidate so far (score, column) and a buffer of CAP candidates.  A
// cell that beats its row's threshold -- and only such a cell asks the caller's "is a candidate" test -- is
// appended through an LDS counter; a row whose buffer is full is compacted to its best k by rank (every lane
// counts the entries that precede its own in the (score, column) order, which is strict since columns are
// distinct) and the threshold moves up.  Cells that found the buffer full try again behind the compaction if
// they still beat the new threshold.  What is dropped is never among the best k of what was seen, so the result
// is the exact best k under that order whatever the order of the appends: bit-reproducible.  Both consumers
// include these functions, so the selection of one is the selection of the other.  toprows.hip selects along the
// other axis of the block -- 64 columns as the keys, rows as the candidates -- with select_block_cols below and
// the same buffers, compaction, select_begin and select_end.
#pragma once
#include "common.h"
#include "score_block.h"

namespace spmf {

// The selection's LDS of one workgroup, CAP = 32 serves k <= 16, CAP = 80 serves k <= 64 (k <= CAP - 16): the
// kernel declares the five arrays (SPMF_SELECT_ROWS_LDS) and hands their addresses on.  (One __shared__ struct
// holding them cost topk_select_kernel 25 .. 70 VGPRs and an occupancy step at CAP = 80.)
template <int CAP>
struct SelectRows {
  float (*cand_s)[CAP];
  int (*cand_c)[CAP];
  float* thr_s;
  int* thr_c;
  int* cnt;
};

#define SPMF_SELECT_ROWS_LDS(CAP_, name_)                \
  __shared__ float name_##_cand_s[64][CAP_];             \
  __shared__ int name_##_cand_c[64][CAP_];               \
  __shared__ float name_##_thr_s[64];                    \
  __shared__ int name_##_thr_c[64];                      \
  __shared__ int name_##_cnt[64];                        \
  const SelectRows<CAP_> name_{name_##_cand_s, name_##_cand_c, name_##_thr_s, name_##_thr_c, name_##_cnt}

// One wave sorts the first n (<= CAP) candidates of a row by rank, keeps min(n, k) and, with k of them,
// sets the row's threshold to the k-th.  Every lane reads all entries before any lane writes one.
template <int CAP>
__device__ __forceinline__ void compact_row(float* cs, int* cc, int n, int k, int lane, int* cnt, float* ts, int* tc) {
  const bool h0 = lane < n, h1 = CAP > 64 && lane + 64 < n;
  const float s0 = h0 ? cs[lane] : 0.f, s1 = h1 ? cs[lane + 64] : 0.f;
  const int c0 = h0 ? cc[lane] : 0, c1 = h1 ? cc[lane + 64] : 0;
  int r0 = 0, r1 = 0;
  for (int j = 0; j < n; ++j) {
    const float sj = cs[j];
    const int cj = cc[j];
    r0 += score_precedes(sj, cj, s0, c0) ? 1 : 0;
    if (CAP > 64) r1 += score_precedes(sj, cj, s1, c1) ? 1 : 0;
  }
  __builtin_amdgcn_wave_barrier();
  if (h0 && r0 < k) {
    cs[r0] = s0;
    cc[r0] = c0;
    if (r0 == k - 1) {
      *ts = s0;
      *tc = c0;
    }
  }
  if (h1 && r1 < k) {
    cs[r1] = s1;
    cc[r1] = c1;
    if (r1 == k - 1) {
      *ts = s1;
      *tc = c1;
    }
  }
  if (lane == 0) *cnt = n < k ? n : k;
}

// before the first block (every thread; a barrier inside)
template <int CAP>
__device__ __forceinline__ void select_begin(const SelectRows<CAP> L) {
  const int t = threadIdx.x;
  if (t < 64) {
    L.thr_s[t] = -INFINITY;
    L.thr_c[t] = 0x7fffffff;
    L.cnt[t] = 0;
  }
  __syncthreads();
}

// The scores sc of the block at rows b0 .., columns d0 .. (score_block's layout) enter the selection.  A cell
// inside [0,B) x [0,D) with a finite score that beats its row's threshold is a candidate iff cand(b, d).  Every
// thread of the workgroup calls it (barriers inside).
template <int CAP, class Cand>
__device__ __forceinline__ void select_block(const SelectRows<CAP> L, const float (&sc)[16], int64_t B, int D, int64_t b0,
                                             int d0, int k, Cand cand) {
  const int t = threadIdx.x;
  const int lane = t & 63, wv = t >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int wr = wv >> 1, wc = wv & 1;
  const int d = d0 + wc * 32 + i32;
  // the lane's 16 cells are column d of 16 different rows
  unsigned pend = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rl = score_tile_row(wr, r, h);
    const int64_t b = b0 + rl;
    const float v = sc[r];
    bool in = b < B && d < D && isfinite(v) && score_precedes(v, d, L.thr_s[rl], L.thr_c[rl]);
    if (in) in = cand(b, d);
    pend |= in ? 1u << r : 0u;
  }
  while (true) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (pend >> r & 1u) {
        const int rl = score_tile_row(wr, r, h);
        const int slot = atomicAdd(&L.cnt[rl], 1);
        if (slot < CAP) {
          L.cand_s[rl][slot] = sc[r];
          L.cand_c[rl][slot] = d;
          pend &= ~(1u << r);
        }
      }
    }
    __syncthreads();
    for (int i = 0; i < 16; ++i) {        // wave wv keeps rows 16 wv .. 16 wv + 15
      const int rl = wv * 16 + i;
      const int n = L.cnt[rl];            // (wave-uniform)
      if (n >= CAP) compact_row<CAP>(L.cand_s[rl], L.cand_c[rl], CAP, k, lane, &L.cnt[rl], &L.thr_s[rl], &L.thr_c[rl]);
    }
    // a cell is still pending only where its row was full, and that row now has CAP - k free slots
    if (!__syncthreads_or(pend != 0)) break;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = score_tile_row(wr, r, h);
      if ((pend >> r & 1u) && !score_precedes(sc[r], d, L.thr_s[rl], L.thr_c[rl])) pend &= ~(1u << r);
    }
  }
}

// select_block with the axes exchanged (toprows.hip): the 64 keys of the workgroup are the COLUMNS d0 .. d0 + 63
// and the blocks it feeds are row blocks; the candidate id kept beside a score is the row, so the order is (score
// descending, row ascending), strict since the rows of a column are distinct.  The key of a lane's 16 cells is one
// column: its threshold is read once.  A cell inside [0,B) x [0,C) with a finite score that beats its column's
// threshold is a candidate iff cand(b, d).  Buffers, counters, compaction and select_begin / select_end are those
// of select_block, with "row" read as "key".  Every thread of the workgroup calls it (barriers inside).
template <int CAP, class Cand>
__device__ __forceinline__ void select_block_cols(const SelectRows<CAP> L, const float (&sc)[16], int64_t B, int C,
                                                  int64_t b0, int d0, int k, Cand cand) {
  const int t = threadIdx.x;
  const int lane = t & 63, wv = t >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int wr = wv >> 1, wc = wv & 1;
  const int cl = wc * 32 + i32;           // the lane's key
  const int d = d0 + cl;
  float ts = L.thr_s[cl];
  int tc = L.thr_c[cl];
  unsigned pend = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t b = b0 + score_tile_row(wr, r, h);
    const float v = sc[r];
    bool in = b < B && d < C && isfinite(v) && score_precedes(v, (int)b, ts, tc);
    if (in) in = cand(b, d);
    pend |= in ? 1u << r : 0u;
  }
  while (true) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (pend >> r & 1u) {
        const int slot = atomicAdd(&L.cnt[cl], 1);
        if (slot < CAP) {
          L.cand_s[cl][slot] = sc[r];
          L.cand_c[cl][slot] = (int)(b0 + score_tile_row(wr, r, h));
          pend &= ~(1u << r);
        }
      }
    }
    __syncthreads();
    for (int i = 0; i < 16; ++i) {        // wave wv keeps keys 16 wv .. 16 wv + 15
      const int kl = wv * 16 + i;
      const int n = L.cnt[kl];            // (wave-uniform)
      if (n >= CAP) compact_row<CAP>(L.cand_s[kl], L.cand_c[kl], CAP, k, lane, &L.cnt[kl], &L.thr_s[kl], &L.thr_c[kl]);
    }
    // a cell is still pending only where its column was full, and that column now has CAP - k free slots
    if (!__syncthreads_or(pend != 0)) break;
    ts = L.thr_s[cl];
    tc = L.thr_c[cl];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if ((pend >> r & 1u) && !score_precedes(sc[r], (int)(b0 + score_tile_row(wr, r, h)), ts, tc)) pend &= ~(1u << r);
    }
  }
}

// behind the last block: the rows' best k in order to cols / scores [slice][B][k], a row with fewer than k
// candidates padded with column -1 / score -inf (every thread; a barrier inside)
template <int CAP>
__device__ __forceinline__ void select_end(const SelectRows<CAP> L, int64_t B, int64_t b0, int k, int slice,
                                           int32_t* __restrict__ cols, float* __restrict__ scores) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int i = 0; i < 16; ++i) {
    const int rl = wv * 16 + i;
    const int n = L.cnt[rl];                // (< CAP: a full row was compacted where it filled up)
    if (n > 0) compact_row<CAP>(L.cand_s[rl], L.cand_c[rl], n, k, lane, &L.cnt[rl], &L.thr_s[rl], &L.thr_c[rl]);
  }
  __syncthreads();
  for (int i = 0; i < 16; ++i) {
    const int rl = wv * 16 + i;
    const int64_t b = b0 + rl;
    if (b < B && lane < k) {
      const bool have = lane < L.cnt[rl];
      const size_t o = ((size_t)slice * B + b) * k + lane;
      cols[o] = have ? L.cand_c[rl][lane] : -1;
      scores[o] = have ? L.cand_s[rl][lane] : -INFINITY;
    }
  }
}

}  // namespace spmf
