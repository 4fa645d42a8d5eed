// rank.hip -- rank_cells: where a list of (held-out) cells lands among its row's candidates, without a
// [B,D] array.
//
// Score, order and candidates are those of topk.hip: score_bd = the fp32 mean over the draws of the rate
// (Poisson column) or sigmoid(logit) (Bernoulli column), formed by score_block (score_block.h, which also holds
// the slice geometry and the bitmap lookup of the two kernels); (score descending, column
// ascending); a candidate of row b is a column with a finite score that the batch does not store (when stored
// cells are excluded).  For a listed cell i = (b, d):
//   score_i = score_bd, with the bits the select kernel gives that cell,
//   cand_i  = the candidates d' != d of row b,
//   rank_i  = those of them that precede (b, d); -1 when score_i is not finite.
//
// Launches over the per-draw tables z[S,B,KP] (encode sweep), V'[S,D,KP], phi[S,D] (prep):
//   topk_mark_kernel (topk.hip) : the bitmap of the stored cells.
//   rank_init_kernel : rank 0 / candidates 0 of every listed cell; a cell outside [0,B) x [0,D), which no
//     workgroup serves, gets its final rank -1 / 0 candidates / score NaN here.
//   rank_kernel      : a workgroup owns 64 rows and a slice of the 64-column blocks (grid: row blocks x column
//     slices, api_stream.hip topk_slices).  The list is sorted by row: 65 binary searches over cell_row, bounded to
//     [0, n_cells), give the segment of each of the 64 rows.  A round takes the next T = kRankMaxPerRow listed
//     cells of every row into an LDS table (column, score); a row with more is served by further rounds of the
//     same workgroup, each round complete in itself, so the result does not depend on the rounds.
//     Phase 1 -- the targets' own scores.  Every column block that holds a listed cell of the round is scored
//       with score_block (all blocks of the row, not only the slice's: every slice needs every target of its
//       rows and forms the same bits), the 64 x 64 scores go through LDS, and the thread of a table slot picks
//       its cell's score.  Slice 0 writes score_out, takes a cell that is itself a candidate out of its own
//       candidate count and sets rank -1 for a non-finite score.
//     Phase 2 -- counting.  The slice's blocks are scored again and go through LDS in the same way.  A wave
//       then owns 16 rows of the block; its 64 lanes hold the 64 cells of one row at a time.  For table slot j
//       of the row the lanes compare their cell with the target (an 8-byte LDS broadcast), one ballot +
//       popcount counts the candidates that precede it, lane j keeps the count and adds it to the slot's LDS
//       counter behind the loop (the row is the wave's alone: a plain add).  The row's candidates are counted
//       by one more ballot.  A slot whose cell has no finite score holds (+inf, column), which no finite score
//       precedes.  Behind the slice's last block every slot adds its two counts to rank_out / cand_out with
//       plain vector integer atomics (several slices, several rounds): only integer adds anywhere, so the
//       result does not depend on any order.
//   A target's score is compared with scores formed by the same function on the same operands, so
//   precedes() is false for the cell itself and exact at ties: rank_i < k <=> column d is entry rank_i of
//   the select kernel's result.
//
// LDS (KC = 32): operand tiles 36 864 B, block scores 16 384 B, table 64 x 32 x 8 B = 16 384 B, slot counters
// 8 192 B, row segments and counts ~1.3 KiB: 79 376 B, two workgroups per CU.  Registers: DESIGN.md section 7e.
#include "common.h"
#include "kernels.h"
#include "score_block.h"

namespace spmf {

namespace {

constexpr int T = kRankMaxPerRow;
static_assert(T <= 64 && 64 * T % 256 == 0, "lane j of a wave keeps the count of table slot j");
constexpr int kSlotsPerThread = 64 * T / 256;

struct alignas(8) Target {
  float s;   // the listed cell's score once phase 1 has seen it; +inf: nothing precedes it
  int c;     // its column, -1: slot unused or cell switched off
};

}  // namespace

__global__ __launch_bounds__(256) void rank_init_kernel(int64_t n_cells, int64_t B, int D,
                                                        const int32_t* __restrict__ cell_row,
                                                        const int32_t* __restrict__ cell_col,
                                                        int32_t* __restrict__ rank, int32_t* __restrict__ cand,
                                                        float* __restrict__ score) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += step) {
    const int b = cell_row[i], d = cell_col[i];
    const bool ok = b >= 0 && (int64_t)b < B && d >= 0 && d < D;
    rank[i] = ok ? 0 : -1;
    cand[i] = 0;
    score[i] = __int_as_float(0x7fc00000);   // (a served cell's score is written by its workgroup of slice 0)
  }
}

template <int KC, int LIK>
__global__ __launch_bounds__(256) void rank_kernel(int64_t B, int D, int KP, int S, int cb_per_slice, int W,
                                                   const float* __restrict__ z, const float* __restrict__ Vp,
                                                   const float* __restrict__ phi, const uint8_t* __restrict__ ctype,
                                                   const uint32_t* __restrict__ stored, int64_t n_cells,
                                                   const int32_t* __restrict__ cell_row,
                                                   const int32_t* __restrict__ cell_col, int32_t* __restrict__ rank_out,
                                                   int32_t* __restrict__ cand_out, float* __restrict__ score_out) {
  __shared__ float tiles[2][2][64][KC + 4];
  __shared__ float bs[64][64];          // phase 1: the scores of one block
  __shared__ Target tg[64][T];
  __shared__ int64_t rstart[65];        // first listed cell of row b0 + t (t = 64: one past the block's last)
  __shared__ int nrow[64];              // listed cells of the row
  __shared__ int ntr[64];               // ... of them in this round
  __shared__ int cnt[64][T];            // the slice's candidates that precede the slot's cell
  __shared__ int rowcand[64];           // the slice's candidates of the row
  __shared__ int nmax;
  const int t = threadIdx.x;
  const int lane = t & 63, wv = t >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int wr = wv >> 1, wc = wv & 1;
  const int64_t b0 = (int64_t)blockIdx.x * 64;
  const int CB = (D + 63) / 64;
  int cb0, cb1;
  slice_blocks(D, cb_per_slice, cb0, cb1);
  const float inv_s = 1.f / (float)S;
  const bool first_slice = blockIdx.y == 0;

  // ---- the rows' segments of the list: lower bounds inside [0, n_cells), whatever the list holds
  if (t == 0) nmax = 0;
  if (t < 65) {
    const int64_t key = b0 + t < B ? b0 + t : B;
    int64_t lo = 0, hi = n_cells;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if ((int64_t)cell_row[mid] < key) lo = mid + 1; else hi = mid;
    }
    rstart[t] = lo;
  }
  __syncthreads();
  if (t < 64) {
    const int64_t n = rstart[t + 1] - rstart[t];     // (negative only on an unsorted list)
    const int nn = n < 0 ? 0 : (n > 0x7fffffff ? 0x7fffffff : (int)n);
    nrow[t] = nn;
    if (nn > 0) atomicMax(&nmax, nn);
  }
  __syncthreads();
  const int rounds = nmax / T + (nmax % T != 0);

  for (int q = 0; q < rounds; ++q) {
    // ---- the round's table: slot (rl, j) = listed cell q T + j of row rl
#pragma unroll
    for (int i = 0; i < kSlotsPerThread; ++i) {
      const int slot = t + 256 * i;
      const int rl = slot / T, j = slot % T;
      const int64_t left = (int64_t)nrow[rl] - (int64_t)q * T;
      const int n = left < 0 ? 0 : (left > T ? T : (int)left);
      int c = -1;
      if (j < n) {
        const int64_t idx = rstart[rl] + (int64_t)q * T + j;     // in [0, n_cells): idx < rstart[rl] + nrow[rl]
        const int d = cell_col[idx];
        if ((int64_t)cell_row[idx] == b0 + rl && b0 + rl < B && d >= 0 && d < D) c = d;
      }
      tg[rl][j].s = INFINITY;
      tg[rl][j].c = c;
      cnt[rl][j] = 0;
      if (j == 0) {
        ntr[rl] = n;
        rowcand[rl] = 0;
      }
    }
    __syncthreads();

    // ---- phase 1: the listed cells' own scores
    for (int cb = 0; cb < CB; ++cb) {
      int any = 0;
#pragma unroll
      for (int i = 0; i < kSlotsPerThread; ++i) {
        const int slot = t + 256 * i;
        const int c = tg[slot / T][slot % T].c;
        any |= (c >= 0 && (c >> 6) == cb) ? 1 : 0;
      }
      if (!__syncthreads_or(any)) continue;
      float sc[16];
      score_block<KC, LIK>(tiles, B, D, KP, S, b0, cb * 64, z, Vp, phi, ctype, inv_s, sc);
#pragma unroll
      for (int r = 0; r < 16; ++r) bs[score_tile_row(wr, r, h)][wc * 32 + i32] = sc[r];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kSlotsPerThread; ++i) {
        const int slot = t + 256 * i;
        const int rl = slot / T, j = slot % T;
        const int c = tg[rl][j].c;
        if (c >= 0 && (c >> 6) == cb) {
          const float v = bs[rl][c & 63];
          const bool fin = isfinite(v);
          if (fin) tg[rl][j].s = v;
          if (first_slice) {
            const int64_t idx = rstart[rl] + (int64_t)q * T + j;
            score_out[idx] = v;
            if (!fin) {
              atomicAdd(&rank_out[idx], -1);
            } else if (not_stored(stored, W, b0 + rl, c)) {
              atomicAdd(&cand_out[idx], -1);     // a candidate itself: not among the candidates beside it
            }
          }
        }
      }
      // (bs is written again only behind the barriers of the next score_block)
    }
    __syncthreads();

    // ---- phase 2: count, per listed cell, the slice's candidates that precede it
    for (int cb = cb0; cb < cb1; ++cb) {
      const int d0 = cb * 64;
      float sc[16];
      score_block<KC, LIK>(tiles, B, D, KP, S, b0, d0, z, Vp, phi, ctype, inv_s, sc);
#pragma unroll
      for (int r = 0; r < 16; ++r) bs[score_tile_row(wr, r, h)][wc * 32 + i32] = sc[r];
      __syncthreads();
      // wave wv counts for rows 16 wv .. 16 wv + 15: its 64 lanes hold the 64 cells of one row of the block
      const int d = d0 + lane;
      for (int i = 0; i < 16; ++i) {
        const int rl = wv * 16 + i;
        const int n = ntr[rl];                       // (wave-uniform)
        const int64_t b = b0 + rl;
        const float v = bs[rl][lane];
        const bool is_cand = b < B && d < D && isfinite(v) && not_stored(stored, W, b, d);
        const int pc = __popcll(__ballot(is_cand));
        if (pc == 0) continue;
        if (lane == 0) rowcand[rl] += pc;
        int mine = 0;
        for (int j = 0; j < n; ++j) {
          const Target th = tg[rl][j];
          const int pj = __popcll(__ballot(is_cand && score_precedes(v, d, th.s, th.c)));
          mine = lane == j ? pj : mine;
        }
        if (lane < n && mine) cnt[rl][lane] += mine;
      }
      // (bs is written again only behind the barriers of the next score_block)
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kSlotsPerThread; ++i) {
      const int slot = t + 256 * i;
      const int rl = slot / T, j = slot % T;
      if (tg[rl][j].c >= 0) {
        const int64_t idx = rstart[rl] + (int64_t)q * T + j;
        const int before = cnt[rl][j], n = rowcand[rl];    // (before != 0 only for a finite score)
        if (before) atomicAdd(&rank_out[idx], before);
        if (n) atomicAdd(&cand_out[idx], n);
      }
    }
    __syncthreads();   // the next round rewrites the table
  }
}

bool launch_rank(const RankArgs& a, hipStream_t st) {
  const DrawTables& t = a.t;
  if (a.n_cells < 1 || t.B < 1 || a.slices < 1 || a.slices > kTopkMaxSlices) return false;
  const SliceGeom g(t.D, a.slices);
  if (a.slices > g.CB) return false;
  bool ok = false;
  with_kc(t.KP, [&](auto kc) {
    ok = with_lik(t.lik, [&](auto lik) {
      if (a.stored && a.nnz > 0) launch_topk_mark(t.B, t.D, a.row_ptr, a.col, a.stored, st);
      const int64_t want = (a.n_cells + 255) / 256;
      hipLaunchKernelGGL(rank_init_kernel, dim3((unsigned)(want > 4096 ? 4096 : want)), dim3(256), 0, st, a.n_cells,
                         t.B, t.D, a.cell_row, a.cell_col, a.rank, a.cand, a.score);
      hipLaunchKernelGGL((rank_kernel<decltype(kc)::value, decltype(lik)::value>), g.grid(t.B), dim3(256), 0, st, t.B,
                         t.D, t.KP, t.S, g.per, g.W, t.z, t.Vp, t.phi, t.ctype, a.stored, a.n_cells, a.cell_row,
                         a.cell_col, a.rank, a.cand, a.score);
    });
  });
  return ok;
}

}  // namespace spmf
