// toprows.hip -- streaming per-column top-k rows of the posterior predictive mean, without a [B,C] array: the
// selection of topk.hip along the other axis of the 64 x 64 score block.
//
// The score of a cell (b, d) is topk.hip's and panel.hip's,
//   score_bd = (1/S) sum_s m_s,   m_s = rate_s (Poisson column) | sigmoid(logit_s) (Bernoulli column),
// formed by score_block (score_block.h) in the operand orientation of panel_kernel and topk_select_kernel: tile 0
// is 64 rows of z, tile 1 is 64 columns of V' -- of the compacted V' of a listed panel (panel_gather_kernel) --, so
// a cell has the bits that predict's 'mean' has.  Per listed column the k candidates with the largest score leave
// the kernel, ordered by (score descending, row ascending); a candidate is a cell with a finite score that is not
// stored in the batch (when stored cells are excluded).  Missing candidates are padded with row -1 / score -inf.
//
// Launches over the per-draw tables z[S,B,KP] (encode sweep), V'[S,D,KP], phi[S,D] (prep):
//   topk_mark_kernel      : (stored cells excluded) the bitmap [B][ceil(D/32)] of topk.hip, over the columns of
//     the tables: a listed column j looks up bit cols[j].
//   panel_gather_kernel   : a listed panel, compacted to C contiguous columns (panel.hip).
//   toprows_select_kernel : a workgroup owns 64 columns of the panel and sweeps the 64-row blocks of its row slice.
//     In score_block's layout a lane holds ONE column for 16 rows, so the key of the selection is lane-constant
//     and the candidate id is the row: select_block_cols (select_rows.h) is select_block with the axes exchanged,
//     on the same thresholds, buffers and rank compaction: the exact top k whatever the order of the appends,
//     bit-reproducible.  Only a cell that beats its column's threshold looks up its bit.
//   topk_merge_kernel     : with few column blocks the rows are split over gridDim.y slices (api_stream.hip
//     toprows_layout: topk_slices with the roles swapped), each writing its k per column; one wave per column
//     ranks the slices' candidates (topk.hip).  Rows are distinct across slices: the order stays strict.
//
// LDS and occupancy: topk.hip's budget (operand tiles 36 864 B at KC = 32, thresholds and counters 768 B,
// candidates 64 x CAP x 8 B: 54 272 B at CAP = 32 for k <= 16, 78 848 B at CAP = 80 for k <= 64).  Registers per
// instantiation: DESIGN.md 7j.
// All arithmetic is fp32 FMA; no atomics on global memory (the bitmap's integer OR is topk.hip's), no float
// atomics, nothing depends on arrival order.
#include "common.h"
#include "kernels.h"
#include "score_block.h"
#include "select_rows.h"

namespace spmf {

// KC, CAP: as topk_select_kernel.  C: the columns of the tables Vp / phi / ctype (the context's D, or the length
// of the compacted list).  Grid (column blocks, row slices); slice y writes rows / scores [y][C][k].  cols: the
// listed columns (null: column j is column j), W: the bitmap's words per row.
template <int KC, int LIK, int CAP>
__global__ __launch_bounds__(256) void toprows_select_kernel(int64_t B, int C, int KP, int S, int k, int rb_per_slice,
                                                             int W, const float* __restrict__ z,
                                                             const float* __restrict__ Vp,
                                                             const float* __restrict__ phi,
                                                             const uint8_t* __restrict__ ctype,
                                                             const uint32_t* __restrict__ stored,
                                                             const int32_t* __restrict__ cols,
                                                             int32_t* __restrict__ rows, float* __restrict__ scores) {
  __shared__ float tiles[2][2][64][KC + 4];
  SPMF_SELECT_ROWS_LDS(CAP, sel);
  const int d0 = blockIdx.x * 64;
  int rb0, rb1;
  slice_blocks(B, rb_per_slice, rb0, rb1);
  const float inv_s = 1.f / (float)S;
  // only a cell that beats its column's threshold looks up its bit.  (Its score is finite, so its column is one of
  // the tables': panel_gather_kernel makes any other NaN.  The comparison keeps the read inside the bitmap's row
  // whatever the list holds.)
  const auto cand = [=](int64_t b, int j) {
    const int dc = cols ? cols[j] : j;
    return (unsigned)(dc >> 5) < (unsigned)W && not_stored(stored, W, b, dc);
  };
  select_begin(sel);
  for (int rb = rb0; rb < rb1; ++rb) {
    const int64_t b0 = (int64_t)rb * 64;
    float sc[16];
    score_block<KC, LIK>(tiles, B, C, KP, S, b0, d0, z, Vp, phi, ctype, inv_s, sc);
    select_block_cols(sel, sc, B, C, b0, d0, k, cand);
  }
  select_end(sel, C, d0, k, (int)blockIdx.y, rows, scores);
}

template <int KC, int LIK, int CAP>
static void launch_select(const TopRowsArgs& a, const DrawTables& t, const SliceGeom& g, int W, int32_t* rows,
                          float* scores, hipStream_t st) {
  const dim3 grid((unsigned)((t.D + 63) / 64), (unsigned)g.slices);
  hipLaunchKernelGGL((toprows_select_kernel<KC, LIK, CAP>), grid, dim3(256), 0, st, t.B, t.D, t.KP, t.S, a.k, g.per, W,
                     t.z, t.Vp, t.phi, t.ctype, a.stored, a.cols, rows, scores);
}

bool launch_toprows(const TopRowsArgs& a, hipStream_t st) {
  DrawTables t = a.t;
  const int C = a.n_cols;
  if (a.k < 1 || a.k > kTopkMaxK || a.slices < 1 || a.slices > kTopkMaxSlices) return false;
  if (!with_kc(t.KP, [](auto) {}) || !with_lik(t.lik, [](auto) {})) return false;
  if (t.B <= 0 || C <= 0) return true;
  const SliceGeom g(t.B, a.slices);            // the blocks of a slice are row blocks
  if (a.slices > g.CB) return false;
  const int W = SliceGeom(t.D, 1).W;           // the bitmap is over the tables' columns
  if (a.stored && a.nnz > 0) launch_topk_mark(t.B, t.D, a.row_ptr, a.col, a.stored, st);
  if (a.cols) {
    uint8_t* ctc = t.lik == 3 ? a.ctc : nullptr;
    launch_panel_gather(t, C, a.cols, a.Vc, a.phic, ctc, st);
    t.Vp = a.Vc;
    t.phi = a.phic;
    t.ctype = ctc;
  }
  t.D = C;
  int32_t* rows = a.slices > 1 ? a.part_rows : a.rows;
  float* scores = a.slices > 1 ? a.part_scores : a.scores;
  with_kc(t.KP, [&](auto kc) {
    with_lik(t.lik, [&](auto lik) {
      constexpr int KC = decltype(kc)::value, LIK = decltype(lik)::value;
      if (a.k <= 16) launch_select<KC, LIK, 32>(a, t, g, W, rows, scores, st);
      else launch_select<KC, LIK, 80>(a, t, g, W, rows, scores, st);
    });
  });
  if (a.slices > 1) launch_topk_merge(C, a.k, a.slices, a.part_rows, a.part_scores, a.rows, a.scores, st);
  return true;
}

}  // namespace spmf
