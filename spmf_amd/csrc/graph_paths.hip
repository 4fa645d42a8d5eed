// graph_paths.hip -- shortest paths along the graph: graph_relax (include/spmf_hip.h spmf_graph_relax has the
// definition; spmf_amd/geodesic.py is the driver it serves, and its NumpyOps.relax the restatement it is held to
// bit for bit).
//
// A sweep is graph_spmm (spectral.hip) in the (min, +) semiring: Y_il = min(X_il, min_j fl(X_jl + w_ij)) over the
// counting entries of row i, a column per source (or set of sources).  The access pattern is graph_spmm's: a row
// owns a group of 16 lanes, four rows to a wave, lane l owns column l, the group walks the row's list together in
// list order, kUnroll entries at a time, all of a step's loads (index, length, the row of X) issued before its
// first compare.  No cross-lane step and no atomic: an entry of Y is a function of its row's list and of its column
// of X alone.  fl(a + w) is monotone in a and a minimum does not depend on the order, so the sweeps repeated to
// a fixed point give the bits of an fp32 Dijkstra that adds the lengths in the same left-to-right order.
//
// An entry that does not count (index outside [0, n_rows), length not finite and > 0, or behind the list's end)
// loads the row's own X_i and is dropped by a select.  A NaN never wins a <: it stays where it is and reaches
// nobody.  The last sweep of a call also tells whether anything moved (a plain store of 1 by every lane that
// lowered its value: every writer stores the same word) and names the predecessors.
#include "common.h"
#include "graph_rows.h"
#include "kernels.h"

namespace spmf {

// kLast: the call's last sweep, which alone writes pred and changed (either may be null)
template <bool kLast>
__global__ __launch_bounds__(256) void graph_relax_kernel(GraphCsr g, const float* __restrict__ x, float* y,
                                                          int32_t* pred, int32_t* changed) {
  const int sub = threadIdx.x & (kRowLanes - 1);
  const RowList r = row_list(g);
  if (!r.live) return;                                // whole groups leave: nothing below crosses lanes
  const uint32_t n32 = (uint32_t)g.n_rows;            // n_rows <= 2^31 - 64 (checked on the host)
  const uint32_t self = (uint32_t)r.i;
  const size_t at = (size_t)r.i * kBlockCols + sub;
  const float xi = x[at];

  float best = INFINITY, xa = INFINITY;               // the smallest sum so far and the X it was made from
  int32_t arg = -1;                                   // its column: the first in list order
  for (int64_t p = r.p0; p < r.p1; p += kUnroll) {
    uint32_t j[kUnroll];
    float w[kUnroll], xj[kUnroll];
    bool ok[kUnroll];
    // the step's loads first: the entries (one address for the group), then what they point to
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t q = min(p + u, r.p1 - 1);         // behind the end: the last entry again, dropped below
      j[u] = (uint32_t)g.indices[q];
      w[u] = g.weights[q];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      ok[u] = p + u < r.p1 && j[u] < n32 && weight_counts(w[u]);
      const uint32_t row = ok[u] ? j[u] : self;        // an entry that does not count reads this row's own
      xj[u] = x[(size_t)row * kBlockCols + sub];
    }
    // list order: a later entry wins only if it is strictly smaller
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const float t = xj[u] + w[u];
      const bool take = ok[u] && t < best;
      best = take ? t : best;
      xa = take ? xj[u] : xa;
      arg = take ? (int32_t)j[u] : arg;
    }
  }
  const bool lower = best < xi;
  const float yi = lower ? best : xi;
  y[at] = yi;
  if (kLast) {
    if (changed && lower) *changed = 1;
    if (pred) pred[at] = (best == yi && yi < INFINITY && xa < yi) ? arg : -1;
  }
}

void launch_graph_relax(const GraphRelaxArgs& a, hipStream_t st) {
  const GraphCsr g{a.n_rows, a.nnz, a.indptr, a.indices, a.lengths};
  const dim3 grid(row_blocks(a.n_rows));
  for (int k = 0; k < a.n_sweeps; ++k) {
    const float* from = a.buf[k & 1];
    if (k < a.n_sweeps - 1) {
      hipLaunchKernelGGL(graph_relax_kernel<false>, grid, dim3(256), 0, st, g, from, a.buf[(k + 1) & 1],
                         (int32_t*)nullptr, (int32_t*)nullptr);
    } else {
      if (a.changed_out) launch_zero(a.changed_out, sizeof(int32_t), st);
      hipLaunchKernelGGL(graph_relax_kernel<true>, grid, dim3(256), 0, st, g, from, a.x_out, a.pred_out,
                         a.changed_out);
    }
  }
}

}  // namespace spmf
