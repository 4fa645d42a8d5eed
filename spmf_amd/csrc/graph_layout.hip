// graph_layout.hip -- graph_layout: the epochs of a 2-D layout of a weighted CSR graph (the full-batch form of
// UMAP's objective; include/spmf_hip.h spmf_graph_layout has the definition).
//
// One launch per epoch.  An epoch reads the positions y of the epoch before it and writes every row's new position
// into the other buffer (Jacobi): row i is written by the group that owns it and by nobody else, so there is no
// atomic and no race, and an epoch is a pure function of (graph, y, epoch, seed).
//
// A row owns a group of kRowLanes = 16 lanes, four rows to a wave.  Lane l of the group takes the entries
// l, l + 16, l + 32, .. of the row's list in ascending order -- one contiguous 64-byte request of the group per
// array and pass, then one 8-byte gather of y_j per lane -- and the negatives m = l, l + 16, .. below M; the five
// per-lane sums (W, the attraction, the repulsion) then go through the fixed DPP tree of group_sum<16>.  So the
// order of a row's additions is a function of its list length and M alone: not of the grid, of the other rows, of
// n_rows or of where the row sits in its wave.  A hub row walks its list in len / 16 passes of its one group: the
// rule by which a row would get more lanes had to depend on its length alone, and at the degrees of a symmetrised
// kNN graph the passes of a hub are hidden behind the other waves of its compute unit.
//
// The position table is 8 bytes a row: it sits in L2 at any n_rows this library takes in one piece, and the kernel
// is bound by the index stream and, at small n_rows, by the launch.
//
// Nothing here trusts the graph: an indptr value is clamped to [0, nnz], an index outside [0, n_rows) reads no
// position, a negative is __umulhi(word, n_rows) < n_rows.
#include "kernels.h"
#include "layout_force.h"

namespace spmf {

__global__ __launch_bounds__(256) void graph_layout_kernel(int64_t n_rows, int64_t nnz,
                                                           const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices,
                                                           const float* __restrict__ weights,
                                                           const float2* __restrict__ y, float2* __restrict__ out,
                                                           int epoch, float alpha, int M, float a, float b,
                                                           float neg2b, float two_gamma_b, float rate_over_m,
                                                           uint32_t seed_lo, uint32_t seed_hi) {
  const int sub = threadIdx.x & (kRowLanes - 1);
  const int64_t i = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x / kRowLanes);
  const bool live = i < n_rows;                            // the same for the 16 lanes of a group
  float2 yi = make_float2(0.f, 0.f);
  int64_t p0 = 0, p1 = 0;
  if (live) {
    yi = y[i];
    p0 = min(max(indptr[i], (int64_t)0), nnz);
    p1 = min(max(indptr[i + 1], (int64_t)0), nnz);
  }
  const bool moves = live && finite2(yi);                  // a non-finite row keeps its bits
  const uint32_t n32 = (uint32_t)n_rows;                   // n_rows <= 2^31 - 64 (checked on the host)

  // attraction: this lane's entries in ascending order
  float W = 0.f, fx = 0.f, fy = 0.f;
  if (moves) {
    for (int64_t p = p0 + sub; p < p1; p += kRowLanes) {
      const uint32_t j = (uint32_t)indices[p];
      const float w = weights[p];
      if (j >= n32 || !(w > 0.f) || !(w < INFINITY)) continue;
      const float2 yj = y[j];
      if (!finite2(yj)) continue;
      W += w;
      attract(yi, yj, w, a, b, neg2b, fx, fy);
    }
  }
  // repulsion: this lane's negatives in ascending order
  float gx = 0.f, gy = 0.f;
  if (moves) {
    for (int m = sub; m < M; m += kRowLanes) {
      const uint32_t r = negative_row((uint32_t)i, m, epoch, 0x554D4150u, seed_lo, seed_hi, n32);    // < n_rows
      if ((int64_t)r == i) continue;
      const float2 yr = y[r];
      if (!finite2(yr)) continue;
      repel(yi, yr, a, b, two_gamma_b, gx, gy);
    }
  }
  W = group_sum<kRowLanes>(W);
  fx = group_sum<kRowLanes>(fx);
  fy = group_sum<kRowLanes>(fy);
  gx = group_sum<kRowLanes>(gx);
  gy = group_sum<kRowLanes>(gy);
  if (sub == 0 && live) {
    float2 o = yi;
    if (moves && W > 0.f) {                                // a row without a valid edge keeps its bits
      const float s = rate_over_m * W, step = alpha / fmaxf(1.f, W);
      o.x = fmaf(step, fmaf(s, gx, fx), yi.x);
      o.y = fmaf(step, fmaf(s, gy, fy), yi.y);
    }
    out[i] = o;
  }
}

void launch_graph_layout(const GraphLayoutArgs& g, hipStream_t st) {
  const unsigned nb = (unsigned)((g.n_rows + kRowsPerBlock - 1) / kRowsPerBlock);   // < 2^27
  for (int k = 0; k < g.s.n_epochs; ++k) {
    const float2* from = g.buf[k & 1];
    float2* to = k == g.s.n_epochs - 1 ? g.y_out : g.buf[(k + 1) & 1];
    const int e = g.s.epoch0 + k;
    const float alpha = (float)(g.s.lr * (1.0 - (double)e / (double)g.s.total_epochs));
    hipLaunchKernelGGL(graph_layout_kernel, dim3(nb), dim3(256), 0, st, g.n_rows, g.nnz, g.indptr, g.indices,
                       g.weights, from, to, e, alpha, g.s.n_negatives, g.s.a, g.s.b, g.s.neg2b,
                       g.s.two_gamma_b, g.s.rate_over_m, g.s.seed_lo, g.s.seed_hi);
  }
}

}  // namespace spmf
