// graph_transform.hip -- graph_transform: new rows laid out on a fitted 2-D map, the reference positions held
// fixed (umap-learn's transform; include/spmf_hip.h spmf_graph_transform has the definition).
//
// One launch for all epochs of the call.  A query row reads the reference positions and its own position, never
// another query row's, so there is nothing to exchange between the epochs: no second buffer, no launch per epoch.
// A row owns a group of kRowLanes = 16 lanes, four rows to a wave.  Lane l of the group takes the entries
// l, l + 16, l + 32, l + 48 of the row's k <= 64 (index, weight) pairs, decides once whether each is valid,
// gathers its reference position once and keeps (y_j, w_ij) in registers for all epochs; a skipped entry is kept
// as weight 0.  W_i and the weighted-mean start come from group_sum<16>.  An epoch is this lane's entries in
// ascending order, its negatives m = l, l + 16, .. below M -- the only memory traffic of an epoch: 8-byte gathers
// from the position table, which sits in L2 -- and four group_sum<16>.  The tree leaves the same bits in all 16
// lanes, so every lane forms the update itself: nothing is broadcast or stored between the epochs, and lane 0
// writes y_out once.
//
// The order of a row's additions is a function of k and M alone: not of the grid, of the other rows, of n_query or
// of where the row sits in its wave.  So rows may be mapped in chunks of any size with the same bits (row0).
//
// Nothing here trusts the inputs: an index outside [0, n_ref) reads no position, a negative is
// __umulhi(word, n_ref) < n_ref, with n_ref == 0 no negative is drawn and nothing of y_ref is read.
#include "kernels.h"
#include "layout_force.h"

namespace spmf {

namespace {
constexpr int kLaneEntries = 4;                            // k <= 64 = kRowLanes * kLaneEntries
}  // namespace

// y_in and y_out may be one array: a row's group reads y_in[i] before its lane 0 writes y_out[i], and no other
// group touches either.
__global__ __launch_bounds__(256) void graph_transform_kernel(GraphTransformArgs g) {
  const int sub = threadIdx.x & (kRowLanes - 1);
  const int64_t i = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x / kRowLanes);
  const bool live = i < g.n_query;                         // the same for the 16 lanes of a group
  const uint32_t n32 = (uint32_t)g.n_ref;                  // n_ref <= 2^31 - 1 (checked on the host)
  const float2* __restrict__ y_ref = g.y_ref;

  // this lane's entries, validity decided once: a skipped entry has weight 0
  float2 yj[kLaneEntries];
  float wj[kLaneEntries];
#pragma unroll
  for (int t = 0; t < kLaneEntries; ++t) {
    yj[t] = make_float2(0.f, 0.f);
    wj[t] = 0.f;
    const int e = sub + t * kRowLanes;
    if (live && e < g.k) {
      const int64_t p = i * g.k + e;
      const uint32_t j = (uint32_t)g.idx[p];
      const float w = g.w[p];
      if (j < n32 && w > 0.f && w < INFINITY) {
        const float2 v = y_ref[j];
        if (finite2(v)) {
          yj[t] = v;
          wj[t] = w;
        }
      }
    }
  }
  float W = 0.f, sx = 0.f, sy = 0.f;
#pragma unroll
  for (int t = 0; t < kLaneEntries; ++t) {
    W += wj[t];
    sx = fmaf(wj[t], yj[t].x, sx);
    sy = fmaf(wj[t], yj[t].y, sy);
  }
  W = group_sum<kRowLanes>(W);
  float2 yi;
  if (g.y_in) {
    yi = live ? g.y_in[i] : make_float2(0.f, 0.f);
  } else {                                                 // the weighted mean of the neighbours; NaN without one
    sx = group_sum<kRowLanes>(sx);
    sy = group_sum<kRowLanes>(sy);
    yi = W > 0.f ? make_float2(sx / W, sy / W) : make_float2(__builtin_nanf(""), __builtin_nanf(""));
  }
  const float s = g.s.rate_over_m * W, inv = fmaxf(1.f, W);
  const uint32_t g32 = (uint32_t)(g.row0 + i);

  for (int e = g.s.epoch0; e < g.s.epoch0 + g.s.n_epochs; ++e) {
    // a row without a valid entry and a row at a non-finite position keep their bits
    const bool moves = live && W > 0.f && finite2(yi);     // the same for the 16 lanes of a group
    float fx = 0.f, fy = 0.f, gx = 0.f, gy = 0.f;
    if (moves) {
#pragma unroll
      for (int t = 0; t < kLaneEntries; ++t) {             // attraction: this lane's entries in ascending order
        if (wj[t] > 0.f) attract(yi, yj[t], wj[t], g.s.a, g.s.b, g.s.neg2b, fx, fy);
      }
      if (n32 > 0) {
        for (int m = sub; m < g.s.n_negatives; m += kRowLanes) {     // repulsion: this lane's negatives
          // (a row below n_ref)
          const float2 yr = y_ref[negative_row(g32, m, e, 0x554D5854u, g.s.seed_lo, g.s.seed_hi, n32)];
          if (!finite2(yr)) continue;
          repel(yi, yr, g.s.a, g.s.b, g.s.two_gamma_b, gx, gy);
        }
      }
    }
    fx = group_sum<kRowLanes>(fx);
    fy = group_sum<kRowLanes>(fy);
    gx = group_sum<kRowLanes>(gx);
    gy = group_sum<kRowLanes>(gy);
    if (moves) {
      const float alpha = (float)(g.s.lr * (1.0 - (double)e / (double)g.s.total_epochs));
      const float step = alpha / inv;
      yi.x = fmaf(step, fmaf(s, gx, fx), yi.x);
      yi.y = fmaf(step, fmaf(s, gy, fy), yi.y);
    }
  }
  if (sub == 0 && live) g.y_out[i] = yi;
}

void launch_graph_transform(const GraphTransformArgs& g, hipStream_t st) {
  const unsigned nb = (unsigned)((g.n_query + kRowsPerBlock - 1) / kRowsPerBlock);   // <= 2^28
  hipLaunchKernelGGL(graph_transform_kernel, dim3(nb), dim3(256), 0, st, g);
}

}  // namespace spmf
