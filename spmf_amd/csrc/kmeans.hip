// kmeans.hip -- one Lloyd step on rows as given (include/spmf_hip.h spmf_kmeans_step has the definition): the
// assignment is launch_knn's (knn.hip: centre, prepare, select, merge, refine) with q = x, r = the centroids and
// k = min(4, G); what is new here turns its refined candidates into the step's outputs.
//
//   kmeans_label_kernel   : a thread per row: label = the first refined candidate (-1: none), its distance, and per
//                           kKmeansStatRows rows the partial sums (dist^2 as doubles, rows whose label changed,
//                           rows without a label), folded over the workgroup's threads by a fixed tree
//   kmeans_stats_kernel   : one workgroup: the partial sums in a fixed order -> stats[3]
//   (launch_group_order, groups.hip: the rows in label order, every cluster padded to whole 64-row blocks)
//   kmeans_sums_kernel    : a workgroup per run of RB row blocks; thread (rr, k) = (t / KP, t % KP) adds column k
//                           of the rows at positions rr, rr + 256 / KP, .. of every block of a segment (the blocks
//                           of one cluster inside the run), blocks ascending, rows ascending inside a block; when
//                           the cluster changes or the run ends the threads of a column are folded over rr in
//                           ascending order into part[segment][k] with ordinary stores
//   kmeans_combine_kernel : a thread per (cluster, k): the cluster's segments in ascending order -> sums, overwritten
//                           (an empty cluster: 0); counts = the ordering's counts
// Every addition is fp64 from the first one on: each fp32 value is converted before it is added.  No fp32 partial
// sums, no floating-point atomics.  One summation order, a pure function of (n_rows, G) and the labels.
#include "common.h"
#include "kernels.h"

namespace spmf {

KmeansGeom kmeans_geom(int64_t n_rows, int G) {
  KmeansGeom q;
  q.NB = (n_rows + 63) / 64 + G;
  q.chunks = (n_rows + kGroupRowChunk - 1) / kGroupRowChunk;
  q.sblocks = (n_rows + kKmeansStatRows - 1) / kKmeansStatRows;
  int64_t runs = q.NB < kKmeansTargetRuns ? q.NB : kKmeansTargetRuns;
  if (runs < 1) runs = 1;
  q.RB = (int)((q.NB + runs - 1) / runs);
  q.runs = (int)((q.NB + q.RB - 1) / q.RB);
  // segments: at most one per run and one per cluster; sized by the run target (>= q.runs) so that the scratch
  // does not shrink as the rows grow
  q.nseg = runs + G;
  return q;
}

// folds v over the 256 threads by halving strides: the same pairs whatever the data
__device__ inline double kmeans_fold256(double* sh, int t, double v) {
  sh[t] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// grid ceil(n / 256), 256 threads; spart [gridDim.x][3]
__global__ __launch_bounds__(kKmeansStatRows) void kmeans_label_kernel(int64_t n, int kc,
                                                                       const int32_t* __restrict__ cand_idx,
                                                                       const float* __restrict__ cand_dist,
                                                                       const int32_t* __restrict__ prev,
                                                                       int32_t* __restrict__ labels,
                                                                       float* __restrict__ dist,
                                                                       double* __restrict__ spart) {
  __shared__ double sh[kKmeansStatRows];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kKmeansStatRows + t;
  double d2 = 0.0, ch = 0.0, un = 0.0;
  if (i < n) {
    const int j = cand_idx[(size_t)i * kc];
    const float dv = cand_dist[(size_t)i * kc];   // (+inf beside -1: knn's padding)
    labels[i] = j;
    if (dist) dist[i] = dv;
    if (j >= 0) d2 = (double)dv * (double)dv;
    else un = 1.0;
    ch = prev ? (prev[i] != j ? 1.0 : 0.0) : 1.0;
  }
  const double s0 = kmeans_fold256(sh, t, d2);
  const double s1 = kmeans_fold256(sh, t, ch);
  const double s2 = kmeans_fold256(sh, t, un);
  if (t == 0) {
    spart[(size_t)blockIdx.x * 3 + 0] = s0;
    spart[(size_t)blockIdx.x * 3 + 1] = s1;
    spart[(size_t)blockIdx.x * 3 + 2] = s2;
  }
}

// one workgroup: thread t adds the partial sums t, t + 256, .. in ascending order, then the fixed tree
__global__ __launch_bounds__(256) void kmeans_stats_kernel(int64_t nb, const double* __restrict__ spart,
                                                           double* __restrict__ stats) {
  __shared__ double sh[256];
  const int t = threadIdx.x;
  for (int q = 0; q < 3; ++q) {
    double s = 0.0;
    for (int64_t b = t; b < nb; b += 256) s += spart[(size_t)b * 3 + q];
    const double r = kmeans_fold256(sh, t, s);
    if (t == 0) stats[q] = r;
  }
}

// grid runs, 256 threads; KP: row_len padded to 4, 8, .., 256
__global__ __launch_bounds__(256) void kmeans_sums_kernel(int Kx, int KP, int RB, const float* __restrict__ x,
                                                          const int32_t* __restrict__ perm,
                                                          const int4* __restrict__ rec,
                                                          const int32_t* __restrict__ n_blocks,
                                                          double* __restrict__ part) {
  __shared__ double fold[256];
  const int t = threadIdx.x;
  const int k = t & (KP - 1), rr = t / KP, RP = 256 / KP;
  const int64_t nb0 = (int64_t)blockIdx.x * RB;
  const int64_t nbe = *n_blocks;
  const int64_t nb1 = nb0 + RB < nbe ? nb0 + RB : nbe;
  if (nb0 >= nb1) return;                  // a surplus run
  double acc = 0.0;
  auto flush = [&](int seg) {              // (every thread of the workgroup takes the same path here)
    fold[t] = acc;
    __syncthreads();
    if (rr == 0 && k < Kx) {
      double s = 0.0;
      for (int i = 0; i < RP; ++i) s += fold[i * KP + k];
      part[(size_t)seg * Kx + k] = s;
    }
    __syncthreads();
  };
  int seg = -1;
  for (int64_t nb = nb0; nb < nb1; ++nb) {
    const int4 r = rec[nb];                // (cluster, valid rows, segment): the same for every thread
    if (r.z != seg) {
      if (seg >= 0) flush(seg);
      seg = r.z;
      acc = 0.0;
    }
    const int valid = r.y;
    if (k < Kx) {
      for (int p = rr; p < valid; p += RP) {
        const int row = perm[nb * 64 + p];
        acc += (double)x[(size_t)row * Kx + k];
      }
    }
  }
  flush(seg);
}

// a thread per (cluster, k)
__global__ __launch_bounds__(256) void kmeans_combine_kernel(int G, int Kx, const int32_t* __restrict__ cnt,
                                                             const int32_t* __restrict__ boff,
                                                             const int4* __restrict__ rec,
                                                             const double* __restrict__ part,
                                                             double* __restrict__ sums,
                                                             int64_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)G * Kx) return;
  const int g = (int)(i / Kx), k = (int)(i - (int64_t)g * Kx);
  const int c = cnt[g];
  if (k == 0) counts[g] = c;
  double a = 0.0;
  if (c > 0) {
    const int seg0 = rec[boff[g]].z, seg1 = rec[boff[g + 1] - 1].z;
    for (int seg = seg0; seg <= seg1; ++seg) a += part[(size_t)seg * Kx + k];
  }
  sums[i] = a;
}

void launch_kmeans(const KmeansArgs& a, hipStream_t st) {
  const KmeansGeom q = kmeans_geom(a.n_rows, a.n_clusters);
  const int G = a.n_clusters;
  const GroupOrder& o = a.ord;
  int KP = 4;
  while (KP < a.row_len) KP *= 2;
  hipLaunchKernelGGL(kmeans_label_kernel, dim3((unsigned)q.sblocks), dim3(kKmeansStatRows), 0, st, a.n_rows, a.kc,
                     a.cand_idx, a.cand_dist, a.prev, a.labels, a.dist, a.spart);
  hipLaunchKernelGGL(kmeans_stats_kernel, dim3(1), dim3(256), 0, st, q.sblocks, a.spart, a.stats);
  launch_group_order(a.n_rows, G, q.RB, a.labels, o, st);
  hipLaunchKernelGGL(kmeans_sums_kernel, dim3((unsigned)q.runs), dim3(256), 0, st, a.row_len, KP, q.RB, a.x, o.perm,
                     o.rec, o.boff + G, a.part);
  const int64_t n = (int64_t)G * a.row_len;
  hipLaunchKernelGGL(kmeans_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, G, a.row_len, o.cnt,
                     o.boff, o.rec, a.part, a.sums, a.counts);
}

}  // namespace spmf
