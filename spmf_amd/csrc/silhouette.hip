// silhouette.hip -- the silhouette of labelled rows as given (include/spmf_hip.h spmf_silhouette has the
// definition): every member's mean distance to its own cluster (a) and to the nearest other one (b) over all
// N^2 pairs, without an [N, N] or [N, G] array and without floating-point atomics.
//
//   sil_label_kernel    : a wave per row: the effective label (the caller's when it lies in [0, G) and the row is
//                         finite -- under cosine with a positive finite norm --, else -1); a non-member's outputs
//                         (NaN, nearest -1) are written here
//   (launch_group_order, groups.hip: the members in label order, every cluster padded to whole 64-row blocks)
//   sil_centre_kernel / sil_centre_finish_kernel : (Euclidean) c = the mean of the member rows: fp64 sums over
//                         kSilCentreBlocks equal runs of the blocks in use, rows as kmeans_sums_kernel takes them,
//                         then the runs in ascending order
//   sil_prepare_kernel  : a wave per padded position: knn_prepare_kernel's working row x' = x - c | x / |x|,
//                         zero-padded to KP, and bias = -1/2 |x'|^2; a pad position holds zeros
//   sil_sweep_kernel    : a workgroup owns one 64-row query block (one cluster) and walks every block in use in
//                         ascending order with score_tile_loop (score_block.h; S = 1, z = the query block, V' = the
//                         reference block, phi = its bias).  Lane (wr, wc, h, i32) holds the 16 query rows
//                         score_tile_row(wr, r, h) against reference position 32 wc + i32 and adds each distance,
//                         converted to fp64 first, onto acc[r]; pad positions and the row itself are selected out.
//                         When rec[nb].x changes the 16 sums are folded over the 32 lanes of a half by the xor
//                         butterfly 16, 8, 4, 2, 1 and the two wave columns added (wc 0 + wc 1): thread t < 64 owns
//                         query row t and turns the total into a (own cluster) or b = min (another, clusters
//                         ascending, so equal means keep the smaller index).  Behind the sweep it forms s in fp64,
//                         scatters through perm and adds the block's s by wave_sum's tree into spart[block].
//   sil_combine_kernel  : a thread per cluster: its blocks' sums in ascending order, and its count
// Every order above is a function of the members' labels alone: rows that are no members change no bit.
#include "common.h"
#include "kernels.h"
#include "score_block.h"

namespace spmf {

SilhouetteGeom silhouette_geom(int64_t n_rows, int G) {
  SilhouetteGeom q;
  q.NB = (n_rows + 63) / 64 + G;
  q.chunks = (n_rows + kGroupRowChunk - 1) / kGroupRowChunk;
  return q;
}

// grid ceil(n / 4), 256 threads; lane l holds k = l, l + 64, l + 128, l + 192 (knn_prepare_kernel's layout, and
// its norm: the same bits decide "positive and finite" here and divide there)
__global__ __launch_bounds__(256) void sil_label_kernel(int64_t n, int Kx, int G, int cosine,
                                                        const float* __restrict__ x,
                                                        const int32_t* __restrict__ labels,
                                                        int32_t* __restrict__ eff, float* __restrict__ sil,
                                                        float* __restrict__ a_out, float* __restrict__ b_out,
                                                        int32_t* __restrict__ nearest) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  float v[4];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = lane + 64 * i;
    v[i] = k < Kx ? x[(size_t)row * Kx + k] : 0.f;
    ok = ok && isfinite(v[i]);
  }
  ok = __all(ok);
  if (cosine) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) ss = fmaf(v[i], v[i], ss);
    const float nrm = sqrtf(wave_sum(ss));
    ok = ok && nrm > 0.f && isfinite(nrm);
  }
  if (lane != 0) return;
  const int g = labels[row];
  const bool member = ok && g >= 0 && g < G;
  eff[row] = member ? g : -1;
  if (!member) {
    const float nan = __int_as_float(0x7fc00000);
    sil[row] = nan;
    if (a_out) a_out[row] = nan;
    if (b_out) b_out[row] = nan;
    if (nearest) nearest[row] = -1;
  }
}

// grid kSilCentreBlocks, 256 threads: run y takes the blocks [y per, (y + 1) per) of the blocks in use, per =
// ceil(in use / kSilCentreBlocks); thread (rr, k) = (t / KP, t % KP) adds column k of the rows at positions rr,
// rr + 256 / KP, .. of every block, blocks ascending; the threads of a column are folded over rr in ascending order
__global__ __launch_bounds__(256) void sil_centre_kernel(int Kx, int KP, const float* __restrict__ x,
                                                         const int32_t* __restrict__ perm,
                                                         const int4* __restrict__ rec,
                                                         const int32_t* __restrict__ n_blocks,
                                                         double* __restrict__ cpart, int32_t* __restrict__ ccnt) {
  __shared__ double fold[256];
  const int t = threadIdx.x;
  const int k = t & (KP - 1), rr = t / KP, RP = 256 / KP;
  const int64_t nbe = *n_blocks;
  const int64_t per = (nbe + kSilCentreBlocks - 1) / kSilCentreBlocks;
  const int64_t nb0 = (int64_t)blockIdx.x * per;
  const int64_t nb1 = nb0 + per < nbe ? nb0 + per : nbe;
  double acc = 0.0;
  int cnt = 0;
  for (int64_t nb = nb0; nb < nb1; ++nb) {
    const int valid = rec[nb].y;
    cnt += valid;
    if (k < Kx) {
      for (int p = rr; p < valid; p += RP) {
        const int row = perm[nb * 64 + p];
        acc += (double)x[(size_t)row * Kx + k];
      }
    }
  }
  fold[t] = acc;
  __syncthreads();
  if (rr == 0) {
    double s = 0.0;
    for (int i = 0; i < RP; ++i) s += fold[i * KP + k];
    cpart[(size_t)blockIdx.x * KP + k] = s;
  }
  if (t == 0) ccnt[blockIdx.x] = cnt;
}

// one workgroup: the runs in ascending order, over the number of members (none: the origin)
__global__ __launch_bounds__(256) void sil_centre_finish_kernel(int KP, const double* __restrict__ cpart,
                                                                const int32_t* __restrict__ ccnt,
                                                                float* __restrict__ centre) {
  const int k = threadIdx.x;
  if (k >= KP) return;
  double s = 0.0;
  int64_t c = 0;
  for (int b = 0; b < kSilCentreBlocks; ++b) {
    s += cpart[(size_t)b * KP + k];
    c += ccnt[b];
  }
  centre[k] = c > 0 ? (float)(s / (double)c) : 0.f;
}

// grid ceil(NP / 4), 256 threads: a wave per padded position p; knn_prepare_kernel's arithmetic on row perm[p]
__global__ __launch_bounds__(256) void sil_prepare_kernel(int64_t NP, int Kx, int KP, int cosine,
                                                          const float* __restrict__ x,
                                                          const int32_t* __restrict__ perm,
                                                          const float* __restrict__ centre, float* __restrict__ w,
                                                          float* __restrict__ bias) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= NP) return;
  const int row = perm[p];
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = lane + 64 * i;
    v[i] = (row >= 0 && k < Kx) ? x[(size_t)row * Kx + k] : 0.f;
  }
  if (row >= 0) {
    if (cosine) {
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) ss = fmaf(v[i], v[i], ss);
      const float nrm = sqrtf(wave_sum(ss));
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = v[i] / nrm;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = lane + 64 * i;
        if (k < Kx) v[i] -= centre[k];
      }
    }
  }
  float b = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) b = fmaf(v[i], v[i], b);
  b = wave_sum(b);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = lane + 64 * i;
    if (k < KP) w[(size_t)p * KP + k] = v[i];
  }
  if (lane == 0) bias[p] = -0.5f * b;
}

// grid NB (the bound; a block at or past the blocks in use exits), 256 threads
template <int KC>
__global__ __launch_bounds__(256) void sil_sweep_kernel(int KP, int cosine, const float* __restrict__ w,
                                                        const float* __restrict__ bias,
                                                        const int32_t* __restrict__ perm,
                                                        const int4* __restrict__ rec,
                                                        const int32_t* __restrict__ cnt,
                                                        const int32_t* __restrict__ n_blocks,
                                                        float* __restrict__ sil, float* __restrict__ a_out,
                                                        float* __restrict__ b_out, int32_t* __restrict__ nearest,
                                                        double* __restrict__ spart) {
  __shared__ float tiles[2][2][64][KC + 4];
  __shared__ double fold[2][64];
  const int t = threadIdx.x;
  const int lane = t & 63, h = lane >> 5, i32 = lane & 31;
  const int wr = t >> 7, wc = t >> 6 & 1;
  const int64_t qb = blockIdx.x;
  const int64_t nbe = *n_blocks;
  if (qb >= nbe) return;                   // a surplus block
  const int4 rq = rec[qb];                 // (cluster, valid rows): the same for every thread
  const int gq = rq.x, vq = rq.y;
  const int nq = cnt[gq];
  const int col = wc * 32 + i32;           // the lane's position inside a reference block
  float bi[16];
  double acc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    bi[r] = bias[qb * 64 + score_tile_row(wr, r, h)];
    acc[r] = 0.0;
  }
  // thread t < 64 owns query row t
  double ra = 0.0, rb = INFINITY;
  int rn = -1;
  auto flush = [&](int g) {                // (every thread of the workgroup takes the same path here)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      double v = acc[r];
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o);
      if (i32 == 0) fold[wc][score_tile_row(wr, r, h)] = v;
      acc[r] = 0.0;
    }
    __syncthreads();
    if (t < 64) {
      const double tot = fold[0][t] + fold[1][t];
      if (g == gq) {
        ra = nq > 1 ? tot / (double)(nq - 1) : 0.0;
      } else {
        const double m = tot / (double)cnt[g];
        if (m < rb) {
          rb = m;
          rn = g;
        }
      }
    }
    __syncthreads();
  };
  const float* qw = w + (size_t)qb * 64 * KP;
  int cur = rec[0].x;
  for (int64_t nb = 0; nb < nbe; ++nb) {
    const int4 rr = rec[nb];
    if (rr.x != cur) {
      flush(cur);
      cur = rr.x;
    }
    const int valid = rr.y;
    const bool own = nb == qb;
    // both blocks are whole in the padded layout: the loop sees a 64 x 64 problem at the blocks' own addresses
    score_tile_loop<KC>(tiles, 64, 64, KP, 1, 0, 0, qw, w + (size_t)nb * 64 * KP, bias + (size_t)nb * 64,
                        [&](int, const score_f32x16& tv, float ph) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        // t_ij = <x'_i, x'_j> + bias_j;  u = -(bias_i + t_ij) = 1/2 |x'_i - x'_j|^2
        const float u = -(bi[r] + (tv[r] + ph));
        const float d = cosine ? fmaxf(0.f, u) : sqrtf(fmaxf(0.f, 2.f * u));
        const bool in = col < valid && !(own && score_tile_row(wr, r, h) == col);
        acc[r] = in ? acc[r] + (double)d : acc[r];
      }
    });
  }
  flush(cur);
  if (t < 64) {
    double s;
    if (rn < 0) {                          // no other cluster has a member
      s = __longlong_as_double(0x7ff8000000000000LL);
      rb = INFINITY;
    } else {
      const double m = ra > rb ? ra : rb;
      s = (nq > 1 && m > 0.0) ? (rb - ra) / m : 0.0;
    }
    const bool scored = t < vq;
    if (scored) {
      const int row = perm[qb * 64 + t];
      sil[row] = (float)s;
      if (a_out) a_out[row] = (float)ra;
      if (b_out) b_out[row] = (float)rb;
      if (nearest) nearest[row] = rn;
    }
    const double tot = wave_sum(scored ? s : 0.0);
    if (t == 0) spart[qb] = tot;
  }
}

// a thread per cluster
__global__ __launch_bounds__(256) void sil_combine_kernel(int G, const int32_t* __restrict__ cnt,
                                                          const int32_t* __restrict__ boff,
                                                          const double* __restrict__ spart,
                                                          double* __restrict__ sums, int64_t* __restrict__ counts) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  counts[g] = cnt[g];
  double a = 0.0;
  for (int nb = boff[g]; nb < boff[g + 1]; ++nb) a += spart[nb];
  sums[g] = a;
}

bool launch_silhouette(const SilhouetteArgs& a, hipStream_t st) {
  const SilhouetteGeom q = silhouette_geom(a.n_rows, a.n_clusters);
  const int G = a.n_clusters, cosine = a.cosine ? 1 : 0;
  const GroupOrder& o = a.ord;
  if (a.row_len < 1 || a.row_len > a.KP || a.n_rows <= 0) return false;
  return with_kc(a.KP, [&](auto kc) {
    constexpr int KC = decltype(kc)::value;
    const int64_t NP = q.NB * 64;
    hipLaunchKernelGGL(sil_label_kernel, dim3((unsigned)((a.n_rows + 3) / 4)), dim3(256), 0, st, a.n_rows, a.row_len, G,
                       cosine, a.x, a.labels, a.eff, a.sil, a.a, a.b, a.nearest);
    // (RB = 1: the ordering's segments are the blocks themselves and are not used here)
    launch_group_order(a.n_rows, G, 1, a.eff, o, st);
    if (!cosine) {
      hipLaunchKernelGGL(sil_centre_kernel, dim3(kSilCentreBlocks), dim3(256), 0, st, a.row_len, a.KP, a.x, o.perm,
                         o.rec, o.boff + G, a.cpart, a.ccnt);
      hipLaunchKernelGGL(sil_centre_finish_kernel, dim3(1), dim3(256), 0, st, a.KP, a.cpart, a.ccnt, a.centre);
    }
    hipLaunchKernelGGL(sil_prepare_kernel, dim3((unsigned)((NP + 3) / 4)), dim3(256), 0, st, NP, a.row_len, a.KP,
                       cosine, a.x, o.perm, a.centre, a.w, a.bias);
    hipLaunchKernelGGL((sil_sweep_kernel<KC>), dim3((unsigned)q.NB), dim3(256), 0, st, a.KP, cosine, a.w, a.bias,
                       o.perm, o.rec, o.cnt, o.boff + G, a.sil, a.a, a.b, a.nearest, a.spart);
    hipLaunchKernelGGL(sil_combine_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, G, o.cnt, o.boff,
                       a.spart, a.cluster_sum, a.counts);
  });
}

}  // namespace spmf
