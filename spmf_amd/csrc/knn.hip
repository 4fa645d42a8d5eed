// knn.hip -- rows in the latent space: the posterior mean encoding of a batch (embed) and the streaming exact
// k nearest rows of a reference set for every query row, without an [Nq, Nr] array.
//
// embed_kernel       : a thread per (row, k): the sum over the draws of z[S,B,KP] in draw order times 1/S and,
//   when asked, the unbiased standard deviation by Welford's recurrence in draw order; unpadded [B][K] output.
// kNN (include/spmf_hip.h spmf_knn has the definition):
//   knn_centre_kernel / knn_centre_finish_kernel : (Euclidean) c = the mean of the finite reference rows, from
//     per-block partial sums in a fixed order and one pass over them in block order -- no float atomics.
//   knn_prepare_kernel : a wave per row: q' = q - c | q / |q|, zero-padded to KP, bias_j = -1/2 |r'_j|^2; a
//     non-finite row (and a zero row under cosine) becomes NaN and so has no finite score.
//   knn_select_kernel  : a workgroup owns 64 queries and sweeps 64-row blocks of the reference set.  The score
//     <q'_i, r'_j> + bias_j = 1/2 |q'_i|^2 - 1/2 |q'_i - r'_j|^2 is likelihood code 0 of score_block (score_block.h)
//     with S = 1, z = Q', V' = R', phi = bias: the larger score is the nearer row, ties go to the smaller index.
//     The selection is select_rows.h, shared with topk.hip; the candidate test is "not the query itself".  With
//     few queries the reference blocks split over gridDim.y slices and topk.hip's merge kernel ranks them.
//     TILE = 1 (KP <= 64) keeps the 64 x KP query tile in LDS for the whole sweep and double-buffers only the
//     reference tile, across block boundaries too; its loop is its own, the MFMA step per 8 floats of K is the
//     tile loop's (score_mfma8): the same bits.
//   knn_refine_kernel  : a wave per query recomputes the distances of the k selected rows from the caller's rows
//     (Euclidean: sqrt of the fmaf chain of squared differences in ascending k; cosine: half that chain over the
//     unit rows) and orders them by (distance ascending, index ascending).  The expansion above only ever
//     decides membership at near-ties; the reported distances carry no cancellation.
// All arithmetic is fp32.
#include "common.h"
#include "kernels.h"
#include "score_block.h"
#include "select_rows.h"

namespace spmf {

// ---- embed -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void embed_kernel(int64_t B, int K, int KP, int S, const float* __restrict__ z,
                                                    float inv_s, float* __restrict__ mean, float* __restrict__ sd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * K) return;
  const int64_t b = i / K;
  const int k = (int)(i - b * K);
  const float* p = z + (size_t)b * KP + k;
  const size_t stride = (size_t)B * KP;
  float sum = 0.f, m = 0.f, m2 = 0.f;
  for (int s = 0; s < S; ++s) {
    const float v = p[(size_t)s * stride];
    sum += v;
    if (sd) {
      const float d = v - m;
      m += d / (float)(s + 1);
      m2 = fmaf(d, v - m, m2);
    }
  }
  mean[i] = sum * inv_s;
  if (sd) sd[i] = sqrtf(m2 / (float)(S - 1));
}

void launch_embed(const DrawTables& t, int K, float* mean, float* sd, hipStream_t st) {
  const int64_t n = t.B * K;
  if (n <= 0) return;
  hipLaunchKernelGGL(embed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t.B, K, t.KP, t.S, t.z,
                     1.f / (float)t.S, mean, sd);
}

// ---- the centre of the finite reference rows ---------------------------------------------------
// Block y sums rows [y per, (y + 1) per): thread (rr, k) = (t / KP, t % KP) takes every (256 / KP)-th row of
// them in ascending order; a row counts when all its row_len values are finite.  The block's threads are then
// folded over rr in ascending order: cpart[y][k], ccnt[y].
__global__ __launch_bounds__(256) void knn_centre_kernel(int64_t n, int Kx, int KP, int64_t per,
                                                         const float* __restrict__ r, float* __restrict__ cpart,
                                                         int32_t* __restrict__ ccnt) {
  __shared__ int bad[2][64];
  __shared__ float part[256];
  __shared__ int pcnt[64];
  const int t = threadIdx.x;
  const int k = t & (KP - 1), rr = t / KP, RP = 256 / KP;
  const int64_t lo = (int64_t)blockIdx.x * per;
  const int64_t hi = lo + per < n ? lo + per : n;
  float sum = 0.f;
  int cnt = 0, par = 0;
  for (int64_t j0 = lo; j0 < hi; j0 += RP, par ^= 1) {
    const int64_t j = j0 + rr;
    const float v = (j < hi && k < Kx) ? r[(size_t)j * Kx + k] : 0.f;
    if (k == 0) bad[par][rr] = 0;
    __syncthreads();
    if (!isfinite(v)) atomicOr(&bad[par][rr], 1);
    __syncthreads();
    if (j < hi && !bad[par][rr]) {
      sum += v;
      cnt += k == 0 ? 1 : 0;
    }
  }
  part[t] = sum;
  if (k == 0) pcnt[rr] = cnt;
  __syncthreads();
  if (rr == 0) {
    float s = 0.f;
    for (int i = 0; i < RP; ++i) s += part[i * KP + k];
    cpart[(size_t)blockIdx.x * KP + k] = s;
  }
  if (t == 0) {
    int c = 0;
    for (int i = 0; i < RP; ++i) c += pcnt[i];
    ccnt[blockIdx.x] = c;
  }
}

// one workgroup: the partial sums in block order, over the number of finite rows (none: the origin)
__global__ __launch_bounds__(256) void knn_centre_finish_kernel(int nb, int KP, const float* __restrict__ cpart,
                                                                const int32_t* __restrict__ ccnt,
                                                                float* __restrict__ centre) {
  const int k = threadIdx.x;
  if (k >= KP) return;
  float s = 0.f;
  int64_t c = 0;
  for (int b = 0; b < nb; ++b) {
    s += cpart[(size_t)b * KP + k];
    c += ccnt[b];
  }
  centre[k] = c > 0 ? s / (float)c : 0.f;
}

// ---- working rows ------------------------------------------------------------------------------
// a wave per row; lane l holds k = l, l + 64, l + 128, l + 192.  bias may be null (query rows).
__global__ __launch_bounds__(256) void knn_prepare_kernel(int64_t n, int Kx, int KP, int cosine,
                                                          const float* __restrict__ x,
                                                          const float* __restrict__ centre, float* __restrict__ w,
                                                          float* __restrict__ bias) {
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
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] / nrm;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = lane + 64 * i;
      if (k < Kx) v[i] -= centre[k];
    }
  }
  float b = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) b = fmaf(v[i], v[i], b);
  b = wave_sum(b);
  const float nan = __int_as_float(0x7fc00000);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = lane + 64 * i;
    if (k < KP) w[(size_t)row * KP + k] = ok ? v[i] : nan;
  }
  if (bias && lane == 0) bias[row] = ok ? -0.5f * b : nan;
}

// ---- selection ---------------------------------------------------------------------------------
// KC, CAP: as topk_select_kernel.  Grid (query blocks, reference slices); slice y writes idx / score [y][NQ][k].
template <int KC, int CAP, int TILE>
__global__ __launch_bounds__(256) void knn_select_kernel(int64_t NQ, int NR, int KP, int k, int cb_per_slice,
                                                         int64_t self_off, const float* __restrict__ qw,
                                                         const float* __restrict__ rw,
                                                         const float* __restrict__ bias, int32_t* __restrict__ idx,
                                                         float* __restrict__ score) {
  SPMF_SELECT_ROWS_LDS(CAP, sel);
  const int64_t b0 = (int64_t)blockIdx.x * 64;
  int cb0, cb1;
  slice_blocks((int64_t)NR, cb_per_slice, cb0, cb1);
  const auto not_self = [=](int64_t b, int d) { return self_off < 0 || (int64_t)d != self_off + b; };
  if constexpr (TILE == 0) {
    __shared__ float tiles[2][2][64][KC + 4];
    select_begin(sel);
    for (int cb = cb0; cb < cb1; ++cb) {
      const int d0 = cb * 64;
      float sc[16];
      score_block<KC, 0>(tiles, NQ, NR, KP, 1, b0, d0, qw, rw, bias, nullptr, 1.f, sc);
      select_block(sel, sc, NQ, NR, b0, d0, k, not_self);
    }
  } else {
    // the query tile stays; the reference tile of (block, K chunk) it + 1 is fetched under the MFMAs of it
    constexpr int QP = 64 + 4;           // pitch of the query tile (KP <= 64)
    constexpr int TQ = 16 * KC;          // float4 per reference tile
    constexpr int NLD = (TQ + 255) / 256;
    __shared__ float qt[64][QP];
    __shared__ float rt[2][64][KC + 4];
    const int t = threadIdx.x;
    const int lane = t & 63, wv = t >> 6;
    const int i32 = lane & 31, h = lane >> 5;
    const int wr = wv >> 1, wc = wv & 1;
    const int NCH = KP > KC ? KP / KC : 1;
    const int KQ = KP > KC ? KP : KC;    // columns of the query tile that the MFMAs read
    for (int i = t; i < 16 * KQ; i += 256) {
      const int row = i / (KQ / 4), kk = 4 * (i % (KQ / 4));
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kk < KP && b0 + row < NQ) v = *reinterpret_cast<const float4*>(qw + (size_t)(b0 + row) * KP + kk);
      *reinterpret_cast<float4*>(&qt[row][kk]) = v;
    }
    const int NIT = (cb1 - cb0) * NCH;
    auto fetch = [&](int it, float4* pre) {
      const int d0 = (cb0 + it / NCH) * 64, kc0 = (it % NCH) * KC;
#pragma unroll
      for (int j = 0; j < NLD; ++j) {
        const int i = t + 256 * j;
        const int row = i / (KC / 4), kk = kc0 + 4 * (i % (KC / 4));
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < TQ && kk < KP && (int64_t)d0 + row < NR) v = *reinterpret_cast<const float4*>(rw + (size_t)(d0 + row) * KP + kk);
        pre[j] = v;
      }
    };
    auto stash = [&](int buf, const float4* pre) {
#pragma unroll
      for (int j = 0; j < NLD; ++j) {
        const int i = t + 256 * j;
        if (i < TQ) *reinterpret_cast<float4*>(&rt[buf][i / (KC / 4)][4 * (i % (KC / 4))]) = pre[j];
      }
    };
    float4 pre[NLD];
    if (NIT > 0) {
      fetch(0, pre);
      stash(0, pre);
    }
    select_begin(sel);                   // (its barrier also publishes the tiles)
    score_f32x16 acc;
    float ph = 0.f;
    for (int it = 0; it < NIT; ++it) {
      const int buf = it & 1, ch = it % NCH;
      const int d0 = (cb0 + it / NCH) * 64;
      const int d = d0 + wc * 32 + i32;
      if (it + 1 < NIT) fetch(it + 1, pre);
      if (ch == 0) {
        ph = d < NR ? bias[d] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      }
      const float* ar = &qt[wr * 32 + i32][ch * KC + 4 * h];
      const float* br = &rt[buf][wc * 32 + i32][4 * h];
#pragma unroll
      for (int qk = 0; qk < KC / 8; ++qk) score_mfma8(ar + 8 * qk, br + 8 * qk, acc);
      if (it + 1 < NIT) stash(buf ^ 1, pre);
      __syncthreads();
      if (ch == NCH - 1) {
        float sc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = (0.f + (acc[r] + ph)) * 1.f;   // (score_block: sum over one draw, times 1/S)
        select_block(sel, sc, NQ, NR, b0, d0, k, not_self);
      }
    }
  }
  select_end(sel, NQ, b0, k, (int)blockIdx.y, idx, score);
}

// ---- refinement --------------------------------------------------------------------------------
// a wave per query; lane l < k takes the l-th selected row
__global__ __launch_bounds__(256) void knn_refine_kernel(int64_t NQ, int Kx, int KP, int k, int cosine,
                                                         const float* __restrict__ q, const float* __restrict__ r,
                                                         const float* __restrict__ qw, const float* __restrict__ rw,
                                                         int32_t* __restrict__ idx, float* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= NQ) return;
  const int j = lane < k ? idx[(size_t)i * k + lane] : -1;
  float dv = INFINITY;
  if (j >= 0) {
    const float* a = cosine ? qw + (size_t)i * KP : q + (size_t)i * Kx;
    const float* b = cosine ? rw + (size_t)j * KP : r + (size_t)j * Kx;
    float s = 0.f;
    for (int kk = 0; kk < Kx; ++kk) {
      const float d = a[kk] - b[kk];
      s = fmaf(d, d, s);
    }
    dv = cosine ? 0.5f * s : sqrtf(s);
  }
  int rank = 0;
  for (int m = 0; m < k; ++m) {
    const int jm = __shfl(j, m);
    const float dm = __shfl(dv, m);
    rank += (jm >= 0 && (dm < dv || (dm == dv && jm < j))) ? 1 : 0;
  }
  const int nv = __popcll(__ballot(j >= 0));
  if (j >= 0) {
    idx[(size_t)i * k + rank] = j;
    dist[(size_t)i * k + rank] = dv;
  } else if (lane < k && lane >= nv) {
    idx[(size_t)i * k + lane] = -1;
    dist[(size_t)i * k + lane] = INFINITY;
  }
}

// no reference row: every slot is padding
__global__ __launch_bounds__(256) void knn_pad_kernel(int64_t n, int32_t* __restrict__ idx, float* __restrict__ dist) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    idx[i] = -1;
    dist[i] = INFINITY;
  }
}

template <int KC, int CAP, int TILE>
static void launch_select(const KnnArgs& a, int32_t* idx, float* score, hipStream_t st) {
  const SliceGeom g(a.n_ref, a.slices);
  hipLaunchKernelGGL((knn_select_kernel<KC, CAP, TILE>), g.grid(a.n_query), dim3(256), 0, st, a.n_query, (int)a.n_ref,
                     a.KP, a.k, g.per, a.self_offset, a.qw, a.rw, a.bias, idx, score);
}

bool launch_knn(const KnnArgs& a, hipStream_t st) {
  if (a.k < 1 || a.k > kTopkMaxK || a.row_len < 1 || a.row_len > a.KP) return false;
  if (a.n_ref > 0 && (a.slices < 1 || a.slices > kTopkMaxSlices || a.slices > SliceGeom(a.n_ref, a.slices).CB)) return false;
  return with_kc(a.KP, [&](auto kc) {
    constexpr int KC = decltype(kc)::value;
    if (a.n_query <= 0) return;
    if (a.n_ref <= 0) {
      const int64_t n = a.n_query * a.k;
      hipLaunchKernelGGL(knn_pad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, a.idx, a.dist);
      return;
    }
    if (!a.cosine) {
      int64_t nb = (a.n_ref + 255) / 256;
      if (nb > kKnnCentreBlocks) nb = kKnnCentreBlocks;
      const int64_t per = (a.n_ref + nb - 1) / nb;
      nb = (a.n_ref + per - 1) / per;
      hipLaunchKernelGGL(knn_centre_kernel, dim3((unsigned)nb), dim3(256), 0, st, a.n_ref, a.row_len, a.KP, per, a.r,
                         a.cpart, a.ccnt);
      hipLaunchKernelGGL(knn_centre_finish_kernel, dim3(1), dim3(256), 0, st, (int)nb, a.KP, a.cpart, a.ccnt, a.centre);
    }
    hipLaunchKernelGGL(knn_prepare_kernel, dim3((unsigned)((a.n_ref + 3) / 4)), dim3(256), 0, st, a.n_ref, a.row_len,
                       a.KP, a.cosine ? 1 : 0, a.r, a.centre, a.rw, a.bias);
    if (a.qw != a.rw)
      hipLaunchKernelGGL(knn_prepare_kernel, dim3((unsigned)((a.n_query + 3) / 4)), dim3(256), 0, st, a.n_query,
                         a.row_len, a.KP, a.cosine ? 1 : 0, a.q, a.centre, a.qw, (float*)nullptr);
    int32_t* idx = a.slices > 1 ? a.part_idx : a.idx;
    float* score = a.slices > 1 ? a.part_score : a.dist;
    const bool wide = a.k > 16;
    if (a.tile == 1 && a.KP <= 64) {
      if (wide) launch_select<KC, 80, 1>(a, idx, score, st);
      else launch_select<KC, 32, 1>(a, idx, score, st);
    } else {
      if (wide) launch_select<KC, 80, 0>(a, idx, score, st);
      else launch_select<KC, 32, 0>(a, idx, score, st);
    }
    if (a.slices > 1) launch_topk_merge(a.n_query, a.k, a.slices, a.part_idx, a.part_score, a.idx, a.dist, st);
    hipLaunchKernelGGL(knn_refine_kernel, dim3((unsigned)((a.n_query + 3) / 4)), dim3(256), 0, st, a.n_query, a.row_len,
                       a.KP, a.k, a.cosine ? 1 : 0, a.q, a.r, a.qw, a.rw, a.idx, a.dist);
  });
}

}  // namespace spmf
