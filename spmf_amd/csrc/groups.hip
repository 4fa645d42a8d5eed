// groups.hip -- streaming per-group sums of the posterior predictive over the rows of a batch, per draw: for
// every draw s, group g and column d of a panel
//   sum[s][g][d]     = sum_{b : labels[b] = g} m_s(b, d)
//   nonzero[s][g][d] = sum_{b : labels[b] = g} -expm1f(-r_s(b, d))   (m_s on a Bernoulli column)
// with r_s = cell_rate(<z_sb, V'_sd>, phi_sd) and m_s = cell_mean(r_s) as in panel.hip: the sums of predict's
// cells, without the [rows, C] block of a draw.  All additions are fp64: every fp32 m_s is converted before the
// first addition it takes part in; no fp32 partial sums, no floating-point atomics.
//
// The ordering (labels -> rows in group order, stable in the row index, every group padded to whole 64-row
// blocks), on the device with no read-back:
//   group_rank_kernel    : per chunk of kGroupRowChunk rows the rank of every labelled row among the earlier
//                          rows of its group inside the chunk, and the chunk's count per group (tbl[chunk][g])
//   group_scan_kernel    : per group the exclusive scan of tbl over the chunks (in place) and the group's count
//   group_offsets_kernel : the first 64-row block of every group (boff[0 .. G], boff[G] = blocks in use) and the
//                          running count of group starts that are not also run starts (fincl), which numbers
//                          the segments below
//   group_fill_kernel    : per block its record (group, valid rows, segment); perm = -1
//   group_scatter_kernel : perm[64 boff[g] + rank in group] = row
//   group_gather_kernel  : zs[s][p][:] = z[s][perm[p]][:], zeros for a pad row (perm < 0)
// Blocks are bounded by NB = ceil(B / 64) + G; grids are sized by that bound and surplus blocks exit.
//
// group_kernel<KC, LIK, PNZ>: a workgroup owns one 64-column block, kGroupDrawChunk draws and a run of RB
// consecutive row blocks.  Per row block score_tile_loop (score_block.h, unchanged) forms the 64 x 64 tile of a
// draw; its callback adds the lane's 16 cells as doubles in ascending accumulator order, rows at or past the
// block's valid count selected out (not multiplied by 0: a pad row holds zeros, but selection is what the
// contract asks for), adds the two lane halves and leaves the 32 column sums of the wave in
// LDS; behind the loop thread (draw, column) adds wave row 0 + wave row 1 onto its register accumulator.  A
// segment = the blocks of one group inside one run; its accumulators go to part[segment][S][CR] with ordinary
// stores when the group changes or the run ends.  group_combine_kernel adds a group's segments in ascending
// order onto the caller's output.  One summation order, a pure function of (B, G, S, C) and the labels.
//
// launch_groups walks column ranges of CR columns (group_kernel + group_combine_kernel per range) so that part
// stays inside its budget; api_stream.hip carves the scratch from the same group_geom.
#include "common.h"
#include "kernels.h"
#include "score_block.h"

namespace spmf {

GroupGeom group_geom(int64_t B, int S, int G, int C) {
  GroupGeom q;
  q.NB = (B + 63) / 64 + G;
  q.chunks = (B + kGroupRowChunk - 1) / kGroupRowChunk;
  const int64_t CB = ((int64_t)C + 63) / 64;
  int64_t runs = CB > 0 ? (kGroupTargetBlocks + CB - 1) / CB : 1;
  if (runs > q.NB) runs = q.NB;
  if (runs < 1) runs = 1;
  q.RB = (int)((q.NB + runs - 1) / runs);
  q.runs = (int)((q.NB + q.RB - 1) / q.RB);
  // segments: at most one per run and one per group.  Sized by the run target, not by q.runs (<= it), which drops
  // when RB steps up: the scratch must not shrink as the rows grow.
  q.nseg = runs + G;
  // part: [nseg][S][CR] doubles, twice (sum, nonzero).  Everything when that fits the budget, else the budget
  // (at least one column block): non-decreasing in B and S.
  const size_t per_col = (size_t)q.nseg * (size_t)(S > 0 ? S : 1) * 2 * sizeof(double);
  const size_t all = per_col * (size_t)(CB * 64), one = per_col * 64;
  const size_t cap = kGroupPartBudget > one ? kGroupPartBudget : one;
  q.part_bytes = all < cap ? all : cap;
  int64_t cr = (int64_t)(q.part_bytes / one) * 64;
  if (cr > CB * 64) cr = CB * 64;
  if (cr > (int64_t)65535 * 64) cr = (int64_t)65535 * 64;
  q.CR = (int)cr;
  return q;
}

// grid ceil(B / kGroupRowChunk), kGroupRowChunk threads; tbl zeroed
__global__ __launch_bounds__(kGroupRowChunk) void group_rank_kernel(int64_t B, int G,
                                                                     const int32_t* __restrict__ labels,
                                                                     int32_t* __restrict__ lrank,
                                                                     int32_t* __restrict__ tbl) {
  __shared__ int32_t lab[kGroupRowChunk];
  const int t = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x * kGroupRowChunk + t;
  int g = -1;
  if (b < B) {
    g = labels[b];
    if (g < 0 || g >= G) g = -1;
  }
  lab[t] = g;
  __syncthreads();
  if (g < 0) return;
  int before = 0, after = 0;
  for (int j = 0; j < kGroupRowChunk; ++j) {
    const bool same = lab[j] == g;
    before += same && j < t;
    after += same && j > t;
  }
  lrank[b] = before;
  if (!after) tbl[(size_t)blockIdx.x * G + g] = before + 1;   // the group's last row of the chunk
}

// grid G, one wave: tbl[chunk][g] -> rows of g in the chunks before; cnt[g] = rows of g
__global__ __launch_bounds__(64) void group_scan_kernel(int64_t chunks, int G, int32_t* __restrict__ tbl,
                                                        int32_t* __restrict__ cnt) {
  const int g = blockIdx.x, lane = threadIdx.x;
  int carry = 0;
  for (int64_t c0 = 0; c0 < chunks; c0 += 64) {
    const int64_t c = c0 + lane;
    const int v = c < chunks ? tbl[(size_t)c * G + g] : 0;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o);
      if (lane >= o) inc += u;
    }
    if (c < chunks) tbl[(size_t)c * G + g] = carry + inc - v;
    carry += __shfl(inc, 63);
  }
  if (lane == 0) cnt[g] = carry;
}

// one workgroup of 256: boff[g] = first block of group g (exclusive scan of ceil(cnt / 64)), boff[G] = blocks in
// use; fincl[g] = groups g' <= g with rows whose first block is not a multiple of RB
__global__ __launch_bounds__(256) void group_offsets_kernel(int G, int RB, const int32_t* __restrict__ cnt,
                                                            int32_t* __restrict__ boff,
                                                            int32_t* __restrict__ fincl) {
  __shared__ int sh[256];
  const int t = threadIdx.x;
  for (int pass = 0; pass < 2; ++pass) {
    int carry = 0;
    for (int g0 = 0; g0 < G; g0 += 256) {
      const int g = g0 + t;
      int v = 0;
      // (pass 1 reads the boff[g] that this thread wrote in pass 0)
      if (g < G) v = pass == 0 ? (cnt[g] + 63) / 64 : (cnt[g] > 0 && boff[g] % RB != 0);
      sh[t] = v;
      __syncthreads();
      for (int o = 1; o < 256; o <<= 1) {
        const int u = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += u;
        __syncthreads();
      }
      const int inc = sh[t], tot = sh[255];
      if (g < G) {
        if (pass == 0) boff[g] = carry + inc - v;
        else fincl[g] = carry + inc;
      }
      carry += tot;
      __syncthreads();
    }
    if (pass == 0 && t == 0) boff[G] = carry;
  }
}

// a thread per padded row slot p < 64 NB: perm[p] = -1; the first of a block writes its record
// (group, valid rows, segment, 0), group -1 for a surplus block
__global__ __launch_bounds__(256) void group_fill_kernel(int64_t NB, int G, int RB, const int32_t* __restrict__ cnt,
                                                         const int32_t* __restrict__ boff,
                                                         const int32_t* __restrict__ fincl,
                                                         int32_t* __restrict__ perm, int4* __restrict__ rec) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= NB * 64) return;
  perm[p] = -1;
  if (p & 63) return;
  const int nb = (int)(p >> 6);
  int4 r = make_int4(-1, 0, 0, 0);
  if (nb < boff[G]) {
    int lo = 0, hi = G - 1;            // the last g with boff[g] <= nb: the one group with rows there
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (boff[mid] <= nb) lo = mid;
      else hi = mid - 1;
    }
    const int left = cnt[lo] - (nb - boff[lo]) * 64;
    r = make_int4(lo, left < 64 ? left : 64, nb / RB + fincl[lo], 0);
  }
  rec[nb] = r;
}

// a thread per row
__global__ __launch_bounds__(256) void group_scatter_kernel(int64_t B, int G, const int32_t* __restrict__ labels,
                                                            const int32_t* __restrict__ lrank,
                                                            const int32_t* __restrict__ tbl,
                                                            const int32_t* __restrict__ boff,
                                                            int32_t* __restrict__ perm) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int g = labels[b];
  if (g < 0 || g >= G) return;
  const int64_t pos = (int64_t)boff[g] * 64 + tbl[(size_t)(b / kGroupRowChunk) * G + g] + lrank[b];
  perm[pos] = (int32_t)b;
}

// grid (ceil(NP * KP / 4 / 256), S): a thread per float4 of a padded row of one draw
__global__ __launch_bounds__(256) void group_gather_kernel(int64_t B, int64_t NP, int KP,
                                                           const int32_t* __restrict__ perm,
                                                           const float* __restrict__ z, float* __restrict__ zs) {
  const int K4 = KP / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= NP * K4) return;
  const int s = blockIdx.y;
  const int64_t p = i / K4;
  const int q = (int)(i - p * K4);
  const int b = perm[p];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (b >= 0) v = *reinterpret_cast<const float4*>(z + ((size_t)s * B + b) * KP + 4 * q);
  *reinterpret_cast<float4*>(zs + ((size_t)s * NP + p) * KP + 4 * q) = v;
}

// grid (runs, column blocks of the range, ceil(S / kGroupDrawChunk)).  C: the columns of Vp / phi / ctype; the
// range starts at column c0; part_*: [segment][S][CR], CR >= 64 gridDim.y.
template <int KC, int LIK, bool PNZ>
__global__ __launch_bounds__(256) void group_kernel(int64_t NP, int C, int KP, int S, int RB, int c0, int CR,
                                                    const float* __restrict__ zs, const float* __restrict__ Vp,
                                                    const float* __restrict__ phi,
                                                    const uint8_t* __restrict__ ctype,
                                                    const int4* __restrict__ rec,
                                                    const int32_t* __restrict__ n_blocks,
                                                    double* __restrict__ part_sum, double* __restrict__ part_nz) {
  constexpr int SC = kGroupDrawChunk;
  constexpr int NA = SC * 64 / 256;        // (draw, column) accumulators per thread
  __shared__ float tiles[2][2][64][KC + 4];
  __shared__ double stage[PNZ ? 2 : 1][2][SC][64];
  const int t = threadIdx.x;
  const int lane = t & 63, h = lane >> 5, i32 = lane & 31;
  const int wr = t >> 7, wc = t >> 6 & 1;
  const int s0 = blockIdx.z * SC;
  const int sc = S - s0 < SC ? S - s0 : SC;
  const int d0 = c0 + blockIdx.y * 64;
  const bool bern = score_col_bern<LIK>(ctype, C, score_tile_col(d0));
  const int64_t nb0 = (int64_t)blockIdx.x * RB;
  const int64_t nbe = *n_blocks;
  const int64_t nb1 = nb0 + RB < nbe ? nb0 + RB : nbe;
  if (nb0 >= nb1) return;                  // a surplus run

  double am[NA], az[PNZ ? NA : 1];
  auto flush = [&](int seg) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int idx = t + 256 * i;
      const int sl = idx >> 6, col = idx & 63;
      if (sl >= sc) continue;
      const size_t o = ((size_t)seg * S + s0 + sl) * CR + blockIdx.y * 64 + col;
      part_sum[o] = am[i];
      if constexpr (PNZ) part_nz[o] = az[i];
    }
  };
  int seg = -1;
  for (int64_t nb = nb0; nb < nb1; ++nb) {
    const int4 r = rec[nb];                // (group, valid rows, segment): the same for every thread
    if (r.z != seg) {
      if (seg >= 0) flush(seg);
      seg = r.z;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        am[i] = 0.0;
        if constexpr (PNZ) az[i] = 0.0;
      }
    }
    const int valid = r.y;
    score_tile_loop<KC>(tiles, NP, C, KP, sc, nb * 64, d0, zs + (size_t)s0 * NP * KP, Vp + (size_t)s0 * C * KP,
                        phi + (size_t)s0 * C, [&](int s, const score_f32x16& acc, float ph) {
      double sm = 0.0, sz = 0.0;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        float ey;
        const float rs = cell_rate(LIK, acc[q], ph, ey);
        const float ms = cell_mean(bern, rs);
        const bool in = score_tile_row(0, q, h) + 32 * wr < valid;
        sm = in ? sm + (double)ms : sm;
        if constexpr (PNZ) {
          const float pz = bern ? ms : -expm1f(-rs);
          sz = in ? sz + (double)pz : sz;
        }
      }
      // the two lane halves hold rows 4 h .. of the same column: one addition, the same bits in both lanes
      const double tm = sm + __shfl_xor(sm, 32);
      if (h == 0) stage[0][wr][s][wc * 32 + i32] = tm;
      if constexpr (PNZ) {
        const double tz = sz + __shfl_xor(sz, 32);
        if (h == 0) stage[PNZ ? 1 : 0][wr][s][wc * 32 + i32] = tz;
      }
    });
    // (the loop's last barrier is behind the last callback; the next loop's first one is behind these reads)
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int idx = t + 256 * i;
      const int sl = idx >> 6, col = idx & 63;
      if (sl >= sc) continue;
      am[i] += stage[0][0][sl][col] + stage[0][1][sl][col];
      if constexpr (PNZ) az[i] += stage[PNZ ? 1 : 0][0][sl][col] + stage[PNZ ? 1 : 0][1][sl][col];
    }
  }
  flush(seg);
}

// a thread per (draw, group, column of the range): out += the group's segments in ascending order
__global__ __launch_bounds__(256) void group_combine_kernel(int S, int G, int C, int c0, int cw, int CR,
                                                            const int32_t* __restrict__ cnt,
                                                            const int32_t* __restrict__ boff,
                                                            const int4* __restrict__ rec,
                                                            const double* __restrict__ part_sum,
                                                            const double* __restrict__ part_nz,
                                                            double* __restrict__ sum, double* __restrict__ nz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)S * G * cw) return;
  const int j = (int)(i % cw);
  const int64_t sg = i / cw;
  const int g = (int)(sg % G), s = (int)(sg / G);
  if (cnt[g] <= 0) return;
  const int seg0 = rec[boff[g]].z, seg1 = rec[boff[g + 1] - 1].z;
  const size_t o = ((size_t)s * G + g) * C + c0 + j;
  double a = sum[o];
  for (int seg = seg0; seg <= seg1; ++seg) a += part_sum[((size_t)seg * S + s) * CR + j];
  sum[o] = a;
  if (nz) {
    double b = nz[o];
    for (int seg = seg0; seg <= seg1; ++seg) b += part_nz[((size_t)seg * S + s) * CR + j];
    nz[o] = b;
  }
}

// The ordering alone (kmeans.hip orders its rows by label with it): tbl [ceil(B / kGroupRowChunk)][G], lrank [B],
// cnt [G], boff [G + 1], fincl [G], perm [64 NB], rec [NB] with NB = ceil(B / 64) + G; RB numbers the segments.
void launch_group_order(int64_t B, int G, int RB, const int32_t* labels, const GroupOrder& o, hipStream_t st) {
  const int64_t chunks = (B + kGroupRowChunk - 1) / kGroupRowChunk;
  const int64_t NB = (B + 63) / 64 + G, NP = NB * 64;
  launch_zero(o.tbl, (size_t)chunks * G * sizeof(int32_t), st);
  hipLaunchKernelGGL(group_rank_kernel, dim3((unsigned)chunks), dim3(kGroupRowChunk), 0, st, B, G, labels, o.lrank,
                     o.tbl);
  hipLaunchKernelGGL(group_scan_kernel, dim3((unsigned)G), dim3(64), 0, st, chunks, G, o.tbl, o.cnt);
  hipLaunchKernelGGL(group_offsets_kernel, dim3(1), dim3(256), 0, st, G, RB, o.cnt, o.boff, o.fincl);
  hipLaunchKernelGGL(group_fill_kernel, dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, st, NB, G, RB, o.cnt, o.boff,
                     o.fincl, o.perm, o.rec);
  hipLaunchKernelGGL(group_scatter_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, B, G, labels, o.lrank,
                     o.tbl, o.boff, o.perm);
}

bool launch_groups(const GroupArgs& a, hipStream_t st) {
  DrawTables t = a.t;
  const int C = a.n_cols, G = a.n_groups;
  if (!with_kc(t.KP, [](auto) {}) || !with_lik(t.lik, [](auto) {})) return false;
  if (t.B <= 0 || C <= 0) return true;
  const GroupGeom q = group_geom(t.B, t.S, G, C);
  const int64_t NP = q.NB * 64;
  const GroupOrder& o = a.ord;

  launch_group_order(t.B, G, q.RB, a.labels, o, st);
  const int64_t n4 = NP * (t.KP / 4);
  hipLaunchKernelGGL(group_gather_kernel, dim3((unsigned)((n4 + 255) / 256), (unsigned)t.S), dim3(256), 0, st, t.B,
                     NP, t.KP, o.perm, t.z, a.zs);
  if (a.cols) {
    uint8_t* ctc = t.lik == 3 ? a.ctc : nullptr;
    launch_panel_gather(t, C, a.cols, a.Vc, a.phic, ctc, st);
    t.Vp = a.Vc;
    t.phi = a.phic;
    t.ctype = ctc;
  }
  double* part_sum = a.part;
  double* part_nz = a.part + (size_t)q.nseg * t.S * q.CR;
  const unsigned gz = (unsigned)((t.S + kGroupDrawChunk - 1) / kGroupDrawChunk);
  for (int c0 = 0; c0 < C; c0 += q.CR) {
    const int cw = C - c0 < q.CR ? C - c0 : q.CR;
    const dim3 grid((unsigned)q.runs, (unsigned)((cw + 63) / 64), gz);
    with_kc(t.KP, [&](auto kc) {
      with_lik(t.lik, [&](auto lik) {
        auto go = [&](auto pz) {
          hipLaunchKernelGGL((group_kernel<decltype(kc)::value, decltype(lik)::value, decltype(pz)::value>), grid,
                             dim3(256), 0, st, NP, C, t.KP, t.S, q.RB, c0, q.CR, a.zs, t.Vp, t.phi, t.ctype, o.rec,
                             o.boff + G, part_sum, part_nz);
        };
        if (a.nonzero) go(std::true_type{});
        else go(std::false_type{});
      });
    });
    const int64_t n = (int64_t)t.S * G * cw;
    hipLaunchKernelGGL(group_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t.S, G, C, c0, cw,
                       q.CR, o.cnt, o.boff, o.rec, part_sum, part_nz, a.sum, a.nonzero);
  }
  return true;
}

}  // namespace spmf
