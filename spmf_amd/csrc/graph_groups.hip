// graph_groups.hip -- the entries of a graph summed by the pair (label of the row, label of the column) into a
// dense G x G table: how often and how heavily every two groups of rows touch (include/spmf_hip.h
// spmf_graph_group_edges has the definition; spmf_amd/paga.py is the driver it serves, and its
// NumpyOps.group_edges the restatement it is held to bit for bit).
//
// Everything is an integer: the count of the entries and the int64 sum of their fixed-point weights.  Integer
// sums are exact in any order, so atomics are allowed here -- on integers only -- and two calls return the same
// bits.  What is not done is one global atomic per entry: in a real labelling most entries stay inside their
// group, and millions of adds would land on the G words of the diagonal.
//
// The rows are ordered by label first (launch_group_order, groups.hip: every group padded to whole 64-row blocks;
// its cnt is size_out).  A workgroup takes a run of RB consecutive blocks.  Every row of a block has the same
// label a, so the workgroup keeps row a of the two tables, count[G] and weight[G], in LDS (16 KB at G = 1024).
// A row owns 16 lanes, four rows to a wave, 16 rows to a pass and four passes to a block.  Its lanes walk the list
// 32 entries at a time, at any length: the index and weight loads of a lane's two entries are issued first, then
// the two label gathers.  An entry with b == a is summed in the lane's registers, across the rows of the
// segment; every other entry is one LDS integer atomic pair.  When the group changes or the run ends the registers
// are folded over the 16 lanes by the fixed xor tree, added to bin a, and the bins that are not zero go to the
// zeroed outputs with 64-bit global atomics: at most G per segment, never one per entry.
//
// Nothing here trusts the graph or the labels: an indptr value is clamped to [0, nnz], a falling indptr is an
// empty row, a column outside [0, n_rows), a weight below 1 or a label outside [0, G) at either end does not
// count; pad slots of the ordering (row -1) and surplus blocks are skipped.
#include "common.h"
#include "kernels.h"

namespace spmf {

namespace {

constexpr int kLanes = 16;
constexpr int kRowsPerPass = 256 / kLanes;
constexpr int kPasses = 64 / kRowsPerPass;            // passes over a 64-row block of the ordering
constexpr int kSlots = 2;                             // entries of a row per lane and step
using u64 = unsigned long long;

__device__ __forceinline__ int64_t clamped(int64_t v, int64_t nnz) { return min(max(v, (int64_t)0), nnz); }

// the fixed tree over an aligned group of 16 lanes: every lane ends up with the same value
__device__ __forceinline__ u64 group16_sum(u64 v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

}  // namespace

GroupEdgesGeom group_edges_geom(int64_t n_rows, int G) {
  GroupEdgesGeom q;
  q.NB = (n_rows + 63) / 64 + G;
  q.chunks = (n_rows + kGroupRowChunk - 1) / kGroupRowChunk;
  const int64_t runs = q.NB < kGroupEdgesTargetRuns ? q.NB : kGroupEdgesTargetRuns;
  q.RB = (int)((q.NB + runs - 1) / runs);
  q.runs = (int)((q.NB + q.RB - 1) / q.RB);
  return q;
}

// grid: the runs of RB blocks; n_blocks: the blocks in use (boff[G])
__global__ __launch_bounds__(256) void group_edges_kernel(GroupEdgesArgs a, int RB,
                                                          const int32_t* __restrict__ n_blocks) {
  __shared__ u64 s_cnt[kGroupEdgesMaxGroups], s_w[kGroupEdgesMaxGroups];
  const int t = threadIdx.x, sub = t & (kLanes - 1), slot0 = t / kLanes;
  const int G = a.n_groups;
  if (blockIdx.x == 0)
    for (int g = t; g < G; g += 256) a.size_out[g] = a.ord.cnt[g];
  const int64_t nb0 = (int64_t)blockIdx.x * RB;
  const int64_t nbe = *n_blocks;
  const int64_t nb1 = nb0 + RB < nbe ? nb0 + RB : nbe;
  if (nb0 >= nb1) return;                             // a surplus run: the same for the workgroup
  for (int b = t; b < G; b += 256) {
    s_cnt[b] = 0;
    s_w[b] = 0;
  }
  __syncthreads();
  const uint32_t n32 = (uint32_t)a.n_rows;            // n_rows <= 2^31 - 64 (checked on the host)
  u64 in_cnt = 0, in_w = 0;                           // the entries with b == a, of this lane, of this segment
  // the segment's bins -> the outputs; the same for the workgroup
  auto flush = [&](int own) {
    in_cnt = group16_sum(in_cnt);
    in_w = group16_sum(in_w);
    if (sub == 0 && in_cnt) {
      atomicAdd(&s_cnt[own], in_cnt);
      atomicAdd(&s_w[own], in_w);
    }
    in_cnt = in_w = 0;
    __syncthreads();
    for (int b = t; b < G; b += 256) {
      const u64 n = s_cnt[b];
      if (n) {                                        // (every counting entry has wq >= 1: no weight without a count)
        const size_t o = (size_t)own * G + b;
        atomicAdd(reinterpret_cast<u64*>(a.count_out) + o, n);
        atomicAdd(reinterpret_cast<u64*>(a.weight_out) + o, s_w[b]);
        s_cnt[b] = 0;
        s_w[b] = 0;
      }
    }
    __syncthreads();
  };
  int own = -1;
  for (int64_t nb = nb0; nb < nb1; ++nb) {
    const int4 r = a.ord.rec[nb];                     // (group, valid rows, ..): the same for every thread
    if (r.x < 0) break;                               // (a surplus block: none below boff[G])
    if (r.x != own) {
      if (own >= 0) flush(own);
      own = r.x;
    }
#pragma unroll
    for (int pass = 0; pass < kPasses; ++pass) {
      const int slot = pass * kRowsPerPass + slot0;
      const int32_t row = slot < r.y ? a.ord.perm[nb * 64 + slot] : -1;
      if (row < 0) continue;                          // a pad slot; the same for the 16 lanes
      const int64_t p0 = clamped(a.indptr[row], a.nnz), p1 = clamped(a.indptr[(int64_t)row + 1], a.nnz);
      for (int64_t q = p0; q < p1; q += kSlots * kLanes) {
        // the loads first: the entries, then what they point to
        uint32_t col[kSlots];
        int64_t w[kSlots];
        bool ok[kSlots];
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
          const int64_t p = q + s * kLanes + sub;
          ok[s] = p < p1;
          const int64_t at = ok[s] ? p : p0;          // behind the end: the first entry again, dropped below
          col[s] = (uint32_t)a.indices[at];
          w[s] = a.wq[at];
        }
        int32_t lab[kSlots];
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
          ok[s] = ok[s] && col[s] < n32 && w[s] >= 1;
          lab[s] = a.labels[ok[s] ? col[s] : (uint32_t)row];   // an entry that does not count reads this row's own
        }
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
          if (!ok[s] || (uint32_t)lab[s] >= (uint32_t)G) continue;
          if (lab[s] == own) {
            in_cnt += 1;
            in_w += (u64)w[s];
          } else {
            atomicAdd(&s_cnt[lab[s]], (u64)1);
            atomicAdd(&s_w[lab[s]], (u64)w[s]);
          }
        }
      }
    }
  }
  if (own >= 0) flush(own);
}

void launch_group_edges(const GroupEdgesArgs& a, hipStream_t st) {
  const int G = a.n_groups;
  const GroupEdgesGeom q = group_edges_geom(a.n_rows, G);
  launch_zero(a.count_out, (size_t)G * G * sizeof(int64_t), st);
  launch_zero(a.weight_out, (size_t)G * G * sizeof(int64_t), st);
  launch_group_order(a.n_rows, G, q.RB, a.labels, a.ord, st);
  hipLaunchKernelGGL(group_edges_kernel, dim3((unsigned)q.runs), dim3(256), 0, st, a, q.RB, a.ord.boff + G);
}

}  // namespace spmf
