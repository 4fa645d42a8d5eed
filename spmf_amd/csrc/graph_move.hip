// graph_move.hip -- one Jacobi sweep of modularity moves (include/spmf_hip.h spmf_graph_move has the definition;
// spmf_amd/communities.py is the driver the sweep serves, and its NumpyOps.move the restatement it is held to bit
// for bit).
//
// Weights are int64 fixed point, so k_i, e_ic and e_ia are exact whatever the order of their additions; the score
// is (double)e - ((gamma (double)k) (double)tot) / (double)m2, each operation rounded once (no contraction).  Both
// kernels form the same integers and call the same score function, so a row that both see gets the same bits.
//
// One method, two tilings: for every entry of a row, the sum of the link weights of the row's entries that carry
// the entry's label (all pairs), then the arg-max of the admitted entries' scores under (score descending, label
// ascending).  Entries that share a label have the same sum and the same score, so the arg-max needs no marking of
// duplicates.
//
// Group path: a row of at most kMoveGroupLen = 64 entries owns 16 lanes, four rows to a wave, as in spectral.hip.
// Lane l holds the entries l, l + 16, l + 32, l + 48 in registers; the index and weight loads of all four are
// issued first, then the four label gathers, then the four gathers of tot, which the broadcast steps hide: one
// step per entry of the list (none for a quarter behind the list's end), in which each of a lane's four slots adds
// the broadcast weight on an equal label.  k_i, e_ia and the arg-max come from the fixed xor tree over the 16 lanes.
// A longer row gets its own label back.
//
// Wide path: a 256-thread workgroup per row of long_rows, launched behind the group path on the same stream.  A
// thread owns one candidate of a 256-entry tile; for every candidate tile the whole row streams through LDS tiles
// of 256 (label, link weight), each read by all threads at one address.  Any length, no table, no capacity, no
// atomic -- at O(d^2 / 256) steps per thread and as many label gathers per row of d entries: the price of having
// no table.  A fixed fold over the workgroup gives the arg-max.
//
// Nothing here trusts the graph or the labels: an indptr value is clamped to [0, nnz], a falling indptr is an
// empty row, a column outside [0, n_rows) or a weight below 1 does not count, a label outside [0, n_rows) is never
// a candidate (tot is not read at it), a row of long_rows outside [0, n_rows) is skipped.
#include "common.h"
#include "kernels.h"

namespace spmf {

namespace {

constexpr int kLanes = 16;
constexpr int kRowsPerBlock = 256 / kLanes;
constexpr int kSlots = kMoveGroupLen / kLanes;        // entries of a row per lane
constexpr int kTile = 256;                            // entries of an LDS tile, candidates of a pass
constexpr int32_t kNone = 0x7fffffff;                 // no candidate: loses to every label
static_assert(kMoveGroupLen == 64 && kSlots == 4, "a lane holds four entries");

// score(c): each operation rounded on its own
__device__ __forceinline__ double move_score(int64_t e, double gk, int64_t tot, double m2) {
#pragma clang fp contract(off)
  const double p = gk * (double)tot;
  const double q = p / m2;
  return (double)e - q;
}

__device__ __forceinline__ double scaled_degree(double gamma, int64_t k) {
#pragma clang fp contract(off)
  return gamma * (double)k;
}

__device__ __forceinline__ bool better(double s, int32_t c, double s0, int32_t c0) {
  return s > s0 || (s == s0 && c < c0);
}

__device__ __forceinline__ bool admitted(int32_t c, int32_t own, int direction) {
  return direction == 0 ? c > own : c < own;
}

__device__ __forceinline__ int64_t clamped(int64_t v, int64_t nnz) { return min(max(v, (int64_t)0), nnz); }

// the fixed tree over an aligned group of 16 lanes: every lane ends up with the same value
__device__ __forceinline__ int64_t group16_sum(int64_t v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

}  // namespace

__global__ __launch_bounds__(256) void graph_move_group_kernel(MoveArgs a) {
  const int sub = threadIdx.x & (kLanes - 1);
  const int64_t i = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x / kLanes);
  if (i >= a.n_rows) return;                          // whole groups leave: a shuffle below stays inside its group
  const uint32_t n32 = (uint32_t)a.n_rows;            // n_rows <= 2^31 - 64 (checked on the host)
  const uint32_t self = (uint32_t)i;
  const int64_t p0 = clamped(a.indptr[i], a.nnz), p1 = clamped(a.indptr[i + 1], a.nnz);
  const int64_t len = p1 - p0;
  const int32_t own = a.labels_in[i];
  if (len <= 0 || len > kMoveGroupLen || (uint32_t)own >= n32) {   // the same for the 16 lanes
    if (sub == 0) a.labels_out[i] = own;
    return;
  }
  // the loads first: the entries, then what they point to
  uint32_t col[kSlots];
  int64_t w[kSlots];
  bool ok[kSlots];
#pragma unroll
  for (int q = 0; q < kSlots; ++q) {
    const int64_t p = p0 + q * kLanes + sub;
    ok[q] = p < p1;
    const int64_t at = ok[q] ? p : p0;                // behind the end: the first entry again, dropped below
    col[q] = (uint32_t)a.indices[at];
    w[q] = a.wq[at];
  }
  int32_t lab[kSlots];
#pragma unroll
  for (int q = 0; q < kSlots; ++q) {
    ok[q] = ok[q] && col[q] < n32 && w[q] >= 1;
    lab[q] = a.labels_in[ok[q] ? col[q] : self];      // an entry that does not count reads this row's own
  }
  int64_t link[kSlots], tot[kSlots];
  bool cand[kSlots];
  int64_t k = 0, ea = 0;
#pragma unroll
  for (int q = 0; q < kSlots; ++q) {
    const bool linked = ok[q] && col[q] != self;
    k += ok[q] ? w[q] : 0;
    link[q] = linked ? w[q] : 0;
    lab[q] = linked ? lab[q] : -1;                    // -1 adds 0 wherever it matches and is never a candidate
    ea += lab[q] == own ? link[q] : 0;
    cand[q] = linked && (uint32_t)lab[q] < n32 && admitted(lab[q], own, a.direction);
    tot[q] = a.tot[cand[q] ? lab[q] : own];
  }
  const int64_t tot_own = a.tot[own];
  // one broadcast step per entry of the list
  int64_t e[kSlots] = {0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    if (s * kLanes < len) {                           // the same for the 16 lanes
#pragma unroll
      for (int src = 0; src < kLanes; ++src) {
        const int32_t bl = __shfl(lab[s], src, kLanes);
        const int64_t bw = __shfl(link[s], src, kLanes);
#pragma unroll
        for (int q = 0; q < kSlots; ++q) e[q] += lab[q] == bl ? bw : 0;
      }
    }
  }
  k = group16_sum(k);
  ea = group16_sum(ea);
  const double gk = scaled_degree(a.gamma, k);
  const double stay = move_score(ea, gk, tot_own - k, a.m2);
  double best = -INFINITY;
  int32_t to = kNone;
#pragma unroll
  for (int q = 0; q < kSlots; ++q) {
    const double s = move_score(e[q], gk, tot[q], a.m2);
    const bool take = cand[q] && better(s, lab[q], best, to);
    best = take ? s : best;
    to = take ? lab[q] : to;
  }
#pragma unroll
  for (int m = 1; m < kLanes; m <<= 1) {
    const double s = __shfl_xor(best, m);
    const int32_t c = __shfl_xor(to, m);
    const bool take = better(s, c, best, to);
    best = take ? s : best;
    to = take ? c : to;
  }
  if (sub == 0) a.labels_out[i] = (k > 0 && to != kNone && best > stay) ? to : own;
}

__global__ __launch_bounds__(256) void graph_move_wide_kernel(MoveArgs a) {
  __shared__ int32_t s_lab[kTile];
  __shared__ int64_t s_link[kTile];
  __shared__ int64_t s_k[kTile], s_ea[kTile];
  __shared__ double s_best[kTile];
  __shared__ int32_t s_to[kTile];
  const int t = threadIdx.x;
  const uint32_t n32 = (uint32_t)a.n_rows;
  const uint32_t self = (uint32_t)a.long_rows[blockIdx.x];
  if (self >= n32) return;                            // the same for the workgroup, as every return below
  const int64_t i = (int64_t)self;
  const int64_t p0 = clamped(a.indptr[i], a.nnz), p1 = clamped(a.indptr[i + 1], a.nnz);
  const int32_t own = a.labels_in[i];
  if (p1 <= p0 || (uint32_t)own >= n32) {
    if (t == 0) a.labels_out[i] = own;
    return;
  }
  // (label, link weight, what the entry adds to k) of the entry at p; behind the end: (-1, 0, 0)
  auto entry = [&](int64_t p, int32_t& lab, int64_t& link, int64_t& kw) {
    const bool in = p < p1;
    const int64_t at = in ? p : p0;
    const uint32_t col = (uint32_t)a.indices[at];
    const int64_t w = a.wq[at];
    const bool ok = in && col < n32 && w >= 1;
    const int32_t l = a.labels_in[ok ? col : self];
    const bool linked = ok && col != self;
    kw = ok ? w : 0;
    link = linked ? w : 0;
    lab = linked ? l : -1;
  };
  // k_i and e_ia: a thread takes the entries t, t + 256, .., then a fixed fold
  int64_t k = 0, ea = 0;
  for (int64_t p = p0 + t; p < p1; p += kTile) {
    int32_t lab;
    int64_t link, kw;
    entry(p, lab, link, kw);
    k += kw;
    ea += lab == own ? link : 0;
  }
  s_k[t] = k;
  s_ea[t] = ea;
  __syncthreads();
  for (int h = kTile / 2; h > 0; h >>= 1) {
    if (t < h) {
      s_k[t] += s_k[t + h];
      s_ea[t] += s_ea[t + h];
    }
    __syncthreads();
  }
  k = s_k[0];
  ea = s_ea[0];
  if (k <= 0) {
    if (t == 0) a.labels_out[i] = own;
    return;
  }
  const double gk = scaled_degree(a.gamma, k);
  const double stay = move_score(ea, gk, a.tot[own] - k, a.m2);
  double best = -INFINITY;
  int32_t to = kNone;
  for (int64_t cb = p0; cb < p1; cb += kTile) {       // a tile of candidates, one per thread
    int32_t mine;
    int64_t mine_link, unused;
    entry(cb + t, mine, mine_link, unused);
    const bool cand = mine_link > 0 && (uint32_t)mine < n32 && admitted(mine, own, a.direction);
    const int64_t tot = a.tot[cand ? mine : own];
    int64_t e = 0;
    for (int64_t sb = p0; sb < p1; sb += kTile) {     // the row, a tile at a time
      int32_t lab;
      int64_t link;
      entry(sb + t, lab, link, unused);
      __syncthreads();                                // the tile before is read
      s_lab[t] = lab;
      s_link[t] = link;
      __syncthreads();
      const int cnt = (int)min((int64_t)kTile, p1 - sb);
#pragma unroll 8
      for (int j = 0; j < cnt; ++j) e += s_lab[j] == mine ? s_link[j] : 0;
    }
    const double s = move_score(e, gk, tot, a.m2);
    const bool take = cand && better(s, mine, best, to);
    best = take ? s : best;
    to = take ? mine : to;
  }
  s_best[t] = best;
  s_to[t] = to;
  __syncthreads();
  for (int h = kTile / 2; h > 0; h >>= 1) {
    if (t < h && better(s_best[t + h], s_to[t + h], s_best[t], s_to[t])) {
      s_best[t] = s_best[t + h];
      s_to[t] = s_to[t + h];
    }
    __syncthreads();
  }
  if (t == 0) a.labels_out[i] = (s_to[0] != kNone && s_best[0] > stay) ? s_to[0] : own;
}

void launch_graph_move(const MoveArgs& a, hipStream_t st) {
  const unsigned blocks = (unsigned)((a.n_rows + kRowsPerBlock - 1) / kRowsPerBlock);   // < 2^27
  hipLaunchKernelGGL(graph_move_group_kernel, dim3(blocks), dim3(256), 0, st, a);
  if (a.n_long > 0)                                   // behind the group path: it wrote these rows' own labels
    hipLaunchKernelGGL(graph_move_wide_kernel, dim3((unsigned)a.n_long), dim3(256), 0, st, a);
}

}  // namespace spmf
