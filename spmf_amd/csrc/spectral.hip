// spectral.hip -- multiplying by the graph: graph_scale, graph_spmm, block_gram, block_rotate (include/spmf_hip.h
// has the definitions; spmf_amd/spectral.py is the eigensolver they serve).
//
// A block is fp32 [n_rows][16] row-major: a row is one 64-byte segment.  graph_spmm is the hot path and has the
// access pattern of graph_layout.hip turned by ninety degrees: a row owns a group of 16 lanes, four rows to a wave,
// but lane l owns COLUMN l of the row and the group walks the row's list together in list order.  The index and
// the weight of an entry are one address for the group, the gather of X_j is the group's one 64-byte request, and a
// column's sum is a chain of fmaf in one lane: no cross-lane reduction, no atomic, and an entry of Y is a function
// of its row's list alone -- not of the grid, of the other rows or of where the row sits in its wave.  The chain
// would be one dependent L2 latency per entry; the list is therefore walked kUnroll entries at a time, all of a
// step's loads (index, weight, scale, the row of X) issued before the first fmaf of the step.  An entry that does
// not count (index outside [0, n_rows), weight not finite and > 0, or behind the list's end) loads the row's own
// X_i instead and is dropped by a select, never multiplied by zero: a NaN reaches the rows that list it only.
//
// graph_scale sums a row's valid weights as graph_layout sums W: lane l takes the entries l, l + 16, .. in
// ascending order, in fp64, then a fixed xor tree over the 16 lanes.
//
// block_gram is x^T y in fp64.  The rows are cut into chunks of kGramChunk, a constant: a 256-thread workgroup
// takes a chunk, thread (a, b) adds x_ra y_rb in ascending r through LDS tiles of 64 rows (the products of two fp32
// are exact in fp64, so only the additions round), and a second launch of one workgroup adds the chunks' partial
// sums in ascending chunk order.  block_rotate reads a row whole, forms its 16 fp64 sums over ascending k against
// R in LDS and rounds each once.
//
// Nothing here trusts the graph: an indptr value is clamped to [0, nnz], a falling indptr is an empty row
// (graph_rows.h: the row of a lane group, shared with graph_paths.hip).
#include "common.h"
#include "graph_rows.h"
#include "kernels.h"

namespace spmf {

namespace {

constexpr int kGramTile = 64;                         // rows of an LDS tile of block_gram
static_assert(kGramChunk % kGramTile == 0, "a chunk is whole tiles");

// the fixed tree over an aligned group of 16 lanes, fp64: every lane ends up with the same bits
__device__ __forceinline__ double group16_sum(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

}  // namespace

__global__ __launch_bounds__(256) void graph_scale_kernel(GraphCsr g, float* __restrict__ scale) {
  const int sub = threadIdx.x & (kRowLanes - 1);
  const RowList r = row_list(g);
  const uint32_t n32 = (uint32_t)g.n_rows;            // n_rows <= 2^31 - 64 (checked on the host)
  double d = 0.0;
  for (int64_t p = r.p0 + sub; p < r.p1; p += kRowLanes) {
    const uint32_t j = (uint32_t)g.indices[p];
    const float w = g.weights[p];
    if (j < n32 && weight_counts(w)) d += (double)w;
  }
  d = group16_sum(d);
  if (sub == 0 && r.live) scale[r.i] = d > 0.0 ? (float)(1.0 / sqrt(d)) : 0.f;
}

__global__ __launch_bounds__(256) void graph_spmm_kernel(GraphCsr g, const float* __restrict__ scale,
                                                         const float* __restrict__ x, const float* z, float* y,
                                                         float cs, BlockCoef coef, float cz) {
  const int sub = threadIdx.x & (kRowLanes - 1);
  const RowList r = row_list(g);
  if (!r.live) return;                                // whole groups leave: nothing below crosses lanes
  const uint32_t n32 = (uint32_t)g.n_rows;
  const uint32_t self = (uint32_t)r.i;
  float cx = 0.f;
#pragma unroll
  for (int k = 0; k < kBlockCols; ++k) cx = sub == k ? coef.cx[k] : cx;
  const size_t at = (size_t)r.i * kBlockCols + sub;
  const float xi = x[at];
  const float si = scale ? scale[r.i] : 1.f;
  const float zi = z ? z[at] : 0.f;

  float acc = 0.f;
  for (int64_t p = r.p0; p < r.p1; p += kUnroll) {
    uint32_t j[kUnroll];
    float w[kUnroll], sj[kUnroll], xj[kUnroll];
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
      sj[u] = scale ? scale[row] : 1.f;
      xj[u] = x[(size_t)row * kBlockCols + sub];
    }
    // list order
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const float t = fmaf(w[u] * sj[u], xj[u], acc);
      acc = ok[u] ? t : acc;
    }
  }
  y[at] = fmaf(cz, zi, fmaf(cx, xi, (cs * si) * acc));
}

__global__ __launch_bounds__(256) void block_gram_kernel(int64_t n_rows, const float* __restrict__ x,
                                                         const float* __restrict__ y, double* __restrict__ partial) {
  __shared__ float xs[kGramTile][kBlockCols];
  __shared__ float ys[kGramTile][kBlockCols];
  const int t = threadIdx.x, a = t / kBlockCols, b = t % kBlockCols;
  const int64_t r0 = (int64_t)blockIdx.x * kGramChunk;
  const int64_t r1 = min(r0 + kGramChunk, n_rows);
  double acc = 0.0;
  for (int64_t base = r0; base < r1; base += kGramTile) {
    const int rows = (int)min((int64_t)kGramTile, r1 - base);       // the same for the workgroup
    // a thread stages four columns of one row of each block (16 bytes)
    const int tr = t / 4, tc = (t % 4) * 4;
    float4 vx = make_float4(0.f, 0.f, 0.f, 0.f), vy = vx;
    if (tr < rows) {
      vx = *reinterpret_cast<const float4*>(x + (size_t)(base + tr) * kBlockCols + tc);
      vy = *reinterpret_cast<const float4*>(y + (size_t)(base + tr) * kBlockCols + tc);
    }
    __syncthreads();                                   // the tile before is read
    *reinterpret_cast<float4*>(&xs[tr][tc]) = vx;
    *reinterpret_cast<float4*>(&ys[tr][tc]) = vy;
    __syncthreads();
    for (int r = 0; r < rows; ++r) acc += (double)xs[r][a] * (double)ys[r][b];   // the product is exact
  }
  partial[(size_t)blockIdx.x * (kBlockCols * kBlockCols) + t] = acc;
}

__global__ __launch_bounds__(256) void block_gram_sum_kernel(int64_t chunks, const double* __restrict__ partial,
                                                             double* __restrict__ g) {
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int64_t c = 0; c < chunks; ++c) acc += partial[(size_t)c * (kBlockCols * kBlockCols) + t];
  g[t] = acc;
}

__global__ __launch_bounds__(256) void block_rotate_kernel(int64_t n_rows, const float* x, BlockRot rot, float* y) {
  __shared__ double rs[kBlockCols][kBlockCols];
  const int t = threadIdx.x, b = t & (kRowLanes - 1);
  rs[t / kBlockCols][b] = rot.r[t];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kRowsPerBlock + (t / kRowLanes);
  if (i >= n_rows) return;
  // the row whole, in every lane of its group, before the group writes any of it: y may be x
  const float4* row = reinterpret_cast<const float4*>(x + (size_t)i * kBlockCols);
  const float4 q0 = row[0], q1 = row[1], q2 = row[2], q3 = row[3];
  const float xr[kBlockCols] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                                q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < kBlockCols; ++k) acc = fma((double)xr[k], rs[k][b], acc);
  y[(size_t)i * kBlockCols + b] = (float)acc;
}

void launch_graph_scale(const GraphCsr& g, float* scale, hipStream_t st) {
  hipLaunchKernelGGL(graph_scale_kernel, dim3(row_blocks(g.n_rows)), dim3(256), 0, st, g, scale);
}

void launch_graph_spmm(const GraphCsr& g, const float* scale, const float* x, const float* z, float* y, float cs,
                       const BlockCoef& cx, float cz, hipStream_t st) {
  hipLaunchKernelGGL(graph_spmm_kernel, dim3(row_blocks(g.n_rows)), dim3(256), 0, st, g, scale, x, z, y, cs, cx, cz);
}

void launch_block_gram(int64_t n_rows, const float* x, const float* y, double* partial, double* g, hipStream_t st) {
  const int64_t chunks = gram_chunks(n_rows);                       // < 2^22
  hipLaunchKernelGGL(block_gram_kernel, dim3((unsigned)chunks), dim3(256), 0, st, n_rows, x, y, partial);
  hipLaunchKernelGGL(block_gram_sum_kernel, dim3(1), dim3(256), 0, st, chunks, partial, g);
}

void launch_block_rotate(int64_t n_rows, const float* x, const BlockRot& r, float* y, hipStream_t st) {
  hipLaunchKernelGGL(block_rotate_kernel, dim3(row_blocks(n_rows)), dim3(256), 0, st, n_rows, x, r, y);
}

}  // namespace spmf
