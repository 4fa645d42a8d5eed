// graph_rows.h -- what the kernels that give a row of a CSR graph a group of 16 lanes, a lane per column of an
// fp32 [n_rows][16] block, have in common (spectral.hip: graph_scale, graph_spmm; graph_paths.hip: graph_relax):
// the tiling's constants, the rule by which a weight counts, and the row of a lane group with its clamped list.
// Nothing here trusts the graph: an indptr value is clamped to [0, nnz], a falling indptr is an empty row.
#pragma once
#include "common.h"
#include "kernels.h"

namespace spmf {

namespace {

constexpr int kRowLanes = kBlockCols;                 // a lane per column
constexpr int kRowsPerBlock = 256 / kRowLanes;
constexpr int kUnroll = 8;                            // entries of a row in flight per lane
static_assert(kBlockCols == 16, "a row is a 16-lane group");

__device__ __forceinline__ bool weight_counts(float w) { return w > 0.f && w < INFINITY; }

// the row of a lane group and its clamped list [p0, p1): empty for a dead group and for a falling indptr
struct RowList {
  int64_t i, p0, p1;
  bool live;
};
__device__ __forceinline__ RowList row_list(const GraphCsr& g) {
  RowList r;
  r.i = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x / kRowLanes);
  r.live = r.i < g.n_rows;                            // the same for the 16 lanes of a group
  r.p0 = r.p1 = 0;
  if (r.live) {
    r.p0 = min(max(g.indptr[r.i], (int64_t)0), g.nnz);
    r.p1 = min(max(g.indptr[r.i + 1], (int64_t)0), g.nnz);
  }
  return r;
}

}  // namespace

// the workgroups of a launch that gives every row a lane group
static unsigned row_blocks(int64_t n_rows) { return (unsigned)((n_rows + kRowsPerBlock - 1) / kRowsPerBlock); }   // < 2^27

}  // namespace spmf
