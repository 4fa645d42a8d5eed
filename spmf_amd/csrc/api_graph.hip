// api_graph.hip -- the calls on a graph as given behind the C-ABI (include/spmf_hip.h): the layout epochs
// (spmf_graph_layout, spmf_graph_transform), the graph products and block operations of spectral.hip
// (spmf_graph_scale, spmf_graph_spmm, spmf_block_gram, spmf_block_rotate), the sweep of graph_move.hip
// (spmf_graph_move), the group-to-group sums of graph_groups.hip (spmf_graph_group_edges) and the shortest-path
// sweeps of graph_paths.hip (spmf_graph_relax).  None runs the draw stage (api_stream.hip).  An entry is: graph_csr_check where it takes the CSR
// triple, its own argument checks, carve_scratch where it has a scratch, its empty return, its launch, `launched`.
// Host-side orchestration only (ctx.h).
#include "ctx.h"

using namespace spmf;

// The checks of every entry `f` that takes a graph as (indptr, indices, weights); the kernels check the values.
template <class W>
static int graph_csr_check(spmf_ctx* c, const std::string& f, int64_t n_rows, int64_t nnz, const int64_t* indptr,
    const int32_t* indices, const W* weights) {
  if (!rows_ok(n_rows)) return fail(c, SPMF_E_ARG, f + "n_rows must be in 0..2^31 - 64");
  if (nnz < 0) return fail(c, SPMF_E_ARG, f + "nnz is negative");
  if (n_rows > 0 && (!indptr || (nnz > 0 && (!indices || !weights)))) return fail(c, SPMF_E_ARG, f + "null argument");
  return SPMF_OK;
}
static std::string rows_shape(int64_t n_rows) { return "n_rows=" + std::to_string((long long)n_rows); }

// The schedule of graph_layout and graph_transform, checked and with every fp32 rounded once from fp64
static int layout_schedule(spmf_ctx* c, const std::string& f, int epoch0, int n_epochs, int total_epochs, double lr,
    double a, double b, double repulsion, double negative_rate, int n_negatives, uint64_t seed, LayoutSchedule& s) {
  auto weight_ok = [](double v) { return v >= 0.0 && v <= 3.0e38; };          // finite, not negative, an fp32
  if (n_negatives < 1 || n_negatives > 64) return fail(c, SPMF_E_ARG, f + "n_negatives must be in 1..64");
  if (epoch0 < 0 || n_epochs < 0 || (int64_t)epoch0 + n_epochs > (int64_t)total_epochs) return fail(c, SPMF_E_ARG,
      f + "epochs: epoch0 >= 0, n_epochs >= 0 and epoch0 + n_epochs <= total_epochs must hold");
  if (!(a > 0.0) || !(b > 0.0) || !(a <= 3.0e38) || !(b <= 3.0e38)) return fail(c, SPMF_E_ARG, f + "a and b must be "
      "positive and finite");
  if (!weight_ok(lr) || !weight_ok(repulsion) || !weight_ok(negative_rate)) return fail(c, SPMF_E_ARG, f + "lr, "
      "repulsion and negative_rate must be finite and not negative");
  s.epoch0 = epoch0; s.n_epochs = n_epochs; s.total_epochs = total_epochs; s.n_negatives = n_negatives;
  s.lr = lr;
  s.a = (float)a; s.b = (float)b;
  s.neg2b = (float)(-2.0 * b);
  s.two_gamma_b = (float)(2.0 * repulsion * b);
  s.rate_over_m = (float)(negative_rate / (double)n_negatives);
  s.seed_lo = (uint32_t)seed; s.seed_hi = (uint32_t)(seed >> 32);
  return SPMF_OK;
}

extern "C" {

// ---- the epochs of a 2-D graph layout (graph_layout.hip) ---------------------------------------
// Scratch of one call: the two position buffers the epochs alternate between; the first takes the start.
static void graph_layout_carve(Arena& a, int64_t rows, GraphLayoutArgs& ga) {
  const size_t n = rows > 0 ? (size_t)rows : 1;
  ga.buf[0] = a.take<float2>(n);
  ga.buf[1] = a.take<float2>(n);
}

size_t spmf_graph_layout_scratch_bytes(const spmf_ctx* c, int64_t n_rows) {
  if (!c || !rows_ok(n_rows)) return 0;
  GraphLayoutArgs ga{};
  return layout_bytes([&](Arena& a) { graph_layout_carve(a, n_rows, ga); });
}

int spmf_graph_layout(spmf_ctx* c, int64_t n_rows, int64_t nnz, const int64_t* indptr, const int32_t* indices,
    const float* weights, const float* y_in, float* y_out, int epoch0, int n_epochs, int total_epochs, double lr,
    double a, double b, double repulsion, double negative_rate, int n_negatives, uint64_t seed, void* scratch,
    size_t scratch_bytes, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "graph_layout: ";
  GraphLayoutArgs ga{};
  int rc = graph_csr_check(c, f, n_rows, nnz, indptr, indices, weights);
  if (!rc) rc = layout_schedule(c, f, epoch0, n_epochs, total_epochs, lr, a, b, repulsion, negative_rate, n_negatives,
      seed, ga.s);
  if (rc) return rc;
  if (n_rows > 0 && (!y_in || !y_out)) return fail(c, SPMF_E_ARG, f + "null argument");
  rc = carve_scratch(c, "graph_layout", scratch, scratch_bytes,
      [&](Arena& ar) { graph_layout_carve(ar, n_rows, ga); }, [&] { return rows_shape(n_rows); });
  if (rc) return rc;
  if (n_rows == 0) return SPMF_OK;
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = (size_t)n_rows * sizeof(float2);
  if (n_epochs == 0) {
    if (y_out != y_in) HIPCHK(c, hipMemcpyAsync(y_out, y_in, bytes, hipMemcpyDeviceToDevice, st));
    return SPMF_OK;
  }
  // the prologue: the start goes into the first buffer, so no epoch reads y_in or y_out (they may be one)
  HIPCHK(c, hipMemcpyAsync(ga.buf[0], y_in, bytes, hipMemcpyDeviceToDevice, st));
  ga.n_rows = n_rows; ga.nnz = nnz;
  ga.indptr = indptr; ga.indices = indices; ga.weights = weights;
  ga.y_out = (float2*)y_out;
  launch_graph_layout(ga, st);
  return launched(c, true, "");
}

// ---- new rows on a fitted 2-D layout (graph_transform.hip) --------------------------------------
// No scratch: the one launch keeps a row's state in registers.
int spmf_graph_transform(spmf_ctx* c, int64_t n_query, int k, const int32_t* idx, const float* w,
    const float* y_ref, int64_t n_ref, const float* y_in, float* y_out, int64_t row0, int epoch0, int n_epochs,
    int total_epochs, double lr, double a, double b, double repulsion, double negative_rate, int n_negatives,
    uint64_t seed, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "graph_transform: ";
  if (k < 1 || k > 64) return fail(c, SPMF_E_ARG, f + "k must be in 1..64");
  if (n_query < 0) return fail(c, SPMF_E_ARG, f + "n_query is negative");
  if (n_ref < 0 || n_ref > ((int64_t)1 << 31) - 1) return fail(c, SPMF_E_ARG, f + "n_ref must be in 0..2^31 - 1");
  if (row0 < 0 || row0 > ((int64_t)1 << 32) || n_query > ((int64_t)1 << 32) - row0) return fail(c, SPMF_E_ARG,
      f + "row0 >= 0 and row0 + n_query <= 2^32 must hold");
  GraphTransformArgs ga{};
  const int rc = layout_schedule(c, f, epoch0, n_epochs, total_epochs, lr, a, b, repulsion, negative_rate,
      n_negatives, seed, ga.s);
  if (rc) return rc;
  if ((n_query > 0 && (!idx || !w || !y_out)) || (n_ref > 0 && !y_ref)) return fail(c, SPMF_E_ARG,
      f + "null argument");
  if (!y_in && epoch0 > 0) return fail(c, SPMF_E_ARG, f + "y_in is null with epoch0 > 0: a continued schedule needs "
      "its positions");
  if (n_query == 0) return SPMF_OK;
  hipStream_t st = (hipStream_t)stream;
  if (n_epochs == 0 && y_in) {
    if (y_out != y_in) HIPCHK(c, hipMemcpyAsync(y_out, y_in, (size_t)n_query * sizeof(float2),
                                                hipMemcpyDeviceToDevice, st));
    return SPMF_OK;
  }
  ga.n_query = n_query; ga.n_ref = n_ref; ga.row0 = row0; ga.k = k;
  ga.idx = idx; ga.w = w;
  ga.y_ref = (const float2*)y_ref; ga.y_in = (const float2*)y_in; ga.y_out = (float2*)y_out;
  launch_graph_transform(ga, st);
  return launched(c, true, "");
}

// ---- multiplying by the graph (spectral.hip) ----------------------------------------------------
static bool coef_ok(double v) { return v >= -3.0e38 && v <= 3.0e38; }        // finite, an fp32

int spmf_graph_scale(spmf_ctx* c, int64_t n_rows, int64_t nnz, const int64_t* indptr, const int32_t* indices,
    const float* weights, float* scale, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "graph_scale: ";
  const int rc = graph_csr_check(c, f, n_rows, nnz, indptr, indices, weights);
  if (rc) return rc;
  if (n_rows > 0 && !scale) return fail(c, SPMF_E_ARG, f + "null argument");
  if (n_rows == 0) return SPMF_OK;
  launch_graph_scale(GraphCsr{n_rows, nnz, indptr, indices, weights}, scale, (hipStream_t)stream);
  return launched(c, true, "");
}

int spmf_graph_spmm(spmf_ctx* c, int64_t n_rows, int64_t nnz, const int64_t* indptr, const int32_t* indices,
    const float* weights, const float* scale, const float* x, const float* z, float* y, double c_s,
    const double* c_x, double c_z, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "graph_spmm: ";
  const int rc = graph_csr_check(c, f, n_rows, nnz, indptr, indices, weights);
  if (rc) return rc;
  if (!c_x || (n_rows > 0 && (!x || !y))) return fail(c, SPMF_E_ARG, f + "null argument");
  if (!coef_ok(c_s) || !coef_ok(c_z)) return fail(c, SPMF_E_ARG, f + "c_s and c_z must be finite");
  BlockCoef cx;
  for (int k = 0; k < kBlockCols; ++k) {
    if (!coef_ok(c_x[k])) return fail(c, SPMF_E_ARG, f + "c_x must be finite");
    cx.cx[k] = (float)c_x[k];
  }
  if (n_rows > 0 && !z && c_z != 0.0) return fail(c, SPMF_E_ARG, f + "null argument: z with c_z != 0");
  if (n_rows > 0 && y == x) return fail(c, SPMF_E_ARG, f + "y aliases x: other rows gather x (y may be z)");
  if (n_rows == 0) return SPMF_OK;
  launch_graph_spmm(GraphCsr{n_rows, nnz, indptr, indices, weights}, scale, x, c_z != 0.0 ? z : nullptr, y,
      (float)c_s, cx, (float)c_z, (hipStream_t)stream);
  return launched(c, true, "");
}

// ---- shortest-path sweeps on the graph (graph_paths.hip) ------------------------------------------
// Scratch of one call: the two blocks the sweeps alternate between; the first takes the start.
static void graph_relax_carve(Arena& a, int64_t rows, GraphRelaxArgs& ga) {
  const size_t n = (rows > 0 ? (size_t)rows : 1) * kBlockCols;
  ga.buf[0] = a.take<float>(n);
  ga.buf[1] = a.take<float>(n);
}

size_t spmf_graph_relax_scratch_bytes(const spmf_ctx* c, int64_t n_rows) {
  if (!c || !rows_ok(n_rows)) return 0;
  GraphRelaxArgs ga{};
  return layout_bytes([&](Arena& a) { graph_relax_carve(a, n_rows, ga); });
}

int spmf_graph_relax(spmf_ctx* c, int64_t n_rows, int64_t nnz, const int64_t* indptr, const int32_t* indices,
    const float* lengths, const float* x_in, float* x_out, int32_t* pred_out, int32_t* changed_out, int n_sweeps,
    void* scratch, size_t scratch_bytes, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "graph_relax: ";
  GraphRelaxArgs ga{};
  int rc = graph_csr_check(c, f, n_rows, nnz, indptr, indices, lengths);
  if (rc) return rc;
  if (n_sweeps < 0) return fail(c, SPMF_E_ARG, f + "n_sweeps is negative");
  if (n_rows > 0 && (!x_in || !x_out)) return fail(c, SPMF_E_ARG, f + "null argument");
  const void* outs[3] = {x_out, pred_out, changed_out};
  const void* ins[4] = {indptr, indices, lengths, x_in};
  for (int o = 0; o < 3; ++o) {
    if (!outs[o]) continue;
    for (int i = 0; i < 4; ++i)
      if (outs[o] == ins[i] && !(o == 0 && i == 3)) return fail(c, SPMF_E_ARG, f + "an output aliases an input: "
          "the sweeps read the graph while they write (only x_out may be x_in)");
    for (int p = 0; p < o; ++p)
      if (outs[o] == outs[p]) return fail(c, SPMF_E_ARG, f + "an output aliases another output");
  }
  rc = carve_scratch(c, "graph_relax", scratch, scratch_bytes,
      [&](Arena& ar) { graph_relax_carve(ar, n_rows, ga); }, [&] { return rows_shape(n_rows); });
  if (rc) return rc;
  if (n_rows == 0) return SPMF_OK;
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = (size_t)n_rows * kBlockCols * sizeof(float);
  if (n_sweeps == 0) {
    if (x_out != x_in) HIPCHK(c, hipMemcpyAsync(x_out, x_in, bytes, hipMemcpyDeviceToDevice, st));
    if (changed_out) launch_zero(changed_out, sizeof(int32_t), st);
    return launched(c, true, "");
  }
  // the prologue: the start goes into the first buffer, so no sweep reads x_in or x_out (they may be one)
  HIPCHK(c, hipMemcpyAsync(ga.buf[0], x_in, bytes, hipMemcpyDeviceToDevice, st));
  ga.n_rows = n_rows; ga.nnz = nnz;
  ga.indptr = indptr; ga.indices = indices; ga.lengths = lengths;
  ga.x_out = x_out; ga.pred_out = pred_out; ga.changed_out = changed_out; ga.n_sweeps = n_sweeps;
  launch_graph_relax(ga, st);
  return launched(c, true, "");
}

// ---- modularity moves on the graph (graph_move.hip) ----------------------------------------------
int spmf_graph_move(spmf_ctx* c, int64_t n_rows, int64_t nnz, const int64_t* indptr, const int32_t* indices,
    const int64_t* wq, const int32_t* labels_in, const int64_t* tot, const int32_t* long_rows, int64_t n_long,
    double gamma, int64_t m2, int direction, int32_t* labels_out, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "graph_move: ";
  const int rc = graph_csr_check(c, f, n_rows, nnz, indptr, indices, wq);
  if (rc) return rc;
  if (!rows_ok(n_long)) return fail(c, SPMF_E_ARG, f + "n_long must be in 0..2^31 - 64");
  if (n_rows > 0 && (!labels_in || !tot || !labels_out)) return fail(c, SPMF_E_ARG, f + "null argument");
  if (n_long > 0 && !long_rows) return fail(c, SPMF_E_ARG, f + "null argument: long_rows with n_long > 0");
  if (!(gamma > 0.0 && gamma <= 1.7e308)) return fail(c, SPMF_E_ARG, f + "gamma must be finite and > 0");
  if (m2 <= 0) return fail(c, SPMF_E_ARG, f + "m2 must be > 0");
  if (direction != 0 && direction != 1) return fail(c, SPMF_E_ARG, f + "direction must be 0 (up) or 1 (down)");
  if (n_rows > 0 && labels_out == labels_in)
    return fail(c, SPMF_E_ARG, f + "labels_out aliases labels_in: other rows read labels_in");
  if (n_rows == 0) return SPMF_OK;
  MoveArgs ma{};
  ma.n_rows = n_rows; ma.nnz = nnz; ma.indptr = indptr; ma.indices = indices; ma.wq = wq;
  ma.labels_in = labels_in; ma.tot = tot; ma.long_rows = long_rows; ma.n_long = n_long;
  ma.gamma = gamma; ma.m2 = (double)m2; ma.direction = direction; ma.labels_out = labels_out;
  launch_graph_move(ma, (hipStream_t)stream);
  return launched(c, true, "");
}

// ---- the entries summed by the labels of their two ends (graph_groups.hip behind groups.hip's ordering) ----------
// Scratch of one call: the ordering of the rows by label (launch_group_order); every region grows with the rows.
static bool group_edges_groups_ok(int32_t G) { return G >= 1 && G <= kGroupEdgesMaxGroups; }
static void group_edges_carve(Arena& a, int64_t rows, int G, GroupEdgesArgs& ga) {
  const GroupEdgesGeom q = group_edges_geom(rows, G);
  group_order_carve(a, rows, G, q.chunks, q.NB, ga.ord);
}

size_t spmf_graph_group_edges_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int32_t n_groups) {
  if (!c || !rows_ok(n_rows) || !group_edges_groups_ok(n_groups)) return 0;
  GroupEdgesArgs ga{};
  return layout_bytes([&](Arena& a) { group_edges_carve(a, n_rows, n_groups, ga); });
}

int spmf_graph_group_edges(spmf_ctx* c, int64_t n_rows, int64_t nnz, const int64_t* indptr, const int32_t* indices,
    const int64_t* wq, const int32_t* labels, int32_t n_groups, int64_t* count_out, int64_t* weight_out,
    int64_t* size_out, void* scratch, size_t scratch_bytes, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "graph_group_edges: ";
  int rc = graph_csr_check(c, f, n_rows, nnz, indptr, indices, wq);
  if (rc) return rc;
  if (!group_edges_groups_ok(n_groups)) return fail(c, SPMF_E_ARG, f + "n_groups must be in 1..1024");
  if (!count_out || !weight_out || !size_out || (n_rows > 0 && !labels)) return fail(c, SPMF_E_ARG,
      f + "null argument");
  const void* outs[3] = {count_out, weight_out, size_out};
  const void* ins[4] = {indptr, indices, wq, labels};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 4; ++i)
      if (outs[o] == ins[i]) return fail(c, SPMF_E_ARG, f + "an output aliases an input: the kernel reads the graph "
          "and the labels while it adds to the outputs");
    for (int p = 0; p < o; ++p)
      if (outs[o] == outs[p]) return fail(c, SPMF_E_ARG, f + "an output aliases another output");
  }
  GroupEdgesArgs ga{};
  rc = carve_scratch(c, "graph_group_edges", scratch, scratch_bytes,
      [&](Arena& a) { group_edges_carve(a, n_rows, n_groups, ga); },
      [&] { return rows_shape(n_rows) + " n_groups=" + std::to_string(n_groups); });
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (n_rows == 0) {
    const size_t table = (size_t)n_groups * n_groups * sizeof(int64_t);
    HIPCHK(c, hipMemsetAsync(count_out, 0, table, st));
    HIPCHK(c, hipMemsetAsync(weight_out, 0, table, st));
    HIPCHK(c, hipMemsetAsync(size_out, 0, (size_t)n_groups * sizeof(int64_t), st));
    return SPMF_OK;
  }
  ga.n_rows = n_rows; ga.nnz = nnz; ga.indptr = indptr; ga.indices = indices; ga.wq = wq;
  ga.labels = labels; ga.n_groups = n_groups;
  ga.count_out = count_out; ga.weight_out = weight_out; ga.size_out = size_out;
  launch_group_edges(ga, st);
  return launched(c, true, "");
}

// ---- blocks of SPMF_BLOCK_COLS columns (spectral.hip) ----------------------------------------------
// Scratch of one block_gram: the chunks' partial sums.
static double* block_gram_carve(Arena& a, int64_t rows) {
  return a.take<double>((size_t)(rows > 0 ? gram_chunks(rows) : 1) * kBlockCols * kBlockCols);
}

size_t spmf_block_gram_scratch_bytes(const spmf_ctx* c, int64_t n_rows) {
  if (!c || !rows_ok(n_rows)) return 0;
  return layout_bytes([&](Arena& a) { block_gram_carve(a, n_rows); });
}

int spmf_block_gram(spmf_ctx* c, int64_t n_rows, const float* x, const float* y, double* g, void* scratch,
    size_t scratch_bytes, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "block_gram: ";
  if (!rows_ok(n_rows)) return fail(c, SPMF_E_ARG, f + "n_rows must be in 0..2^31 - 64");
  if (!g || (n_rows > 0 && (!x || !y))) return fail(c, SPMF_E_ARG, f + "null argument");
  double* partial = nullptr;
  const int rc = carve_scratch(c, "block_gram", scratch, scratch_bytes,
      [&](Arena& a) { partial = block_gram_carve(a, n_rows); }, [&] { return rows_shape(n_rows); });
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (n_rows == 0) {
    HIPCHK(c, hipMemsetAsync(g, 0, (size_t)kBlockCols * kBlockCols * sizeof(double), st));
    return SPMF_OK;
  }
  launch_block_gram(n_rows, x, y, partial, g, st);
  return launched(c, true, "");
}

int spmf_block_rotate(spmf_ctx* c, int64_t n_rows, const float* x, const double* r, float* y, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "block_rotate: ";
  if (!rows_ok(n_rows)) return fail(c, SPMF_E_ARG, f + "n_rows must be in 0..2^31 - 64");
  if (!r || (n_rows > 0 && (!x || !y))) return fail(c, SPMF_E_ARG, f + "null argument");
  BlockRot rot;
  for (int k = 0; k < kBlockCols * kBlockCols; ++k) {
    if (!(r[k] >= -1.7e308 && r[k] <= 1.7e308)) return fail(c, SPMF_E_ARG, f + "r must be finite");
    rot.r[k] = r[k];
  }
  if (n_rows == 0) return SPMF_OK;
  launch_block_rotate(n_rows, x, rot, y, (hipStream_t)stream);
  return launched(c, true, "");
}

}  // extern "C"
