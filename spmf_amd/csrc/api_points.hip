// api_points.hip -- the calls on rows as given behind the C-ABI (include/spmf_hip.h): spmf_knn, spmf_kmeans_step and
// spmf_silhouette take points [n][row_len] from the caller and never run the draw stage (api_stream.hip).  An entry
// is: its argument checks, carve_scratch with its layout, its empty return, its launches, `launched`.  Host-side
// orchestration only (ctx.h).
#include <stdlib.h>

#include "ctx.h"

using namespace spmf;

extern "C" {

// ---- exact k nearest rows (knn.hip) -----------------------------------------------------------
// Scratch of one call: the working rows of the reference set and of the queries (sized for both, whether or not
// the call passes one array as both), the biases, the centre and its per-block partial sums, and the slices'
// results (sized for k = kTopkMaxK: the size does not depend on the call's k).
// The shape (the padded row length; the reference slices of the select launch, where the queries take the place
// of top-k's rows and the reference rows that of its columns) and the scratch of a call, all into ka
// (part_slots >= 0: the slots of the slices' results to carve instead of knn's own count -- kmeans_layout)
static void knn_layout(Arena& a, const spmf_ctx* c, int64_t n_query, int64_t n_ref, int row_len, KnnArgs& ka,
    int64_t part_slots = -1) {
  ka.n_query = n_query; ka.n_ref = n_ref; ka.row_len = row_len;
  ka.KP = padded_k(row_len);
  ka.slices = n_ref > 0 ? topk_slices(n_query, (int)n_ref, device_cus(c)) : 1;
  const size_t nq = n_query, nr = n_ref, KP = ka.KP;
  ka.rw = a.take<float>(nr * KP);
  ka.bias = a.take<float>(nr);
  ka.qw = a.take<float>(nq * KP);
  ka.cpart = a.take<float>(kKnnCentreBlocks * KP);
  ka.ccnt = a.take<int32_t>(kKnnCentreBlocks);
  ka.centre = a.take<float>(KP);
  const size_t part = part_slots >= 0 ? (size_t)part_slots : ka.slices > 1 ? (size_t)ka.slices * nq * kTopkMaxK : 0;
  ka.part_idx = a.take<int32_t>(part);
  ka.part_score = a.take<float>(part);
}
static bool row_len_ok(int row_len) { return row_len >= 1 && row_len <= 256; }

size_t spmf_knn_scratch_bytes(const spmf_ctx* c, int64_t n_query, int64_t n_ref, int row_len) {
  if (!c || n_query < 0 || n_ref < 0 || n_ref > 0x7fffffffLL || !row_len_ok(row_len)) return 0;
  KnnArgs ka{};
  return layout_bytes([&](Arena& a) { knn_layout(a, c, n_query, n_ref, row_len, ka); });
}

// SPMF_KNN_TILE = 0 | 1 picks the tile function of the select kernel (knn.hip); both give the same bits
static int knn_tile() {
  const char* e = getenv("SPMF_KNN_TILE");
  return e && e[0] == '1' ? 1 : (e && e[0] == '0' ? 0 : kKnnDefaultTile);
}

int spmf_knn(spmf_ctx* c, const float* q, int64_t n_query, const float* r, int64_t n_ref, int row_len, int k,
    unsigned flags, int64_t self_offset, int32_t* idx_out, float* dist_out, void* scratch, size_t scratch_bytes,
    void* stream) {
  if (!c) return SPMF_E_ARG;
  if (n_query < 0 || n_ref < 0) return fail(c, SPMF_E_ARG, "knn: n_query and n_ref must not be negative");
  if (n_ref > 0x7fffffffLL) return fail(c, SPMF_E_ARG, "knn: n_ref above 2^31 - 1 (the indices are int32)");
  if (!rows_ok(n_query)) return fail(c, SPMF_E_ARG, "knn: too many queries in one call");
  if (!row_len_ok(row_len)) return fail(c, SPMF_E_ARG, "knn: row_len must be in 1..256");
  if (k < 1 || k > kTopkMaxK) return fail(c, SPMF_E_ARG, "knn: k must be in 1..64");
  if (flags & ~1u) return fail(c, SPMF_E_ARG, "knn: unknown flag (bit 0: cosine)");
  if (self_offset < -1) return fail(c, SPMF_E_ARG, "knn: self_offset must be -1 (none) or the reference row of "
      "query 0");
  if ((n_query > 0 && (!q || !idx_out || !dist_out)) || (n_ref > 0 && !r)) return fail(c, SPMF_E_ARG,
      "knn: null argument");
  KnnArgs ka{};
  const int rc = carve_scratch(c, "knn", scratch, scratch_bytes,
      [&](Arena& a) { knn_layout(a, c, n_query, n_ref, row_len, ka); },
      [&] { return "n_query=" + std::to_string((long long)n_query) + " n_ref=" + std::to_string((long long)n_ref) +
                " row_len=" + std::to_string(row_len); });
  if (rc) return rc;
  if (n_query == 0) return SPMF_OK;
  ka.k = k;
  ka.cosine = (flags & 1u) != 0; ka.tile = knn_tile(); ka.self_offset = self_offset;
  ka.q = q; ka.r = r;
  if (q == r && n_query == n_ref) ka.qw = ka.rw;
  ka.idx = idx_out; ka.dist = dist_out;
  return launched(c, launch_knn(ka, (hipStream_t)stream), "knn: no kernel for this row_len / k");
}

// ---- labelled rows: what spmf_kmeans_step and spmf_silhouette check and say alike ----------------
constexpr int32_t kKmeansMaxClusters = 65536;
static bool clusters_ok(int32_t G) { return G >= 1 && G <= kKmeansMaxClusters; }
static int labelled_rows_check(spmf_ctx* c, const std::string& f, int64_t n_rows, int32_t G, int row_len) {
  if (!clusters_ok(G)) return fail(c, SPMF_E_ARG, f + "n_clusters must be in 1..65536");
  if (!row_len_ok(row_len)) return fail(c, SPMF_E_ARG, f + "row_len must be in 1..256");
  if (!rows_ok(n_rows)) return fail(c, SPMF_E_ARG, f + "n_rows must be in 0..2^31 - 64");
  return SPMF_OK;
}
static std::string labelled_rows_shape(int64_t n_rows, int32_t G, int row_len) {
  return "n_rows=" + std::to_string((long long)n_rows) + " n_clusters=" + std::to_string(G) + " row_len=" +
      std::to_string(row_len);
}

// ---- one Lloyd step of k-means (kmeans.hip behind knn.hip and groups.hip's ordering) -----------
// Scratch of one call: knn's carve for the rows as queries and the centroids as reference set, the refined
// candidates [rows][4], the ordering of the rows by label (launch_group_order), the segments' partial sums and the
// statistics' partial sums (kernels.h kmeans_geom bounds them).  knn's slices drop to one as the rows grow, and
// their results with them; here they are carved at their bound over all row counts, slices * rows <= 64 * (2 CUs +
// row blocks) with at most 4 candidates each, so that the size is non-decreasing in the rows.
constexpr int kKmeansCand = 4;
static void kmeans_layout(Arena& a, const spmf_ctx* c, int64_t rows, int G, int row_len, KnnArgs& ka, KmeansArgs& ma) {
  const KmeansGeom q = kmeans_geom(rows, G);
  const size_t nr = rows;
  knn_layout(a, c, rows, G, row_len, ka, 64 * (2 * (int64_t)device_cus(c) + (rows + 63) / 64) * kKmeansCand);
  ka.k = ma.kc = G < kKmeansCand ? G : kKmeansCand;
  ka.idx = a.take<int32_t>(nr * kKmeansCand);
  ka.dist = a.take<float>(nr * kKmeansCand);
  group_order_carve(a, rows, G, q.chunks, q.NB, ma.ord);
  ma.part = a.take<double>((size_t)q.nseg * row_len);
  ma.spart = a.take<double>((size_t)q.sblocks * 3);
}

size_t spmf_kmeans_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int32_t n_clusters, int row_len) {
  if (!c || !rows_ok(n_rows) || !clusters_ok(n_clusters) || !row_len_ok(row_len)) return 0;
  KnnArgs ka{};
  KmeansArgs ma{};
  return layout_bytes([&](Arena& a) { kmeans_layout(a, c, n_rows, n_clusters, row_len, ka, ma); });
}

int spmf_kmeans_step(spmf_ctx* c, const float* x, int64_t n_rows, int row_len, const float* centroids,
    int32_t n_clusters, const int32_t* prev_labels, int32_t* labels_out, float* dist_out, double* sums_out,
    int64_t* counts_out, double* stats_out, void* scratch, size_t scratch_bytes, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "kmeans_step: ";
  int rc = labelled_rows_check(c, f, n_rows, n_clusters, row_len);
  if (rc) return rc;
  if (prev_labels && prev_labels == labels_out) return fail(c, SPMF_E_ARG, f + "prev_labels must not be labels_out");
  if (!sums_out || !counts_out || !stats_out || (n_rows > 0 && (!x || !centroids || !labels_out))) return fail(c,
      SPMF_E_ARG, f + "null argument");
  KnnArgs ka{};
  KmeansArgs ma{};
  rc = carve_scratch(c, "kmeans_step", scratch, scratch_bytes,
      [&](Arena& a) { kmeans_layout(a, c, n_rows, n_clusters, row_len, ka, ma); },
      [&] { return labelled_rows_shape(n_rows, n_clusters, row_len); });
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (n_rows == 0) {
    HIPCHK(c, hipMemsetAsync(sums_out, 0, (size_t)n_clusters * row_len * sizeof(double), st));
    HIPCHK(c, hipMemsetAsync(counts_out, 0, (size_t)n_clusters * sizeof(int64_t), st));
    HIPCHK(c, hipMemsetAsync(stats_out, 0, 3 * sizeof(double), st));
    return SPMF_OK;
  }
  // the assignment: spmf_knn's launches with q = x, r = centroids, k = min(4, G), Euclidean, no self
  ka.cosine = false; ka.tile = knn_tile(); ka.self_offset = -1;
  ka.q = x; ka.r = centroids;
  if (!launch_knn(ka, st)) return fail(c, SPMF_E_UNSUPPORTED, f + "no kernel for this row_len");
  ma.n_rows = n_rows; ma.row_len = row_len; ma.n_clusters = n_clusters;
  ma.x = x; ma.cand_idx = ka.idx; ma.cand_dist = ka.dist; ma.prev = prev_labels;
  ma.labels = labels_out; ma.dist = dist_out; ma.sums = sums_out; ma.counts = counts_out; ma.stats = stats_out;
  launch_kmeans(ma, st);
  return launched(c, true, "");
}

// ---- the silhouette of labelled rows (silhouette.hip behind groups.hip's ordering) -------------
// Scratch of one call: the effective labels, the ordering of the members by label (launch_group_order), the
// working rows and biases in that order, the centre with its partial sums, and the blocks' sums of s (kernels.h
// silhouette_geom bounds the blocks).  Every region grows with the rows.
static void silhouette_layout(Arena& a, int64_t rows, int G, int row_len, SilhouetteArgs& sa) {
  const SilhouetteGeom q = silhouette_geom(rows, G);
  sa.n_rows = rows; sa.row_len = row_len; sa.n_clusters = G;
  sa.KP = padded_k(row_len);
  const size_t NB = (size_t)q.NB, KP = sa.KP;
  sa.eff = a.take<int32_t>((size_t)rows);
  group_order_carve(a, rows, G, q.chunks, q.NB, sa.ord);
  sa.w = a.take<float>(NB * 64 * KP);
  sa.bias = a.take<float>(NB * 64);
  sa.cpart = a.take<double>((size_t)kSilCentreBlocks * KP);
  sa.ccnt = a.take<int32_t>(kSilCentreBlocks);
  sa.centre = a.take<float>(KP);
  sa.spart = a.take<double>(NB);
}

size_t spmf_silhouette_scratch_bytes(const spmf_ctx* c, int64_t n_rows, int32_t n_clusters, int row_len) {
  if (!c || !rows_ok(n_rows) || !clusters_ok(n_clusters) || !row_len_ok(row_len)) return 0;
  SilhouetteArgs sa{};
  return layout_bytes([&](Arena& a) { silhouette_layout(a, n_rows, n_clusters, row_len, sa); });
}

int spmf_silhouette(spmf_ctx* c, const float* x, int64_t n_rows, int row_len, const int32_t* labels,
    int32_t n_clusters, unsigned flags, float* sil_out, float* a_out, float* b_out, int32_t* nearest_out,
    double* cluster_sum_out, int64_t* counts_out, void* scratch, size_t scratch_bytes, void* stream) {
  if (!c) return SPMF_E_ARG;
  const std::string f = "silhouette: ";
  int rc = labelled_rows_check(c, f, n_rows, n_clusters, row_len);
  if (rc) return rc;
  if (flags & ~1u) return fail(c, SPMF_E_ARG, f + "unknown flag (bit 0: cosine)");
  if (!cluster_sum_out || !counts_out || (n_rows > 0 && (!x || !labels || !sil_out))) return fail(c, SPMF_E_ARG,
      f + "null argument");
  SilhouetteArgs sa{};
  rc = carve_scratch(c, "silhouette", scratch, scratch_bytes,
      [&](Arena& a) { silhouette_layout(a, n_rows, n_clusters, row_len, sa); },
      [&] { return labelled_rows_shape(n_rows, n_clusters, row_len); });
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (n_rows == 0) {
    HIPCHK(c, hipMemsetAsync(cluster_sum_out, 0, (size_t)n_clusters * sizeof(double), st));
    HIPCHK(c, hipMemsetAsync(counts_out, 0, (size_t)n_clusters * sizeof(int64_t), st));
    return SPMF_OK;
  }
  sa.cosine = (flags & 1u) != 0;
  sa.x = x; sa.labels = labels;
  sa.sil = sil_out; sa.a = a_out; sa.b = b_out; sa.nearest = nearest_out;
  sa.cluster_sum = cluster_sum_out; sa.counts = counts_out;
  return launched(c, launch_silhouette(sa, st), "silhouette: no kernel for this row_len");
}

}  // extern "C"
