// knn.hip — the exact k-nearest-neighbour graph of n embeddings: for every row its top-K other rows by cosine.
//
// The reference disambiguates events with it (encapsulation/database/graph_db/event_graphrag_neo4j.py:600-672,
// _disambiguate_events_with_gds): gds.knn.write over every Event embedding with topK: 10, similarityCutoff: 0.85 writes a
// SIMILAR_TO edge from each node to its K most similar others.  That needs a Neo4j server with the GDS plugin (the reference
// swallows the failure when it is absent, :671-672) and GDS's kNN is NN-descent: approximate.  Here the answer is exact, and it
// is the second self-join next to pairs.hip (all pairs with cosine >= threshold), built from the same parts:
//
//   once:                    rows -> fp16 image of the normalised rows + float64 inverse norms     pairs_prepare_kernel (pairs.hip)
//   per super-block of <= 4096 COLUMNS (a column j is the row whose neighbours are sought), thr[j] = cutoff - eps:
//     per chunk of rows:     list[j] += {(s, i) : s = image[i]·image[j] >= thr[j]}                 rarc_gemm_f16_select_n (encoder.hip: the
//                                                                                                   score GEMM, select in its epilogue)
//                            thr[j] = max(cutoff - eps, a_K - 2 eps); list[j] cut back to >= thr   knn_tighten_kernel
//     at the end:            exact float64 cosine of every nominee, self and < cutoff dropped,
//                            the K best by (cosine desc, i asc) written with their count           knn_finalize_kernel
//   The chunks are max(512, 2 (K + 1)) rows, then x4 each (wide.hip's ladder): under the K-th best score of the S rows seen so
//   far a chunk of g S more rows lets about g K through, so a list holds K plus a margin, not a share of the corpus.
//
// Exactness (wide.hip's argument, per column).  cos(i, j) is the float64 cosine pairs.hip returns; s the fp32-accumulated product
// of the two fp16 image rows; eps = pairs_eps(d_pad) >= |s - cos| for unit rows (a zero row has s = cos = 0).  Let a_K be the
// K-th best s among the rows i != j seen so far.  Then K rows other than j have cos >= a_K - eps, so the K-th best cosine of
// the final answer, L, is >= a_K - eps (more rows only raise it), and a row of the answer has cos >= L, hence
// s >= L - eps >= a_K - 2 eps: nothing under thr = max(cutoff - eps, a_K - 2 eps) can be in the answer, ever (a_K only rises; thr
// is rounded DOWN where fp32 forms it).  Likewise a row with cos >= cutoff has s >= cutoff - eps.  The nominees that reach the
// finalize therefore contain every row i != j with cos >= max(cutoff, L), ties at L included, whatever their index.
//   Why the column's own row must not count towards a_K: it is in its own list (s ~ 1) but never in its answer.  Counted, it
//   would be one of the "K rows with cos >= a_K - eps" while only K - 1 of them can be neighbours: L >= a_K - eps no longer
//   follows, and the true K-th neighbour could be cut.  It is left out of the select by index and dropped by index in the
//   finalize — not by value: a bit-identical copy of row j is a neighbour with cosine ~ 1.
//
// The exact score is pairs.hip's (pairs_common.h: pairs_exact_cos — float64 dot product of the fp32 rows in a fixed lane-tree
// order, times the inverse norm of the lower-indexed row, then of the higher), so cos(i, j) is the same bits in row i's answer,
// in row j's and in rarc_similar_pairs.  A list that fills up sets flag bit 0 (the caller repeats with a larger cand_cap;
// cand_cap >= n_pad cannot overflow).
//
// Cost: n^2 d_pad MFMA flops — the full square, twice what pairs.hip multiplies.  cos(i, j) = cos(j, i) would let the upper
// triangle serve both rows, but then every row's list has to stay resident until the last super-block; not done.
#include "pairs_common.h"
#include "canon_topk.h"   // the radix select of the k-th largest key

int rarc_gemm_f16_select_n(const uint16_t* a, const uint16_t* w, int m, int n, int k, const float* thr, unsigned long long* cand,
                           uint32_t* count, uint32_t* status, uint32_t cap, uint32_t row0, uint32_t n_valid, hipStream_t s);

namespace {
constexpr int KNN_KMAX = 256;             // largest top_k (the finalize keeps the running answer in a quarter of its LDS buffer)
constexpr int KNN_MAX_CHUNK = 1 << 20;    // rows per GEMM once the ladder has grown (wide.hip: WIDE_FUSED_CHUNK)

// float64 -> 64 bits ordered like the number (the finalize sorts on it), and back
__device__ __forceinline__ uint64_t knn_ord(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double knn_unord(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
}  // namespace

// One workgroup per column j = col0 + q, after a chunk of rows: a_K = the top_k-th best approximate score in the list with the
// column's own row left out (radix select, canon_topk.h; up to 4096 entries from LDS), thr[q] raised to a_K - 2 eps (rounded
// down), and the list compacted IN PLACE to what stays >= thr: 256 entries are read, then — after a barrier — the survivors
// written to the front; a survivor's place is below the number of entries read so far, so nothing unread is overwritten.
// count[q] comes out as the list's length (<= cap); a list the GEMM overran sets flag bit 0.
__global__ __launch_bounds__(256) void knn_tighten_kernel(unsigned long long* cand, uint32_t* count, uint32_t cap, int64_t col0,
                                                          int64_t n, uint32_t top_k, float two_eps, float* thr, uint32_t* flags) {
  constexpr uint32_t LDS_KEYS = 4096;
  __shared__ uint32_t s_keys[LDS_KEYS];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_pick[2];
  __shared__ uint32_t s_n, s_self;
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  const int64_t j = col0 + q;
  if (j >= n) return;
  const uint32_t c_all = count[q], c = c_all < cap ? c_all : cap;
  if (c_all > cap && tid == 0) atomicOr(flags, 1u);
  unsigned long long* list = cand + (size_t)q * cap;
  const uint32_t self = (uint32_t)j;
  if (tid == 0) { s_n = 0; s_self = 0; }
  __syncthreads();
  const bool in_lds = c <= LDS_KEYS;
  for (uint32_t i = tid; i < c; i += 256) {
    const unsigned long long key = list[i];
    const bool is_self = rarc_candrow(key) == self;
    if (is_self) s_self = 1;
    if (in_lds) s_keys[i] = is_self ? 0u : (uint32_t)(key >> 32);      // (0 is below every score's key)
  }
  __syncthreads();
  float t = thr[q];
  bool raised = false;
  if (c - s_self >= top_k) {
    const uint32_t kth =
        in_lds ? wide_kth_largest_u32([&](uint32_t i) { return s_keys[i]; }, c, top_k, s_hist, s_pick)
               : wide_kth_largest_u32(
                     [&](uint32_t i) {
                       const unsigned long long key = list[i];
                       return rarc_candrow(key) == self ? 0u : (uint32_t)(key >> 32);
                     },
                     c, top_k, s_hist, s_pick);
    float nt = rarc_unordkey(kth) - two_eps * 1.000001f;
    nt = nt - fabsf(nt) * 1.2e-7f - 1e-37f;        // (rounded down: the bound must not be overstated by the subtraction)
    if (nt > t) { t = nt; raised = true; }
  }
  if (!raised) {                                   // every entry was nominated against this threshold: nothing to drop
    if (tid == 0) count[q] = c;
    return;
  }
  for (uint32_t e0 = 0; e0 < c; e0 += 256) {
    const uint32_t e = e0 + tid;
    const unsigned long long key = e < c ? list[e] : 0ull;
    const bool keep = e < c && rarc_candscore(key) >= t;
    __syncthreads();                               // this tile is read by everyone before anyone writes into it
    if (keep) list[atomicAdd(&s_n, 1u)] = key;
  }
  __syncthreads();
  if (tid == 0) {
    thr[q] = t;
    count[q] = s_n;
  }
}

// One workgroup per column j = col0 + q, one wave per nominee: the exact float64 cosine (pairs_exact_cos), the column's own row
// and everything under the cutoff dropped, the top_k best by (cosine desc, index asc) kept.  The running answer sits at the
// front of a 1024-entry LDS buffer; the rest is filled with the next nominees' scores, the buffer sorted (bitonic, on the
// ordered cosine then the index — a total order, so the answer does not depend on which wave scored what), and cut at top_k.
// A list of K plus a margin is one round; a cluster of duplicates larger than the buffer takes several.
__global__ __launch_bounds__(256) void knn_finalize_kernel(const float* __restrict__ rows, int64_t ld, int d,
                                                           const double* __restrict__ inv_norm, const unsigned long long* cand,
                                                           const uint32_t* count, uint32_t cap, int64_t col0, int64_t n,
                                                           double cutoff, uint32_t top_k, int64_t* out_ids, double* out_scores,
                                                           int32_t* out_count) {
  constexpr uint32_t BUF = 1024;
  static_assert(KNN_KMAX * 4 <= BUF, "knn_finalize_kernel: every round must take in new nominees");
  __shared__ uint64_t s_key[BUF];
  __shared__ uint32_t s_row[BUF];
  __shared__ uint32_t s_fill;
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  const int64_t j = col0 + q;
  if (j >= n) return;
  const uint32_t c_raw = count[q], c = c_raw < cap ? c_raw : cap;
  const unsigned long long* list = cand + (size_t)q * cap;
  const int wave = tid >> 6, lane = tid & 63;
  const float* y = rows + (size_t)j * ld;
  const double inv_j = inv_norm[j];
  uint32_t kept = 0, e0 = 0;
  do {
    const uint32_t e1 = c - e0 < BUF - kept ? c : e0 + (BUF - kept);
    if (tid == 0) s_fill = kept;
    __syncthreads();
    for (uint32_t e = e0 + wave; e < e1; e += 4) {
      const int64_t i = (int64_t)rarc_candrow(list[e]);                // (wave-uniform: the whole wave reads the same entry)
      if (i == j) continue;                                            // self goes by index, not by value
      const double inv_i = inv_norm[i];
      double cosv = pairs_exact_cos(rows + (size_t)i * ld, y, d, lane, i < j ? inv_i : inv_j, i < j ? inv_j : inv_i);
      cosv = cosv + 0.0;                                               // (-0 -> +0: a zero row's cosines tie, the index decides)
      if (lane == 0 && cosv >= cutoff) {
        const uint32_t slot = atomicAdd(&s_fill, 1u);
        s_key[slot] = knn_ord(cosv);
        s_row[slot] = (uint32_t)i;
      }
    }
    __syncthreads();
    const uint32_t fill = s_fill;
    uint32_t pow2 = 1;
    while (pow2 < fill) pow2 <<= 1;
    for (uint32_t t = fill + tid; t < pow2; t += 256) {                // padding sorts behind every real entry
      s_key[t] = 0;
      s_row[t] = 0xffffffffu;
    }
    __syncthreads();
    for (uint32_t kb = 2; kb <= pow2; kb <<= 1)
      for (uint32_t jb = kb >> 1; jb > 0; jb >>= 1) {
        for (uint32_t t = tid; t < pow2; t += 256) {
          const uint32_t u = t ^ jb;
          if (u > t) {
            const uint64_t ka = s_key[t], kb2 = s_key[u];
            const uint32_t ra = s_row[t], rb = s_row[u];
            const bool a_first = ka > kb2 || (ka == kb2 && ra < rb);   // a ranks before b: larger cosine, then smaller index
            const bool b_first = kb2 > ka || (ka == kb2 && rb < ra);
            const bool desc = (t & kb) == 0;
            if (desc ? b_first : a_first) {
              s_key[t] = kb2; s_key[u] = ka;
              s_row[t] = rb;  s_row[u] = ra;
            }
          }
        }
        __syncthreads();
      }
    kept = fill < top_k ? fill : top_k;
    e0 = e1;
  } while (e0 < c);
  for (uint32_t t = tid; t < top_k; t += 256) {
    const bool have = t < kept;
    out_ids[(size_t)j * top_k + t] = have ? (int64_t)s_row[t] : -1;
    out_scores[(size_t)j * top_k + t] = have ? knn_unord(s_key[t]) : -(double)INFINITY;
  }
  if (tid == 0) out_count[j] = (int32_t)kept;
}

// fewer than two rows: nobody has a neighbour
__global__ void knn_empty_kernel(int64_t n, uint32_t top_k, int64_t* out_ids, double* out_scores, int32_t* out_count) {
  for (int64_t r = 0; r < n; ++r) {
    for (uint32_t t = threadIdx.x; t < top_k; t += blockDim.x) {
      out_ids[(size_t)r * top_k + t] = -1;
      out_scores[(size_t)r * top_k + t] = -(double)INFINITY;
    }
    if (threadIdx.x == 0) out_count[r] = 0;
  }
}

extern "C" size_t rarc_knn_graph_workspace_bytes(int64_t n_rows, int d, int top_k, int cand_cap) {
  if (n_rows <= 0 || n_rows >= (int64_t)0x7fffff00ll || d < 1 || d > 4096 || top_k < 1 || top_k > KNN_KMAX || cand_cap <= 0) return 0;
  return pairs_ws_bytes(n_rows, pairs_d_pad(d), cand_cap);
}

// d_rows: fp32 [n_rows][ld] on the device, any scale (they are normalised here).  Row i of the answer: d_out_ids[i][0 .. top_k)
// the neighbours by (cosine desc, index asc), d_out_scores their float64 cosines, (-1, -inf) past d_out_count[i].  *d_flags
// (zeroed here) bit 0 = a nomination list of cand_cap entries overflowed: the answer is incomplete, call again with a larger
// cand_cap (cand_cap >= n_rows rounded up to 256 cannot overflow).
extern "C" int rarc_knn_graph(const float* d_rows, int64_t ld, int64_t n_rows, int d, int top_k, double cutoff, void* d_ws,
                              size_t ws_bytes, int cand_cap, int64_t* d_out_ids, double* d_out_scores, int32_t* d_out_count,
                              uint32_t* d_flags, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_rows && d_ws && d_out_ids && d_out_scores && d_out_count && d_flags, RARC_E_INVALID, "rarc_knn_graph: null pointer");
  RARC_REQUIRE(n_rows >= 0 && n_rows < (int64_t)0x7fffff00ll && d >= 1 && d <= 4096 && ld >= d && cand_cap >= 1, RARC_E_INVALID,
               "rarc_knn_graph: bad shape (n=%lld d=%d ld=%lld cand_cap=%d; 1 <= d <= 4096)", (long long)n_rows, d, (long long)ld, cand_cap);
  RARC_REQUIRE(top_k >= 1 && top_k <= KNN_KMAX, RARC_E_INVALID, "rarc_knn_graph: top_k %d outside 1..%d", top_k, KNN_KMAX);
  RARC_REQUIRE(cutoff >= -1.0 && cutoff <= 1.0, RARC_E_INVALID, "rarc_knn_graph: cutoff %g outside [-1, 1]", cutoff);
  const int d_pad = pairs_d_pad(d);
  RARC_REQUIRE(n_rows < 2 || ws_bytes >= pairs_ws_bytes(n_rows, d_pad, cand_cap), RARC_E_WORKSPACE,
               "rarc_knn_graph: workspace of %zu bytes, %zu needed", ws_bytes, pairs_ws_bytes(n_rows, d_pad, cand_cap));
  hipStream_t s = (hipStream_t)stream;
  RARC_HIP_CHECK(hipMemsetAsync(d_flags, 0, 4, s));
  if (n_rows < 2) {
    if (n_rows == 1) {
      hipLaunchKernelGGL(knn_empty_kernel, dim3(1), dim3(256), 0, s, n_rows, (uint32_t)top_k, d_out_ids, d_out_scores, d_out_count);
      RARC_HIP_CHECK(hipGetLastError());
    }
    return RARC_OK;
  }
  const PairsWs w = pairs_carve(d_ws, n_rows, d_pad);
  const int64_t n_pad = pad256(n_rows);
  if (int rc = rarc_pairs_prepare(d_rows, ld, n_rows, d, d_pad, w.image, w.inv_norm, s)) return rc;
  const float eps = pairs_eps(d_pad);
  const float t0 = (float)cutoff - eps;
  // the first chunk: enough rows that K others are among them twice over, and two row tiles of the GEMM
  int64_t first = 2 * ((int64_t)top_k + 1) > 512 ? 2 * ((int64_t)top_k + 1) : 512;
  first = pad256(first);
  for (int64_t col0 = 0; col0 < n_rows; col0 += PAIRS_COLS) {
    const int64_t cols = n_pad - col0 < PAIRS_COLS ? n_pad - col0 : PAIRS_COLS;      // a multiple of 256
    const int64_t live = n_rows - col0 < cols ? n_rows - col0 : cols;
    if (int rc = rarc_pairs_reset(w, t0, col0, n_rows, s)) return rc;
    int64_t chunk = first;
    for (int64_t at = 0; at < n_pad;) {
      int64_t m = n_pad - at < chunk ? n_pad - at : chunk;
      if (n_pad - at - m < first) m = n_pad - at;             // (a last sliver joins the chunk before it)
      const int64_t valid = n_rows - at < m ? n_rows - at : m;
      if (int rc = rarc_gemm_f16_select_n(w.image + (size_t)at * d_pad, w.image + (size_t)col0 * d_pad, (int)m, (int)cols, d_pad, w.thr,
                                          w.cand, w.count, w.status, (uint32_t)cand_cap, (uint32_t)at, (uint32_t)valid, s))
        return rc;
      hipLaunchKernelGGL(knn_tighten_kernel, dim3((unsigned)live), dim3(256), 0, s, w.cand, w.count, (uint32_t)cand_cap, col0, n_rows,
                         (uint32_t)top_k, 2.0f * eps, w.thr, d_flags);
      RARC_HIP_CHECK(hipGetLastError());
      at += m;
      chunk = chunk * 4 < KNN_MAX_CHUNK ? chunk * 4 : KNN_MAX_CHUNK;
    }
    hipLaunchKernelGGL(knn_finalize_kernel, dim3((unsigned)live), dim3(256), 0, s, d_rows, ld, d, w.inv_norm, w.cand, w.count,
                       (uint32_t)cand_cap, col0, n_rows, cutoff, (uint32_t)top_k, d_out_ids, d_out_scores, d_out_count);
    RARC_HIP_CHECK(hipGetLastError());
  }
  return RARC_OK;
}
