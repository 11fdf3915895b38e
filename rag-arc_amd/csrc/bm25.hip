// bm25.hip — Okapi BM25 scoring and exact top-k over a term-major posting index (core/retrieval/bm25.py:276-333, whose
// scores come from rank_bm25 0.2.2's BM25Okapi.get_scores).
//
// Index (built on the host, rag_arc_amd/hip/bm25.py): post_off[V+1] int64, post_doc int32 (ascending within a term),
// post_w fp64 = tf*(k1+1) / (tf + k1*((1-b) + b*dl/avgdl)), the reference's per-document fraction for that term.
// Queries: q_off[nq+1] int32 into q_term int32 / q_idf fp64, tokens in query order, duplicates kept, OOV tokens dropped
// by the host (their contribution is an exact zero).
//
// Parity: score[d] = sum over the query's tokens, IN ORDER, of idf * w, in fp64, one correctly rounded multiply and one
// add per term (built with -ffp-contract=off: no fused multiply-add).  A document a token does not reach gets an exact
// zero from the reference, and x + 0 == x, so skipping it changes no bit.
//
// Three launches per batch:
//   1. rarc_bm25_bounds_kernel: one thread per (query token, tile boundary) — the first posting of that term at or after
//      the boundary (binary search).  Every tile then knows its posting range per token without searching.
//   2. rarc_bm25_tile_kernel: one workgroup per (tile of BM_T documents, query).  The tile's scores live in LDS (BM_T
//      doubles); tokens are applied one after another with a barrier in between; inside one token a document appears
//      once, so lanes never share a slot.  Then the tile's k best (score desc, doc asc) over ALL its slots — untouched
//      documents score 0.0 and count — or, for the dense entry, every score is written out.
//   3. rarc_bm25_merge_kernel: groups of tile candidate lists -> one list of k, repeated until one list is left, which
//      is sorted into the answer.
// Selection (bm_select) is exact: bisection over order-preserving 64-bit keys of the scores for the k-th best value,
// then, among the documents equal to it, bisection over the doc id.  Nothing uses float atomics.
#include "rarc_common.h"

constexpr int BM_T = 8192;          // documents per tile (64 KiB of fp64 scores in LDS)
constexpr int BM_THREADS = 512;
constexpr int BM_WAVES = BM_THREADS / 64;
constexpr int BM_ITEMS = BM_T / BM_THREADS;   // selection items per thread
constexpr int BM_MAX_K = 1024;
constexpr int64_t BM_MAX_DOCS = 0x7fffffffLL - BM_T;   // ids of a last tile's unused slots stay below 2^31

// score -> key: larger key == larger score (+0.0 -> 0x8000000000000000).  Keys 0 and 1 are below every real score
// (-inf -> 0x000fffffffffffff): 1 marks a tile slot past the last document, 0 an item slot past the last candidate.
__device__ static inline uint64_t bm_key(double s) {
  const uint64_t u = (uint64_t)__double_as_longlong(s);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ static inline double bm_unkey(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// block-wide sum / min / max; `slot` alternates between calls so that one barrier per call suffices
__device__ static inline int bm_sum(int v, int* s_red, int& slot) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  int* r = s_red + slot * BM_WAVES;
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < BM_WAVES; ++w) t += r[w];
  slot ^= 1;
  return t;
}
__device__ static inline uint64_t bm_minmax(uint64_t v, bool want_max, uint64_t* s_red64, int& slot) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t u = (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    v = want_max ? (u > v ? u : v) : (u < v ? u : v);
  }
  uint64_t* r = s_red64 + slot * BM_WAVES;
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t t = r[0];
#pragma unroll
  for (int w = 1; w < BM_WAVES; ++w) t = want_max ? (r[w] > t ? r[w] : t) : (r[w] < t ? r[w] : t);
  slot ^= 1;
  return t;
}

struct BmSel {
  bool exact;       // select key >= thr
  uint64_t thr;     // (exact) threshold; (!exact) the k-th best key S: select key > S, or key == S and id <= id_cut
  uint32_t id_cut;
};

// The k best of BM_T items (key[i], id[i]) held BM_ITEMS per thread (k <= number of items; ids unique).  Every thread
// gets the same answer.
__device__ static BmSel bm_select(const uint64_t (&key)[BM_ITEMS], const uint32_t (&id)[BM_ITEMS], int k, int* s_red,
                                  uint64_t* s_red64, int& slot, int& slot64) {
  uint64_t mn = ~0ull, mx = 0;
#pragma unroll
  for (int i = 0; i < BM_ITEMS; ++i) {
    mn = key[i] < mn ? key[i] : mn;
    mx = key[i] > mx ? key[i] : mx;
  }
  uint64_t lo = bm_minmax(mn, false, s_red64, slot64);
  uint64_t hi = bm_minmax(mx, true, s_red64, slot64);
  BmSel r{false, lo, 0};
  // invariant: count(key >= lo) > k (all BM_T items, k < BM_T), count(key >= hi) = c_hi < k (hi = max + 1 to start;
  // max < 2^64 - 1: no NaN key)
  ++hi;
  int c_hi = 0;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    int c = 0;
#pragma unroll
    for (int i = 0; i < BM_ITEMS; ++i) c += (int)(key[i] >= mid);
    c = bm_sum(c, s_red, slot);
    if (c == k) return BmSel{true, mid, 0};
    if (c > k) lo = mid;
    else { hi = mid; c_hi = c; }
  }
  // lo = S, the k-th best key; take need = k - c_hi of the items equal to S, lowest ids first
  const int need = k - c_hi;
  int64_t ilo = -1, ihi = 0x7fffffff;   // count(key == S && id <= ilo) < need <= count(... <= ihi)
  while (ihi - ilo > 1) {
    const int64_t mid = ilo + (ihi - ilo) / 2;
    int c = 0;
#pragma unroll
    for (int i = 0; i < BM_ITEMS; ++i) c += (int)((key[i] == lo) & ((int64_t)id[i] <= mid));
    c = bm_sum(c, s_red, slot);
    if (c >= need) ihi = mid;
    else ilo = mid;
  }
  r.thr = lo;
  r.id_cut = (uint32_t)ihi;
  return r;
}

__device__ static inline bool bm_selected(const BmSel& s, uint64_t key, uint32_t id) {
  return s.exact ? key >= s.thr : (key > s.thr || (key == s.thr && id <= s.id_cut));
}

// output position of a selected item: one LDS atomic per wave
__device__ static inline int bm_append(bool sel, int* s_count) {
  const uint64_t m = __ballot(sel);
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0 && m) base = atomicAdd(s_count, __popcll(m));
  base = __shfl(base, 0, 64);
  const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
  return base + below;
}

// ---- 1. posting range of every (token, tile boundary) ---------------------------------------------------------------
__global__ __launch_bounds__(256) void rarc_bm25_bounds_kernel(const int64_t* post_off, const int32_t* post_doc,
                                                               const int32_t* q_term, int64_t n_terms, int64_t n_tok,
                                                               int n_tiles, int64_t n_docs, int64_t* bounds) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int nb = n_tiles + 1;
  if (g >= n_tok * nb) return;
  const int64_t tok = g / nb;
  const int j = (int)(g - tok * nb);
  const int32_t term = q_term[tok];
  int64_t a = 0, b = 0;
  if (term >= 0 && term < n_terms) {
    a = post_off[term];
    b = post_off[term + 1];
  }
  const int64_t key = (int64_t)j * BM_T < n_docs ? (int64_t)j * BM_T : n_docs;
  while (a < b) {   // first posting with doc >= key
    const int64_t m = a + (b - a) / 2;
    if ((int64_t)post_doc[m] < key) a = m + 1;
    else b = m;
  }
  bounds[g] = a;
}

// ---- 2. one tile of one query ---------------------------------------------------------------------------------------
// DENSE: write the tile's scores to out_scores[q][n_docs]; else its k best to cand_key / cand_id [q][tile][k].
template <bool DENSE>
__global__ __launch_bounds__(BM_THREADS) void rarc_bm25_tile_kernel(const int32_t* post_doc, const double* post_w,
                                                                    const int32_t* q_off, const double* q_idf,
                                                                    const int64_t* bounds, int64_t n_tok, int n_tiles,
                                                                    int64_t n_docs, int k, uint64_t* cand_key, uint32_t* cand_id,
                                                                    double* out_scores) {
  __shared__ double s_acc[BM_T];
  __shared__ int s_red[2 * BM_WAVES];
  __shared__ uint64_t s_red64[2 * BM_WAVES];
  __shared__ int s_count;
  const int tile = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
  const int64_t base = (int64_t)tile * BM_T;
  for (int i = tid; i < BM_T; i += BM_THREADS) s_acc[i] = 0.0;
  if (tid == 0) s_count = 0;
  __syncthreads();
  const int64_t t0 = max((int64_t)q_off[q], (int64_t)0), t1 = min((int64_t)q_off[q + 1], n_tok);
  for (int64_t t = t0; t < t1; ++t) {
    const double idf = q_idf[t];
    const int64_t p0 = bounds[(int64_t)t * (n_tiles + 1) + tile], p1 = bounds[(int64_t)t * (n_tiles + 1) + tile + 1];
    // four postings in flight per lane before the first read-add-write
    for (int64_t p = p0 + tid; p < p1; p += 4 * BM_THREADS) {
      int32_t d[4];
      double w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t pu = p + (int64_t)u * BM_THREADS;
        d[u] = pu < p1 ? post_doc[pu] : -1;
        w[u] = pu < p1 ? post_w[pu] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t slot = (int64_t)d[u] - base;
        if (slot >= 0 && slot < BM_T) s_acc[slot] = s_acc[slot] + idf * w[u];
      }
    }
    __syncthreads();
  }
  const int n_here = (int)(n_docs - base < BM_T ? n_docs - base : BM_T);
  if (DENSE) {
    for (int i = tid; i < n_here; i += BM_THREADS) out_scores[(int64_t)q * n_docs + base + i] = s_acc[i];
    return;
  }
  uint64_t key[BM_ITEMS];
  uint32_t id[BM_ITEMS];
#pragma unroll
  for (int i = 0; i < BM_ITEMS; ++i) {
    const int s = i * BM_THREADS + tid;
    key[i] = s < n_here ? bm_key(s_acc[s]) : 1ull;
    id[i] = (uint32_t)(base + s);
  }
  int slot = 0, slot64 = 0;
  const BmSel sel = bm_select(key, id, k, s_red, s_red64, slot, slot64);
  const int64_t out0 = ((int64_t)q * n_tiles + tile) * k;
#pragma unroll
  for (int i = 0; i < BM_ITEMS; ++i) {
    const bool take = bm_selected(sel, key[i], id[i]);
    const int pos = bm_append(take, &s_count);
    if (take && pos < k) {
      cand_key[out0 + pos] = key[i];
      cand_id[out0 + pos] = id[i];
    }
  }
}

// ---- 3. merge groups of `group` candidate lists (k each) into one; the last round sorts its list into the answer --------
__global__ __launch_bounds__(BM_THREADS) void rarc_bm25_merge_kernel(const uint64_t* in_key, const uint32_t* in_id,
                                                                     int n_lists, int group, int k, uint64_t* out_key,
                                                                     uint32_t* out_id, int64_t* final_ids,
                                                                     double* final_scores) {
  __shared__ uint64_t s_key[BM_MAX_K];
  __shared__ uint32_t s_id[BM_MAX_K];
  __shared__ int s_red[2 * BM_WAVES];
  __shared__ uint64_t s_red64[2 * BM_WAVES];
  __shared__ int s_count;
  const int g = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
  const int n_groups = gridDim.x;
  const int l0 = g * group, l1 = l0 + group < n_lists ? l0 + group : n_lists;
  const int n_items = (l1 - l0) * k;
  const int64_t in0 = ((int64_t)q * n_lists + l0) * k;
  if (tid == 0) s_count = 0;
  uint64_t key[BM_ITEMS];
  uint32_t id[BM_ITEMS];
#pragma unroll
  for (int i = 0; i < BM_ITEMS; ++i) {
    const int s = i * BM_THREADS + tid;
    key[i] = s < n_items ? in_key[in0 + s] : 0ull;
    id[i] = s < n_items ? in_id[in0 + s] : 0xffffffffu - (uint32_t)s;   // never selected (key 0), but distinct
  }
  int slot = 0, slot64 = 0;
  const BmSel sel = bm_select(key, id, k, s_red, s_red64, slot, slot64);
  const bool last = final_ids != nullptr;
  const int64_t out0 = ((int64_t)q * n_groups + g) * k;
#pragma unroll
  for (int i = 0; i < BM_ITEMS; ++i) {
    const bool take = bm_selected(sel, key[i], id[i]);
    const int pos = bm_append(take, &s_count);
    if (!take || pos >= k) continue;
    if (last) {
      s_key[pos] = key[i];
      s_id[pos] = id[i];
    } else {
      out_key[out0 + pos] = key[i];
      out_id[out0 + pos] = id[i];
    }
  }
  if (!last) return;
  __syncthreads();
  // rank = #{better items}: score descending, doc ascending
  for (int i = tid; i < k; i += BM_THREADS) {
    const uint64_t ki = s_key[i];
    const uint32_t ii = s_id[i];
    int pos = 0;
    for (int j = 0; j < k; ++j) {
      const uint64_t kj = s_key[j];
      pos += (int)(kj > ki) | ((int)(kj == ki) & (int)(s_id[j] < ii));
    }
    final_ids[(int64_t)q * k + pos] = (int64_t)ii;
    final_scores[(int64_t)q * k + pos] = bm_unkey(ki);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
static inline size_t bm_align(size_t b) { return (b + 255) & ~(size_t)255; }
static inline int bm_tiles(int64_t n_docs) { return (int)((n_docs + BM_T - 1) / BM_T); }
static inline int bm_group(int k) { return BM_T / k; }

struct BmWs {
  int64_t* bounds;
  uint64_t* key_a;
  uint32_t* id_a;
  uint64_t* key_b;
  uint32_t* id_b;
  size_t bytes;
};
static BmWs bm_ws_carve(void* base, int nq, int64_t n_tok, int64_t n_docs, int k) {
  const int n_tiles = bm_tiles(n_docs);
  char* p = (char*)base;
  BmWs w;
  size_t off = 0;
  w.bounds = (int64_t*)(p + off);
  off += bm_align((size_t)n_tok * (n_tiles + 1) * sizeof(int64_t));
  const size_t na = k > 0 ? (size_t)nq * n_tiles * k : 0;
  const size_t nb = k > 0 ? (size_t)nq * ((n_tiles + bm_group(k) - 1) / bm_group(k)) * k : 0;
  w.key_a = (uint64_t*)(p + off);
  off += bm_align(na * 8);
  w.id_a = (uint32_t*)(p + off);
  off += bm_align(na * 4);
  w.key_b = (uint64_t*)(p + off);
  off += bm_align(nb * 8);
  w.id_b = (uint32_t*)(p + off);
  off += bm_align(nb * 4);
  w.bytes = off;
  return w;
}

extern "C" size_t rarc_bm25_workspace_bytes(int nq, int64_t n_query_tokens, int64_t n_docs, int k) {
  if (nq < 0 || n_query_tokens < 0 || n_docs < 1 || n_docs > BM_MAX_DOCS || k < 0 || k > BM_MAX_K) return 0;
  return bm_ws_carve(nullptr, nq, n_query_tokens, n_docs, k).bytes;
}

static int bm_check_common(const char* fn, const int64_t* d_post_off, const int32_t* d_post_doc, const double* d_post_w,
                           int64_t n_terms, int64_t n_docs, const int32_t* d_q_off, const int32_t* d_q_term,
                           const double* d_q_idf, int nq, int64_t n_tok, const void* d_ws) {
  RARC_REQUIRE(d_post_off && d_post_doc && d_post_w && d_q_off && d_ws, RARC_E_INVALID, "%s: null pointer", fn);
  RARC_REQUIRE(n_tok == 0 || (d_q_term && d_q_idf), RARC_E_INVALID, "%s: null pointer (query tokens)", fn);
  RARC_REQUIRE(n_terms >= 1 && n_terms <= 0x7fffffffLL, RARC_E_INVALID,
               "%s: post_off covers %lld terms (1 .. 2^31 - 1)", fn, (long long)n_terms);
  RARC_REQUIRE(n_docs >= 1 && n_docs <= BM_MAX_DOCS, RARC_E_UNSUPPORTED, "%s: n_docs=%lld outside 1 .. %lld", fn,
               (long long)n_docs, (long long)BM_MAX_DOCS);
  RARC_REQUIRE(nq >= 0 && nq <= 65535 && n_tok >= 0 && n_tok <= 0x7fffffffLL, RARC_E_INVALID,
               "%s: bad query batch (nq=%d, tokens=%lld)", fn, nq, (long long)n_tok);
  return RARC_OK;
}

static int bm_launch_bounds(const int64_t* d_post_off, const int32_t* d_post_doc, int64_t n_terms, int64_t n_docs,
                            const int32_t* d_q_term, int64_t n_tok, int64_t* bounds, hipStream_t st) {
  const int n_tiles = bm_tiles(n_docs);
  const int64_t n = n_tok * (n_tiles + 1);
  if (n == 0) return RARC_OK;
  hipLaunchKernelGGL(rarc_bm25_bounds_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_post_off, d_post_doc,
                     d_q_term, n_terms, n_tok, n_tiles, n_docs, bounds);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_bm25_topk(const int64_t* d_post_off, const int32_t* d_post_doc, const double* d_post_w,
                              int64_t n_terms, int64_t n_docs, const int32_t* d_q_off, const int32_t* d_q_term,
                              const double* d_q_idf, int nq, int64_t n_query_tokens, int k, void* d_workspace,
                              size_t workspace_bytes, int64_t* d_out_ids, double* d_out_scores, void* stream) {
  RARC_RANGE();
  int rc = bm_check_common("rarc_bm25_topk", d_post_off, d_post_doc, d_post_w, n_terms, n_docs, d_q_off, d_q_term,
                           d_q_idf, nq, n_query_tokens, d_workspace);
  if (rc != RARC_OK) return rc;
  RARC_REQUIRE(d_out_ids && d_out_scores, RARC_E_INVALID, "rarc_bm25_topk: null pointer (outputs)");
  RARC_REQUIRE(k >= 1 && k <= BM_MAX_K && k <= n_docs, RARC_E_UNSUPPORTED,
               "rarc_bm25_topk: k=%d outside 1 .. min(%d, n_docs=%lld)", k, BM_MAX_K, (long long)n_docs);
  const BmWs ws = bm_ws_carve(d_workspace, nq, n_query_tokens, n_docs, k);
  RARC_REQUIRE(workspace_bytes >= ws.bytes, RARC_E_WORKSPACE, "rarc_bm25_topk: workspace %zu bytes, needs %zu",
               workspace_bytes, ws.bytes);
  if (nq == 0) return RARC_OK;
  hipStream_t st = (hipStream_t)stream;
  rc = bm_launch_bounds(d_post_off, d_post_doc, n_terms, n_docs, d_q_term, n_query_tokens, ws.bounds, st);
  if (rc != RARC_OK) return rc;
  const int n_tiles = bm_tiles(n_docs);
  hipLaunchKernelGGL(rarc_bm25_tile_kernel<false>, dim3(n_tiles, nq), dim3(BM_THREADS), 0, st, d_post_doc, d_post_w,
                     d_q_off, d_q_idf, ws.bounds, n_query_tokens, n_tiles, n_docs, k, ws.key_a, ws.id_a, nullptr);
  RARC_HIP_CHECK(hipGetLastError());
  const int group = bm_group(k);
  uint64_t *src_k = ws.key_a, *dst_k = ws.key_b;
  uint32_t *src_i = ws.id_a, *dst_i = ws.id_b;
  int n_lists = n_tiles;
  while (n_lists > group) {
    const int n_groups = (n_lists + group - 1) / group;
    hipLaunchKernelGGL(rarc_bm25_merge_kernel, dim3(n_groups, nq), dim3(BM_THREADS), 0, st, src_k, src_i, n_lists, group,
                       k, dst_k, dst_i, nullptr, nullptr);
    RARC_HIP_CHECK(hipGetLastError());
    uint64_t* tk = src_k; src_k = dst_k; dst_k = tk;
    uint32_t* ti = src_i; src_i = dst_i; dst_i = ti;
    n_lists = n_groups;
  }
  hipLaunchKernelGGL(rarc_bm25_merge_kernel, dim3(1, nq), dim3(BM_THREADS), 0, st, src_k, src_i, n_lists, group, k,
                     nullptr, nullptr, d_out_ids, d_out_scores);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_bm25_scores(const int64_t* d_post_off, const int32_t* d_post_doc, const double* d_post_w,
                                int64_t n_terms, int64_t n_docs, const int32_t* d_q_off, const int32_t* d_q_term,
                                const double* d_q_idf, int nq, int64_t n_query_tokens, void* d_workspace,
                                size_t workspace_bytes, double* d_out_scores, void* stream) {
  RARC_RANGE();
  int rc = bm_check_common("rarc_bm25_scores", d_post_off, d_post_doc, d_post_w, n_terms, n_docs, d_q_off, d_q_term,
                           d_q_idf, nq, n_query_tokens, d_workspace);
  if (rc != RARC_OK) return rc;
  RARC_REQUIRE(d_out_scores, RARC_E_INVALID, "rarc_bm25_scores: null pointer (output)");
  const BmWs ws = bm_ws_carve(d_workspace, nq, n_query_tokens, n_docs, 0);
  RARC_REQUIRE(workspace_bytes >= ws.bytes, RARC_E_WORKSPACE, "rarc_bm25_scores: workspace %zu bytes, needs %zu",
               workspace_bytes, ws.bytes);
  if (nq == 0) return RARC_OK;
  hipStream_t st = (hipStream_t)stream;
  rc = bm_launch_bounds(d_post_off, d_post_doc, n_terms, n_docs, d_q_term, n_query_tokens, ws.bounds, st);
  if (rc != RARC_OK) return rc;
  const int n_tiles = bm_tiles(n_docs);
  hipLaunchKernelGGL(rarc_bm25_tile_kernel<true>, dim3(n_tiles, nq), dim3(BM_THREADS), 0, st, d_post_doc, d_post_w,
                     d_q_off, d_q_idf, ws.bounds, n_query_tokens, n_tiles, n_docs, 0, nullptr, nullptr, d_out_scores);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}
