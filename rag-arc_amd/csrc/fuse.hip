// fuse.hip — rank-level kernels after retrieval.
//   rarc_rrf_fuse      RRFusion.fuse                 core/utils/Fusion.py:45-76
//   rarc_rerank_order  Qwen3Reranker score -> order  core/rerank/Reranker_Qwen3.py:41-49, :70-74
//   rarc_mmr_select    _mmr_select, one query, gathered fp32 candidates
//   rarc_mmr_select_rows  the same selection for a batch of queries, candidates read from the resident rows
//
// Both are small per-query problems (usually a few hundred items, at most 4096); one workgroup per query, O(n^2)
// all-pairs in LDS.  What matters here is bit-exactness, not bandwidth:
//   * RRF adds 1.0/(k + rank) in fp64 in the reference's order: lists in order, positions in
//     order, per key (Python float += is fp64; `sorted(..., reverse=True)` is stable, so ties
//     keep first-insertion order).
//   * rerank: p_yes = exp(log_softmax([z_no, z_yes])[1]) through fp16 tensors, then Python's
//     stable sort descending (ties keep retrieval order).  A NaN p_yes — (inf, inf) or (-inf, -inf) logits, which is
//     what a pair beyond +-65504 becomes in fp16, or a NaN logit — ranks below every number and NaNs keep retrieval
//     order among themselves (oracle.stable_desc_order: a stable argsort of -s puts NaN last).  The score written out
//     stays NaN; only the order key is replaced.  out_perm is a permutation of [0, n) for every input.
#include "rarc_common.h"

constexpr int RRF_MAX_ITEMS = 4096;

// 1024 threads per query: FOUR lanes per item (item t = tid / 4 + 256 m, lane part s = tid & 3 takes the partners
// u = s, s + 4, ...), so an all-pairs sweep is n / 4 steps per thread and 16 waves per CU hide each other's latency —
// with one thread per item every step of the three sweeps waited out its own dependency chain (135 cycles per step,
// 45 us per call whatever the number of queries).  Predicates are combined with bitwise operators (written with
// && / || the compiler emitted a chain of exec-masked branches per step).  The order-free parts (first occurrence =
// a minimum, next occurrence = a minimum, output position = a count) are reduced over the four lanes; the fp64 sum of
// a key's terms — whose ORDER is the reference's — walks the key's occurrence chain sequentially (usually two links).
constexpr int RRF_THREADS = 1024;
__global__ __launch_bounds__(RRF_THREADS) void rarc_rrf_kernel(const int64_t* keys, const int32_t* lens, int n_lists,
                                                               int max_len, double rrf_k, int top_k, int64_t* out_keys,
                                                               double* out_scores, int32_t* out_n) {
  __shared__ int64_t s_key[RRF_MAX_ITEMS];
  __shared__ double s_score[RRF_MAX_ITEMS];   // each item's own term, then (first occurrences) the key's sum
  __shared__ int32_t s_first[RRF_MAX_ITEMS];  // first occurrence of the item's key
  __shared__ int32_t s_next[RRF_MAX_ITEMS];   // next occurrence of the same key after this item, or n
  __shared__ int32_t s_off[64 + 1];
  __shared__ int32_t s_nuniq;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    int o = 0;
    for (int r = 0; r < n_lists; ++r) {
      s_off[r] = o;
      int l = lens[b * n_lists + r];
      l = l < 0 ? 0 : (l > max_len ? max_len : l);
      o += l;
    }
    s_off[n_lists] = o;
    s_nuniq = 0;
  }
  __syncthreads();
  const int n = s_off[n_lists];
  for (int r = 0; r < n_lists; ++r) {
    const int o = s_off[r], l = s_off[r + 1] - o;
    for (int i = threadIdx.x; i < l; i += blockDim.x) {
      s_key[o + i] = keys[((size_t)b * n_lists + r) * max_len + i];
      s_score[o + i] = 1.0 / (rrf_k + (double)(i + 1));   // rank = position + 1 inside its list
    }
  }
  __syncthreads();
  const int part = threadIdx.x & 3, item0 = threadIdx.x >> 2, per = RRF_THREADS / 4;
  const int n_round = (n + per - 1) / per * per;   // whole waves run every trip (the lane-group reductions need all four)
  // first occurrence of every key in (list, position) order
  for (int t = item0; t < n_round; t += per) {
    const bool live = t < n;
    const int64_t k = live ? s_key[t] : 0;
    int f = live ? t : 0;
#pragma unroll 4
    for (int u = part; u < t && u < n; u += 4) f = ((int)(s_key[u] == k) & (int)(u < f)) ? u : f;
    f = min(f, __shfl_xor(f, 1, 64));
    f = min(f, __shfl_xor(f, 2, 64));
    if (live && part == 0) s_first[t] = f;
  }
  __syncthreads();
  // next occurrence of the same key (chains the occurrences of a key in order)
  for (int t = item0; t < n_round; t += per) {
    const bool live = t < n;
    const int f = live ? s_first[t] : -1;
    int nx = n;
    const int u0 = t + 1 + ((part - (t + 1)) & 3);   // smallest u > t with u = part (mod 4)
#pragma unroll 4
    for (int u = u0; u < n; u += 4) nx = ((int)(s_first[u] == f) & (int)(u < nx)) ? u : nx;
    nx = min(nx, __shfl_xor(nx, 1, 64));
    nx = min(nx, __shfl_xor(nx, 2, 64));
    if (live && part == 0) s_next[t] = nx;
  }
  __syncthreads();
  // score of each distinct key: sequential fp64 sum over its occurrences, in order (what the reference's `+=` does)
  double my_sum[(RRF_MAX_ITEMS + RRF_THREADS - 1) / RRF_THREADS];
  {
    int m = 0;
    for (int t = threadIdx.x; t < n; t += blockDim.x, ++m) {
      double sum = 0.0;
      if (s_first[t] == t)
        for (int u = t; u < n; u = s_next[u]) sum += s_score[u];
      my_sum[m] = sum;
    }
  }
  __syncthreads();  // every term has been read before any is overwritten by a sum
  {
    int m = 0;
    for (int t = threadIdx.x; t < n; t += blockDim.x, ++m) {
      if (s_first[t] != t) continue;
      s_score[t] = my_sum[m];
      atomicAdd(&s_nuniq, 1);
    }
  }
  __syncthreads();
  // stable descending order by counting: position = #{distinct u better than t}
  for (int t = item0; t < n_round; t += per) {
    const bool mine = t < n && s_first[t] == t;
    const double sc = mine ? s_score[t] : 0.0;
    int pos = 0;
#pragma unroll 4
    for (int u = part; u < n; u += 4) {
      const double su = s_score[u];
      pos += (int)(s_first[u] == u) & (int)(u != t) & ((int)(su > sc) | ((int)(su == sc) & (int)(u < t)));
    }
    pos += __shfl_xor(pos, 1, 64);
    pos += __shfl_xor(pos, 2, 64);
    if (mine && part == 0 && pos < top_k) {
      out_keys[(size_t)b * top_k + pos] = s_key[t];
      out_scores[(size_t)b * top_k + pos] = sc;
    }
  }
  if (threadIdx.x == 0) out_n[b] = s_nuniq < top_k ? s_nuniq : top_k;
}

extern "C" int rarc_rrf_fuse(const int64_t* d_keys, const int32_t* d_len, int nq, int n_lists, int max_len,
                             double rrf_k, int top_k, int64_t* d_out_keys, double* d_out_scores,
                             int32_t* d_out_n, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_keys && d_len && d_out_keys && d_out_scores && d_out_n, RARC_E_INVALID, "rarc_rrf_fuse: null pointer");
  RARC_REQUIRE(nq >= 0 && n_lists >= 1 && n_lists <= 64 && max_len >= 0 && top_k >= 0, RARC_E_INVALID,
               "rarc_rrf_fuse: bad sizes (nq=%d lists=%d max_len=%d top_k=%d)", nq, n_lists, max_len, top_k);
  RARC_REQUIRE((int64_t)n_lists * max_len <= RRF_MAX_ITEMS, RARC_E_UNSUPPORTED,
               "rarc_rrf_fuse: %d lists x %d items exceeds %d items per query", n_lists, max_len, RRF_MAX_ITEMS);
  if (nq == 0) return RARC_OK;
  hipLaunchKernelGGL(rarc_rrf_kernel, dim3(nq), dim3(RRF_THREADS), 0, (hipStream_t)stream, d_keys, d_len, n_lists,
                     max_len, rrf_k, top_k, d_out_keys, d_out_scores, d_out_n);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

// ---- reranker: fp16 logits -> fp16 p_yes -> stable descending permutation -----------------------
constexpr int RERANK_MAX = 4096;

__global__ __launch_bounds__(256) void rarc_rerank_kernel(const half_t* z_no, const half_t* z_yes, int n,
                                                          half_t* out_scores, int32_t* out_perm) {
  __shared__ float s_p[RERANK_MAX];
  const int b = blockIdx.x;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float zn = (float)z_no[(size_t)b * n + i], zy = (float)z_yes[(size_t)b * n + i];
    const float m = fmaxf(zn, zy);
    const float sum = expf(zn - m) + expf(zy - m);
    const half_t ls = (half_t)((zy - m) - logf(sum));  // log_softmax output tensor is fp16
    const half_t pr = (half_t)expf((float)ls);         // .exp() on the fp16 tensor
    out_scores[(size_t)b * n + i] = pr;
    const float pf = (float)pr;
    s_p[i] = pf == pf ? pf : -INFINITY;   // the ORDER key: NaN below every number (p_yes itself is never below 0)
  }
  __syncthreads();
  // position = #{u ahead of i} under the total order (key desc, index asc): a bijection onto [0, n), so every slot of
  // out_perm is written exactly once — which needs NO NaN among the keys (a NaN compares false both ways)
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float s = s_p[i];
    int pos = 0;
    for (int u = 0; u < n; ++u) {
      const float su = s_p[u];
      pos += (int)(su > s) | ((int)(su == s) & (int)(u < i));
    }
    out_perm[(size_t)b * n + pos] = i;
  }
}

extern "C" int rarc_rerank_order(const uint16_t* d_z_no, const uint16_t* d_z_yes, int nq, int n,
                                 uint16_t* d_out_scores_f16, int32_t* d_out_perm, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_z_no && d_z_yes && d_out_scores_f16 && d_out_perm, RARC_E_INVALID, "rarc_rerank_order: null pointer");
  RARC_REQUIRE(nq >= 0 && n >= 0 && n <= RERANK_MAX, RARC_E_UNSUPPORTED, "rarc_rerank_order: n=%d exceeds %d", n,
               RERANK_MAX);
  if (nq == 0 || n == 0) return RARC_OK;
  hipLaunchKernelGGL(rarc_rerank_kernel, dim3(nq), dim3(256), 0, (hipStream_t)stream, (const half_t*)d_z_no,
                     (const half_t*)d_z_yes, n, (half_t*)d_out_scores_f16, d_out_perm);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

// ---- maximal marginal relevance: the greedy selection of _mmr_select (VectorStore_Faiss.py:16-62) --------------
// n candidates (fetch_k, a few dozen) of dimension d, float64 arithmetic like the reference's numpy on python floats:
//   pick candidate 0; then k - 1 times: score_i = lambda·<q, e_i> − (1 − lambda)·max(0, max_{s selected} <e_s, e_i>),
//   take the FIRST candidate with the largest score among the remaining ones (python's max).
// Candidates come as fp32 (the resident rows, gathered) and are widened; `normalize` divides them (and the query) by
// their float64 norms first, as max_marginal_relevance_search_by_vector does for cosine stores (:308-312, :355-359).
// One workgroup; instead of an n x n similarity matrix the running maximum per candidate is updated with the newest
// pick each round: O(k·n·d).  d_work: n·d + d doubles.
constexpr int MMR_MAX_N = 1024;

// THE sum of both MMR kernels: W independent sequential float64 sums s[j] = sum over m = 0 .. d-1, ascending, of
// a(m, j) * b(m, j) — one rounded product, one rounded addition per term (the library is built with -ffp-contract=off).
// Norms (a == b), <q, e_i> and <e_s, e_i> all go through here, so the two kernels agree bit for bit on every value they
// compare.  W > 1 interleaves sums that do not depend on each other (W dependency chains in flight per thread); the order
// INSIDE each sum is the same for every W and U.
// U > 1 fetches the operands of U consecutive terms before it adds them, in the same order: a walk whose every term waits
// for its own loads pays a memory round trip per term, one that fetches U ahead pays it per U terms.
// b = MmrSquare{}: the sum of squares — each term squares ONE fetched value.
struct MmrSquare {};
template <int W, int U = 1, class FA, class FB>
__device__ __forceinline__ void mmr_seq_sums(int d, FA a, FB b, double (&s)[W]) {
  constexpr bool SQ = __is_same(FB, MmrSquare);
  const auto second = [&](int m, int j, double x) {
    if constexpr (SQ) return x;
    else return b(m, j);
  };
#pragma unroll
  for (int j = 0; j < W; ++j) s[j] = 0.0;
  int m = 0;
  if constexpr (U > 1) {
    for (; m + U <= d; m += U) {
      double av[U][W], bv[U][W];
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int j = 0; j < W; ++j) { av[u][j] = a(m + u, j); bv[u][j] = second(m + u, j, av[u][j]); }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int j = 0; j < W; ++j) s[j] += av[u][j] * bv[u][j];
      }
    }
  }
  for (; m < d; ++m) {
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const double x = a(m, j);
      s[j] += x * second(m, j, x);
    }
  }
}

__global__ __launch_bounds__(256) void rarc_mmr_kernel(const float* cand, int64_t ld, const double* query, int n, int d,
                                                       int normalize, int k, double lambda, double* work, int32_t* out) {
  __shared__ double s_qsim[MMR_MAX_N];
  __shared__ double s_maxsim[MMR_MAX_N];
  __shared__ int32_t s_taken[MMR_MAX_N];
  __shared__ double s_red[256];
  __shared__ int32_t s_best, s_first;
  const int tid = threadIdx.x;
  double* e = work;                 // [n][d] widened (normalised) candidates
  double* qn = work + (size_t)n * d;  // [d]
  // sequential float64 sums per vector: one thread per vector (n is small); numpy's dot / norm use a blocked order,
  // which can differ in the last place — selections differ from the reference's only across ties that close
  for (int i = tid; i <= n; i += blockDim.x) {
    const bool isq = i == n;
    double ss[1] = {0.0};
    if (normalize) {
      const auto v = [&](int m, int) { return isq ? query[m] : (double)cand[(size_t)i * ld + m]; };
      mmr_seq_sums<1>(d, v, MmrSquare{}, ss);
    }
    const double nr = normalize ? sqrt(ss[0]) : 1.0;
    for (int m = 0; m < d; ++m) {
      const double v = isq ? query[m] : (double)cand[(size_t)i * ld + m];
      (isq ? qn : e + (size_t)i * d)[m] = normalize ? v / nr : v;
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += blockDim.x) {
    double s[1];
    mmr_seq_sums<1>(d, [&](int m, int) { return qn[m]; }, [&](int m, int) { return e[(size_t)i * d + m]; }, s);
    s_qsim[i] = s[0];
    s_maxsim[i] = 0.0;   // (the reference's max_sim starts from 0)
    s_taken[i] = i == 0;
  }
  if (tid == 0) out[0] = 0;
  __syncthreads();
  int last = 0;
  for (int step = 1; step < k && step < n; ++step) {
    double best = -INFINITY;
    int best_i = 0x7fffffff, first_i = 0x7fffffff;
    for (int i = tid; i < n; i += blockDim.x) {
      if (s_taken[i]) continue;
      first_i = min(first_i, i);
      double sim[1];
      mmr_seq_sums<1>(d, [&](int m, int) { return e[(size_t)last * d + m]; }, [&](int m, int) { return e[(size_t)i * d + m]; }, sim);
      const double s = sim[0];
      const double mx = s > s_maxsim[i] ? s : s_maxsim[i];
      s_maxsim[i] = mx;
      const double val = lambda * s_qsim[i] - (1.0 - lambda) * mx;
      if (val > best) { best = val; best_i = i; }   // (i ascends per thread: the first maximum is kept)
    }
    s_red[tid] = best;
    __syncthreads();
    if (tid == 0) {
      double b = -INFINITY;
      for (int t = 0; t < (int)blockDim.x; ++t) b = s_red[t] > b ? s_red[t] : b;
      s_red[0] = b;
      s_best = 0x7fffffff;
      s_first = 0x7fffffff;
    }
    __syncthreads();
    if (best_i != 0x7fffffff && best == s_red[0]) atomicMin(&s_best, best_i);  // the lowest index among equal scores
    if (first_i != 0x7fffffff) atomicMin(&s_first, first_i);
    __syncthreads();
    // nothing left compares above -inf (NaN values: a zero vector under `normalize`): the lowest remaining index, never
    // an index outside [0, n)
    last = s_best != 0x7fffffff ? s_best : s_first;
    if (tid == 0) { out[step] = last; s_taken[last] = 1; }
    __syncthreads();
  }
}

extern "C" size_t rarc_mmr_workspace_doubles(int n, int d) { return n > 0 && d > 0 ? (size_t)n * d + d : 0; }

extern "C" int rarc_mmr_select(const float* d_cand, int64_t ld, const double* d_query, int n, int d, int normalize, int k,
                               double lambda, double* d_work, int32_t* d_out, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_cand && d_query && d_work && d_out, RARC_E_INVALID, "rarc_mmr_select: null pointer");
  RARC_REQUIRE(n >= 1 && n <= MMR_MAX_N && d >= 1 && ld >= d && k >= 1, RARC_E_INVALID,
               "rarc_mmr_select: bad sizes (n=%d of at most %d, d=%d, k=%d)", n, MMR_MAX_N, d, k);
  hipLaunchKernelGGL(rarc_mmr_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, d_cand, ld, d_query, n, d, normalize, k,
                     lambda, d_work, d_out);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

// ---- the same selection for a batch of queries, candidates read straight from the resident rows ---------------------------
// One workgroup per query.  The picks are, index for index, rarc_mmr_select's on the gathered fp32 candidates: the values
// compared are built from the same widened elements (fp16 exactly; fp8 decoded to fp32 and multiplied by the row scale in
// fp32; fp32 as is; elements 0 .. d-1 only) through mmr_seq_sums, v / sqrt(ss), and the same value expression.  Only what
// runs beside what differs:
//   * all 256 threads widen the rows in 16-byte loads and lay them out TRANSPOSED, et[m][i]: in every later sum thread i
//     walks column i, so adjacent lanes read adjacent doubles;
//   * one thread per candidate forms a sum (norm, <q, e_i>, <e_last, e_i>); beyond 256 candidates a thread carries four
//     interleaved sums; the division by the norms runs over all (m, i) at once;
//   * up to MMR_GRAM_N candidates, when the pairs take fewer passes than the rounds would, every <e_s, e_i> (s < i) is formed
//     ONCE before the rounds (<e_i, e_s> has the same bits: the products commute, the order is the same), by all threads, and
//     the rounds read LDS (32 KB of dynamic LDS, asked for only by launches with n <= MMR_GRAM_N); otherwise each round scores its newest pick, as rarc_mmr_kernel does;
//   * the argmax (largest value, lowest index among equals; nothing above -inf: lowest remaining index) is a shuffle
//     reduction.
// Candidates are the entries of the query's id list that name a row (id - id_base in [0, n_rows)), in order; anything else
// (the -1 padding) is dropped before a row is read.  Workspace per query: n·d + d doubles (et, then the query).
constexpr int MMR_GRAM_N = 64;

template <int FMT> struct MmrRowFmt;
template <> struct MmrRowFmt<0> { static constexpr int E = 8, BYTES = 2; };
template <> struct MmrRowFmt<1> { static constexpr int E = 16, BYTES = 1; };
template <> struct MmrRowFmt<2> { static constexpr int E = 4, BYTES = 4; };

template <int FMT>
__device__ __forceinline__ void mmr_widen16(const uint4 v, float scale, double (&o)[MmrRowFmt<FMT>::E]) {
  if constexpr (FMT == 0) {
    const half8 h = __builtin_bit_cast(half8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (double)(float)h[j];
  } else if constexpr (FMT == 1) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float f[4];
      rarc_f8x4_to_f32(w[c], f);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[4 * c + j] = (double)(f[j] * scale);   // (fp32 product, as the gathered copy forms it)
    }
  } else {
    o[0] = (double)__builtin_bit_cast(float, v.x);
    o[1] = (double)__builtin_bit_cast(float, v.y);
    o[2] = (double)__builtin_bit_cast(float, v.z);
    o[3] = (double)__builtin_bit_cast(float, v.w);
  }
}

// s[j] = sum over m of a(m) * et[m][tid + 256 j]; a column beyond nc reads column 0 (the caller ignores its sum)
template <int W, class FA>
__device__ __forceinline__ void mmr_column_sums(int d, int nc, const double* et, FA a, double (&s)[W]) {
  int col[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const int i = (int)threadIdx.x + 256 * j;
    col[j] = i < nc ? i : 0;
  }
  mmr_seq_sums<W, 16 / W>(d, [&](int m, int) { return a(m); }, [&](int m, int j) { return et[(size_t)m * nc + col[j]]; }, s);
}

struct MmrRowsLds {
  double qsim[MMR_MAX_N];
  double maxsim[MMR_MAX_N];     // (the candidates' norms while they are being divided out)
  int64_t id[MMR_MAX_N];        // the query's candidates: their ids as given
  int32_t taken[MMR_MAX_N];
  double wbest[4];
  double qnorm;
  int32_t wbi[4], wfi[4], wcnt[4];
};

// everything after the widened candidates are in place (W sums per thread: 1 up to 256 candidates, 4 beyond)
template <int W>
__device__ __forceinline__ void mmr_rows_select(MmrRowsLds& L, double* gram_lds, int nc, int d, int normalize, int k, double lambda, double* et,
                                                double* qn, int64_t* out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool live = tid < nc;                   // (W = 4: nc > 256, every thread has a candidate)
  if (normalize) {
    for (int i0 = tid; i0 <= nc; i0 += 256 * W) {
      // columns i0 + 256 j; column nc is the query
      double ss[W];
      int col[W];
#pragma unroll
      for (int j = 0; j < W; ++j) col[j] = i0 + 256 * j <= nc ? i0 + 256 * j : 0;
      const auto v = [&](int m, int j) { return col[j] == nc ? qn[m] : et[(size_t)m * nc + col[j]]; };
      mmr_seq_sums<W, 16 / W>(d, v, MmrSquare{}, ss);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const int i = i0 + 256 * j;
        if (i < nc) L.maxsim[i] = sqrt(ss[j]);
        else if (i == nc) L.qnorm = sqrt(ss[j]);
      }
    }
    __syncthreads();
    const size_t total = (size_t)nc * d;
    int i = tid % nc;                          // (idx mod nc, carried along: idx advances by 256)
    const int step = 256 % nc;
    for (size_t idx = tid; idx < total; idx += 256) {
      et[idx] = et[idx] / L.maxsim[i];
      i += step;
      i = i >= nc ? i - nc : i;
    }
    for (int m = tid; m < d; m += 256) qn[m] = qn[m] / L.qnorm;
    __syncthreads();
  }
  {
    double s[W];
    if (live) mmr_column_sums<W>(d, nc, et, [&](int m) { return qn[m]; }, s);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int i = tid + 256 * j;
      if (i < nc) {
        L.qsim[i] = s[j];
        L.maxsim[i] = 0.0;   // (the reference's max_sim starts from 0)
        L.taken[i] = i == 0;
      }
    }
  }
  const int pairs = nc * (nc - 1) / 2;
  const bool gram = W == 1 && gram_lds != nullptr && nc <= MMR_GRAM_N && (pairs + 255) / 256 < k - 1;
  if (gram) {
    for (int p = tid; p < pairs; p += 256) {      // p = i (i - 1) / 2 + s, s < i
      int i = 1;
      while (i * (i + 1) / 2 <= p) ++i;
      const int s = p - i * (i - 1) / 2;
      double g[1];
      mmr_seq_sums<1, 16>(d, [&](int m, int) { return et[(size_t)m * nc + s]; }, [&](int m, int) { return et[(size_t)m * nc + i]; }, g);
      gram_lds[s * MMR_GRAM_N + i] = g[0];
      gram_lds[i * MMR_GRAM_N + s] = g[0];
    }
  }
  if (tid == 0) out[0] = L.id[0];
  __syncthreads();
  int last = 0;
  for (int step = 1; step < k; ++step) {          // (k < nc here)
    double best = -INFINITY;
    int best_i = 0x7fffffff, first_i = 0x7fffffff;
    double sim[W];
    if (!gram && live) mmr_column_sums<W>(d, nc, et, [&](int m) { return et[(size_t)m * nc + last]; }, sim);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int i = tid + 256 * j;
      if (i < nc && !L.taken[i]) {
        first_i = min(first_i, i);
        const double s = gram ? gram_lds[last * MMR_GRAM_N + (i & (MMR_GRAM_N - 1))] : sim[j];
        const double mx = s > L.maxsim[i] ? s : L.maxsim[i];
        L.maxsim[i] = mx;
        const double val = lambda * L.qsim[i] - (1.0 - lambda) * mx;
        if (val > best) { best = val; best_i = i; }   // (i ascends per thread: the first maximum is kept)
      }
    }
    // the largest value, the lowest index among equal values; and the lowest index still to be taken
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      const double ob = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(best_i, off, 64), of = __shfl_xor(first_i, off, 64);
      if ((int)(ob > best) | ((int)(ob == best) & (int)(oi < best_i))) { best = ob; best_i = oi; }
      first_i = min(first_i, of);
    }
    if (lane == 0) { L.wbest[wave] = best; L.wbi[wave] = best_i; L.wfi[wave] = first_i; }
    __syncthreads();
    best = L.wbest[0]; best_i = L.wbi[0]; first_i = L.wfi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const double ob = L.wbest[w];
      const int oi = L.wbi[w];
      if ((int)(ob > best) | ((int)(ob == best) & (int)(oi < best_i))) { best = ob; best_i = oi; }
      first_i = min(first_i, L.wfi[w]);
    }
    // nothing left compares above -inf (NaN values: a zero vector under `normalize`): the lowest remaining index
    last = best_i != 0x7fffffff ? best_i : first_i;
    if (tid == 0) { out[step] = L.id[last]; L.taken[last] = 1; }
    __syncthreads();
  }
}

template <int FMT>
__global__ __launch_bounds__(256) void rarc_mmr_rows_kernel(const void* rows, const float* rowscale, int64_t n_rows, int d_pad, int d,
                                                            const double* queries, int64_t ldq, const int64_t* cand_ids, int n,
                                                            int64_t id_base, int normalize, int k, double lambda, int64_t* out_ids,
                                                            double* ws) {
  constexpr int E = MmrRowFmt<FMT>::E, BYTES = MmrRowFmt<FMT>::BYTES;
  __shared__ MmrRowsLds L;
  extern __shared__ double s_gram[];          // MMR_GRAM_N x MMR_GRAM_N when the launch has n <= MMR_GRAM_N, nothing otherwise
  double* gram_lds = n <= MMR_GRAM_N ? s_gram : nullptr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t q = blockIdx.x;
  const int64_t* ids = cand_ids + q * (size_t)n;
  int64_t* out = out_ids + q * (size_t)k;
  // the candidates: the entries that name a row, kept in order
  int nc = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + tid;
    const int64_t id = i < n ? ids[i] : -1;
    const bool ok = id >= 0 && id >= id_base && id - id_base < n_rows;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(ok);
    if (lane == 0) L.wcnt[wave] = __builtin_popcountll(bal);
    __syncthreads();
    int off = nc;
    for (int w = 0; w < wave; ++w) off += L.wcnt[w];
    if (ok) L.id[off + __builtin_popcountll(bal & ((1ull << lane) - 1ull))] = id;
    nc += L.wcnt[0] + L.wcnt[1] + L.wcnt[2] + L.wcnt[3];
    __syncthreads();
  }
  if (k >= nc) {      // everything is selected: the given order (as _mmr_select), -1 behind it
    for (int i = tid; i < k; i += 256) out[i] = i < nc ? L.id[i] : -1;
    return;
  }
  double* et = ws + q * ((size_t)n * d + d);   // [d][nc]
  double* qn = et + (size_t)n * d;             // [d]
  const int chunks = (d + E - 1) / E;          // (d <= d_pad, d_pad a multiple of 16: the last chunk stays inside the row)
  for (int idx = tid; idx < nc * chunks; idx += 256) {
    const int i = idx % nc, c = idx / nc;
    const int64_t r = L.id[i] - id_base;
    const uint4 v = *(const uint4*)((const char*)rows + ((size_t)r * d_pad + (size_t)c * E) * BYTES);
    double o[E];
    mmr_widen16<FMT>(v, FMT == 1 ? rowscale[r] : 1.0f, o);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const int m = c * E + j;
      if (m < d) et[(size_t)m * nc + i] = o[j];
    }
  }
  for (int m = tid; m < d; m += 256) qn[m] = queries[q * (size_t)ldq + m];
  __syncthreads();
  if (nc <= 256) mmr_rows_select<1>(L, gram_lds, nc, d, normalize, k, lambda, et, qn, out);
  else mmr_rows_select<4>(L, gram_lds, nc, d, normalize, k, lambda, et, qn, out);
}

extern "C" size_t rarc_mmr_rows_workspace_bytes(int nq, int n, int d) {
  return nq > 0 && n > 0 && n <= MMR_MAX_N && d > 0 ? (size_t)nq * ((size_t)n * d + d) * sizeof(double) : 0;
}

extern "C" int rarc_mmr_select_rows(const void* d_rows, int fmt, const float* d_rowscale, int64_t n_rows, int d_pad, int d,
                                    const double* d_queries, int64_t ldq, int nq, const int64_t* d_cand_ids, int n,
                                    int64_t id_base, int normalize, int k, double lambda, int64_t* d_out_ids, void* d_ws,
                                    size_t ws_bytes, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_rows && d_queries && d_cand_ids && d_out_ids && d_ws, RARC_E_INVALID, "rarc_mmr_select_rows: null pointer");
  RARC_REQUIRE(nq >= 0 && n >= 1 && d >= 1 && d <= d_pad && d_pad % 16 == 0 && ldq >= d && k >= 1 && n_rows >= 0, RARC_E_INVALID,
               "rarc_mmr_select_rows: bad sizes (nq=%d, n=%d, d=%d of d_pad=%d (a multiple of 16), ldq=%lld, k=%d, n_rows=%lld)", nq,
               n, d, d_pad, (long long)ldq, k, (long long)n_rows);
  RARC_REQUIRE(n <= MMR_MAX_N, RARC_E_UNSUPPORTED, "rarc_mmr_select_rows: n=%d exceeds %d candidates per query", n, MMR_MAX_N);
  RARC_REQUIRE(fmt >= 0 && fmt <= 2, RARC_E_INVALID, "rarc_mmr_select_rows: unknown row format %d (0 fp16, 1 fp8, 2 fp32)", fmt);
  RARC_REQUIRE(fmt != 1 || d_rowscale, RARC_E_INVALID, "rarc_mmr_select_rows: fp8 rows need their row scales");
  RARC_REQUIRE(((uintptr_t)d_rows & 15) == 0, RARC_E_INVALID, "rarc_mmr_select_rows: the rows must be 16-byte aligned");
  RARC_REQUIRE(((uintptr_t)d_ws & 7) == 0 && ws_bytes >= rarc_mmr_rows_workspace_bytes(nq, n, d), RARC_E_WORKSPACE,
               "rarc_mmr_select_rows: workspace of %zu bytes, %zu needed (8-byte aligned)", ws_bytes,
               rarc_mmr_rows_workspace_bytes(nq, n, d));
  if (nq == 0) return RARC_OK;
  const hipStream_t s = (hipStream_t)stream;
  double* ws = (double*)d_ws;
  const size_t gram_bytes = n <= MMR_GRAM_N ? sizeof(double) * MMR_GRAM_N * MMR_GRAM_N : 0;   // (the pairs-first form's matrix)
#define MMR_ROWS(F)                                                                                                                \
  hipLaunchKernelGGL(rarc_mmr_rows_kernel<F>, dim3(nq), dim3(256), gram_bytes, s, d_rows, d_rowscale, n_rows, d_pad, d, d_queries, ldq,      \
                     d_cand_ids, n, id_base, normalize, k, lambda, d_out_ids, ws)
  if (fmt == 0) MMR_ROWS(0);
  else if (fmt == 1) MMR_ROWS(1);
  else MMR_ROWS(2);
#undef MMR_ROWS
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}
