// subset.hip — exact top-k over a LIST of rows of one index: the search behind a metadata filter (FlatIndexF16.search_filtered,
// HipFlatVectorStore's `filter=`), with one filter for the call or one PER QUERY (search_filtered_many, the store's `filters=`
// and its coalescing front).  The scans and the chunked-GEMM search read every stored row; a filter that lets a thousandth of
// them through wants the allowed rows and nothing else.
//
//   rarc_search_rows      every listed row scored canonically, once per query, and ranked by the finalize's own 64-bit key
//                         (rarc_candkey; (0 - dist, ~row) for metric "l2"): no approximate pass, no bound, nothing to overflow
//   rarc_strike_rows      the other way to a filtered answer: an ordinary top-k' answer with the rows outside a bitmask struck
//                         out and each query's first k survivors kept in order (the over-fetch leg; a query with fewer
//                         survivors than it should have is then answered by rarc_search_rows)
//   rarc_search_rows_grouped, rarc_strike_rows_grouped
//                         the same two with a list / a mask per query: the queries of a call arrive sorted by group, each
//                         group with a row list of its own, all lists concatenated in one buffer
//
// The two forms differ in how a workgroup finds its queries, its list and its count, and in nothing else: there is ONE walk
// over list entries (sub_walk), ONE select (sub_select) and ONE strike (sub_strike), each a device function that the kernels of
// both forms call, so each query's answer under the grouped form is rarc_search_rows's for its list, bit for bit, by
// construction.
//
// A search walks its list(s) in slabs.  Per slab:
//   score    a workgroup stages QT queries in LDS (fp32; QT = 8 up to 2048 padded dimensions, 4 beyond: at most 64 KB) and
//            walks 32 listed rows per step, eight lanes per row (canon_topk.h: wide_canon_dot8n — a row is fetched from HBM once
//            for the QT queries, in 16-byte loads, two in flight per lane).  The key of (query, row) goes to the query's list,
//            behind the k best kept from the slabs before.  QT = 1 (the reference's call: one query) is a pure gather,
//            m · 2 · d_pad bytes.
//              subset_score_kernel          queries [QT blockIdx.y, + QT) of the call, the slab handed in by the host
//              subset_score_grouped_kernel  the tile table d_tiles (int64 [n_tiles][4] = first query, queries (<= QT), where the
//                                           group's list starts in d_lists, its length m_g) cuts the queries into tiles that
//                                           never span two groups; workgroup (x, tile) walks entries [round slab, (round + 1)
//                                           slab) of its group's list, if the list reaches that far
//   select   one workgroup per query: the k best keys of (kept + slab) by radix select (canon_topk.h) back to the front of the
//            list; behind the last slab they are sorted and written out.
//              subset_select_kernel          the count handed in by the host
//              subset_select_grouped_kernel  the count worked out from the group's m_g: a slab is longer than any k, so every
//                                            round but a group's last leaves more than k keys — a query keeps 0 keys before
//                                            round 0 and k before any other, and both follow from the table; nothing is uploaded
//                                            per round.  The select between rounds runs for the queries whose list goes on; ONE
//                                            last select answers every query over its own count (a group that ended earlier has
//                                            kept its keys untouched until then).
// The workspace is 256 lists of k + slab keys, whatever m is: slab = 8M keys / nq - k clamped to [32768, 262144] rows — a
// single query takes long slabs (its select is one workgroup: few of them), a full batch short ones (84 MB at k = 8192).
//
// The caller's contract: a list holds row numbers, STRICTLY ASCENDING, each < n_rows.  Neither is checked (a check would
// read the list back); distinct rows are what makes a query's keys distinct, which the select counts on.
#include <type_traits>

#include "rarc_common.h"
#include "canon_topk.h"

namespace {
constexpr int SUB_KMAX = 8192;                 // largest k (the select holds its answer in LDS: 64 KB)
constexpr int SUB_BUDGET_KEYS = 8 << 20;       // keys of one slab over all queries (64 MB)
constexpr int SUB_SLAB_MIN = 32768, SUB_SLAB_MAX = 262144;
static_assert(SUB_SLAB_MIN > SUB_KMAX, "a full slab must leave more than k keys: sub_round_kept counts on it");

int sub_slab_rows(int nq, int k) {
  int64_t s = (int64_t)SUB_BUDGET_KEYS / nq - k;
  s = s < SUB_SLAB_MIN ? SUB_SLAB_MIN : (s > SUB_SLAB_MAX ? SUB_SLAB_MAX : s);
  return (int)(s / 32 * 32);
}
size_t sub_ws_bytes(int nq, int k) { return 1024 + (size_t)nq * ((size_t)k + sub_slab_rows(nq, k)) * 8; }

// what a query of a group holds when round `round` of its list begins, and how many list entries that round adds
__device__ __forceinline__ uint32_t sub_round_kept(uint32_t round, uint32_t k) { return round ? k : 0u; }
__device__ __forceinline__ uint32_t sub_round_n(int64_t m, uint32_t round, uint32_t slab) {
  const int64_t left = m - (int64_t)round * (int64_t)slab;
  return left <= 0 ? 0u : (left < (int64_t)slab ? (uint32_t)left : slab);
}

// metric "l2": qn[q] = canonical dot(q, q) — the finalize's arithmetic with the query block as the "rows"
__global__ __launch_bounds__(256) void subset_qn_kernel(const float* __restrict__ q32, int d_pad, int nq, float* __restrict__ qn) {
  const int q = blockIdx.x * 32 + (threadIdx.x >> 3), j = threadIdx.x & 7;
  const int qc = q < nq ? q : nq - 1;
  const float s = wide_canon_dot8<true>(q32 + (size_t)qc * d_pad, q32, (size_t)qc, d_pad, j, nullptr);
  if (q < nq && j == 0) qn[q] = s;
}

// s_q[t][0 .. d_pad) = query q0 + t for t < cnt, zeros for t in [cnt, staged)
__device__ __forceinline__ void sub_stage_queries(float* s_q, const float* __restrict__ q32, int d_pad, int q0, int cnt, int staged) {
  for (int i = threadIdx.x; i < staged * d_pad; i += 256) s_q[i] = i / d_pad < cnt ? q32[(size_t)q0 * d_pad + i] : 0.f;
  __syncthreads();
}

// THE walk: keys[q0 + t][kept + i] = key of (query q0 + t, row list[i]) for i < n_list, t < cnt, the QN staged queries in s_q.
// xn: null = inner-product keys; else the rows' squared norms and qn the queries' (metric "l2").
template <bool F32ROWS, int QN>
__device__ __forceinline__ void sub_walk(const float* s_q, uint4* s_stage, const void* __restrict__ rows, int d_pad, int q0, int cnt,
                                         const int64_t* __restrict__ list, uint32_t n_list, uint64_t* __restrict__ keys,
                                         uint32_t stride, uint32_t kept, const float* __restrict__ xn, const float* __restrict__ qn) {
  const int j = threadIdx.x & 7;
  uint4* stage = s_stage + (threadIdx.x & ~7);              // 128 bytes per 8-lane group
  // whole groups of 32 rows per step: the lanes of a group stay together through the shuffles; entries past the end of the
  // list are read as its last one and not written
  for (uint32_t i0 = blockIdx.x * 32; i0 < n_list; i0 += gridDim.x * 32) {
    const uint32_t i = i0 + (threadIdx.x >> 3);
    const bool live = i < n_list;
    const uint32_t row = (uint32_t)list[live ? i : n_list - 1];
    float s[QN];
    wide_canon_dot8n<F32ROWS, QN>(s_q, d_pad, rows, (size_t)row, d_pad, j, stage, s);
    if (live && j == 0) {
      const float xr = xn ? xn[row] : 0.f;
#pragma unroll
      for (int t = 0; t < QN; ++t)
        if (t < cnt)
          keys[(size_t)(q0 + t) * stride + kept + i] = rarc_candkey(xn ? wide_l2_neg_dist(qn[q0 + t], xr, s[t]) : s[t], row);
    }
  }
}

template <bool F32ROWS, int QT>
__global__ __launch_bounds__(256) void subset_score_kernel(const void* __restrict__ rows, int d_pad, const float* __restrict__ q32,
                                                           int nq, const int64_t* __restrict__ list, uint32_t n_list,
                                                           uint64_t* __restrict__ keys, uint32_t stride, uint32_t kept,
                                                           const float* __restrict__ xn, const float* __restrict__ qn) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_q = (float*)smem;                                // [QT][d_pad]
  __shared__ uint4 s_stage[256];
  const int q0 = blockIdx.y * QT;
  const int cnt = nq - q0 < QT ? nq - q0 : QT;
  sub_stage_queries(s_q, q32, d_pad, q0, cnt, QT);
  sub_walk<F32ROWS, QT>(s_q, s_stage, rows, d_pad, q0, cnt, list, n_list, keys, stride, kept, xn, qn);
}

// Every exit and branch below depends on the tile's entry and blockIdx only: a workgroup takes it as a whole.
template <bool F32ROWS, int QT>
__global__ __launch_bounds__(256) void subset_score_grouped_kernel(const void* __restrict__ rows, int d_pad, const float* __restrict__ q32,
                                                                   int nq, const int64_t* __restrict__ lists,
                                                                   const int64_t* __restrict__ tiles, uint32_t round, uint32_t slab,
                                                                   uint32_t k, uint64_t* __restrict__ keys, uint32_t stride,
                                                                   const float* __restrict__ xn, const float* __restrict__ qn) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_q = (float*)smem;                                // [QT][d_pad]
  __shared__ uint4 s_stage[256];
  const int64_t* tile = tiles + 4 * (size_t)blockIdx.y;
  const int64_t q0l = tile[0];
  const uint32_t n_list = sub_round_n(tile[3], round, slab);
  if (q0l < 0 || q0l >= nq || blockIdx.x * 32u >= n_list) return;       // this group's list ended in an earlier round
  const int q0 = (int)q0l;
  int cnt = (int)(tile[1] < QT ? tile[1] : QT);
  cnt = cnt < nq - q0 ? cnt : nq - q0;
  if (cnt < 1) return;
  sub_stage_queries(s_q, q32, d_pad, q0, cnt, cnt == 1 ? 1 : QT);
  const int64_t* list = lists + tile[2] + (int64_t)round * (int64_t)slab;
  const uint32_t kept = sub_round_kept(round, k);
  // a tile of one query (256 tenants, one query each) is a gather
  if (QT > 1 && cnt == 1) sub_walk<F32ROWS, 1>(s_q, s_stage, rows, d_pad, q0, 1, list, n_list, keys, stride, kept, xn, qn);
  else sub_walk<F32ROWS, QT>(s_q, s_stage, rows, d_pad, q0, cnt, list, n_list, keys, stride, kept, xn, qn);
}

// THE select: one workgroup over the c keys of query q.  last == 0: the k best (c > k) move to the front of the list, in no
// particular order.  last != 0: the min(k, c) best in exact order are the answer; (-1, -inf) — metric "l2": (-1, +inf) — behind
// them.  s_top: [pow2 >= min(k, c)] keys of dynamic LDS.
template <bool L2>
__device__ __forceinline__ void sub_select(uint64_t* s_top, uint64_t* keys, uint32_t q, uint32_t c, uint32_t k, int last,
                                           int64_t id_base, int64_t* out_ids, float* out_scores, uint32_t* status) {
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_pick[2];
  __shared__ uint32_t s_cnt[2];
  const uint32_t kk = k < c ? k : c;
  uint32_t pow2 = 1;
  while (pow2 < kk) pow2 <<= 1;
  wide_topk_keys(keys, c, kk, pow2, s_top, s_hist, s_pick, s_cnt, last != 0);
  if (!last) {          // (every read of the list is behind the barriers of wide_topk_keys)
    for (uint32_t i = threadIdx.x; i < kk; i += blockDim.x) keys[i] = s_top[i];
    return;
  }
  wide_write_topk<L2>(s_top, kk, k, id_base, out_ids + (size_t)q * k, out_scores + (size_t)q * k);
  if (q == 0)
    for (uint32_t i = threadIdx.x; i < RARC_MAX_QUERIES; i += blockDim.x) status[i] = RARC_Q_OK;     // nothing here can overflow
}

template <bool L2>
__global__ __launch_bounds__(1024) void subset_select_kernel(uint64_t* keys_all, uint32_t stride, uint32_t c, uint32_t k, int last,
                                                             int64_t id_base, int64_t* out_ids, float* out_scores, uint32_t* status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t q = blockIdx.x;
  sub_select<L2>((uint64_t*)smem, keys_all + (size_t)q * stride, q, c, k, last, id_base, out_ids, out_scores, status);
}

// last == 0: behind round `round`, for the queries whose list has a further round (k + slab keys); last != 0: every query.
template <bool L2>
__global__ __launch_bounds__(1024) void subset_select_grouped_kernel(uint64_t* keys_all, uint32_t stride, const int64_t* __restrict__ tiles,
                                                                     int n_tiles, uint32_t round, uint32_t slab, uint32_t k, int last,
                                                                     int64_t id_base, int64_t* out_ids, float* out_scores,
                                                                     uint32_t* status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ long long s_m;
  const uint32_t q = blockIdx.x;
  if (threadIdx.x == 0) s_m = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n_tiles; i += blockDim.x) {          // the one tile that holds this query
    const int64_t* tile = tiles + 4 * (size_t)i;
    if ((int64_t)q >= tile[0] && (int64_t)q < tile[0] + tile[1]) s_m = tile[3];
  }
  __syncthreads();
  const int64_t m = s_m;
  const int64_t rounds = (m + slab - 1) / slab;
  uint32_t c;
  if (!last) {
    if ((int64_t)round + 1 >= rounds) return;              // (the whole workgroup: m is the same in every thread)
    c = sub_round_kept(round, k) + slab;
  } else {
    c = rounds <= 0 ? 0u : sub_round_kept((uint32_t)(rounds - 1), k) + sub_round_n(m, (uint32_t)(rounds - 1), slab);
  }
  sub_select<L2>((uint64_t*)smem, keys_all + (size_t)q * stride, q, c, k, last, id_base, out_ids, out_scores, status);
}

// THE strike: out[q][0 .. k) = the first k entries of in[q][0 .. kp) whose row has its bit set in `bits` (keep_all: whatever
// its bit), in order, padding behind them; count[q] = how many were found before the walk ended (it ends at k).  256 threads
// walk 256 entries per step.
__device__ __forceinline__ void sub_strike(const int64_t* __restrict__ ids, const float* __restrict__ scores, int kp,
                                           const uint32_t* __restrict__ bits, bool keep_all, int64_t n_rows, int64_t id_base, int k,
                                           float pad, int64_t* __restrict__ out_ids, float* __restrict__ out_scores,
                                           uint32_t* __restrict__ count) {
  __shared__ uint32_t s_wave[4];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint32_t base = 0;
  for (int i0 = 0; i0 < kp && base < (uint32_t)k; i0 += 256) {      // (base is the same in every thread)
    const int i = i0 + tid;
    bool ok = false;
    int64_t id = -1;
    float s = pad;
    if (i < kp) {
      id = ids[(size_t)q * kp + i];
      s = scores[(size_t)q * kp + i];
      const int64_t r = id - id_base;
      ok = id >= 0 && r >= 0 && r < n_rows && (keep_all || ((bits[r >> 5] >> (r & 31)) & 1u));
    }
    const unsigned long long b = __builtin_amdgcn_ballot_w64(ok);
    if (lane == 0) s_wave[w] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    uint32_t pos = base + (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1ull));
    for (int v = 0; v < w; ++v) pos += s_wave[v];
    if (ok && pos < (uint32_t)k) {
      out_ids[(size_t)q * k + pos] = id;
      out_scores[(size_t)q * k + pos] = s;
    }
    base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
  for (uint32_t i = base + tid; i < (uint32_t)k; i += 256) {
    out_ids[(size_t)q * k + i] = -1;
    out_scores[(size_t)q * k + i] = pad;
  }
  if (tid == 0) count[q] = base < (uint32_t)k ? base : (uint32_t)k;
}

// one mask for every query / the mask of query q starting at word bits_off[q] of bits_all (negative: every row stays).  Two
// kernels around the one body: the one-filter strike keeps the instructions it had before the offsets existed.
__global__ __launch_bounds__(256) void strike_rows_kernel(const int64_t* __restrict__ ids, const float* __restrict__ scores, int kp,
                                                          const uint32_t* __restrict__ bits, int64_t n_rows, int64_t id_base, int k,
                                                          float pad, int64_t* __restrict__ out_ids, float* __restrict__ out_scores,
                                                          uint32_t* __restrict__ count) {
  sub_strike(ids, scores, kp, bits, false, n_rows, id_base, k, pad, out_ids, out_scores, count);
}
__global__ __launch_bounds__(256) void strike_rows_grouped_kernel(const int64_t* __restrict__ ids, const float* __restrict__ scores,
                                                                  int kp, const uint32_t* __restrict__ bits_all,
                                                                  const int64_t* __restrict__ bits_off, int64_t n_rows, int64_t id_base,
                                                                  int k, float pad, int64_t* __restrict__ out_ids,
                                                                  float* __restrict__ out_scores, uint32_t* __restrict__ count) {
  const int64_t off = bits_off[blockIdx.x];
  sub_strike(ids, scores, kp, bits_all + (off < 0 ? 0 : off), off < 0, n_rows, id_base, k, pad, out_ids, out_scores, count);
}

// ------------------------------------------------------------------------------------------------------------------- host side
// Launch kernel K with up to 64 KB of dynamic LDS: the attribute is set once per device and per kernel (one flag set per K).
template <auto K, typename... Args>
int sub_launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
  static RarcPerDevice attr_done;
  if (size_t& done = attr_done.cur(); !done) {
    RARC_HIP_CHECK(hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    done = 1;
  }
  hipLaunchKernelGGL(K, grid, block, lds, s, args...);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

// THE dispatch: f(rows are fp32, queries per score workgroup) with both as types — QT = 1 for a single query, 4 beyond 2048
// padded dimensions, else 8 — and f(metric is "l2") for the selects.
template <typename F>
int sub_with_bool(bool b, F f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
template <typename F>
int sub_with_rows_and_tile(int fmt, int nq, int d_pad, F f) {
  return sub_with_bool(fmt == 2, [&](auto f32) {
    return nq == 1         ? f(f32, std::integral_constant<int, 1>{})
           : d_pad > 2048 ? f(f32, std::integral_constant<int, 4>{})
                          : f(f32, std::integral_constant<int, 8>{});
  });
}

// enough score workgroups to fill 256 CUs a few times over, each staging its queries once for several steps; n_list: the
// entries of the (longest) list this launch walks — a shorter one's spare workgroups leave at once
dim3 sub_score_grid(uint32_t n_list, uint32_t qtiles) {
  const uint32_t steps = (n_list + 31) / 32;
  uint32_t gx = 2048 / qtiles;
  gx = gx < 8 ? 8 : gx;
  gx = gx > steps ? steps : gx;
  return dim3(gx, qtiles);
}
size_t sub_select_lds(int k) {
  uint32_t pow2 = 1;
  while (pow2 < (uint32_t)k) pow2 <<= 1;
  return (size_t)pow2 * 8;
}

// what the two searches share once their arguments are checked: the carved workspace and query block
struct SubCall {
  float* qn;          // [256] the queries' squared norms (metric "l2")
  uint64_t* keys;     // [nq][stride = k + slab]
  int slab;
  uint32_t stride;
  RarcQb qb;
  const float* xn;    // the rows' squared norms, null unless metric "l2"
};

// THE prologue of rarc_search_rows (m_name "m") and rarc_search_rows_grouped ("m_max"): the argument checks under the name `fn`
// of the function the caller called, the workspace carve, and the queries' norms for metric "l2".
int sub_begin(const char* fn, const char* m_name, const void* d_rows, int fmt, int64_t n_rows, int d_pad, const void* d_qblock, int nq,
              const int64_t* d_list, int64_t m, int k, const float* d_xn, int l2, const int64_t* d_out_ids, const float* d_out_scores,
              const uint32_t* d_status, void* d_ws, size_t ws_bytes, hipStream_t s, SubCall* c) {
  RARC_REQUIRE(d_rows && d_qblock && d_out_ids && d_out_scores && d_status && d_ws && (d_list || m == 0), RARC_E_INVALID,
               "%s: null pointer", fn);
  RARC_REQUIRE(fmt == 0 || fmt == 2, RARC_E_INVALID, "%s: fmt 0 (fp16 rows) or 2 (fp32 rows), got %d", fn, fmt);
  RARC_REQUIRE(!l2 || d_xn, RARC_E_INVALID, "%s: null pointer (d_xn: metric l2 needs the rows' squared norms, rarc_row_sqnorms)", fn);
  RARC_REQUIRE(d_pad > 0 && d_pad % RARC_DIM_ALIGN == 0 && d_pad <= 4096, RARC_E_UNSUPPORTED,
               "%s: padded dim %d unsupported (multiple of %d, <= 4096)", fn, d_pad, RARC_DIM_ALIGN);
  RARC_REQUIRE(nq >= 1 && nq <= RARC_MAX_QUERIES && k >= 1 && k <= SUB_KMAX, RARC_E_INVALID,
               "%s: need 1 <= nq <= %d, 1 <= k <= %d (nq=%d k=%d)", fn, RARC_MAX_QUERIES, SUB_KMAX, nq, k);
  RARC_REQUIRE(n_rows >= 0 && n_rows < (int64_t)0xffffff00ll && m >= 0 && m <= n_rows, RARC_E_INVALID,
               "%s: need 0 <= %s <= n_rows < 2^32 - 256 (%s=%lld n_rows=%lld)", fn, m_name, m_name, (long long)m, (long long)n_rows);
  char* wsb = (char*)(((uintptr_t)d_ws + 255) & ~(uintptr_t)255);
  RARC_REQUIRE(wsb + sub_ws_bytes(nq, k) <= (char*)d_ws + ws_bytes, RARC_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn,
               ws_bytes, sub_ws_bytes(nq, k) + 256);
  c->qn = (float*)wsb;
  c->keys = (uint64_t*)(wsb + 1024);
  c->slab = sub_slab_rows(nq, k);
  c->stride = (uint32_t)(k + c->slab);
  c->qb = rarc_qb_carve(d_qblock, d_pad);
  c->xn = l2 ? d_xn : nullptr;
  if (l2 && m > 0) {
    hipLaunchKernelGGL(subset_qn_kernel, dim3((nq + 31) / 32), dim3(256), 0, s, c->qb.q32, d_pad, nq, c->qn);
    RARC_HIP_CHECK(hipGetLastError());
  }
  return RARC_OK;
}
}  // namespace

extern "C" size_t rarc_search_rows_workspace_bytes(int nq, int k) {
  return (nq >= 1 && nq <= RARC_MAX_QUERIES && k >= 1 && k <= SUB_KMAX) ? sub_ws_bytes(nq, k) + 256 : 0;
}
extern "C" size_t rarc_search_rows_grouped_workspace_bytes(int nq, int k) { return rarc_search_rows_workspace_bytes(nq, k); }

extern "C" int rarc_search_rows(const void* d_rows, int fmt, int64_t n_rows, int d_pad, const void* d_qblock, int nq,
                                const int64_t* d_list, int64_t m, int k, int64_t id_base, const float* d_xn, int l2,
                                int64_t* d_out_ids, float* d_out_scores, uint32_t* d_status, void* d_ws, size_t ws_bytes,
                                void* stream) {
  RARC_RANGE();
  hipStream_t s = (hipStream_t)stream;
  SubCall c;
  int rc = sub_begin("rarc_search_rows", "m", d_rows, fmt, n_rows, d_pad, d_qblock, nq, d_list, m, k, d_xn, l2, d_out_ids, d_out_scores,
                     d_status, d_ws, ws_bytes, s, &c);
  if (rc != RARC_OK) return rc;
  auto select = [&](uint32_t count, int last) {
    return sub_with_bool(l2 != 0, [&](auto is_l2) {
      return sub_launch<subset_select_kernel<decltype(is_l2)::value>>(dim3(nq), dim3(1024), sub_select_lds(k), s, c.keys, c.stride, count,
                                                                      (uint32_t)k, last, id_base, d_out_ids, d_out_scores, d_status);
    });
  };
  uint32_t kept = 0;
  for (int64_t at = 0; at < m; at += c.slab) {
    const uint32_t n = (uint32_t)(m - at < c.slab ? m - at : c.slab);
    rc = sub_with_rows_and_tile(fmt, nq, d_pad, [&](auto f32, auto qt) {
      constexpr int QT = decltype(qt)::value;
      return sub_launch<subset_score_kernel<decltype(f32)::value, QT>>(sub_score_grid(n, (uint32_t)((nq + QT - 1) / QT)), dim3(256),
                                                                       (size_t)QT * d_pad * 4, s, d_rows, d_pad, c.qb.q32, nq, d_list + at,
                                                                       n, c.keys, c.stride, kept, c.xn, c.qn);
    });
    if (rc != RARC_OK) return rc;
    kept += n;
    if (at + c.slab < m && kept > (uint32_t)k) {       // more slabs follow: keep the k best (the last slab's select is the answer's)
      if ((rc = select(kept, 0)) != RARC_OK) return rc;
      kept = (uint32_t)k;
    }
  }
  return select(kept, 1);
}

extern "C" int rarc_search_rows_grouped(const void* d_rows, int fmt, int64_t n_rows, int d_pad, const void* d_qblock, int nq,
                                        const int64_t* d_lists, const int64_t* d_tiles, int n_tiles, int64_t m_max, int k,
                                        int64_t id_base, const float* d_xn, int l2, int64_t* d_out_ids, float* d_out_scores,
                                        uint32_t* d_status, void* d_ws, size_t ws_bytes, void* stream) {
  RARC_RANGE();
  hipStream_t s = (hipStream_t)stream;
  RARC_REQUIRE(d_tiles, RARC_E_INVALID, "rarc_search_rows_grouped: null pointer");
  RARC_REQUIRE(n_tiles >= 1 && n_tiles <= nq, RARC_E_INVALID,
               "rarc_search_rows_grouped: need 1 <= n_tiles <= nq: every query in one tile (n_tiles=%d nq=%d)", n_tiles, nq);
  SubCall c;
  int rc = sub_begin("rarc_search_rows_grouped", "m_max", d_rows, fmt, n_rows, d_pad, d_qblock, nq, d_lists, m_max, k, d_xn, l2, d_out_ids,
                     d_out_scores, d_status, d_ws, ws_bytes, s, &c);
  if (rc != RARC_OK) return rc;
  auto select = [&](uint32_t round, int last) {
    return sub_with_bool(l2 != 0, [&](auto is_l2) {
      return sub_launch<subset_select_grouped_kernel<decltype(is_l2)::value>>(dim3(nq), dim3(1024), sub_select_lds(k), s, c.keys, c.stride,
                                                                              d_tiles, n_tiles, round, (uint32_t)c.slab, (uint32_t)k, last,
                                                                              id_base, d_out_ids, d_out_scores, d_status);
    });
  };
  uint32_t round = 0;
  for (int64_t at = 0; at < m_max; at += c.slab, ++round) {
    const uint32_t n = (uint32_t)(m_max - at < c.slab ? m_max - at : c.slab);      // of the longest list still walking
    rc = sub_with_rows_and_tile(fmt, nq, d_pad, [&](auto f32, auto qt) {
      constexpr int QT = decltype(qt)::value;
      return sub_launch<subset_score_grouped_kernel<decltype(f32)::value, QT>>(sub_score_grid(n, (uint32_t)n_tiles), dim3(256),
                                                                               (size_t)QT * d_pad * 4, s, d_rows, d_pad, c.qb.q32, nq,
                                                                               d_lists, d_tiles, round, (uint32_t)c.slab, (uint32_t)k,
                                                                               c.keys, c.stride, c.xn, c.qn);
    });
    if (rc != RARC_OK) return rc;
    if (at + c.slab < m_max && (rc = select(round, 0)) != RARC_OK) return rc;      // some list goes on: its queries keep their k best
  }
  return select(0, 1);
}

// rarc_strike_rows (d_bits_off null: one mask) and rarc_strike_rows_grouped (d_bits_off[q] = the word of d_bits at which query
// q's mask starts, negative = keep every row: an unfiltered caller in the same batch)
static int sub_strike_launch(const char* fn, const int64_t* d_ids, const float* d_scores, int nq, int kprime, const uint32_t* d_bits,
                             const int64_t* d_bits_off, int64_t n_rows, int64_t id_base, int k, int l2, int64_t* d_out_ids,
                             float* d_out_scores, uint32_t* d_count, void* stream) {
  RARC_REQUIRE(d_ids && d_scores && d_bits && d_out_ids && d_out_scores && d_count, RARC_E_INVALID, "%s: null pointer", fn);
  RARC_REQUIRE(nq >= 1 && k >= 1 && kprime >= 1 && n_rows >= 0, RARC_E_INVALID,
               "%s: need nq >= 1, k >= 1, kprime >= 1 (nq=%d k=%d kprime=%d)", fn, nq, k, kprime);
  const float pad = l2 ? INFINITY : -INFINITY;
  if (d_bits_off)
    hipLaunchKernelGGL(strike_rows_grouped_kernel, dim3(nq), dim3(256), 0, (hipStream_t)stream, d_ids, d_scores, kprime, d_bits, d_bits_off,
                       n_rows, id_base, k, pad, d_out_ids, d_out_scores, d_count);
  else
    hipLaunchKernelGGL(strike_rows_kernel, dim3(nq), dim3(256), 0, (hipStream_t)stream, d_ids, d_scores, kprime, d_bits, n_rows, id_base, k,
                       pad, d_out_ids, d_out_scores, d_count);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_strike_rows(const int64_t* d_ids, const float* d_scores, int nq, int kprime, const uint32_t* d_bits,
                                int64_t n_rows, int64_t id_base, int k, int l2, int64_t* d_out_ids, float* d_out_scores,
                                uint32_t* d_count, void* stream) {
  RARC_RANGE();
  return sub_strike_launch("rarc_strike_rows", d_ids, d_scores, nq, kprime, d_bits, nullptr, n_rows, id_base, k, l2, d_out_ids,
                           d_out_scores, d_count, stream);
}

extern "C" int rarc_strike_rows_grouped(const int64_t* d_ids, const float* d_scores, int nq, int kprime, const uint32_t* d_bits,
                                        const int64_t* d_bits_off, int64_t n_rows, int64_t id_base, int k, int l2, int64_t* d_out_ids,
                                        float* d_out_scores, uint32_t* d_count, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_bits_off, RARC_E_INVALID, "rarc_strike_rows_grouped: null pointer");
  return sub_strike_launch("rarc_strike_rows_grouped", d_ids, d_scores, nq, kprime, d_bits, d_bits_off, n_rows, id_base, k, l2,
                           d_out_ids, d_out_scores, d_count, stream);
}
