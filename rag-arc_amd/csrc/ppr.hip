// ppr.hip — personalized PageRank over the GRAPH blob rarc_graph_csr wrote, for a batch of queries at once:
// the retrieval a graph store is queried with (HippoRAG-style retrievers run one per query; with Neo4j it is
// gds.pageRank.stream(graph, {sourceNodes, dampingFactor: 0.85, maxIterations: 20})).  A power iteration over B queries is a
// sparse-matrix x dense-matrix product: the state is int64 [n][B], vertex-major, so one neighbour's B values are one
// contiguous read.
//
// The rule is fixed point (tests/ppr_ref.py restates it in Python integers).  rarc_graph_csr fills a row of the adjacency with
// atomics, so the order inside a row is arbitrary: a floating-point sum would depend on thread timing.  Integer sums are
// associative — the answer is the same bits for any edge order, any launch shape, either form of the step and any batch.
//   ONE = 2^40 is the unit of mass, a = round(damping * 65536), W(u) = u's weighted degree (uint32 weights >= 1).
//   t_q(v) = sum over q's seed slots (v, w) of (w << 40) // Wq, Wq = the sum of q's slot weights (w <= 2^20, <= 64 slots);  p_0 = t_q
//   c(u) = p(u) // W(u);   flow(v) = sum over neighbours u of w_uv * c(u)   (W(v) = 0: flow(v) = p(v), an isolated vertex keeps its mass)
//   p'(v) = ((65536 - a) * t_q(v) + a * flow(v)) >> 16;   delta_q = max_v |p' - p|;   delta_q <= tol: q is frozen from then on
//
// Why nothing overflows.  sum_v t_q(v) <= ONE (every slot is floored).  If sum_v p(v) <= ONE then, summing flow over v, every
// u contributes c(u) * sum_v w_uv = c(u) W(u) <= p(u) (an isolated v contributes p(v)): sum_v flow(v) <= sum_u p(u) <= ONE, and
// sum_v p'(v) <= ((65536 - a) ONE + a ONE) / 65536 = ONE.  By induction the total mass never exceeds ONE = 2^40, so
//   w_uv * c(u) <= W(u) * c(u) <= p(u) <= 2^40,   flow(v) <= 2^40,   (65536 - a) t + a flow <= 65536 * 2^40 = 2^56 < 2^57,
// and the seed's (w << 40) <= 2^60.  W(u) itself fits 32 bits because the caller keeps the total edge weight below 2^31 (as
// every level of Louvain does).  All of it is non-negative: the kernels compute in uint64.
//
// What is stored.  c = p // W is kept beside p so that the step divides once per (vertex, query), not once per (edge, query):
// a step reads c of slot `cur` at the neighbours and writes p (in place: only v's own thread reads p(v)) and c of the other
// slot.  t is dense [n][B].  The workspace is {delta u64 [256], done u32 [256], positive counts u32 [256]} | t | p | c0 | c1;
// rarc_ppr_topk builds its keys in the c slot the next step would overwrite.
//
// The step has two forms of one kernel; the launcher picks by B (PPR_VERTEX_PARALLEL_MAX_B, reported by rarc_ppr_limits):
//   query-parallel  (B > 32)   a lane is a query (two queries, one 16-byte load, when B is even and > 64); a wave walks one
//                              vertex's neighbours, its address arithmetic scalar
//   vertex-parallel (B <= 32)  BP = the power of two >= B; a wave's lanes are 64 / BP neighbour slots x BP queries: the slots
//                              share the vertex's neighbours and are joined by integer shuffle-adds
// and in both a vertex of more than LV_DEG_WAVE = 64 neighbours (the degree lists 2 and 3 of the blob) is split across the four
// waves of a workgroup, which are joined by integer adds in LDS: each wave writes 64 (or 128) consecutive 8-byte words, wave 0
// reads them back the same way — consecutive lanes on consecutive bank pairs, no conflict.
//
// Typed PPR (tests/typed_ppr_ref.py restates it): query q carries a uint32 filter F_q and the rule above runs on
// the graph of the edges whose mask shares a bit with it, each at its full weight:
//   W_q(u) = sum over u's slots (v, M, w) with M & F_q != 0 of w;   c(u) = p(u) // W_q(u);   flow(v) sums the same slots
//   (W_q(v) = 0: flow(v) = p(v), a vertex isolated under the filter keeps its mass)
// The step already walks every slot of v's row once per query lane, so W_q(v) is a second accumulator beside flow(v), summed
// under the same test and joined by the same shuffles and the same LDS words — no [n][B] array of degrees.  It is 32 bits wide:
// W_q <= W < 2^31.  The slots come from the typed adjacency with its weight plane (rarc_graph_types_weighted: neighbour, mask
// and weight side by side); the state, the workspace, the degree lists (by total degree, which is what bounds the walk) and
// every reader are the untyped ones.  The overflow argument carries over word for word with W_q for W: u contributes
// c(u) * sum over its allowed slots of w = c(u) W_q(u) <= p(u) to the flows, a vertex with W_q = 0 contributes p(v), so mass
// is still never created, w_uv * c(u) <= W_q(u) * c(u) <= p(u) <= 2^40 and every bound above holds.  A lane whose filters meet
// none of a slot's types does not load that neighbour's row of c.
//
// The last section projects the state through a mention map onto chunks (rarc_ppr_chunks*): its rule, its
// bounds and its guards are stated there.
#include "graph_csr.h"
#include "graph_types.h"
#include "chunk_ws.h"
#include "canon_topk.h"

constexpr int PPR_MAX_SEEDS = 64;
constexpr int PPR_MAX_K = 8192;
constexpr int PPR_VERTEX_PARALLEL_MAX_B = 32;
constexpr int PPR_SPLIT_DEGREE = LV_DEG_WAVE;               // a vertex of more neighbours is split across a workgroup's waves
constexpr uint32_t PPR_MAX_SEED_WEIGHT = 1u << 20;
constexpr int PPR_ONE_SHIFT = 40;
constexpr int64_t PPR_TOPK_N_LIMIT = 1ll << 24;             // the top-k key carries the vertex in 24 bits
constexpr size_t PPR_CTL_BYTES = 4096;                      // delta u64 [256] | done u32 [256] | positive u32 [256]

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

struct PprWs {
  u64* delta;
  uint32_t* done;
  uint32_t* positive;
  u64* t;
  u64* p;
  u64* c[2];
  size_t bytes;
};
static inline bool ppr_shape_ok(int64_t n, int64_t m, int nq) { return lv_shape_ok(n, m) && nq >= 1 && nq <= PPR_MAX_B; }
static PprWs ppr_carve(const void* base, int64_t n, int nq) {
  char* b = (char*)base;
  size_t o = 0;
  PprWs w;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  char* ctl = take(PPR_CTL_BYTES);
  w.delta = (u64*)ctl;
  w.done = (uint32_t*)(ctl + 2048);
  w.positive = (uint32_t*)(ctl + 3072);
  const size_t state = (size_t)n * (size_t)nq * 8;
  w.t = (u64*)take(state);
  w.p = (u64*)take(state);
  w.c[0] = (u64*)take(state);
  w.c[1] = (u64*)take(state);
  w.bytes = o;
  return w;
}

// ---- seeds ------------------------------------------------------------------------------------------------------------------------
// one thread per query: only it writes column q of t (zeroed before), so duplicated vertices add up without atomics.  A slot
// whose vertex lies outside [0, n) is unused; a weight above 2^20 counts as 2^20 (the callers refuse both before they get here)
__global__ __launch_bounds__(256) void ppr_seed_kernel(const int64_t* __restrict__ seeds, const uint32_t* __restrict__ weights, int B, int s,
                                                       int64_t n, u64* t) {
  const int q = threadIdx.x;
  if (q >= B) return;
  u64 wq = 0;
  for (int j = 0; j < s; ++j) {
    const int64_t v = seeds[(size_t)q * s + j];
    const uint32_t w = weights[(size_t)q * s + j];
    if (v >= 0 && v < n) wq += w < PPR_MAX_SEED_WEIGHT ? w : PPR_MAX_SEED_WEIGHT;
  }
  if (!wq) return;
  for (int j = 0; j < s; ++j) {
    const int64_t v = seeds[(size_t)q * s + j];
    uint32_t w = weights[(size_t)q * s + j];
    w = w < PPR_MAX_SEED_WEIGHT ? w : PPR_MAX_SEED_WEIGHT;
    if (v >= 0 && v < n && w) t[(size_t)v * B + q] += ((u64)w << PPR_ONE_SHIFT) / wq;
  }
}
// p_0 = t, c_0 = t // W.  TYPED: c_0 = 0 here, ppr_seed_typed_kernel writes t // W_q at the seeds (t is 0 elsewhere)
template <bool TYPED>
__global__ __launch_bounds__(256) void ppr_init_kernel(int64_t n, int B, const uint32_t* __restrict__ k, const u64* __restrict__ t, u64* p,
                                                       u64* c) {
  const int64_t total = n * B;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const u64 x = t[i];
    p[i] = x;
    u64 cv = 0;
    if (!TYPED && x) {
      const u64 w = k[i / B];
      cv = w ? x / w : 0;
    }
    c[i] = cv;
  }
}
// a wave per (query, seed slot): W_q of the seed vertex from its typed row, c_0(v) = t_q(v) // W_q(v).  t_q is non-zero on
// the seeds only; a vertex that repeats among q's slots is written twice with the same value
__global__ __launch_bounds__(256) void ppr_seed_typed_kernel(const int64_t* __restrict__ seeds, const uint32_t* __restrict__ filters, int B, int s,
                                                             int64_t n, const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ mask,
                                                             const uint32_t* __restrict__ adj_w, const u64* __restrict__ t, u64* c) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);                // (wave-uniform)
  if (item >= B * s) return;
  const int q = item / s;
  const int64_t v = seeds[item];
  if (v < 0 || v >= n) return;
  const uint32_t f = filters[q];
  const int64_t r0 = row_ptr[v], r1 = row_ptr[v + 1];
  uint32_t wq = 0;
  for (int64_t e = r0 + lane; e < r1; e += 64) wq += (mask[e] & f) ? adj_w[e] : 0u;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) wq += (uint32_t)__shfl_xor((int)wq, d, 64);
  if (lane == 0) {
    const size_t at = (size_t)v * B + q;
    c[at] = wq ? t[at] / wq : 0;
  }
}

// ---- the step -----------------------------------------------------------------------------------------------------------------------
struct PprStepArgs {
  const int64_t* row_ptr;
  const int32_t* adj;
  const uint32_t* adj_w;
  const uint32_t* k;
  const uint32_t* mask;                                     // TYPED: adj | mask | adj_w are the typed slot arrays, `k` is not read
  const uint32_t* filters;                                  // TYPED: uint32 [B]
  const u64* t;
  u64* p;
  const u64* c_old;
  u64* c_new;
  u64* delta;
  const uint32_t* done;
  int64_t n;
  int B;
  uint32_t a;
};

template <int QPL>
__device__ __forceinline__ void ppr_load(const u64* at, u64 (&x)[QPL]) {
  if (QPL == 2) {
    const u64x2 v = *(const u64x2*)at;      // B even, q even, the state 256-byte aligned: 16-byte aligned
    x[0] = v[0];
    x[QPL - 1] = v[1];
  } else {
    x[0] = *at;
  }
}

// BP: query lanes per neighbour slot (64: a lane is a query), QPL: queries per lane, SPLIT: a workgroup per vertex of a degree
// list, its waves joined in LDS; otherwise a wave per (vertex, chunk of BP * QPL queries) over every vertex, those of more
// than PPR_SPLIT_DEGREE neighbours left to the SPLIT launch.  TYPED: a slot counts for query q iff its mask meets F_q, and
// W_q(v), summed beside flow(v) under that test, stands where the untyped step reads k[v]
template <int BP, int QPL, bool SPLIT, bool TYPED = false>
__global__ __launch_bounds__(256) void ppr_step_kernel(const PprStepArgs p, const int32_t* __restrict__ list, const int64_t* __restrict__ list_count) {
  constexpr int NSLOT = 64 / BP;
  constexpr int STEP = SPLIT ? 4 * NSLOT : NSLOT;
  __shared__ u64 s_part[SPLIT ? 4 * BP * QPL : 1];
  __shared__ uint32_t s_wq[SPLIT && TYPED ? 4 * BP * QPL : 1];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = lane / BP, ql = lane % BP;
  const int B = p.B;
  const int chunks = (B + BP * QPL - 1) / (BP * QPL);
  const int64_t items = (SPLIT ? *list_count : p.n) * chunks;
  const int64_t first = SPLIT ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave;
  const int64_t stride = SPLIT ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4;
  u64 my_delta[QPL];
#pragma unroll
  for (int i = 0; i < QPL; ++i) my_delta[i] = 0;
  int q_prev = -1;
  uint32_t dn[QPL];
  uint32_t f[QPL];                                                     // TYPED: the filters of this lane's live queries, 0 for a frozen one
  uint32_t f_any = 0;                                                  // ... and their OR: a slot it does not meet is not loaded
  for (int64_t item = first; item < items; item += stride) {
    const int64_t vi = item / chunks;
    const int chunk = (int)(item - vi * chunks);
    const int64_t v = SPLIT ? (int64_t)list[vi] : vi;
    const int64_t r0 = p.row_ptr[v], deg = p.row_ptr[v + 1] - r0;
    if (!SPLIT && deg > PPR_SPLIT_DEGREE) continue;                    // (wave-uniform)
    const int q = chunk * BP * QPL + ql * QPL;                         // this lane's first query; q + QPL <= B or q >= B
    const bool in_b = q < B;
    if (q != q_prev) {                                                 // (once: the launcher's grids keep a wave on its chunk)
#pragma unroll
      for (int i = 0; i < QPL; ++i) dn[i] = in_b ? p.done[q + i] : 1u;
      if (TYPED) {
        f_any = 0;
#pragma unroll
        for (int i = 0; i < QPL; ++i) {
          f[i] = dn[i] ? 0u : p.filters[q + i];                        // (dn = 1 past the batch: nothing is read there)
          f_any |= f[i];
        }
      }
      if (q_prev >= 0 && q_prev < B) {
#pragma unroll
        for (int i = 0; i < QPL; ++i)
          if (my_delta[i]) atomicMax(&p.delta[q_prev + i], my_delta[i]);
      }
#pragma unroll
      for (int i = 0; i < QPL; ++i) my_delta[i] = 0;
      q_prev = q;
    }
    bool live = false;                                                 // a lane whose queries are all frozen reads no neighbour
#pragma unroll
    for (int i = 0; i < QPL; ++i) live = live || !dn[i];
    u64 acc[QPL];
    uint32_t wq[QPL];                                                  // TYPED: W_q(v) <= W(v) < 2^31
#pragma unroll
    for (int i = 0; i < QPL; ++i) acc[i] = 0, wq[i] = 0;
    if (live) {
      int64_t e = (SPLIT ? wave * NSLOT : 0) + slot;
      for (; e + 3 * STEP < deg; e += 4 * STEP) {                      // four neighbours in flight
        int32_t u[4];
        uint32_t w[4];
        uint32_t mk[4];
        u64 x[4][QPL];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          u[j] = p.adj[r0 + e + j * STEP];
          w[j] = p.adj_w[r0 + e + j * STEP];
          if (TYPED) mk[j] = p.mask[r0 + e + j * STEP];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!TYPED || (mk[j] & f_any)) {
            ppr_load<QPL>(p.c_old + (size_t)u[j] * B + q, x[j]);
          } else {
#pragma unroll
            for (int i = 0; i < QPL; ++i) x[j][i] = 0;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < QPL; ++i) {
            const uint32_t wj = !TYPED || (mk[j] & f[i]) ? w[j] : 0u;
            acc[i] += (u64)wj * x[j][i];
            if (TYPED) wq[i] += wj;
          }
      }
      for (; e < deg; e += STEP) {
        const int32_t u = p.adj[r0 + e];
        const uint32_t w = p.adj_w[r0 + e];
        const uint32_t mk = TYPED ? p.mask[r0 + e] : 0u;
        u64 x[QPL];
        if (!TYPED || (mk & f_any)) {
          ppr_load<QPL>(p.c_old + (size_t)u * B + q, x);
        } else {
#pragma unroll
          for (int i = 0; i < QPL; ++i) x[i] = 0;
        }
#pragma unroll
        for (int i = 0; i < QPL; ++i) {
          const uint32_t wj = !TYPED || (mk & f[i]) ? w : 0u;
          acc[i] += (u64)wj * x[i];
          if (TYPED) wq[i] += wj;
        }
      }
    }
    // the slots of a wave: integer shuffle-adds (every lane takes part, a frozen or idle one with zeros)
#pragma unroll
    for (int i = 0; i < QPL; ++i)
#pragma unroll
      for (int d = BP; d < 64; d <<= 1) {
        acc[i] += (u64)__shfl_xor((long long)acc[i], d, 64);
        if (TYPED) wq[i] += (uint32_t)__shfl_xor((int)wq[i], d, 64);
      }
    if (SPLIT) {                                                       // the waves of the workgroup: integer adds in LDS
      if (slot == 0) {
#pragma unroll
        for (int i = 0; i < QPL; ++i) {
          s_part[(wave * BP + ql) * QPL + i] = acc[i];
          if (TYPED) s_wq[(wave * BP + ql) * QPL + i] = wq[i];
        }
      }
      __syncthreads();
      if (wave == 0 && slot == 0) {
#pragma unroll
        for (int i = 0; i < QPL; ++i) {
          acc[i] = (s_part[ql * QPL + i] + s_part[(BP + ql) * QPL + i]) + (s_part[(2 * BP + ql) * QPL + i] + s_part[(3 * BP + ql) * QPL + i]);
          if (TYPED) wq[i] = (s_wq[ql * QPL + i] + s_wq[(BP + ql) * QPL + i]) + (s_wq[(2 * BP + ql) * QPL + i] + s_wq[(3 * BP + ql) * QPL + i]);
        }
      }
      __syncthreads();
    }
    if (slot == 0 && in_b && (!SPLIT || wave == 0)) {
      const u64 wk = TYPED ? 0 : p.k[v];
      const size_t at = (size_t)v * B + q;
#pragma unroll
      for (int i = 0; i < QPL; ++i) {
        const u64 wv = TYPED ? (u64)wq[i] : wk;
        if (dn[i]) {                                                   // frozen: p stays, c moves to the slot the next step reads
          p.c_new[at + i] = p.c_old[at + i];
          continue;
        }
        const u64 pv = p.p[at + i], tv = p.t[at + i];
        const u64 flow = wv ? acc[i] : pv;
        const u64 pn = ((u64)(65536u - p.a) * tv + (u64)p.a * flow) >> 16;
        const u64 d = pn > pv ? pn - pv : pv - pn;
        my_delta[i] = d > my_delta[i] ? d : my_delta[i];
        p.p[at + i] = pn;
        p.c_new[at + i] = wv ? pn / wv : 0;
      }
    }
  }
  if (slot == 0 && q_prev >= 0 && q_prev < B && (!SPLIT || wave == 0)) {
#pragma unroll
    for (int i = 0; i < QPL; ++i)
      if (my_delta[i]) atomicMax(&p.delta[q_prev + i], my_delta[i]);
  }
}

// after a step: a query whose delta is within the tolerance is frozen (and stays so); done_out, when given, receives the flags
__global__ __launch_bounds__(256) void ppr_mark_kernel(int B, const u64* __restrict__ delta, u64 tol, uint32_t* done, uint32_t* done_out) {
  const int q = threadIdx.x;
  if (q >= B) return;
  const uint32_t d = (done[q] || delta[q] <= tol) ? 1u : 0u;
  done[q] = d;
  if (done_out) done_out[q] = d;
}

// ---- the answer -----------------------------------------------------------------------------------------------------------------
// [n][B] -> [B][n] through a 64 x 64 tile in LDS (rows of 65 words: the column reads of a 32-lane half fall on distinct bank
// pairs).  KEYS: (p << 24) | (~v & 0xFFFFFF) where p > 0, else 0 — below every real key — and the positives counted per query;
// otherwise p / 2^40 as float64, exact because p <= 2^40 < 2^53.  A vertex that holds ALL the mass (p = 2^40: one seed and
// damping 0, or an isolated seed) is keyed as 2^40 - 1: every other vertex of the query then holds 0, the order stands, and the
// score of an answer is read from p, not from its key.  SHIFT: the score is x / 2^SHIFT (40 for the vertices; the chunks of
// the passage projection below are transposed, keyed and ranked by the same kernels over their state S, at 28)
template <bool KEYS, int SHIFT = PPR_ONE_SHIFT>
__global__ __launch_bounds__(256) void ppr_transpose_kernel(int64_t n, int B, const u64* __restrict__ p, u64* keys, double* scores,
                                                            uint32_t* positive) {
  __shared__ u64 s_tile[64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qtiles = (B + 63) / 64;
  const int64_t tiles = ((n + 63) / 64) * qtiles;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t v0 = (tile / qtiles) * 64;
    const int q0 = (int)(tile % qtiles) * 64;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int64_t v = v0 + wave * 16 + i;
      s_tile[wave * 16 + i][lane] = (v < n && q0 + lane < B) ? p[(size_t)v * B + q0 + lane] : 0;
    }
    __syncthreads();
    const int64_t v = v0 + lane;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int q = q0 + wave * 16 + i;                                // (wave-uniform)
      if (q >= B) break;
      const u64 x = s_tile[lane][wave * 16 + i];
      if (KEYS) {
        const bool pos = v < n && x > 0;
        if (v < n) keys[(size_t)q * n + v] = pos ? ((x >> PPR_ONE_SHIFT ? (1ull << PPR_ONE_SHIFT) - 1 : x) << 24) | (u64)(~(uint32_t)v & 0xFFFFFFu) : 0;
        const u64 mask = __builtin_amdgcn_ballot_w64(pos);
        if (lane == 0 && mask) atomicAdd(&positive[q], (uint32_t)__builtin_popcountll(mask));
      } else if (v < n) {
        scores[(size_t)q * n + v] = (double)x * (1.0 / (double)(1ull << SHIFT));
      }
    }
    __syncthreads();
  }
}

// one workgroup per query: the min(k, positives) best keys in exact order (canon_topk.h), (-1, -inf) behind them
template <int SHIFT>
__global__ __launch_bounds__(1024) void ppr_topk_kernel(const u64* __restrict__ keys_all, uint32_t n, int B, uint32_t k,
                                                        const uint32_t* __restrict__ positive, const u64* __restrict__ p,
                                                        int64_t* out_ids, double* out_scores, int32_t* out_count) {
  extern __shared__ __attribute__((aligned(16))) char ppr_smem[];
  uint64_t* s_top = (uint64_t*)ppr_smem;                   // [pow2 >= min(k, positives)]
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_pick[2];
  __shared__ uint32_t s_cnt[2];
  const uint32_t q = blockIdx.x;
  const uint64_t* keys = (const uint64_t*)keys_all + (size_t)q * n;
  const uint32_t have = positive[q] < n ? positive[q] : n;
  const uint32_t kk = k < have ? k : have;
  uint32_t pow2 = 1;
  while (pow2 < kk) pow2 <<= 1;
  wide_topk_keys(keys, n, kk, pow2, s_top, s_hist, s_pick, s_cnt, true);
  for (uint32_t i = threadIdx.x; i < k; i += blockDim.x) {
    const bool real = i < kk;
    const uint32_t v = real ? ~(uint32_t)s_top[i] & 0xFFFFFFu : 0u;
    out_ids[(size_t)q * k + i] = real ? (int64_t)v : -1;
    out_scores[(size_t)q * k + i] = real && v < n ? (double)p[(size_t)v * B + q] * (1.0 / (double)(1ull << SHIFT)) : -(double)INFINITY;
  }
  if (threadIdx.x == 0) out_count[q] = (int32_t)kk;
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" int rarc_ppr_limits(int* out6) {
  RARC_REQUIRE(out6, RARC_E_INVALID, "rarc_ppr_limits: null pointer");
  out6[0] = PPR_SPLIT_DEGREE;
  out6[1] = PPR_VERTEX_PARALLEL_MAX_B;
  out6[2] = PPR_MAX_B;
  out6[3] = PPR_MAX_SEEDS;
  out6[4] = PPR_MAX_K;
  out6[5] = 24;
  return RARC_OK;
}

extern "C" size_t rarc_ppr_workspace_bytes(int64_t n, int64_t m, int nq) {
  if (!ppr_shape_ok(n, m, nq)) return 0;
  return ppr_carve(nullptr, n, nq).bytes;
}

#define PPR_SHAPE_CHECKS(NAME)                                                                                                          \
  RARC_REQUIRE(lv_shape_ok(n, m), RARC_E_INVALID, NAME ": n=%lld m=%lld out of range (2 <= n < 2^31 - 1, 1 <= m < 2^30)", (long long)n, \
               (long long)m);                                                                                                           \
  RARC_REQUIRE(nq >= 1 && nq <= PPR_MAX_B, RARC_E_INVALID, NAME ": %d queries out of range (1 <= B <= %d per call)", nq, PPR_MAX_B);    \
  const PprWs ws = ppr_carve(d_ws, n, nq);                                                                                              \
  RARC_REQUIRE(ws_bytes >= ws.bytes, RARC_E_WORKSPACE, NAME ": workspace of %zu bytes, %zu needed", ws_bytes, ws.bytes)

extern "C" int rarc_ppr_seed(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, const int64_t* d_seeds,
                             const uint32_t* d_seed_weights, int nq, int n_slots, void* d_ws, size_t ws_bytes, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_graph && d_seeds && d_seed_weights && d_ws, RARC_E_INVALID, "rarc_ppr_seed: null pointer");
  PPR_SHAPE_CHECKS("rarc_ppr_seed");
  RARC_REQUIRE(n_slots >= 1 && n_slots <= PPR_MAX_SEEDS, RARC_E_INVALID, "rarc_ppr_seed: %d seed slots out of range (1 <= s <= %d)", n_slots,
               PPR_MAX_SEEDS);
  const LvGraph g = lv_graph_carve(d_graph, n, m);
  RARC_REQUIRE(graph_bytes >= g.bytes, RARC_E_WORKSPACE, "rarc_ppr_seed: graph workspace of %zu bytes, %zu needed", graph_bytes, g.bytes);
  hipStream_t s = (hipStream_t)stream;
  RARC_HIP_CHECK(hipMemsetAsync(ws.delta, 0, PPR_CTL_BYTES, s));
  RARC_HIP_CHECK(hipMemsetAsync(ws.t, 0, (size_t)n * nq * 8, s));
  hipLaunchKernelGGL(ppr_seed_kernel, dim3(1), dim3(256), 0, s, d_seeds, d_seed_weights, nq, n_slots, n, ws.t);
  hipLaunchKernelGGL(ppr_init_kernel<false>, dim3(lv_grid(n * nq, 256, 4096)), dim3(256), 0, s, n, nq, (const uint32_t*)g.k, (const u64*)ws.t, ws.p,
                     ws.c[0]);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

template <int BP, int QPL, bool TYPED>
static void ppr_launch_step(const PprStepArgs& p, const LvGraph& g, int64_t n, int64_t m, hipStream_t s) {
  const int chunks = (p.B + BP * QPL - 1) / (BP * QPL);
  // every grid is a multiple of the chunk count, so the stride of a wave's walk is one too: a wave keeps its chunk of queries
  auto grid = [chunks](int64_t items, int per_block, int cap) { return (lv_grid(items, per_block, cap) + chunks - 1) / chunks * chunks; };
  hipLaunchKernelGGL((ppr_step_kernel<BP, QPL, false, TYPED>), dim3(grid(n * chunks, 4, 8192)), dim3(256), 0, s, p, (const int32_t*)nullptr,
                     (const int64_t*)nullptr);
  const int64_t dmax = lv_max_degree(n, m);              // no vertex of this graph has more neighbours: skip the lists that must be empty
  if (dmax > LV_DEG_WAVE)
    hipLaunchKernelGGL((ppr_step_kernel<BP, QPL, true, TYPED>), dim3(grid(n * chunks, 1, 2048)), dim3(256), 0, s, p, (const int32_t*)g.list[2],
                       (const int64_t*)&g.hdr[LV_H_LIST + 2]);
  if (dmax > LV_DEG_LDS)
    hipLaunchKernelGGL((ppr_step_kernel<BP, QPL, true, TYPED>), dim3(grid((n / LV_DEG_LDS + 1) * chunks, 1, 2048)), dim3(256), 0, s, p,
                       (const int32_t*)g.list[3], (const int64_t*)&g.hdr[LV_H_LIST + 3]);
}

// the form: vertex-parallel up to PPR_VERTEX_PARALLEL_MAX_B queries (BP = the power of two >= B), query-parallel beyond,
// two queries per lane when B is even and more than one wave wide
template <bool TYPED>
static void ppr_pick_step(const PprStepArgs& p, const LvGraph& g, int64_t n, int64_t m, hipStream_t s) {
  const int nq = p.B;
  if (nq > PPR_VERTEX_PARALLEL_MAX_B) {
    if (nq > 64 && nq % 2 == 0) ppr_launch_step<64, 2, TYPED>(p, g, n, m, s);
    else ppr_launch_step<64, 1, TYPED>(p, g, n, m, s);
  } else if (nq > 16) ppr_launch_step<32, 1, TYPED>(p, g, n, m, s);
  else if (nq > 8) ppr_launch_step<16, 1, TYPED>(p, g, n, m, s);
  else if (nq > 4) ppr_launch_step<8, 1, TYPED>(p, g, n, m, s);
  else if (nq > 2) ppr_launch_step<4, 1, TYPED>(p, g, n, m, s);
  else if (nq > 1) ppr_launch_step<2, 1, TYPED>(p, g, n, m, s);
  else ppr_launch_step<1, 1, TYPED>(p, g, n, m, s);
}

extern "C" int rarc_ppr_step(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, int nq, int damping_q16, int64_t tolerance,
                             int cur, void* d_ws, size_t ws_bytes, uint32_t* d_done_out, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_graph && d_ws, RARC_E_INVALID, "rarc_ppr_step: null pointer");
  PPR_SHAPE_CHECKS("rarc_ppr_step");
  RARC_REQUIRE(damping_q16 >= 0 && damping_q16 < 65536, RARC_E_INVALID, "rarc_ppr_step: damping %d / 65536 out of range (0 <= damping < 1)",
               damping_q16);
  RARC_REQUIRE(tolerance >= 0 && tolerance <= (1ll << PPR_ONE_SHIFT), RARC_E_INVALID,
               "rarc_ppr_step: tolerance of %lld units out of range (0 <= tolerance <= 2^40)", (long long)tolerance);
  RARC_REQUIRE(cur == 0 || cur == 1, RARC_E_INVALID, "rarc_ppr_step: slot %d is neither 0 nor 1", cur);
  const LvGraph g = lv_graph_carve(d_graph, n, m);
  RARC_REQUIRE(graph_bytes >= g.bytes, RARC_E_WORKSPACE, "rarc_ppr_step: graph workspace of %zu bytes, %zu needed", graph_bytes, g.bytes);
  hipStream_t s = (hipStream_t)stream;
  PprStepArgs p;
  p.row_ptr = g.row_ptr;
  p.adj = g.adj;
  p.adj_w = g.adj_w;
  p.k = g.k;
  p.mask = nullptr;
  p.filters = nullptr;
  p.t = ws.t;
  p.p = ws.p;
  p.c_old = ws.c[cur];
  p.c_new = ws.c[cur ^ 1];
  p.delta = ws.delta;
  p.done = ws.done;
  p.n = n;
  p.B = nq;
  p.a = (uint32_t)damping_q16;
  RARC_HIP_CHECK(hipMemsetAsync(ws.delta, 0, (size_t)PPR_MAX_B * 8, s));
  ppr_pick_step<false>(p, g, n, m, s);
  hipLaunchKernelGGL(ppr_mark_kernel, dim3(1), dim3(256), 0, s, nq, (const u64*)ws.delta, (u64)tolerance, ws.done, d_done_out);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

// ---- typed PPR: the entries ------------------------------------------------------------------------------------------
#define PPR_ALIGNED(P, A) (((uintptr_t)(P) & (uintptr_t)((A)-1)) == 0)
// what the typed entries add to the untyped checks: the weighted typed adjacency and the filters
#define PPR_TYPED_CHECKS(NAME)                                                                                                          \
  RARC_REQUIRE(PPR_ALIGNED(d_types, 256), RARC_E_INVALID, NAME ": the typed adjacency is not 256-byte aligned");                   \
  RARC_REQUIRE(PPR_ALIGNED(d_filters, 4), RARC_E_INVALID, NAME ": the filters are not 4-byte aligned");                            \
  PPR_SHAPE_CHECKS(NAME);                                                                                                               \
  const LvGraph g = lv_graph_carve(d_graph, n, m);                                                                                      \
  RARC_REQUIRE(graph_bytes >= g.bytes, RARC_E_WORKSPACE, NAME ": graph workspace of %zu bytes, %zu needed", graph_bytes, g.bytes);      \
  const KhopTypes ty = khop_types_carve(d_types, n, m);                                                                                 \
  RARC_REQUIRE(types_bytes == ty.weighted_bytes, RARC_E_WORKSPACE,                                                                      \
               NAME ": typed adjacency of %zu bytes, not the %zu of rarc_graph_types_weighted (the unweighted one has no weight plane)", \
               types_bytes, ty.weighted_bytes)

extern "C" int rarc_ppr_seed_typed(const void* d_graph, size_t graph_bytes, const void* d_types, size_t types_bytes, const uint32_t* d_filters,
                                   int64_t n, int64_t m, const int64_t* d_seeds, const uint32_t* d_seed_weights, int nq, int n_slots, void* d_ws,
                                   size_t ws_bytes, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_graph && d_types && d_filters && d_seeds && d_seed_weights && d_ws, RARC_E_INVALID, "rarc_ppr_seed_typed: null pointer");
  PPR_TYPED_CHECKS("rarc_ppr_seed_typed");
  RARC_REQUIRE(n_slots >= 1 && n_slots <= PPR_MAX_SEEDS, RARC_E_INVALID, "rarc_ppr_seed_typed: %d seed slots out of range (1 <= s <= %d)",
               n_slots, PPR_MAX_SEEDS);
  hipStream_t s = (hipStream_t)stream;
  RARC_HIP_CHECK(hipMemsetAsync(ws.delta, 0, PPR_CTL_BYTES, s));
  RARC_HIP_CHECK(hipMemsetAsync(ws.t, 0, (size_t)n * nq * 8, s));
  hipLaunchKernelGGL(ppr_seed_kernel, dim3(1), dim3(256), 0, s, d_seeds, d_seed_weights, nq, n_slots, n, ws.t);
  hipLaunchKernelGGL(ppr_init_kernel<true>, dim3(lv_grid(n * nq, 256, 4096)), dim3(256), 0, s, n, nq, (const uint32_t*)nullptr, (const u64*)ws.t,
                     ws.p, ws.c[0]);
  hipLaunchKernelGGL(ppr_seed_typed_kernel, dim3((nq * n_slots + 3) / 4), dim3(256), 0, s, d_seeds, d_filters, nq, n_slots, n,
                     (const int64_t*)g.row_ptr, (const uint32_t*)ty.mask, (const uint32_t*)ty.w, (const u64*)ws.t, ws.c[0]);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_ppr_step_typed(const void* d_graph, size_t graph_bytes, const void* d_types, size_t types_bytes, const uint32_t* d_filters,
                                   int64_t n, int64_t m, int nq, int damping_q16, int64_t tolerance, int cur, void* d_ws, size_t ws_bytes,
                                   uint32_t* d_done_out, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_graph && d_types && d_filters && d_ws, RARC_E_INVALID, "rarc_ppr_step_typed: null pointer");
  PPR_TYPED_CHECKS("rarc_ppr_step_typed");
  RARC_REQUIRE(damping_q16 >= 0 && damping_q16 < 65536, RARC_E_INVALID,
               "rarc_ppr_step_typed: damping %d / 65536 out of range (0 <= damping < 1)", damping_q16);
  RARC_REQUIRE(tolerance >= 0 && tolerance <= (1ll << PPR_ONE_SHIFT), RARC_E_INVALID,
               "rarc_ppr_step_typed: tolerance of %lld units out of range (0 <= tolerance <= 2^40)", (long long)tolerance);
  RARC_REQUIRE(cur == 0 || cur == 1, RARC_E_INVALID, "rarc_ppr_step_typed: slot %d is neither 0 nor 1", cur);
  hipStream_t s = (hipStream_t)stream;
  PprStepArgs p;
  p.row_ptr = g.row_ptr;
  p.adj = ty.adj;
  p.adj_w = ty.w;
  p.k = nullptr;
  p.mask = ty.mask;
  p.filters = d_filters;
  p.t = ws.t;
  p.p = ws.p;
  p.c_old = ws.c[cur];
  p.c_new = ws.c[cur ^ 1];
  p.delta = ws.delta;
  p.done = ws.done;
  p.n = n;
  p.B = nq;
  p.a = (uint32_t)damping_q16;
  RARC_HIP_CHECK(hipMemsetAsync(ws.delta, 0, (size_t)PPR_MAX_B * 8, s));
  ppr_pick_step<true>(p, g, n, m, s);
  hipLaunchKernelGGL(ppr_mark_kernel, dim3(1), dim3(256), 0, s, nq, (const u64*)ws.delta, (u64)tolerance, ws.done, d_done_out);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_ppr_scores(int64_t n, int64_t m, int nq, const void* d_ws, size_t ws_bytes, double* d_out_scores, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_ws && d_out_scores, RARC_E_INVALID, "rarc_ppr_scores: null pointer");
  PPR_SHAPE_CHECKS("rarc_ppr_scores");
  hipStream_t s = (hipStream_t)stream;
  const int64_t tiles = ((n + 63) / 64) * ((nq + 63) / 64);
  hipLaunchKernelGGL(ppr_transpose_kernel<false>, dim3(lv_grid(tiles, 1, 8192)), dim3(256), 0, s, n, nq, (const u64*)ws.p, (u64*)nullptr,
                     d_out_scores, (uint32_t*)nullptr);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_ppr_topk(int64_t n, int64_t m, int nq, int top_k, int cur, void* d_ws, size_t ws_bytes, int64_t* d_out_ids,
                             double* d_out_scores, int32_t* d_out_count, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_ws && d_out_ids && d_out_scores && d_out_count, RARC_E_INVALID, "rarc_ppr_topk: null pointer");
  RARC_REQUIRE(n < PPR_TOPK_N_LIMIT, RARC_E_UNSUPPORTED,
               "rarc_ppr_topk: n=%lld vertices: the top-k key carries the vertex in 24 bits, n < 2^24 = 16777216 (rarc_ppr_scores has no such limit)",
               (long long)n);
  PPR_SHAPE_CHECKS("rarc_ppr_topk");
  RARC_REQUIRE(top_k >= 1 && top_k <= PPR_MAX_K, RARC_E_INVALID, "rarc_ppr_topk: top_k=%d out of range (1 <= k <= %d)", top_k, PPR_MAX_K);
  RARC_REQUIRE(cur == 0 || cur == 1, RARC_E_INVALID, "rarc_ppr_topk: slot %d is neither 0 nor 1", cur);
  hipStream_t s = (hipStream_t)stream;
  static RarcPerDevice attr_done;
  if (size_t& done = attr_done.cur(); !done) {
    RARC_HIP_CHECK(hipFuncSetAttribute((const void*)ppr_topk_kernel<PPR_ONE_SHIFT>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    done = 1;
  }
  u64* keys = ws.c[cur ^ 1];                               // the slot the next step overwrites anyway: [B][n] keys
  RARC_HIP_CHECK(hipMemsetAsync(ws.positive, 0, (size_t)PPR_MAX_B * 4, s));
  const int64_t tiles = ((n + 63) / 64) * ((nq + 63) / 64);
  hipLaunchKernelGGL(ppr_transpose_kernel<true>, dim3(lv_grid(tiles, 1, 8192)), dim3(256), 0, s, n, nq, (const u64*)ws.p, keys, (double*)nullptr,
                     ws.positive);
  const uint32_t kmax = (uint32_t)((int64_t)top_k < n ? (int64_t)top_k : n);
  uint32_t pow2 = 1;
  while (pow2 < kmax) pow2 <<= 1;
  hipLaunchKernelGGL(ppr_topk_kernel<PPR_ONE_SHIFT>, dim3(nq), dim3(1024), (size_t)pow2 * 8, s, (const u64*)keys, (uint32_t)n, nq, (uint32_t)top_k,
                     (const uint32_t*)ws.positive, (const u64*)ws.p, d_out_ids, d_out_scores, d_out_count);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

// ---- passages: the PPR mass of the entities pushed through the mention links onto the chunks ---------------------
// What a PPR-based graph retriever returns is chunks, not entities (the reference stores the link: (chunk)-[:MENTIONS]->(entity)).
// The rule continues the one above (tests/passage_ref.py restates it in Python integers): a mention map is a set of triples
// (c, e, w), 0 <= c < n_chunks, 0 <= e < n, w an integer in [1, 2^12), every (c, e) once, held as a CSR by chunk, and
//   S_q(c) = (sum over c's mentions (e, w) of w * p_q(e)) >> 12,   score = S / 2^28  ( = sum w p / ONE floored to 2^-28, exact)
// Nothing overflows: sum_e p_q(e) <= ONE = 2^40 and every (c, e) appears once, so sum w p <= (2^12 - 1) ONE < 2^52, and
// S < 2^40 strictly: the top-k key (S << 24) | (~c & 0xFFFFFF) needs no "all the mass" case.  Integer sums: the same bits for
// any order of the mentions, either form of the kernel and any batch; a frozen query is projected like any other.
//
// The kernel is the step's sibling, not an instantiation of it: the same two forms (chunk-parallel up to 32 queries, a lane a
// query beyond, two queries and one 16-byte load per lane for even B > 64), four loads in flight, a chunk of more than
// PPR_CHUNK_SPLIT_DEGREE mentions split across the four waves of a workgroup and joined in LDS — but none of the step's
// delta / done / teleport work, and guards the step does not need, because the CSR comes from the caller and no host entry can
// read it: a chunk's range is clamped to [0, nnz], an entry with e outside [0, n) or w outside [1, 2^12) contributes nothing
// (its row of p is not read), and a listed chunk outside [0, n_chunks) is skipped.  Whatever the arrays hold, no index leaves
// its buffer.  The chunks of more than PPR_CHUNK_SPLIT_DEGREE mentions are listed by the host while it builds the CSR; one that
// the list omits scores 0 (the first launch writes that, the second overwrites it for the listed ones).
//
// The chunk workspace is {positive counts u32 [256]} | S u64 [n_chunks][B] | keys u64 [B][n_chunks]: the PPR workspace is only
// read, so stepping — and rarc_ppr_topk — may go on afterwards.
constexpr int PPR_CHUNK_SPLIT_DEGREE = LV_DEG_WAVE;
constexpr int PPR_CHUNK_SCORE_SHIFT = PPR_ONE_SHIFT - PPR_CHUNK_WEIGHT_BITS;
// (the workspace is carved by chunk_ws.h, which csrc/khop.hip shares: it writes S from hop levels instead)

struct PprChunkArgs {
  const int64_t* row_ptr;
  const int32_t* ent;
  const uint32_t* w;
  const u64* p;
  u64* s;
  int64_t n;
  int64_t n_chunks;
  int64_t nnz;
  int B;
};

// one mention: the weight that counts (0 for an entry outside the rule) and the row of p it reads (row 0 when it counts for nothing)
__device__ __forceinline__ void ppr_chunk_entry(int32_t e, uint32_t w, int64_t n, size_t& row, u64& weight) {
  const bool ok = e >= 0 && (int64_t)e < n && w >= 1u && w < (1u << PPR_CHUNK_WEIGHT_BITS);
  row = ok ? (size_t)e : 0;
  weight = ok ? (u64)w : 0;
}

// BP, QPL, SPLIT as in ppr_step_kernel; list: the chunks of more than PPR_CHUNK_SPLIT_DEGREE mentions, list_count of them
template <int BP, int QPL, bool SPLIT>
__global__ __launch_bounds__(256) void ppr_chunks_kernel(const PprChunkArgs a, const int32_t* __restrict__ list, int64_t list_count) {
  constexpr int NSLOT = 64 / BP;
  constexpr int STEP = SPLIT ? 4 * NSLOT : NSLOT;
  __shared__ u64 s_part[SPLIT ? 4 * BP * QPL : 1];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = lane / BP, ql = lane % BP;
  const int B = a.B;
  const int chunks = (B + BP * QPL - 1) / (BP * QPL);
  const int64_t items = (SPLIT ? list_count : a.n_chunks) * chunks;
  const int64_t first = SPLIT ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave;
  const int64_t stride = SPLIT ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4;
  for (int64_t item = first; item < items; item += stride) {
    const int64_t ci = item / chunks;
    const int chunk = (int)(item - ci * chunks);
    const int64_t c = SPLIT ? (int64_t)list[ci] : ci;
    if (SPLIT && (c < 0 || c >= a.n_chunks)) continue;                 // (workgroup-uniform: every thread reads the same entry)
    int64_t r0 = a.row_ptr[c], r1 = a.row_ptr[c + 1];
    r0 = r0 < 0 ? 0 : (r0 > a.nnz ? a.nnz : r0);
    r1 = r1 < r0 ? r0 : (r1 > a.nnz ? a.nnz : r1);
    const int64_t deg = r1 - r0;
    const int q = chunk * BP * QPL + ql * QPL;                         // this lane's first query; q + QPL <= B or q >= B
    const bool in_b = q < B;
    u64 acc[QPL];
#pragma unroll
    for (int i = 0; i < QPL; ++i) acc[i] = 0;
    if (in_b && (SPLIT || deg <= PPR_CHUNK_SPLIT_DEGREE)) {            // (a lane past the batch reads no row of p)
      int64_t e = (SPLIT ? wave * NSLOT : 0) + slot;
      for (; e + 3 * STEP < deg; e += 4 * STEP) {                      // four mentions in flight
        size_t row[4];
        u64 w[4];
        u64 x[4][QPL];
#pragma unroll
        for (int j = 0; j < 4; ++j) ppr_chunk_entry(a.ent[r0 + e + j * STEP], a.w[r0 + e + j * STEP], a.n, row[j], w[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) ppr_load<QPL>(a.p + row[j] * B + q, x[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < QPL; ++i) acc[i] += w[j] * x[j][i];
      }
      for (; e < deg; e += STEP) {
        size_t row;
        u64 w;
        ppr_chunk_entry(a.ent[r0 + e], a.w[r0 + e], a.n, row, w);
        u64 x[QPL];
        ppr_load<QPL>(a.p + row * B + q, x);
#pragma unroll
        for (int i = 0; i < QPL; ++i) acc[i] += w * x[i];
      }
    }
    // the slots of a wave: integer shuffle-adds (every lane takes part, an idle one with zeros)
#pragma unroll
    for (int i = 0; i < QPL; ++i)
#pragma unroll
      for (int d = BP; d < 64; d <<= 1) acc[i] += (u64)__shfl_xor((long long)acc[i], d, 64);
    if (SPLIT) {                                                       // the waves of the workgroup: integer adds in LDS
      if (slot == 0) {
#pragma unroll
        for (int i = 0; i < QPL; ++i) s_part[(wave * BP + ql) * QPL + i] = acc[i];
      }
      __syncthreads();
      if (wave == 0 && slot == 0) {
#pragma unroll
        for (int i = 0; i < QPL; ++i)
          acc[i] = (s_part[ql * QPL + i] + s_part[(BP + ql) * QPL + i]) + (s_part[(2 * BP + ql) * QPL + i] + s_part[(3 * BP + ql) * QPL + i]);
      }
      __syncthreads();
    }
    if (slot == 0 && in_b && (!SPLIT || wave == 0)) {                  // (a chunk left to the SPLIT launch: 0 until that overwrites it)
#pragma unroll
      for (int i = 0; i < QPL; ++i) a.s[(size_t)c * B + q + i] = acc[i] >> PPR_CHUNK_WEIGHT_BITS;
    }
  }
}

template <int BP, int QPL>
static void ppr_launch_chunks(const PprChunkArgs& a, const int32_t* d_split, int64_t n_split, hipStream_t s) {
  const int chunks = (a.B + BP * QPL - 1) / (BP * QPL);
  hipLaunchKernelGGL((ppr_chunks_kernel<BP, QPL, false>), dim3(lv_grid(a.n_chunks * chunks, 4, 8192)), dim3(256), 0, s, a, (const int32_t*)nullptr,
                     (int64_t)0);
  if (n_split > 0)
    hipLaunchKernelGGL((ppr_chunks_kernel<BP, QPL, true>), dim3(lv_grid(n_split * chunks, 1, 2048)), dim3(256), 0, s, a, d_split, n_split);
}

extern "C" int rarc_ppr_chunks_limits(int* out4) {
  RARC_REQUIRE(out4, RARC_E_INVALID, "rarc_ppr_chunks_limits: null pointer");
  out4[0] = PPR_CHUNK_SPLIT_DEGREE;
  out4[1] = PPR_CHUNK_WEIGHT_BITS;
  out4[2] = PPR_CHUNK_SCORE_SHIFT;
  out4[3] = 24;
  return RARC_OK;
}

extern "C" size_t rarc_ppr_chunks_workspace_bytes(int64_t n_chunks, int nq) {
  if (!ppr_chunk_shape_ok(n_chunks, nq)) return 0;
  return ppr_chunk_carve(nullptr, n_chunks, nq).bytes;
}

#define PPR_CHUNK_SHAPE_CHECKS(NAME)                                                                                                     \
  RARC_REQUIRE(n_chunks >= 1 && n_chunks < PPR_CHUNK_N_LIMIT, RARC_E_INVALID, NAME ": n_chunks=%lld out of range (1 <= n_chunks < 2^31 - 1)", \
               (long long)n_chunks);                                                                                                     \
  RARC_REQUIRE(nq >= 1 && nq <= PPR_MAX_B, RARC_E_INVALID, NAME ": %d queries out of range (1 <= B <= %d per call)", nq, PPR_MAX_B);     \
  RARC_REQUIRE(PPR_ALIGNED(d_cws, 256), RARC_E_INVALID, NAME ": the chunk workspace is not 256-byte aligned");                           \
  const PprChunkWs cws = ppr_chunk_carve(d_cws, n_chunks, nq);                                                                           \
  RARC_REQUIRE(cws_bytes >= cws.bytes, RARC_E_WORKSPACE, NAME ": chunk workspace of %zu bytes, %zu needed", cws_bytes, cws.bytes)

extern "C" int rarc_ppr_chunks(int64_t n, int64_t m, int nq, int cur, const void* d_ws, size_t ws_bytes, const int64_t* d_row_ptr,
                               const int32_t* d_ent, const uint32_t* d_w, int64_t n_chunks, int64_t nnz, const int32_t* d_split,
                               int64_t n_split, void* d_cws, size_t cws_bytes, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_ws && d_row_ptr && d_ent && d_w && d_cws && (d_split || n_split == 0), RARC_E_INVALID, "rarc_ppr_chunks: null pointer");
  RARC_REQUIRE(PPR_ALIGNED(d_ws, 256), RARC_E_INVALID, "rarc_ppr_chunks: the PPR workspace is not 256-byte aligned");
  RARC_REQUIRE(PPR_ALIGNED(d_row_ptr, 8) && PPR_ALIGNED(d_ent, 4) && PPR_ALIGNED(d_w, 4) && PPR_ALIGNED(d_split, 4), RARC_E_INVALID,
               "rarc_ppr_chunks: a mention array is not aligned to its element (row_ptr 8 bytes, entities, weights and the split list 4)");
  PPR_SHAPE_CHECKS("rarc_ppr_chunks");
  PPR_CHUNK_SHAPE_CHECKS("rarc_ppr_chunks");
  RARC_REQUIRE(nnz >= 1, RARC_E_INVALID, "rarc_ppr_chunks: nnz=%lld mentions out of range (nnz >= 1)", (long long)nnz);
  RARC_REQUIRE(n_split >= 0 && n_split <= n_chunks, RARC_E_INVALID, "rarc_ppr_chunks: %lld split chunks out of range (0 <= n_split <= n_chunks)",
               (long long)n_split);
  RARC_REQUIRE(cur == 0 || cur == 1, RARC_E_INVALID, "rarc_ppr_chunks: slot %d is neither 0 nor 1", cur);
  hipStream_t s = (hipStream_t)stream;
  PprChunkArgs a;
  a.row_ptr = d_row_ptr;
  a.ent = d_ent;
  a.w = d_w;
  a.p = ws.p;                                              // p is written in place by every step: the same array for either `cur`
  a.s = cws.s;
  a.n = n;
  a.n_chunks = n_chunks;
  a.nnz = nnz;
  a.B = nq;
  if (nq > PPR_VERTEX_PARALLEL_MAX_B) {
    if (nq > 64 && nq % 2 == 0) ppr_launch_chunks<64, 2>(a, d_split, n_split, s);
    else ppr_launch_chunks<64, 1>(a, d_split, n_split, s);
  } else if (nq > 16) ppr_launch_chunks<32, 1>(a, d_split, n_split, s);
  else if (nq > 8) ppr_launch_chunks<16, 1>(a, d_split, n_split, s);
  else if (nq > 4) ppr_launch_chunks<8, 1>(a, d_split, n_split, s);
  else if (nq > 2) ppr_launch_chunks<4, 1>(a, d_split, n_split, s);
  else if (nq > 1) ppr_launch_chunks<2, 1>(a, d_split, n_split, s);
  else ppr_launch_chunks<1, 1>(a, d_split, n_split, s);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_ppr_chunks_scores(int64_t n_chunks, int nq, const void* d_cws, size_t cws_bytes, double* d_out_scores, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_cws && d_out_scores, RARC_E_INVALID, "rarc_ppr_chunks_scores: null pointer");
  RARC_REQUIRE(PPR_ALIGNED(d_out_scores, 8), RARC_E_INVALID, "rarc_ppr_chunks_scores: the scores are not 8-byte aligned");
  PPR_CHUNK_SHAPE_CHECKS("rarc_ppr_chunks_scores");
  hipStream_t s = (hipStream_t)stream;
  const int64_t tiles = ((n_chunks + 63) / 64) * ((nq + 63) / 64);
  hipLaunchKernelGGL((ppr_transpose_kernel<false, PPR_CHUNK_SCORE_SHIFT>), dim3(lv_grid(tiles, 1, 8192)), dim3(256), 0, s, n_chunks, nq,
                     (const u64*)cws.s, (u64*)nullptr, d_out_scores, (uint32_t*)nullptr);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_ppr_chunks_topk(int64_t n_chunks, int nq, int top_k, void* d_cws, size_t cws_bytes, int64_t* d_out_ids,
                                    double* d_out_scores, int32_t* d_out_count, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_cws && d_out_ids && d_out_scores && d_out_count, RARC_E_INVALID, "rarc_ppr_chunks_topk: null pointer");
  RARC_REQUIRE(PPR_ALIGNED(d_out_ids, 8) && PPR_ALIGNED(d_out_scores, 8) && PPR_ALIGNED(d_out_count, 4), RARC_E_INVALID,
               "rarc_ppr_chunks_topk: an output is not aligned to its element (ids and scores 8 bytes, counts 4)");
  RARC_REQUIRE(n_chunks < PPR_TOPK_N_LIMIT, RARC_E_UNSUPPORTED,
               "rarc_ppr_chunks_topk: n_chunks=%lld: the top-k key carries the chunk in 24 bits, n_chunks < 2^24 = 16777216 "
               "(rarc_ppr_chunks_scores has no such limit)",
               (long long)n_chunks);
  PPR_CHUNK_SHAPE_CHECKS("rarc_ppr_chunks_topk");
  RARC_REQUIRE(top_k >= 1 && top_k <= PPR_MAX_K, RARC_E_INVALID, "rarc_ppr_chunks_topk: top_k=%d out of range (1 <= k <= %d)", top_k, PPR_MAX_K);
  hipStream_t s = (hipStream_t)stream;
  static RarcPerDevice attr_done;
  if (size_t& done = attr_done.cur(); !done) {
    RARC_HIP_CHECK(hipFuncSetAttribute((const void*)ppr_topk_kernel<PPR_CHUNK_SCORE_SHIFT>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    done = 1;
  }
  RARC_HIP_CHECK(hipMemsetAsync(cws.positive, 0, (size_t)PPR_MAX_B * 4, s));
  const int64_t tiles = ((n_chunks + 63) / 64) * ((nq + 63) / 64);
  hipLaunchKernelGGL((ppr_transpose_kernel<true, PPR_CHUNK_SCORE_SHIFT>), dim3(lv_grid(tiles, 1, 8192)), dim3(256), 0, s, n_chunks, nq,
                     (const u64*)cws.s, cws.keys, (double*)nullptr, cws.positive);
  const uint32_t kmax = (uint32_t)((int64_t)top_k < n_chunks ? (int64_t)top_k : n_chunks);
  uint32_t pow2 = 1;
  while (pow2 < kmax) pow2 <<= 1;
  hipLaunchKernelGGL(ppr_topk_kernel<PPR_CHUNK_SCORE_SHIFT>, dim3(nq), dim3(1024), (size_t)pow2 * 8, s, (const u64*)cws.keys, (uint32_t)n_chunks, nq,
                     (uint32_t)top_k, (const uint32_t*)cws.positive, (const u64*)cws.s, d_out_ids, d_out_scores, d_out_count);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}
