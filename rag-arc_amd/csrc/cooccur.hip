// cooccur.hip — the co-occurrence projection of the mention CSR: two entities are joined when a chunk mentions
// both, weighted by how many chunks do —
//     MATCH (a:Entity)<-[:MENTIONS]-(c:Chunk)-[:MENTIONS]->(b:Entity) WHERE id(a) < id(b) RETURN a, b, count(c) AS weight
// — the edge list an EntityGraph is built from when nobody extracted relations.  The mention map is resident already
// (csrc/ppr.hip reads it, csrc/merge.hip contracts it); the pairs are expanded, sorted and summed next to it.
//
// The rule (tests/cooccur_ref.py restates it in Python).  The CSR is taken exactly as rarc_ppr_chunks and rarc_merge_mentions take
// it: a row's range clamped to [0, nnz], an entry with e outside [0, n) or w outside [1, 2^12) skipped and counted.  d_c = the
// valid entries of chunk c.  A chunk contributes iff 2 <= d_c <= max_mentions (a chunk of more is counted and gives nothing: one
// chunk of 4096 mentions is 8.4 M pairs).  A contributing chunk gives, for every two positions i < j of its valid entries, the key
// (min(e_i, e_j), max(e_i, e_j)) with the value 1 ("count") or w_i * w_j ("product", below 2^24); two equal entities (a malformed
// row) give the key (e, e), which the last step drops.  T = sum d_c (d_c - 1) / 2.  W(a, b) = the sum of the values of (a, b): an
// integer sum over a set, the same bits for any order of the mentions and from run to run.
//
// Three entries around rarc_sort_reduce (csrc/merge.hip), which the caller runs in between:
//   count  8 lanes a chunk count its valid entries; a scan of d (d - 1) / 2 gives every chunk its first slot, the same scan numbers
//          the chunks of each degree class into two lists
//   emit   a wave per chunk of at most CO_DEG_WAVE valid entries, a workgroup per chunk above it, the valid entries compacted into
//          LDS in row order first (32 KB at CO_MAX_MENTIONS).  The outer loop is over i, the lanes are over j > i: the pairs of i
//          are the run [base + i d - i (i + 1) / 2, + d - 1 - i), written with coalesced vector stores from the scanned offsets —
//          no atomic cursor, no square root
//   edges  the distinct keys and their sums -> (a, b) int64 pairs and uint32 weights, keeping a < b and W >= min_weight by
//          flag / scan / write: the ascending order of the keys is the order of the edges
// An entity id is never an index here: only row_ptr and the scanned offsets address memory, and every store is guarded by the end
// of its chunk's run and by T.
//
// The count workspace is {T, contributing, over max_mentions, skipped, chunks in list 0, in list 1} i64 | d u32 [n_chunks] |
// first slot i64 [n_chunks + 1] | list 0 i32 [n_chunks] | list 1 i32 [n_chunks] | tile sums u64 [2][tiles + 1]; the workspace of
// the edges step is {edges, largest W, below min_weight} | tile sums u64 [tiles + 1].
#include "chunk_ws.h"       // lv_align / lv_grid, the limits on n and n_chunks, the bits of a mention weight

typedef unsigned long long u64;

constexpr int CO_DEG_WAVE = LV_DEG_WAVE;                    // the most valid entries a single wave expands
constexpr int CO_MAX_MENTIONS = 4096;                       // the largest max_mentions: the row of a workgroup in LDS, 32 KB
constexpr int CO_PRODUCT_BITS = 2 * PPR_CHUNK_WEIGHT_BITS;  // w_a * w_b < 2^24
constexpr int CO_COUNT_LANES = 8;                           // lanes that count a chunk's valid entries
constexpr int CO_TILE = LV_SCAN_TILE;                       // items of a scan tile: 256 threads x 8
constexpr int64_t CO_T_LIMIT = 1ll << 31;                   // T < 2^31: rarc_sort_reduce's count limit
constexpr int64_t CO_NNZ_LIMIT = 1ll << 31;
constexpr size_t CO_CTL_BYTES = 256;
enum { CO_C_T = 0, CO_C_CONTRIB = 1, CO_C_OVER = 2, CO_C_SKIPPED = 3, CO_C_LIST = 4 };               // the count workspace's words
enum { CO_E_EDGES = 0, CO_E_MAX = 1, CO_E_BELOW = 2 };                                                // the edges workspace's words
enum { CO_MODE_COUNT = 0, CO_MODE_PRODUCT = 1 };

static inline int64_t co_tiles(int64_t n) { return (n + CO_TILE - 1) / CO_TILE; }
static inline int co_bits(int64_t n) {                      // ceil(log2 n), at least 1: the bits of an entity in a key
  int b = 1;
  while (b < 63 && (1ll << b) < n) ++b;
  return b;
}

struct CoWs {
  int64_t* ctl;
  uint32_t* deg;                                            // d_c of a contributing chunk, 0 of every other
  int64_t* offs;                                            // [n_chunks + 1]: the first slot of a chunk's pairs; the last is T
  int32_t* list[2];
  u64* bsum;                                                // [2][tiles + 1]: pairs | chunks of list 0 + (chunks of list 1 << 32)
  size_t bytes;
};
static CoWs co_carve(const void* base, int64_t n_chunks) {
  char* b = (char*)base;
  size_t o = 0;
  CoWs w;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  w.ctl = (int64_t*)take(CO_CTL_BYTES);
  w.deg = (uint32_t*)take((size_t)n_chunks * 4);
  w.offs = (int64_t*)take((size_t)(n_chunks + 1) * 8);
  for (int i = 0; i < 2; ++i) w.list[i] = (int32_t*)take((size_t)n_chunks * 4);
  w.bsum = (u64*)take((size_t)(co_tiles(n_chunks) + 1) * 16);
  w.bytes = o;
  return w;
}
struct CoEdgeWs {
  int64_t* ctl;
  u64* bsum;
  size_t bytes;
};
static CoEdgeWs co_edge_carve(const void* base, int64_t distinct) {
  char* b = (char*)base;
  size_t o = 0;
  CoEdgeWs w;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  w.ctl = (int64_t*)take(CO_CTL_BYTES);
  w.bsum = (u64*)take((size_t)(co_tiles(distinct) + 1) * 8);
  w.bytes = o;
  return w;
}

struct CoCsr {
  const int64_t* row_ptr;
  const int32_t* ent;
  const uint32_t* w;
  int64_t n_chunks;
  int64_t nnz;
  int64_t n;
};
// the clamped range of chunk c
__device__ __forceinline__ void co_row(const CoCsr& m, int64_t c, int64_t& r0, int64_t& r1) {
  r0 = m.row_ptr[c];
  r1 = m.row_ptr[c + 1];
  r0 = r0 < 0 ? 0 : (r0 > m.nnz ? m.nnz : r0);
  r1 = r1 < r0 ? r0 : (r1 > m.nnz ? m.nnz : r1);
}
__device__ __forceinline__ bool co_valid(const CoCsr& m, int32_t e, uint32_t w) {
  return (uint32_t)e < (u64)m.n && w >= 1u && w < (1u << PPR_CHUNK_WEIGHT_BITS);
}
__device__ __forceinline__ u64 co_pairs_of(uint32_t d) { return (u64)d * (u64)(d ? d - 1 : 0) / 2; }

// ---- count --------------------------------------------------------------------------------------------------------------------------
// CO_COUNT_LANES lanes a chunk, lane j entries j, j + 8, ..; d[c] = the valid entries if the chunk contributes, else 0.  The three
// totals stay in registers over the grid-stride loop and reach the control words once a workgroup: one atomic a wave on one word
// is what the kernel then waits for (1.5 ms at 1,000,000 chunks, measured)
__global__ __launch_bounds__(256) void co_count_kernel(const CoCsr m, int max_mentions, uint32_t* __restrict__ deg, int64_t* ctl) {
  __shared__ u64 s_tot[4][3];
  constexpr int GPB = 256 / CO_COUNT_LANES;
  const int sub = threadIdx.x % CO_COUNT_LANES, grp = threadIdx.x / CO_COUNT_LANES;
  u64 tot[3] = {0, 0, 0};                                              // this thread's chunks that contribute, are over, its entries skipped
  for (int64_t c0 = (int64_t)blockIdx.x * GPB; c0 < m.n_chunks; c0 += (int64_t)gridDim.x * GPB) {             // (workgroup-uniform)
    const int64_t c = c0 + grp;
    uint32_t good = 0;
    if (c < m.n_chunks) {
      int64_t r0, r1;
      co_row(m, c, r0, r1);
      for (int64_t i = r0 + sub; i < r1; i += CO_COUNT_LANES) {
        const bool ok = co_valid(m, m.ent[i], m.w[i]);
        good += ok ? 1u : 0u;
        tot[2] += ok ? 0u : 1u;
      }
    }
#pragma unroll
    for (int d = CO_COUNT_LANES / 2; d >= 1; d >>= 1) good += __shfl_xor(good, d, CO_COUNT_LANES);
    if (sub == 0 && c < m.n_chunks) {
      const bool over = good > (uint32_t)max_mentions, contrib = good >= 2u && !over;
      deg[c] = contrib ? good : 0u;
      tot[0] += contrib ? 1u : 0u;
      tot[1] += over ? 1u : 0u;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) tot[k] += __shfl_xor(tot[k], d, 64);
    if ((threadIdx.x & 63) == 0) s_tot[threadIdx.x >> 6][k] = tot[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const u64 t = (s_tot[0][threadIdx.x] + s_tot[1][threadIdx.x]) + (s_tot[2][threadIdx.x] + s_tot[3][threadIdx.x]);
    const int word = threadIdx.x == 0 ? CO_C_CONTRIB : (threadIdx.x == 1 ? CO_C_OVER : CO_C_SKIPPED);
    if (t) atomicAdd((u64*)&ctl[word], t);
  }
}

// inclusive scan of one value per thread over the block (s: 256 words of LDS)
__device__ __forceinline__ u64 co_block_scan(u64 x, u64* s) {
  s[threadIdx.x] = x;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const u64 o = threadIdx.x >= (unsigned)d ? s[threadIdx.x - d] : 0;
    __syncthreads();
    s[threadIdx.x] += o;
    __syncthreads();
  }
  const u64 r = s[threadIdx.x];
  __syncthreads();
  return r;
}
// what a chunk of d valid entries adds to the two scans: its pairs, and 1 in the half of its list
__device__ __forceinline__ u64 co_class_of(uint32_t d) { return d < 2u ? 0ull : (d <= (uint32_t)CO_DEG_WAVE ? 1ull : 1ull << 32); }

// the tile sums of both scans: bsum[tile] the pairs, bsum[nb + 1 + tile] the chunks of the two lists
__global__ __launch_bounds__(256) void co_scan_sums_kernel(const uint32_t* __restrict__ deg, int64_t n_chunks, u64* __restrict__ bsum) {
  __shared__ u64 s[256];
  const int64_t base = (int64_t)blockIdx.x * CO_TILE + (int64_t)threadIdx.x * 8;
  u64 pairs = 0, cls = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (base + j < n_chunks) {
      const uint32_t d = deg[base + j];
      pairs += co_pairs_of(d);
      cls += co_class_of(d);
    }
  const u64 ip = co_block_scan(pairs, s), ic = co_block_scan(cls, s);
  if (threadIdx.x == 255) {
    bsum[blockIdx.x] = ip;
    bsum[gridDim.x + 1 + blockIdx.x] = ic;
  }
}
// one workgroup: each of the two arrays of nb tile sums becomes exclusive offsets, its slot nb their total
__global__ __launch_bounds__(256) void co_scan_offsets_kernel(u64* bsum, int64_t nb, int arrays) {
  __shared__ u64 s[256];
  for (int a = 0; a < arrays; ++a) {
    u64* b = bsum + (int64_t)a * (nb + 1);
    u64 carry = 0;
    for (int64_t base = 0; base < nb; base += 256) {
      const int64_t i = base + threadIdx.x;
      const u64 x = i < nb ? b[i] : 0;
      const u64 incl = co_block_scan(x, s);
      if (i < nb) b[i] = carry + incl - x;
      if (threadIdx.x == 255) s[0] = incl;
      __syncthreads();
      carry += s[0];
      __syncthreads();
    }
    if (threadIdx.x == 0) b[nb] = carry;
  }
}
// the tiles again: offs[c] = the pairs before c; a contributing chunk enters its list at the rank the scan gives it, so the lists
// are ascending
__global__ __launch_bounds__(256) void co_scan_apply_kernel(const uint32_t* __restrict__ deg, int64_t n_chunks, const u64* __restrict__ bsum,
                                                            int64_t* __restrict__ offs, int32_t* __restrict__ list0, int32_t* __restrict__ list1,
                                                            int64_t* ctl) {
  __shared__ u64 s[256];
  const int64_t base = (int64_t)blockIdx.x * CO_TILE + (int64_t)threadIdx.x * 8;
  uint32_t d[8];
  u64 pairs = 0, cls = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    d[j] = base + j < n_chunks ? deg[base + j] : 0u;
    pairs += co_pairs_of(d[j]);
    cls += co_class_of(d[j]);
  }
  u64 run_p = bsum[blockIdx.x] + co_block_scan(pairs, s) - pairs;
  u64 run_c = bsum[gridDim.x + 1 + blockIdx.x] + co_block_scan(cls, s) - cls;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (base + j < n_chunks) {
      offs[base + j] = (int64_t)run_p;
      const int64_t at0 = (int64_t)(run_c & 0xffffffffull), at1 = (int64_t)(run_c >> 32);
      if (d[j] >= 2u && d[j] <= (uint32_t)CO_DEG_WAVE && at0 < n_chunks) list0[at0] = (int32_t)(base + j);
      if (d[j] > (uint32_t)CO_DEG_WAVE && at1 < n_chunks) list1[at1] = (int32_t)(base + j);
    }
    run_p += co_pairs_of(d[j]);
    run_c += co_class_of(d[j]);
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    const u64 total = bsum[gridDim.x], lists = bsum[2 * gridDim.x + 1];
    offs[n_chunks] = (int64_t)total;
    ctl[CO_C_T] = (int64_t)total;
    ctl[CO_C_LIST] = (int64_t)(lists & 0xffffffffull);
    ctl[CO_C_LIST + 1] = (int64_t)(lists >> 32);
  }
}

// ---- emit ---------------------------------------------------------------------------------------------------------------------------
struct CoEmitArgs {
  CoCsr m;
  const int64_t* ctl;
  const int64_t* offs;
  u64* keys;
  uint32_t* values;                                         // null in mode "count"
  int64_t total;                                            // T as the caller read it: no slot at or past it is written
  int bits;
};
// the pair of the valid entries (ea, wa) and (eb, wb) goes to slot `at`
template <bool PRODUCT>
__device__ __forceinline__ void co_store(const CoEmitArgs& a, int64_t at, int64_t end, int32_t ea, uint32_t wa, int32_t eb, uint32_t wb) {
  if (at >= end) return;
  const u64 lo = (u64)(uint32_t)(ea < eb ? ea : eb), hi = (u64)(uint32_t)(ea < eb ? eb : ea);
  a.keys[at] = lo << a.bits | hi;                                      // (lo == hi, a malformed row: dropped by rarc_cooccur_edges)
  if (PRODUCT) a.values[at] = ea == eb ? 0u : wa * wb;
}
// the slots of chunk c: [first, end), never past T nor past what the scan gave the chunk
__device__ __forceinline__ void co_slots(const CoEmitArgs& a, int64_t c, int64_t& first, int64_t& end) {
  first = a.offs[c];
  end = a.offs[c + 1];
  first = first < 0 ? 0 : first;
  end = end > a.total ? a.total : end;
}

// a wave per chunk of list 0 (2 .. CO_DEG_WAVE valid entries), four chunks a workgroup
template <bool PRODUCT>
__global__ __launch_bounds__(256) void co_emit_wave_kernel(const CoEmitArgs a, const int32_t* __restrict__ list) {
  __shared__ int32_t s_ent[4][CO_DEG_WAVE];
  __shared__ uint32_t s_w[4][CO_DEG_WAVE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
  int64_t n_list = a.ctl[CO_C_LIST];
  n_list = n_list < 0 ? 0 : (n_list > a.m.n_chunks ? a.m.n_chunks : n_list);
  for (int64_t l0 = (int64_t)blockIdx.x * 4; l0 < n_list; l0 += (int64_t)gridDim.x * 4) {                      // (workgroup-uniform)
    const int64_t li = l0 + wave;
    int64_t c = li < n_list ? (int64_t)list[li] : -1;
    c = c < a.m.n_chunks ? c : -1;
    int d = 0;
    if (c >= 0) {
      int64_t r0, r1;
      co_row(a.m, c, r0, r1);
      for (int64_t i0 = r0; i0 < r1; i0 += 64) {                       // (wave-uniform) the valid entries, in row order
        const int64_t i = i0 + lane;
        const int32_t e = i < r1 ? a.m.ent[i] : -1;
        const uint32_t w = i < r1 ? a.m.w[i] : 0u;
        const bool ok = i < r1 && co_valid(a.m, e, w);
        const u64 mask = __builtin_amdgcn_ballot_w64(ok);
        const int at = d + __builtin_popcountll(mask & below);
        if (ok && at < CO_DEG_WAVE) {
          s_ent[wave][at] = e;
          s_w[wave][at] = w;
        }
        d += __builtin_popcountll(mask);
      }
      d = d > CO_DEG_WAVE ? CO_DEG_WAVE : d;
    }
    __syncthreads();
    if (c >= 0) {
      int64_t first, end;
      co_slots(a, c, first, end);
      const int j0 = lane + 1;
      for (int i = 0; i + 1 < d; ++i) {                                // the pairs of i: one run of d - 1 - i slots
        const int j = i + j0;
        if (j < d)
          co_store<PRODUCT>(a, first + (int64_t)(i * d - i * (i + 1) / 2) + lane, end, s_ent[wave][i], s_w[wave][i], s_ent[wave][j], s_w[wave][j]);
      }
    }
    __syncthreads();
  }
}

// a workgroup per chunk of list 1 (CO_DEG_WAVE + 1 .. CO_MAX_MENTIONS valid entries): wave v takes i = v, v + 4, ..
template <bool PRODUCT>
__global__ __launch_bounds__(256) void co_emit_block_kernel(const CoEmitArgs a, const int32_t* __restrict__ list) {
  __shared__ int32_t s_ent[CO_MAX_MENTIONS];
  __shared__ uint32_t s_w[CO_MAX_MENTIONS];
  __shared__ int s_cnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
  int64_t n_list = a.ctl[CO_C_LIST + 1];
  n_list = n_list < 0 ? 0 : (n_list > a.m.n_chunks ? a.m.n_chunks : n_list);
  for (int64_t li = blockIdx.x; li < n_list; li += gridDim.x) {                                                  // (workgroup-uniform)
    const int64_t c = list[li];
    if (c < 0 || c >= a.m.n_chunks) continue;
    int64_t r0, r1;
    co_row(a.m, c, r0, r1);
    int d = 0;
    for (int64_t i0 = r0; i0 < r1; i0 += 256) {                        // (workgroup-uniform) the valid entries, in row order
      const int64_t i = i0 + threadIdx.x;
      const int32_t e = i < r1 ? a.m.ent[i] : -1;
      const uint32_t w = i < r1 ? a.m.w[i] : 0u;
      const bool ok = i < r1 && co_valid(a.m, e, w);
      const u64 mask = __builtin_amdgcn_ballot_w64(ok);
      if (lane == 0) s_cnt[wave] = __builtin_popcountll(mask);
      __syncthreads();
      int before = 0;
      for (int v = 0; v < wave; ++v) before += s_cnt[v];
      const int at = d + before + __builtin_popcountll(mask & below);
      if (ok && at < CO_MAX_MENTIONS) {
        s_ent[at] = e;
        s_w[at] = w;
      }
      d += (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
      __syncthreads();
    }
    d = d > CO_MAX_MENTIONS ? CO_MAX_MENTIONS : d;
    int64_t first, end;
    co_slots(a, c, first, end);
    for (int i = wave; i + 1 < d; i += 4) {
      const int64_t run = first + ((int64_t)i * d - (int64_t)i * (i + 1) / 2);
      const int32_t ei = s_ent[i];
      const uint32_t wi = s_w[i];
      for (int j = i + 1 + lane; j < d; j += 64) co_store<PRODUCT>(a, run + (j - i - 1), end, ei, wi, s_ent[j], s_w[j]);
    }
    __syncthreads();
  }
}

// ---- edges --------------------------------------------------------------------------------------------------------------------------
struct CoEdgeArgs {
  const u64* keys;
  const u64* sums;
  int64_t distinct;
  int bits;
  u64 min_weight;
};
__device__ __forceinline__ bool co_is_edge(const CoEdgeArgs& a, int64_t i) { return (a.keys[i] >> a.bits) < (a.keys[i] & ((1ull << a.bits) - 1ull)); }

__global__ __launch_bounds__(256) void co_edge_sums_kernel(const CoEdgeArgs a, u64* __restrict__ bsum) {
  __shared__ u64 s[256];
  const int64_t base = (int64_t)blockIdx.x * CO_TILE + (int64_t)threadIdx.x * 8;
  u64 acc = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (base + j < a.distinct) acc += co_is_edge(a, base + j) && a.sums[base + j] >= a.min_weight ? 1u : 0u;
  const u64 incl = co_block_scan(acc, s);
  if (threadIdx.x == 255) bsum[blockIdx.x] = incl;
}
__global__ __launch_bounds__(256) void co_edge_write_kernel(const CoEdgeArgs a, const u64* __restrict__ bsum, int64_t* __restrict__ out_pairs,
                                                            uint32_t* __restrict__ out_w, int64_t* ctl) {
  __shared__ u64 s[256];
  const int64_t base = (int64_t)blockIdx.x * CO_TILE + (int64_t)threadIdx.x * 8;
  bool keep[8];
  u64 acc = 0, largest = 0, n_below = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    keep[j] = false;
    if (base + j < a.distinct && co_is_edge(a, base + j)) {
      const u64 w = a.sums[base + j];
      keep[j] = w >= a.min_weight;
      largest = w > largest ? w : largest;
      n_below += keep[j] ? 0u : 1u;
    }
    acc += keep[j] ? 1u : 0u;
  }
  u64 run = bsum[blockIdx.x] + co_block_scan(acc, s) - acc;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (keep[j]) {
      if ((int64_t)run < a.distinct) {                                 // (always: run counts kept keys in front of this one)
        const u64 k = a.keys[base + j];
        out_pairs[2 * run] = (int64_t)(k >> a.bits);
        out_pairs[2 * run + 1] = (int64_t)(k & ((1ull << a.bits) - 1ull));
        out_w[run] = (uint32_t)a.sums[base + j];                       // (the caller narrows: the largest sum is reported)
      }
      ++run;
    }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 o = __shfl_xor(largest, d, 64);
    largest = o > largest ? o : largest;
    n_below += __shfl_xor(n_below, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (largest) atomicMax((u64*)&ctl[CO_E_MAX], largest);
    if (n_below) atomicAdd((u64*)&ctl[CO_E_BELOW], n_below);
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) ctl[CO_E_EDGES] = (int64_t)bsum[gridDim.x];
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define CO_ALIGNED(P, A) (((uintptr_t)(P) & (uintptr_t)((A)-1)) == 0)
static inline bool co_shape_ok(int64_t n_chunks, int64_t nnz) { return n_chunks >= 1 && n_chunks < PPR_CHUNK_N_LIMIT && nnz >= 1 && nnz < CO_NNZ_LIMIT; }
static inline bool co_n_ok(int64_t n) { return n >= 2 && n < LV_N_LIMIT; }

// the checks count and emit share; leaves `ws` and `m` behind
#define CO_CSR_CHECKS(NAME)                                                                                                                \
  RARC_REQUIRE(CO_ALIGNED(d_row_ptr, 8) && CO_ALIGNED(d_ent, 4) && CO_ALIGNED(d_w, 4), RARC_E_INVALID,                                      \
               NAME ": an array of the CSR is not aligned to its element (row_ptr 8 bytes, entities and weights 4)");                      \
  RARC_REQUIRE(n_chunks >= 1 && n_chunks < PPR_CHUNK_N_LIMIT, RARC_E_INVALID, NAME ": n_chunks=%lld out of range (1 <= n_chunks < 2^31 - 1)", \
               (long long)n_chunks);                                                                                                       \
  RARC_REQUIRE(nnz >= 1 && nnz < CO_NNZ_LIMIT, RARC_E_INVALID, NAME ": nnz=%lld mentions out of range (1 <= nnz < 2^31)", (long long)nnz);   \
  RARC_REQUIRE(co_n_ok(n), RARC_E_INVALID, NAME ": n=%lld out of range (2 <= n < 2^31 - 1)", (long long)n);                                 \
  RARC_REQUIRE(CO_ALIGNED(d_ws, 256), RARC_E_INVALID, NAME ": the workspace is not 256-byte aligned");                                      \
  const CoWs ws = co_carve(d_ws, n_chunks);                                                                                                \
  RARC_REQUIRE(ws_bytes >= ws.bytes, RARC_E_WORKSPACE, NAME ": workspace of %zu bytes, %zu needed", ws_bytes, ws.bytes);                    \
  const CoCsr m = {d_row_ptr, d_ent, d_w, n_chunks, nnz, n}

extern "C" int rarc_cooccur_limits(int* out4) {
  RARC_REQUIRE(out4, RARC_E_INVALID, "rarc_cooccur_limits: null pointer");
  out4[0] = CO_DEG_WAVE;
  out4[1] = CO_MAX_MENTIONS;
  out4[2] = CO_PRODUCT_BITS;
  out4[3] = 31;                                                        // T < 2^31
  return RARC_OK;
}

extern "C" size_t rarc_cooccur_workspace_bytes(int64_t n_chunks, int64_t nnz) {
  if (!co_shape_ok(n_chunks, nnz)) return 0;
  return co_carve(nullptr, n_chunks).bytes;
}

extern "C" int rarc_cooccur_count(const int64_t* d_row_ptr, const int32_t* d_ent, const uint32_t* d_w, int64_t n_chunks, int64_t nnz, int64_t n,
                                  int max_mentions, void* d_ws, size_t ws_bytes, int64_t* d_out4, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_row_ptr && d_ent && d_w && d_ws && d_out4, RARC_E_INVALID, "rarc_cooccur_count: null pointer");
  RARC_REQUIRE(CO_ALIGNED(d_out4, 8), RARC_E_INVALID, "rarc_cooccur_count: the counts are not 8-byte aligned");
  RARC_REQUIRE(max_mentions >= 2 && max_mentions <= CO_MAX_MENTIONS, RARC_E_INVALID, "rarc_cooccur_count: max_mentions=%d out of range (2 <= max_mentions <= %d)",
               max_mentions, CO_MAX_MENTIONS);
  CO_CSR_CHECKS("rarc_cooccur_count");
  hipStream_t s = (hipStream_t)stream;
  const unsigned tiles = (unsigned)co_tiles(n_chunks);
  RARC_HIP_CHECK(hipMemsetAsync(ws.ctl, 0, CO_CTL_BYTES, s));
  hipLaunchKernelGGL(co_count_kernel, dim3(lv_grid(n_chunks, 256 / CO_COUNT_LANES, 4096)), dim3(256), 0, s, m, max_mentions, ws.deg, ws.ctl);
  hipLaunchKernelGGL(co_scan_sums_kernel, dim3(tiles), dim3(256), 0, s, (const uint32_t*)ws.deg, n_chunks, ws.bsum);
  hipLaunchKernelGGL(co_scan_offsets_kernel, dim3(1), dim3(256), 0, s, ws.bsum, (int64_t)tiles, 2);
  hipLaunchKernelGGL(co_scan_apply_kernel, dim3(tiles), dim3(256), 0, s, (const uint32_t*)ws.deg, n_chunks, (const u64*)ws.bsum, ws.offs, ws.list[0],
                     ws.list[1], ws.ctl);
  RARC_HIP_CHECK(hipGetLastError());
  RARC_HIP_CHECK(hipMemcpyAsync(d_out4, ws.ctl, 32, hipMemcpyDeviceToDevice, s));
  return RARC_OK;
}

extern "C" int rarc_cooccur_emit(const int64_t* d_row_ptr, const int32_t* d_ent, const uint32_t* d_w, int64_t n_chunks, int64_t nnz, int64_t n,
                                 int mode, const void* d_ws, size_t ws_bytes, uint64_t* d_keys, uint32_t* d_values, int64_t total, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_row_ptr && d_ent && d_w && d_ws && d_keys, RARC_E_INVALID, "rarc_cooccur_emit: null pointer");
  RARC_REQUIRE(mode == CO_MODE_COUNT || mode == CO_MODE_PRODUCT, RARC_E_INVALID, "rarc_cooccur_emit: mode=%d is neither 0 (count) nor 1 (product)", mode);
  RARC_REQUIRE(mode == CO_MODE_COUNT || d_values, RARC_E_INVALID, "rarc_cooccur_emit: null pointer (mode 1 writes the values)");
  RARC_REQUIRE(CO_ALIGNED(d_keys, 8) && CO_ALIGNED(d_values, 4), RARC_E_INVALID,
               "rarc_cooccur_emit: an output is not aligned to its element (keys 8 bytes, values 4)");
  RARC_REQUIRE(total >= 1 && total < CO_T_LIMIT, RARC_E_INVALID, "rarc_cooccur_emit: T=%lld pairs out of range (1 <= T < 2^31)", (long long)total);
  CO_CSR_CHECKS("rarc_cooccur_emit");
  hipStream_t s = (hipStream_t)stream;
  CoEmitArgs a;
  a.m = m;
  a.ctl = ws.ctl;
  a.offs = ws.offs;
  a.keys = (u64*)d_keys;
  a.values = mode == CO_MODE_PRODUCT ? d_values : nullptr;
  a.total = total;
  a.bits = co_bits(n);                                                 // key = a << bits | b: 2 bits <= 62
  // a list of a degree class holds at most nnz / (its smallest degree) chunks
  auto at_most = [&](int64_t least_degree) { const int64_t c = nnz / least_degree; return c < n_chunks ? c : n_chunks; };
  const unsigned wave_grid = lv_grid(at_most(2), 4, 16384), block_grid = lv_grid(at_most(CO_DEG_WAVE + 1), 1, 2048);
  if (mode == CO_MODE_PRODUCT) {
    if (nnz >= 2) hipLaunchKernelGGL(co_emit_wave_kernel<true>, dim3(wave_grid), dim3(256), 0, s, a, (const int32_t*)ws.list[0]);
    if (nnz > CO_DEG_WAVE) hipLaunchKernelGGL(co_emit_block_kernel<true>, dim3(block_grid), dim3(256), 0, s, a, (const int32_t*)ws.list[1]);
  } else {
    if (nnz >= 2) hipLaunchKernelGGL(co_emit_wave_kernel<false>, dim3(wave_grid), dim3(256), 0, s, a, (const int32_t*)ws.list[0]);
    if (nnz > CO_DEG_WAVE) hipLaunchKernelGGL(co_emit_block_kernel<false>, dim3(block_grid), dim3(256), 0, s, a, (const int32_t*)ws.list[1]);
  }
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" size_t rarc_cooccur_edges_workspace_bytes(int64_t distinct) {
  if (distinct < 1 || distinct >= CO_T_LIMIT) return 0;
  return co_edge_carve(nullptr, distinct).bytes;
}

extern "C" int rarc_cooccur_edges(const uint64_t* d_keys, const uint64_t* d_sums, int64_t distinct, int64_t n, int64_t min_weight, void* d_ws,
                                  size_t ws_bytes, int64_t* d_out_pairs, uint32_t* d_out_weights, int64_t* d_out3, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_keys && d_sums && d_ws && d_out_pairs && d_out_weights && d_out3, RARC_E_INVALID, "rarc_cooccur_edges: null pointer");
  RARC_REQUIRE(CO_ALIGNED(d_keys, 8) && CO_ALIGNED(d_sums, 8) && CO_ALIGNED(d_out_pairs, 8) && CO_ALIGNED(d_out_weights, 4) && CO_ALIGNED(d_out3, 8),
               RARC_E_INVALID, "rarc_cooccur_edges: an array is not aligned to its element (weights 4 bytes, every other 8)");
  RARC_REQUIRE(distinct >= 1 && distinct < CO_T_LIMIT, RARC_E_INVALID, "rarc_cooccur_edges: distinct=%lld keys out of range (1 <= distinct < 2^31)",
               (long long)distinct);
  RARC_REQUIRE(co_n_ok(n), RARC_E_INVALID, "rarc_cooccur_edges: n=%lld out of range (2 <= n < 2^31 - 1)", (long long)n);
  RARC_REQUIRE(min_weight >= 1, RARC_E_INVALID, "rarc_cooccur_edges: min_weight=%lld out of range (min_weight >= 1)", (long long)min_weight);
  RARC_REQUIRE(CO_ALIGNED(d_ws, 256), RARC_E_INVALID, "rarc_cooccur_edges: the workspace is not 256-byte aligned");
  const CoEdgeWs ws = co_edge_carve(d_ws, distinct);
  RARC_REQUIRE(ws_bytes >= ws.bytes, RARC_E_WORKSPACE, "rarc_cooccur_edges: workspace of %zu bytes, %zu needed", ws_bytes, ws.bytes);
  hipStream_t s = (hipStream_t)stream;
  const unsigned tiles = (unsigned)co_tiles(distinct);
  const CoEdgeArgs a = {(const u64*)d_keys, (const u64*)d_sums, distinct, co_bits(n), (u64)min_weight};
  RARC_HIP_CHECK(hipMemsetAsync(ws.ctl, 0, CO_CTL_BYTES, s));
  hipLaunchKernelGGL(co_edge_sums_kernel, dim3(tiles), dim3(256), 0, s, a, ws.bsum);
  hipLaunchKernelGGL(co_scan_offsets_kernel, dim3(1), dim3(256), 0, s, ws.bsum, (int64_t)tiles, 1);
  hipLaunchKernelGGL(co_edge_write_kernel, dim3(tiles), dim3(256), 0, s, a, (const u64*)ws.bsum, d_out_pairs, d_out_weights, ws.ctl);
  RARC_HIP_CHECK(hipGetLastError());
  RARC_HIP_CHECK(hipMemcpyAsync(d_out3, ws.ctl, 24, hipMemcpyDeviceToDevice, s));
  return RARC_OK;
}
