// khop.hip — k-hop neighbourhoods over the GRAPH blob rarc_graph_csr wrote, for a batch of queries at once: the
// traversal a graph store is asked for with MATCH (s)-[*..h]-(v), as one bit-parallel multi-source breadth-first search.
//
// The rule (tests/khop_ref.py restates it in Python): edge weights are ignored; hop_q(v) is the fewest edges from any seed of
// query q to v, a seed has hop 0, and v is in q's neighbourhood iff hop_q(v) <= hops (0 <= hops <= 8).
//
// The state is one bit per (vertex, query): W = ceil(nq / 64) 64-bit words per vertex, in `seen` (every level so far) and in
// one array per level 0 .. hops.  With at most 64 queries a vertex's state is ONE word, and one word is what moves.
//   seed   clears everything and sets bit q of level 0 and of seen at each of q's seeds (atomicOr: a repeated seed is idempotent)
//   step   level[hop](v) = (OR over v's neighbours u of level[hop - 1](u)) & ~seen(v);   seen(v) |= level[hop](v)
// The step is the pull form: only v's own lanes write v's words, the words they read (level[hop - 1]) are written by nobody in
// that launch, and OR is idempotent and associative: the answer is the same bits for any order of the edges, any launch shape
// and any batch.  Each hop is stepped once, in order 1, 2, .. after a seed; the `grew` word tells whether any query reached a new
// vertex, and once it is 0 every later level is empty — it already is, because the seed cleared it.
//
// A lane whose word of seen(v) already holds every query of the batch reads no neighbour: late hops on a saturated graph cost
// the read of seen and the write of an empty word.  KHOP_GROUP = 16 lanes share a vertex of up to KHOP_SPLIT_DEGREE = 64
// neighbours, as 16 / WP neighbour slots x WP words (WP = the power of two >= W), joined by shuffle-ORs; a vertex of more
// neighbours (the degree lists 2 and 3 of the blob) is split across the 256 threads of a workgroup, joined in LDS.
//
// The answers read the levels:
//   counts  [q][h] = vertices at hop h exactly, never capped
//   levels  uint8 [q][v] = hop_q(v), 255 for "not within hops"
//   list    per query the neighbourhood by (hop ascending, vertex ascending), cut at max_vertices.  count / scan / write: a tile of
//           KHOP_TILE vertices counts its bits per (level, query), a scan over the tiles turns the counts into offsets, and the
//           tiles write at offset + rank inside the tile (ballot + popcount) — the position of an entry is a function of the
//           levels alone
//   chunks  S_q(c) = sum over c's mentions (e, w) with hop_q(e) <= hops of w * decay[hop_q(e)], an integer sum, written where
//           rarc_ppr_chunks writes its S (chunk_ws.h): rarc_ppr_chunks_scores and rarc_ppr_chunks_topk read it unchanged, as
//           S / 2^28.  w < 2^12 summed per chunk and decay <= 2^16 give S < 2^28.  The kernel guards itself as rarc_ppr_chunks
//           does: a chunk's range is clamped to [0, nnz], an entry with e outside [0, n) or w outside [1, 2^12) contributes
//           nothing, a listed chunk outside [0, n_chunks) is skipped, a chunk of more than 64 mentions that the list omits
//           scores 0.  A lane is a query; the entries of a chunk are loaded once, one per lane, and handed round by readlane.
//   edges   the relations inside the neighbourhood (tests/subgraph_ref.py restates it): the caller's table of
//           r rows (a, b), any orientation, repeats and a == b allowed; row e has level max(hop_q(a), hop_q(b)) and is in q's
//           subgraph iff that is <= hops.  With S_h(x) the OR of levels 0 .. h of x, the rows at level h exactly are
//           E_h = S_h(a) & S_h(b) & ~(S_{h-1}(a) & S_{h-1}(b)); a row with an end outside [0, n) is in no subgraph.  The same
//           count / scan / write over tiles of KHOP_TILE rows, the counts in a workspace of their own; the CSR is not read
//
// Connecting paths (tests/paths_ref.py restates it): allShortestPaths between the sources of one traversal.  For a
// pair p = (A, B) of its columns, d_p = min over v of hop_A(v) + hop_B(v) and v is on p's paths at position i iff hop_A(v) == i
// and hop_B(v) == d_p - i.  The answer is written as a k-hop state of its own, a column a pair and a level a position, so every
// reader above (counts, levels, list, chunks) takes it unchanged.
//   dist        an integer atomicMin per pair of hop_A over the vertices that hold B's bit at level 0; 0xFFFFFFFF = -1 stays
//               where nothing within the bound joins the two, or a pair names no column
//   mark        a wave per vertex, a lane a pair: the vertex's (hops + 1) x W level words are loaded once, one per lane, and
//               handed round by shuffles; the words of the path state are assembled with ballots.  The two columns of a pair
//               sit at any bit of any word, so this is a test per pair, not an AND of words
//   path edges  row (a, b) is at level i + 1 iff one end is at position i and the other at i + 1 — on the path state the two
//               ends share a word, E_{i+1} = P_i(a) & P_{i+1}(b) | P_{i+1}(a) & P_i(b) — through the count / scan / write of `edges`
//
// Typed traversal (tests/typed_ref.py restates it): MATCH (s)-[:CAUSAL|SEQUENTIAL*..h]-(v).  An edge carries a
// uint32 mask M of its relation types, a query a uint32 filter F_q, and q may cross the edge iff M & F_q != 0; a seed has hop 0
// whatever its filter.  With Q_t the queries whose filter holds t and A(M) = OR over t in M of Q_t,
//   step   level[hop](v) = (OR over v's slots (u, M) of level[hop - 1](u) & A(M)) & ~seen(v);   seen(v) |= level[hop](v)
// in the same launch shapes, over a second pair of slot arrays (rarc_graph_types) that holds neighbour and mask side by side.
// Q_t is 32 x W words, built in LDS from the filters once a workgroup.  The state is the untyped one, so every reader above
// takes it unchanged; a row (a, b, t) of a typed relation table additionally needs F_q to hold t, which ANDs its level words
// with Q_t.  Untyped entries launch the kernels they launched before: the typed ones are instantiations of their own.
//
// The workspace is {grew u32 | level totals i32 [256][9]} | seen | level 0 .. hops | tile counts u32 [tiles][hops + 1][W * 64].
#include <type_traits>

#include "graph_csr.h"
#include "chunk_ws.h"

constexpr int KHOP_MAX_HOPS = 8;
constexpr int KHOP_MAX_B = PPR_MAX_B;
constexpr int KHOP_MAX_SEEDS = 64;
constexpr int KHOP_MAX_VERTICES = 65536;
constexpr int KHOP_MAX_EDGES = 65536;
constexpr int KHOP_SPLIT_DEGREE = LV_DEG_WAVE;              // a vertex of more neighbours is split across a workgroup
constexpr int KHOP_GROUP = 16;                              // lanes that share a vertex of up to KHOP_SPLIT_DEGREE neighbours
constexpr int KHOP_TILE = 1024;                             // vertices, or relation rows, a wave counts and writes for a list
constexpr int KHOP_TYPES = 32;                              // relation types: the bits of an edge mask and of a query filter
constexpr uint32_t KHOP_MAX_DECAY = 1u << 16;
constexpr size_t KHOP_CTL_BYTES = 256 + (size_t)KHOP_MAX_B * (KHOP_MAX_HOPS + 1) * 4;

typedef unsigned long long u64;

struct KhopWs {
  uint32_t* grew;
  int32_t* totals;                                          // [nq][hops + 1]
  u64* seen;
  u64* level;                                               // [hops + 1][n][W]
  uint32_t* tiles;                                          // [tiles][hops + 1][W * 64]
  size_t level_words;                                       // n * W
  size_t clear_bytes;                                       // seen and every level, from `seen`
  size_t bytes;
};
static inline int khop_words(int nq) { return (nq + 63) / 64; }
__host__ __device__ static inline int64_t khop_tiles(int64_t n) { return (n + KHOP_TILE - 1) / KHOP_TILE; }
static inline bool khop_shape_ok(int64_t n, int64_t m, int nq, int hops) {
  return lv_shape_ok(n, m) && nq >= 1 && nq <= KHOP_MAX_B && hops >= 0 && hops <= KHOP_MAX_HOPS;
}
static KhopWs khop_carve(const void* base, int64_t n, int nq, int hops) {
  char* b = (char*)base;
  size_t o = 0;
  KhopWs w;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  char* ctl = take(KHOP_CTL_BYTES);
  w.grew = (uint32_t*)ctl;
  w.totals = (int32_t*)(ctl + 256);
  const int W = khop_words(nq);
  w.level_words = (size_t)n * W;
  const size_t state = lv_align(w.level_words * 8);         // (every array a multiple of 256 bytes: they are cleared as one)
  w.seen = (u64*)take(state);
  w.level = (u64*)take(state * (size_t)(hops + 1));
  w.clear_bytes = state * (size_t)(hops + 2);
  w.tiles = (uint32_t*)take((size_t)khop_tiles(n) * (size_t)(hops + 1) * W * 64 * 4);
  w.bytes = o;
  return w;
}
static inline u64* khop_level(const KhopWs& w, int h) { return w.level + (lv_align(w.level_words * 8) / 8) * (size_t)h; }

// the edge workspace: level totals i32 [256][9] | tile counts u32 [tiles of r rows][hops + 1][W * 64]
struct KhopEdgeWs {
  int32_t* totals;
  uint32_t* tiles;
  size_t bytes;
};
static inline bool khop_rows_ok(int64_t r) { return r >= 1 && r < LV_N_LIMIT; }
static KhopEdgeWs khop_edge_carve(const void* base, int64_t r, int nq, int hops) {
  char* b = (char*)base;
  KhopEdgeWs w;
  w.totals = (int32_t*)b;
  const size_t o = lv_align((size_t)KHOP_MAX_B * (KHOP_MAX_HOPS + 1) * 4);
  w.tiles = (uint32_t*)(b + o);
  w.bytes = o + lv_align((size_t)khop_tiles(r) * (size_t)(hops + 1) * khop_words(nq) * 64 * 4);
  return w;
}

// the queries of the batch that word `word` holds, as a mask
__device__ __forceinline__ u64 khop_query_mask(int nq, int word) {
  const int left = nq - word * 64;
  return left <= 0 ? 0ull : (left >= 64 ? ~0ull : (1ull << left) - 1ull);
}

// ---- the typed adjacency ------------------------------------------------------------------------------------------
// t_adj int32 [2m] | t_mask uint32 [2m] | cursor uint32 [n] | bad u32: a second pair of slot arrays over the blob's row_ptr.
// rarc_graph_csr hands out a row's slots through an atomic cursor, so no array can be aligned to its `adj` afterwards; here the
// neighbour and the mask of a slot are written together, in one pass over the pair list that built the graph
#include "graph_types.h"
// the rule of lv_edge_ok (csrc/louvain.hip): a pair rarc_graph_csr skipped has no slots and is skipped here too
__device__ __forceinline__ bool khop_pair_ok(int64_t a, int64_t b, int64_t n) { return a >= 0 && a < b && b < n; }

// a thread per pair: one slot in each end's row, taken through the cursor.  A slot at or beyond the end of the row (or of the
// arrays) is not written and counted in `bad`: the pair list is not the one the blob was built from.  WEIGHTED: the pair's
// weight goes into the same slot of a third plane, `w`; a null `weights` is weight 1 for every pair
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void khop_types_fill_kernel(const int64_t* __restrict__ pairs, const uint32_t* __restrict__ masks,
                                                              const uint32_t* __restrict__ weights, int64_t m, int64_t n,
                                                              const int64_t* __restrict__ row_ptr, uint32_t* cursor, int32_t* adj, uint32_t* mask,
                                                              uint32_t* w, uint32_t* bad) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256) {
    const int64_t a = pairs[2 * e], b = pairs[2 * e + 1];
    if (!khop_pair_ok(a, b, n)) continue;
    const uint32_t mk = masks[e];
    const uint32_t we = WEIGHTED && weights ? weights[e] : 1u;
    const int64_t pa = row_ptr[a] + atomicAdd(&cursor[a], 1u), pb = row_ptr[b] + atomicAdd(&cursor[b], 1u);
    const bool fa = pa >= 0 && pa < row_ptr[a + 1] && pa < 2 * m, fb = pb >= 0 && pb < row_ptr[b + 1] && pb < 2 * m;
    if (fa) {
      adj[pa] = (int32_t)b;
      mask[pa] = mk;
      if (WEIGHTED) w[pa] = we;
    }
    if (fb) {
      adj[pb] = (int32_t)a;
      mask[pb] = mk;
      if (WEIGHTED) w[pb] = we;
    }
    if (!fa || !fb) atomicAdd(bad, 1u);
  }
}

// ---- seeds ------------------------------------------------------------------------------------------------------------------------
// one thread per (query, slot); a slot whose vertex lies outside [0, n) is unused
__global__ __launch_bounds__(256) void khop_seed_kernel(const int64_t* __restrict__ seeds, int nq, int s, int64_t n, int W, u64* seen, u64* level0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nq * s) return;
  const int q = i / s;
  const int64_t v = seeds[i];
  if (v < 0 || v >= n) return;
  const size_t at = (size_t)v * W + (q >> 6);
  const u64 bit = 1ull << (q & 63);
  atomicOr(&level0[at], bit);
  atomicOr(&seen[at], bit);
}

// ---- the step -----------------------------------------------------------------------------------------------------------------------
struct KhopStepArgs {
  const int64_t* row_ptr;
  const int32_t* adj;
  const u64* prev;
  u64* next;
  u64* seen;
  uint32_t* grew;
  int64_t n;
  int W;
  int nq;
};

// ---- typed traversal: the allow table ----------------------------------------------------------------------------
// Q_t, the queries whose filter holds type t, as STRIDE words per type in LDS: word w of type t at [t * STRIDE + w].  The 256
// threads of the workgroup are the 256 queries of a batch, wave w holds word w; a word past the batch is 0.  Ends in a barrier
template <int STRIDE>
__device__ __forceinline__ void khop_build_allow(u64* s_allow, const uint32_t* __restrict__ filters, int nq) {
  static_assert(KHOP_MAX_B == 256 && KHOP_TYPES == 32, "a thread of the workgroup is a query, a lane below 32 stores a type's word");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t f = tid < nq ? filters[tid] : 0u;
  u64 mine = 0;
#pragma unroll
  for (int t = 0; t < KHOP_TYPES; ++t) {
    const u64 holds = __builtin_amdgcn_ballot_w64((f >> t) & 1u);
    mine = lane == t ? holds : mine;
  }
  if (lane < KHOP_TYPES && wave < STRIDE) s_allow[lane * STRIDE + wave] = mine;
  __syncthreads();
}
// A(M) = the OR of Q_t over the types of mask M, for one word: one LDS read where M has one bit; 0 for M = 0
template <int STRIDE>
__device__ __forceinline__ u64 khop_allow(const u64* s_allow, uint32_t mask, int word) {
  if (!mask) return 0ull;
  u64 a = s_allow[__builtin_ctz(mask) * STRIDE + word];
  for (uint32_t rest = mask & (mask - 1u); rest; rest &= rest - 1u) a |= s_allow[__builtin_ctz(rest) * STRIDE + word];
  return a;
}

// the typed side of a step: p.adj is then the typed slot array, `mask` lies beside it slot for slot
struct KhopStepTypes {
  const uint32_t* mask;
  const uint32_t* filters;                                  // [nq]
};

// WP: lanes per neighbour slot, one per word (the power of two >= W).  SPLIT: a workgroup per vertex of a degree list, its
// waves joined in LDS; otherwise KHOP_GROUP lanes per vertex over every vertex, those of more than KHOP_SPLIT_DEGREE
// neighbours left to the SPLIT launch.  TYPED: a neighbour's word is ANDed with A(mask of the slot); s_allow is the workgroup's
// table (32 x WP words), built by the caller
template <int WP, bool SPLIT, bool TYPED>
__device__ __forceinline__ void khop_step_body(const KhopStepArgs& p, const int32_t* __restrict__ list, const int64_t* __restrict__ list_count,
                                               const uint32_t* __restrict__ slot_mask, const u64* s_allow) {
  constexpr int LANES = SPLIT ? 256 : KHOP_GROUP;
  constexpr int NSLOT = LANES / WP;
  constexpr int PER_BLOCK = SPLIT ? 1 : 256 / KHOP_GROUP;
  __shared__ u64 s_part[SPLIT ? 4 * WP : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int gl = tid % LANES;
  const int word = gl % WP, slot = gl / WP;
  const int W = p.W;
  const u64 qmask = word < W ? khop_query_mask(p.nq, word) : 0ull;
  int64_t items = p.n;
  if (SPLIT) {
    items = *list_count;
    items = items < 0 ? 0 : (items > p.n ? p.n : items);
  }
  bool grew = false;
  for (int64_t base = (int64_t)blockIdx.x * PER_BLOCK; base < items; base += (int64_t)gridDim.x * PER_BLOCK) {     // (workgroup-uniform)
    const int64_t vi = base + (SPLIT ? 0 : tid / KHOP_GROUP);
    bool live = vi < items;
    int64_t v = 0, r0 = 0, deg = 0;
    if (live) {
      v = SPLIT ? (int64_t)list[vi] : vi;
      live = v >= 0 && v < p.n;
      v = live ? v : 0;
      r0 = p.row_ptr[v];
      deg = p.row_ptr[v + 1] - r0;
      if (!SPLIT && deg > KHOP_SPLIT_DEGREE) live = false;
    }
    const size_t at = (size_t)v * W + word;
    u64 sv = 0, need = 0;
    if (live && qmask) {
      sv = p.seen[at];
      need = ~sv & qmask;
    }
    u64 acc = 0;
    if (need) {                                                        // a word that holds every query already reads no neighbour
#pragma unroll 4
      for (int64_t e = slot; e < deg; e += NSLOT) {
        const int32_t u = p.adj[r0 + e];
        if constexpr (TYPED) {                                           // an edge no query still needed may cross: its end's word is not read
          const u64 allow = khop_allow<WP>(s_allow, slot_mask[r0 + e], word) & need;
          if (allow) acc |= p.prev[(size_t)u * W + word] & allow;
        } else {
          acc |= p.prev[(size_t)u * W + word];
        }
      }
    }
#pragma unroll
    for (int d = WP; d < (SPLIT ? 64 : KHOP_GROUP); d <<= 1) acc |= (u64)__shfl_xor((long long)acc, d, 64);
    if (SPLIT) {                                                       // the waves of the workgroup: ORs in LDS
      if (lane < WP) s_part[wave * WP + lane] = acc;
      __syncthreads();
      if (tid < WP) acc = (s_part[tid] | s_part[WP + tid]) | (s_part[2 * WP + tid] | s_part[3 * WP + tid]);
      __syncthreads();
    }
    if (slot == 0 && live && qmask) {
      const u64 nw = acc & need;
      p.next[at] = nw;
      if (nw) {
        p.seen[at] = sv | nw;
        grew = true;
      }
    }
  }
  if (__builtin_amdgcn_ballot_w64(grew) && lane == 0) atomicOr(p.grew, 1u);
}
template <int WP, bool SPLIT>
__global__ __launch_bounds__(256) void khop_step_kernel(const KhopStepArgs p, const int32_t* __restrict__ list, const int64_t* __restrict__ list_count) {
  khop_step_body<WP, SPLIT, false>(p, list, list_count, nullptr, nullptr);
}
template <int WP, bool SPLIT>
__global__ __launch_bounds__(256) void khop_step_typed_kernel(const KhopStepArgs p, const int32_t* __restrict__ list,
                                                              const int64_t* __restrict__ list_count, const KhopStepTypes ty) {
  __shared__ u64 s_allow[KHOP_TYPES * WP];
  khop_build_allow<WP>(s_allow, ty.filters, p.nq);
  khop_step_body<WP, SPLIT, true>(p, list, list_count, ty.mask, s_allow);
}

// ---- counting: shared by the counts and the list --------------------------------------------------------------------------------
// lane b's counter gains the number of lanes whose x has bit b
__device__ __forceinline__ uint32_t khop_count_bits(u64 x, int lane, uint32_t cnt) {
  if (__builtin_amdgcn_ballot_w64(x != 0) == 0) return cnt;
#pragma unroll 8
  for (int b = 0; b < 64; ++b) {
    const u64 mask = __builtin_amdgcn_ballot_w64((x >> b) & 1ull);
    cnt += lane == b ? (uint32_t)__builtin_popcountll(mask) : 0u;
  }
  return cnt;
}

// a wave per (tile, level, word): tiles[tile][h][word * 64 + b] = vertices of the tile at hop h for query word * 64 + b
__global__ __launch_bounds__(256) void khop_tile_count_kernel(const u64* __restrict__ level, size_t level_stride, int64_t n, int W, int H,
                                                              uint32_t* tiles) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t items = khop_tiles(n) * H * W;
  for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < items; item += (int64_t)gridDim.x * 4) {
    const int word = (int)(item % W);
    const int h = (int)((item / W) % H);
    const int64_t tile = item / ((int64_t)W * H);
    const u64* lv = level + level_stride * (size_t)h;
    uint32_t cnt = 0;
    for (int c = 0; c < KHOP_TILE / 64; ++c) {
      const int64_t v = tile * KHOP_TILE + c * 64 + lane;
      cnt = khop_count_bits(v < n ? lv[(size_t)v * W + word] : 0ull, lane, cnt);
    }
    tiles[((size_t)tile * H + h) * ((size_t)W * 64) + word * 64 + lane] = cnt;
  }
}

// a thread per (level, query): the counts of the tiles become exclusive offsets, in place; totals[q][h] = their sum
__global__ __launch_bounds__(256) void khop_tile_scan_kernel(int64_t n_tiles, int W, int H, int nq, uint32_t* tiles, int32_t* totals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * nq) return;
  const int h = i / nq, q = i % nq;
  const size_t stride = (size_t)H * W * 64;
  uint32_t* at = tiles + (size_t)h * W * 64 + q;
  uint32_t run = 0;
  for (int64_t t = 0; t < n_tiles; ++t) {
    const uint32_t c = at[(size_t)t * stride];
    at[(size_t)t * stride] = run;
    run += c;
  }
  totals[(size_t)q * H + h] = (int32_t)run;
}

// the caller's relation table and the `seen` words of the traversal it is read against
struct KhopRelations {
  const int64_t* rows;                                                 // [r][2]
  const u64* seen;
  int64_t r;
};

// the level words of the rows of the relation table: E_h of a row from the cumulative ORs of its two ends.  For most rows
// seen(a) & seen(b) is 0 and no level is loaded
struct KhopEdgeBits {
  const int64_t* __restrict__ rel;
  const u64* __restrict__ seen;
  const u64* __restrict__ level;
  size_t level_stride;
  int64_t r;
  int64_t n;
  // the queries of `word` that reach both ends of row e at all, and where the ends' words lie; 0 for a row past the table or
  // with an end outside [0, n)
  __device__ __forceinline__ u64 within(int64_t e, int word, int W, size_t& ia, size_t& ib) const {
    ia = ib = 0;
    if (e >= r) return 0ull;
    const int64_t a = rel[2 * e], b = rel[2 * e + 1];
    if (a < 0 || a >= n || b < 0 || b >= n) return 0ull;
    ia = (size_t)a * W + word;
    ib = (size_t)b * W + word;
    return seen[ia] & seen[ib];
  }
  template <bool PATHS>
  __device__ __forceinline__ u64 word(int64_t e, int h, int word, int W) const {
    size_t ia, ib;
    if (within(e, word, W, ia, ib) == 0) return 0ull;
    if constexpr (PATHS) {                                             // consecutive positions, either way round
      if (h == 0) return 0ull;
      const u64* lo = level + level_stride * (size_t)(h - 1);
      const u64* hi = level + level_stride * (size_t)h;
      return (lo[ia] & hi[ib]) | (hi[ia] & lo[ib]);
    }
    u64 sa = 0, sb = 0;
    for (int k = 0; k < h; ++k) {
      sa |= level[level_stride * (size_t)k + ia];
      sb |= level[level_stride * (size_t)k + ib];
    }
    const u64 below = sa & sb;                                         // both ends within h - 1
    sa |= level[level_stride * (size_t)h + ia];
    sb |= level[level_stride * (size_t)h + ib];
    return sa & sb & ~below;
  }
};

// a row's level words, level by level, from the words of its two ends.  Subgraphs: both ends within h and not both within
// h - 1.  PATHS: one end at position h - 1 and the other at h
template <bool PATHS>
struct KhopRowWalk {
  u64 a = 0, b = 0, below = 0;
  __device__ __forceinline__ u64 next(u64 xa, u64 xb) {
    if constexpr (PATHS) {
      const u64 e = (a & xb) | (xa & b);
      a = xa;
      b = xb;
      return e;
    } else {
      a |= xa;
      b |= xb;
      const u64 both = a & b, e = both & ~below;
      below = both;
      return e;
    }
  }
};

// the types of the rows of a typed relation table: a row is in q's answer only if F_q holds its type.  `type`
// holds a type id per row (one outside [0, 32) is allowed to nobody) or, with `masks`, the row's mask as an edge carries it
struct KhopRowTypes {
  const int32_t* type;                                                 // [r]
  const uint32_t* filters;                                             // [nq]
  int masks;
};
constexpr int KHOP_ROW_STRIDE = KHOP_MAX_B / 64;                       // the allow table of the row kernels: every word of a batch
__device__ __forceinline__ u64 khop_row_allow(const KhopRowTypes& ty, const u64* s_allow, int64_t e, int64_t r, int word) {
  if (e >= r) return 0ull;
  const uint32_t t = (uint32_t)ty.type[e];
  return khop_allow<KHOP_ROW_STRIDE>(s_allow, ty.masks ? t : (t < (uint32_t)KHOP_TYPES ? 1u << t : 0u), word);
}

// a wave per (tile of relation rows, word): every level of a row in one walk up its ends' words;
// tiles[tile][h][word * 64 + b] = rows of the tile at level h for query word * 64 + b.  TYPED: the queries that may not take the
// row's type are cleared from its words first
template <bool PATHS, bool TYPED>
__device__ __forceinline__ void khop_edge_count_body(const KhopEdgeBits& src, int W, int H, uint32_t* tiles, const KhopRowTypes& ty,
                                                     const u64* s_allow) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t items = khop_tiles(src.r) * W;
  for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < items; item += (int64_t)gridDim.x * 4) {
    const int word = (int)(item % W);
    const int64_t tile = item / W;
    uint32_t cnt[KHOP_MAX_HOPS + 1] = {};                              // (indexed by unrolled loops only: registers)
    for (int c = 0; c < KHOP_TILE / 64; ++c) {
      size_t ia, ib;
      u64 in = src.within(tile * KHOP_TILE + c * 64 + lane, word, W, ia, ib);
      if constexpr (TYPED) {
        if (in) in &= khop_row_allow(ty, s_allow, tile * KHOP_TILE + c * 64 + lane, src.r, word);
      }
      if (__builtin_amdgcn_ballot_w64(in != 0) == 0) continue;
      KhopRowWalk<PATHS> walk;
#pragma unroll
      for (int h = 0; h <= KHOP_MAX_HOPS; ++h) {
        if (h < H) {                                                   // (wave-uniform)
          u64 xa = 0, xb = 0;
          if (in) {
            xa = src.level[src.level_stride * (size_t)h + ia];
            xb = src.level[src.level_stride * (size_t)h + ib];
          }
          if constexpr (TYPED) {                                       // (untyped: a level is inside `in` already)
            xa &= in;
            xb &= in;
          }
          cnt[h] = khop_count_bits(walk.next(xa, xb), lane, cnt[h]);
        }
      }
    }
#pragma unroll
    for (int h = 0; h <= KHOP_MAX_HOPS; ++h)
      if (h < H) tiles[((size_t)tile * H + h) * ((size_t)W * 64) + word * 64 + lane] = cnt[h];
  }
}
template <bool PATHS>
__global__ __launch_bounds__(256) void khop_edge_count_kernel(const KhopEdgeBits src, int W, int H, uint32_t* tiles) {
  khop_edge_count_body<PATHS, false>(src, W, H, tiles, KhopRowTypes{nullptr, nullptr, 0}, nullptr);
}
template <bool PATHS>
__global__ __launch_bounds__(256) void khop_edge_count_typed_kernel(const KhopEdgeBits src, int W, int H, int nq, uint32_t* tiles,
                                                                    const KhopRowTypes ty) {
  __shared__ u64 s_allow[KHOP_TYPES * KHOP_ROW_STRIDE];
  khop_build_allow<KHOP_ROW_STRIDE>(s_allow, ty.filters, nq);
  khop_edge_count_body<PATHS, true>(src, W, H, tiles, ty, s_allow);
}

// a wave per (tile, word): the entries of its items, level by level, at offset + rank; block 0 also writes the counts.
// EDGES: the items are the rows of `rel` and a row's level word is derived from its ends' (PATHS: by the rule of the connecting
// paths); otherwise they are the vertices.  TYPED (EDGES only): a row's word keeps the queries whose filter holds its type
template <bool EDGES, bool PATHS, bool TYPED>
__device__ __forceinline__ void khop_list_body(const u64* __restrict__ level, size_t level_stride, int64_t n, int W, int H, int nq,
                                               const uint32_t* __restrict__ tiles, const int32_t* __restrict__ totals, uint32_t max_vertices,
                                               int64_t* out_ids, int32_t* out_hops, int32_t* out_count, const KhopRelations& rel,
                                               const KhopRowTypes& ty, const u64* s_allow) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (blockIdx.x == 0) {
    for (int q = threadIdx.x; q < nq; q += 256) {
      int64_t size = 0;
      for (int h = 0; h < H; ++h) size += totals[(size_t)q * H + h];
      out_count[q] = (int32_t)(size < (int64_t)max_vertices ? size : (int64_t)max_vertices);
    }
  }
  const u64 below = (1ull << lane) - 1ull;
  const KhopEdgeBits rows = {rel.rows, rel.seen, level, level_stride, rel.r, n};
  const int64_t items = khop_tiles(EDGES ? rel.r : n) * W;
  for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < items; item += (int64_t)gridDim.x * 4) {
    const int word = (int)(item % W);
    const int64_t tile = item / W;
    const int q = word * 64 + lane;                                    // the query whose cursor this lane keeps
    uint32_t before = 0;                                               // entries of q's list at the levels below h
    for (int h = 0; h < H; ++h) {
      uint32_t cursor = max_vertices;
      if (q < nq) {
        const uint32_t off = before + tiles[((size_t)tile * H + h) * ((size_t)W * 64) + q];
        cursor = off < max_vertices ? off : max_vertices;
        const uint32_t total = (uint32_t)totals[(size_t)q * H + h];      // (< 2^31, and `before` stays <= max_vertices: no wrap)
        before = before + total < max_vertices ? before + total : max_vertices;
      }
      if (__builtin_amdgcn_ballot_w64(cursor < max_vertices) == 0) continue;   // every list of this word is full before this tile
      const u64* lv = level + level_stride * (size_t)h;
      for (int c = 0; c < KHOP_TILE / 64; ++c) {
        const int64_t v = tile * KHOP_TILE + c * 64 + lane;
        u64 x;
        if constexpr (EDGES) x = rows.template word<PATHS>(v, h, word, W);
        else x = v < n ? lv[(size_t)v * W + word] : 0ull;
        if constexpr (TYPED) {
          if (x) x &= khop_row_allow(ty, s_allow, v, rel.r, word);
        }
        if (__builtin_amdgcn_ballot_w64(x != 0) == 0) continue;
        for (int b = 0; b < 64; ++b) {                                 // (b is wave-uniform)
          const bool mine = (x >> b) & 1ull;
          const u64 mask = __builtin_amdgcn_ballot_w64(mine);
          if (!mask) continue;
          const uint32_t cb = (uint32_t)__shfl((int)cursor, b, 64);
          const uint32_t pos = cb + (uint32_t)__builtin_popcountll(mask & below);
          if (mine && pos < max_vertices && word * 64 + b < nq) {
            const size_t o = (size_t)(word * 64 + b) * max_vertices + pos;
            out_ids[o] = v;
            out_hops[o] = h;
          }
          if (lane == b) {
            const uint32_t nc = cursor + (uint32_t)__builtin_popcountll(mask);
            cursor = nc < max_vertices ? nc : max_vertices;
          }
        }
      }
    }
  }
}
template <bool EDGES, bool PATHS = false>
__global__ __launch_bounds__(256) void khop_list_kernel(const u64* __restrict__ level, size_t level_stride, int64_t n, int W, int H, int nq,
                                                        const uint32_t* __restrict__ tiles, const int32_t* __restrict__ totals, uint32_t max_vertices,
                                                        int64_t* out_ids, int32_t* out_hops, int32_t* out_count, const KhopRelations rel) {
  khop_list_body<EDGES, PATHS, false>(level, level_stride, n, W, H, nq, tiles, totals, max_vertices, out_ids, out_hops, out_count, rel,
                                      KhopRowTypes{nullptr, nullptr, 0}, nullptr);
}
template <bool PATHS>
__global__ __launch_bounds__(256) void khop_list_typed_kernel(const u64* __restrict__ level, size_t level_stride, int64_t n, int W, int H, int nq,
                                                              const uint32_t* __restrict__ tiles, const int32_t* __restrict__ totals,
                                                              uint32_t max_vertices, int64_t* out_ids, int32_t* out_hops, int32_t* out_count,
                                                              const KhopRelations rel, const KhopRowTypes ty) {
  __shared__ u64 s_allow[KHOP_TYPES * KHOP_ROW_STRIDE];
  khop_build_allow<KHOP_ROW_STRIDE>(s_allow, ty.filters, nq);
  khop_list_body<true, PATHS, true>(level, level_stride, n, W, H, nq, tiles, totals, max_vertices, out_ids, out_hops, out_count, rel, ty, s_allow);
}

// ---- the dense answer ---------------------------------------------------------------------------------------------------------------
// a wave per (64 vertices, word), a lane a vertex.  The levels of a (vertex, query) are disjoint, so the hop is read off four
// bit planes (plane k = the OR of the levels whose number has bit k) and `in` = the OR of all: no per-lane table
__global__ __launch_bounds__(256) void khop_levels_kernel(const u64* __restrict__ level, size_t level_stride, int64_t n, int W, int H, int nq,
                                                          uint8_t* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t items = ((n + 63) / 64) * W;
  for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < items; item += (int64_t)gridDim.x * 4) {
    const int word = (int)(item % W);
    const int64_t v = (item / W) * 64 + lane;
    u64 in = 0, p0 = 0, p1 = 0, p2 = 0, p3 = 0;
    if (v < n) {
      for (int h = 0; h < H; ++h) {
        const u64 x = level[level_stride * (size_t)h + (size_t)v * W + word];
        in |= x;
        p0 |= (h & 1) ? x : 0ull;
        p1 |= (h & 2) ? x : 0ull;
        p2 |= (h & 4) ? x : 0ull;
        p3 |= (h & 8) ? x : 0ull;
      }
    }
    const int nb = nq - word * 64 < 64 ? nq - word * 64 : 64;
    if (v < n) {
      for (int b = 0; b < nb; ++b) {
        const uint32_t d = (uint32_t)((p0 >> b) & 1ull) | (uint32_t)((p1 >> b) & 1ull) << 1 | (uint32_t)((p2 >> b) & 1ull) << 2 |
                           (uint32_t)((p3 >> b) & 1ull) << 3;
        out[(size_t)(word * 64 + b) * (size_t)n + (size_t)v] = (uint8_t)(((in >> b) & 1ull) ? d : 255u);
      }
    }
  }
}

// ---- chunks -------------------------------------------------------------------------------------------------------------------------
struct KhopChunkArgs {
  const int64_t* row_ptr;
  const int32_t* ent;
  const uint32_t* w;
  const u64* level;
  u64* s;
  size_t level_stride;
  int64_t n;
  int64_t n_chunks;
  int64_t nnz;
  int W;
  int H;
  int nq;
  uint32_t decay[KHOP_MAX_HOPS + 1];
};

// a wave per (chunk, word), a lane a query; SPLIT: a workgroup per listed chunk, its waves take 64 mentions each in turn and
// are joined by integer adds in LDS
template <bool SPLIT>
__global__ __launch_bounds__(256) void khop_chunks_kernel(const KhopChunkArgs a, const int32_t* __restrict__ list, int64_t list_count) {
  __shared__ u64 s_part[SPLIT ? 4 * 64 : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int W = a.W;
  const int64_t items = (SPLIT ? list_count : a.n_chunks) * W;
  const int64_t first = SPLIT ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave;
  const int64_t stride = SPLIT ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4;
  for (int64_t item = first; item < items; item += stride) {
    const int word = (int)(item % W);
    const int64_t ci = item / W;
    const int64_t c = SPLIT ? (int64_t)list[ci] : ci;
    if (SPLIT && (c < 0 || c >= a.n_chunks)) continue;                 // (workgroup-uniform: every thread reads the same entry)
    int64_t r0 = a.row_ptr[c], r1 = a.row_ptr[c + 1];
    r0 = r0 < 0 ? 0 : (r0 > a.nnz ? a.nnz : r0);
    r1 = r1 < r0 ? r0 : (r1 > a.nnz ? a.nnz : r1);
    const int64_t deg = r1 - r0;
    const int q = word * 64 + lane;
    u64 acc = 0;
    if (SPLIT || deg <= KHOP_SPLIT_DEGREE) {
      for (int64_t i0 = SPLIT ? wave * 64 : 0; i0 < deg; i0 += SPLIT ? 256 : 64) {
        // this lane's mention: its entity's row of the levels, or -1 for an entry outside the rule, and its weight
        int32_t row = -1;
        uint32_t wt = 0;
        if (i0 + lane < deg) {
          const int32_t e = a.ent[r0 + i0 + lane];
          const uint32_t w = a.w[r0 + i0 + lane];
          if (e >= 0 && (int64_t)e < a.n && w >= 1u && w < (1u << PPR_CHUNK_WEIGHT_BITS)) {
            row = e;
            wt = w;
          }
        }
        const int cnt = deg - i0 < 64 ? (int)(deg - i0) : 64;
        for (int i = 0; i < cnt; ++i) {                                // (i is wave-uniform: every lane takes mention i)
          const int32_t e = __shfl(row, i, 64);
          const uint32_t w = (uint32_t)__shfl((int)wt, i, 64);
          if (e < 0) continue;
          const u64* at = a.level + (size_t)e * W + word;
          uint32_t dec = 0;
#pragma unroll
          for (int h = 0; h <= KHOP_MAX_HOPS; ++h)
            if (h < a.H) dec += ((at[a.level_stride * (size_t)h] >> lane) & 1ull) ? a.decay[h] : 0u;
          acc += (u64)w * dec;
        }
      }
    }
    if (SPLIT) {
      s_part[wave * 64 + lane] = acc;
      __syncthreads();
      if (wave == 0) acc = (s_part[lane] + s_part[64 + lane]) + (s_part[128 + lane] + s_part[192 + lane]);
      __syncthreads();
    }
    if (q < a.nq && (!SPLIT || wave == 0)) a.s[(size_t)c * a.nq + q] = acc;     // (a chunk left to the SPLIT launch: 0 until that overwrites it)
  }
}

// ---- connecting paths ---------------------------------------------------------------------------------------------------------------
// a thread per vertex: one that holds a level-0 bit of the traversal is an end of some source; for every pair whose B it ends,
// its hop from A lowers the pair's distance.  A pair that names no column is skipped and keeps 0xFFFFFFFF.  The pairs are
// staged in LDS once a workgroup (ia | ib << 8, or -1): an end of many sources walks them there, not in global memory
__global__ __launch_bounds__(256) void khop_path_dist_kernel(const u64* __restrict__ level, size_t level_stride, int64_t n, int W, int H, int ns,
                                                             const int32_t* __restrict__ pairs, int np, uint32_t* dist) {
  static_assert(KHOP_MAX_B == 256, "one thread of the workgroup stages one pair");
  __shared__ int32_t s_pair[KHOP_MAX_B];
  int code = -1;
  if ((int)threadIdx.x < np) {
    const int ia = pairs[2 * threadIdx.x], ib = pairs[2 * threadIdx.x + 1];
    if (ia >= 0 && ia < ns && ib >= 0 && ib < ns) code = ia | ib << 8;
  }
  s_pair[threadIdx.x] = code;
  __syncthreads();
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    const u64* at = level + (size_t)v * W;
    u64 ends = 0;
    for (int w = 0; w < W; ++w) ends |= at[w];
    if (!ends) continue;
    for (int p = 0; p < np; ++p) {
      const int c = s_pair[p];
      if (c < 0) continue;
      const int ia = c & 255, ib = c >> 8;
      if (!((at[ib >> 6] >> (ib & 63)) & 1ull)) continue;
      for (int h = 0; h < H; ++h) {
        if ((at[level_stride * (size_t)h + (ia >> 6)] >> (ia & 63)) & 1ull) {
          atomicMin(&dist[p], (uint32_t)h);
          break;
        }
      }
    }
  }
}

struct KhopPathArgs {
  const u64* seen;                                                     // the traversal: ns columns, W words a vertex
  const u64* level;
  u64* pseen;                                                          // the path state: np columns, PW words a vertex
  u64* plevel;
  const int32_t* pairs;
  const int32_t* dist;
  size_t level_stride;
  size_t plevel_stride;
  int64_t n;
  int W;
  int PW;
  int H;
  int ns;
  int np;
};

// a wave per vertex, a lane a pair, of each of the PW words of pairs in turn (the pairs are staged in LDS once a workgroup).
// Lane k < H * W holds word k % W of level k / W of the vertex, and lane k < (H + 1) * PW collects word k % PW of the path
// state's seen (k / PW == 0) or of position k / PW - 1.  The levels of a (vertex, column) are disjoint: hop_A is the one level
// that holds A's bit, and B is looked up at d - hop_A alone
__global__ __launch_bounds__(256) void khop_path_mark_kernel(const KhopPathArgs a) {
  static_assert(KHOP_MAX_B == 256, "one thread of the workgroup stages one pair");
  __shared__ int32_t s_code[KHOP_MAX_B];                               // ia | ib << 8 | d << 16 of a pair, or -1 for one without paths
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int W = a.W, PW = a.PW, H = a.H;
  int code = -1;
  if ((int)threadIdx.x < a.np) {
    const int ia = a.pairs[2 * threadIdx.x], ib = a.pairs[2 * threadIdx.x + 1], d = a.dist[threadIdx.x];
    if (ia >= 0 && ia < a.ns && ib >= 0 && ib < a.ns && d >= 0 && d < H) code = ia | ib << 8 | d << 16;
  }
  s_code[threadIdx.x] = code;
  __syncthreads();
  const bool loads = lane < H * W, stores = lane < (H + 1) * PW;
  const size_t src = loads ? a.level_stride * (size_t)(lane / W) + (size_t)(lane % W) : 0;
  u64* const dst = !stores ? nullptr : (lane < PW ? a.pseen + lane : a.plevel + a.plevel_stride * (size_t)(lane / PW - 1) + lane % PW);
  for (int64_t v = (int64_t)blockIdx.x * 4 + wave; v < a.n; v += (int64_t)gridDim.x * 4) {     // (v is wave-uniform)
    const u64 sv = lane < W ? a.seen[(size_t)v * W + lane] : 0ull;
    u64 out = 0;
    if (__builtin_amdgcn_ballot_w64(sv != 0) != 0) {                   // a vertex no source reached: zeros, its levels unread
      const u64 x = loads ? a.level[src + (size_t)v * W] : 0ull;
      for (int wp = 0; wp < PW; ++wp) {                                // (wave-uniform: every lane takes part in every shuffle)
        const int c = s_code[wp * 64 + lane];
        const int ia = c < 0 ? 0 : c & 255, ib = c < 0 ? 0 : (c >> 8) & 255, d = c >> 16;
        int pos = -1;
#pragma unroll
        for (int h = 0; h <= KHOP_MAX_HOPS; ++h) {
          if (h < H) {
            const u64 xa = (u64)__shfl((long long)x, h * W + (ia >> 6), 64);
            pos = ((xa >> (ia & 63)) & 1ull) ? h : pos;
          }
        }
        const bool both = c >= 0 && pos >= 0 && pos <= d;
        const u64 xb = (u64)__shfl((long long)x, (both ? d - pos : 0) * W + (ib >> 6), 64);
        pos = both && ((xb >> (ib & 63)) & 1ull) ? pos : -1;
        const u64 on = __builtin_amdgcn_ballot_w64(pos >= 0);
        out = lane == wp ? on : out;
#pragma unroll
        for (int i = 0; i <= KHOP_MAX_HOPS; ++i) {
          if (i < H) {
            const u64 at = __builtin_amdgcn_ballot_w64(pos == i);
            out = lane == (i + 1) * PW + wp ? at : out;
          }
        }
      }
    }
    if (stores) dst[(size_t)v * PW] = out;
  }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" int rarc_khop_limits(int* out5) {
  RARC_REQUIRE(out5, RARC_E_INVALID, "rarc_khop_limits: null pointer");
  out5[0] = KHOP_MAX_HOPS;
  out5[1] = KHOP_MAX_B;
  out5[2] = KHOP_MAX_SEEDS;
  out5[3] = KHOP_MAX_VERTICES;
  out5[4] = KHOP_SPLIT_DEGREE;
  return RARC_OK;
}

extern "C" size_t rarc_khop_workspace_bytes(int64_t n, int64_t m, int nq, int hops) {
  if (!khop_shape_ok(n, m, nq, hops)) return 0;
  return khop_carve(nullptr, n, nq, hops).bytes;
}

#define KHOP_ALIGNED(P, A) (((uintptr_t)(P) & (uintptr_t)((A)-1)) == 0)
#define KHOP_SHAPE_CHECKS(NAME)                                                                                                          \
  RARC_REQUIRE(lv_shape_ok(n, m), RARC_E_INVALID, NAME ": n=%lld m=%lld out of range (2 <= n < 2^31 - 1, 1 <= m < 2^30)", (long long)n,  \
               (long long)m);                                                                                                            \
  RARC_REQUIRE(nq >= 1 && nq <= KHOP_MAX_B, RARC_E_INVALID, NAME ": %d queries out of range (1 <= B <= %d per call)", nq, KHOP_MAX_B);   \
  RARC_REQUIRE(hops >= 0, RARC_E_INVALID, NAME ": hops=%d out of range (0 <= hops <= %d)", hops, KHOP_MAX_HOPS);                         \
  RARC_REQUIRE(hops <= KHOP_MAX_HOPS, RARC_E_UNSUPPORTED, NAME ": hops=%d: at most %d levels are kept (0 <= hops <= %d)", hops,          \
               KHOP_MAX_HOPS, KHOP_MAX_HOPS);                                                                                            \
  RARC_REQUIRE(KHOP_ALIGNED(d_ws, 256), RARC_E_INVALID, NAME ": the workspace is not 256-byte aligned");                                 \
  const KhopWs ws = khop_carve(d_ws, n, nq, hops);                                                                                       \
  RARC_REQUIRE(ws_bytes >= ws.bytes, RARC_E_WORKSPACE, NAME ": workspace of %zu bytes, %zu needed", ws_bytes, ws.bytes);                 \
  const int W = khop_words(nq), H = hops + 1;                                                                                            \
  const size_t level_stride = lv_align(ws.level_words * 8) / 8;                                                                          \
  (void)W;                                                                                                                               \
  (void)H;                                                                                                                               \
  (void)level_stride

extern "C" int rarc_khop_seed(int64_t n, int64_t m, const int64_t* d_seeds, int nq, int n_slots, int hops, void* d_ws, size_t ws_bytes,
                              void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_seeds && d_ws, RARC_E_INVALID, "rarc_khop_seed: null pointer");
  RARC_REQUIRE(KHOP_ALIGNED(d_seeds, 8), RARC_E_INVALID, "rarc_khop_seed: the seeds are not 8-byte aligned");
  KHOP_SHAPE_CHECKS("rarc_khop_seed");
  RARC_REQUIRE(n_slots >= 1 && n_slots <= KHOP_MAX_SEEDS, RARC_E_INVALID, "rarc_khop_seed: %d seed slots out of range (1 <= s <= %d)", n_slots,
               KHOP_MAX_SEEDS);
  hipStream_t s = (hipStream_t)stream;
  RARC_HIP_CHECK(hipMemsetAsync(ws.grew, 0, KHOP_CTL_BYTES, s));
  RARC_HIP_CHECK(hipMemsetAsync(ws.seen, 0, ws.clear_bytes, s));
  hipLaunchKernelGGL(khop_seed_kernel, dim3((nq * n_slots + 255) / 256), dim3(256), 0, s, d_seeds, nq, n_slots, n, W, ws.seen, khop_level(ws, 0));
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

// TYPED: the same three launches of khop_step_typed_kernel, `ty` beside the arguments
template <int WP, bool TYPED = false>
static void khop_launch_step(const KhopStepArgs& p, const LvGraph& g, int64_t n, int64_t m, hipStream_t s, const KhopStepTypes ty = {}) {
  auto launch = [&](auto split, unsigned grid, const int32_t* list, const int64_t* count) {
    constexpr bool SPLIT = decltype(split)::value;
    if constexpr (TYPED) hipLaunchKernelGGL((khop_step_typed_kernel<WP, SPLIT>), dim3(grid), dim3(256), 0, s, p, list, count, ty);
    else hipLaunchKernelGGL((khop_step_kernel<WP, SPLIT>), dim3(grid), dim3(256), 0, s, p, list, count);
  };
  launch(std::false_type{}, lv_grid(n, 256 / KHOP_GROUP, 16384), nullptr, nullptr);
  const int64_t dmax = lv_max_degree(n, m);              // no vertex of this graph has more neighbours: skip the lists that must be empty
  if (dmax > LV_DEG_WAVE) launch(std::true_type{}, lv_grid(n, 1, 2048), g.list[2], &g.hdr[LV_H_LIST + 2]);
  if (dmax > LV_DEG_LDS) launch(std::true_type{}, lv_grid(n / LV_DEG_LDS + 1, 1, 2048), g.list[3], &g.hdr[LV_H_LIST + 3]);
}

extern "C" size_t rarc_graph_types_workspace_bytes(int64_t n, int64_t m) {
  if (!lv_shape_ok(n, m)) return 0;
  return khop_types_carve(nullptr, n, m).bytes;
}

// the body of rarc_graph_types and rarc_graph_types_weighted: the same checks, the same fill kernel, the same wait for `bad`
template <bool WEIGHTED>
static int khop_graph_types(const char* name, const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, const int64_t* d_pairs,
                            const uint32_t* d_masks, const uint32_t* d_weights, void* d_out, size_t out_bytes, void* stream) {
  RARC_REQUIRE(d_graph && d_pairs && d_masks && d_out, RARC_E_INVALID, "%s: null pointer", name);
  RARC_REQUIRE(KHOP_ALIGNED(d_graph, 256) && KHOP_ALIGNED(d_out, 256), RARC_E_INVALID,
               "%s: the graph or the typed adjacency is not 256-byte aligned", name);
  RARC_REQUIRE(KHOP_ALIGNED(d_pairs, 8) && KHOP_ALIGNED(d_masks, 4) && KHOP_ALIGNED(d_weights, 4), RARC_E_INVALID,
               "%s: an array is not aligned to its element (pairs 8 bytes, masks%s 4)", name, WEIGHTED ? " and weights" : "");
  RARC_REQUIRE(lv_shape_ok(n, m), RARC_E_INVALID, "%s: n=%lld m=%lld out of range (2 <= n < 2^31 - 1, 1 <= m < 2^30)", name, (long long)n,
               (long long)m);
  const LvGraph g = lv_graph_carve(d_graph, n, m);
  RARC_REQUIRE(graph_bytes >= g.bytes, RARC_E_WORKSPACE, "%s: graph workspace of %zu bytes, %zu needed", name, graph_bytes, g.bytes);
  const KhopTypes t = khop_types_carve(d_out, n, m);
  const size_t need = WEIGHTED ? t.weighted_bytes : t.bytes;
  RARC_REQUIRE(out_bytes >= need, RARC_E_WORKSPACE, "%s: typed adjacency of %zu bytes, %zu needed", name, out_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  RARC_HIP_CHECK(hipMemsetAsync(d_out, 0, need, s));     // a slot no pair fills: neighbour 0 under mask 0 (and weight 0), crossed by nobody
  hipLaunchKernelGGL(khop_types_fill_kernel<WEIGHTED>, dim3(lv_grid(m, 256, 4096)), dim3(256), 0, s, d_pairs, d_masks, d_weights, m, n,
                     (const int64_t*)g.row_ptr, t.cursor, t.adj, t.mask, t.w, t.bad);
  RARC_HIP_CHECK(hipGetLastError());
  uint32_t bad = 0;                                      // built once a graph: the entry waits for the count and reports it
  RARC_HIP_CHECK(hipMemcpyAsync(&bad, t.bad, 4, hipMemcpyDeviceToHost, s));
  RARC_HIP_CHECK(hipStreamSynchronize(s));
  RARC_REQUIRE(bad == 0, RARC_E_INVALID, "%s: %u pairs found their rows full: not the pair list the graph was built from", name, bad);
  return RARC_OK;
}

extern "C" int rarc_graph_types(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, const int64_t* d_pairs, const uint32_t* d_masks,
                                void* d_out, size_t out_bytes, void* stream) {
  RARC_RANGE();
  return khop_graph_types<false>("rarc_graph_types", d_graph, graph_bytes, n, m, d_pairs, d_masks, nullptr, d_out, out_bytes, stream);
}

// the typed adjacency with a weight plane behind it: the first rarc_graph_types_workspace_bytes(n, m) bytes are
// what rarc_graph_types writes, so the typed k-hop entries take the same buffer
extern "C" size_t rarc_graph_types_weighted_workspace_bytes(int64_t n, int64_t m) {
  if (!lv_shape_ok(n, m)) return 0;
  return khop_types_carve(nullptr, n, m).weighted_bytes;
}

extern "C" int rarc_graph_types_weighted(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, const int64_t* d_pairs,
                                         const uint32_t* d_masks, const uint32_t* d_weights, void* d_out, size_t out_bytes, void* stream) {
  RARC_RANGE();
  return khop_graph_types<true>("rarc_graph_types_weighted", d_graph, graph_bytes, n, m, d_pairs, d_masks, d_weights, d_out, out_bytes, stream);
}

extern "C" int rarc_khop_step(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, int nq, int hops, int hop, void* d_ws,
                              size_t ws_bytes, uint32_t* d_grew_out, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_graph && d_ws, RARC_E_INVALID, "rarc_khop_step: null pointer");
  RARC_REQUIRE(KHOP_ALIGNED(d_graph, 256), RARC_E_INVALID, "rarc_khop_step: the graph is not 256-byte aligned");
  RARC_REQUIRE(KHOP_ALIGNED(d_grew_out, 4), RARC_E_INVALID, "rarc_khop_step: the grew word is not 4-byte aligned");
  KHOP_SHAPE_CHECKS("rarc_khop_step");
  RARC_REQUIRE(hop >= 1 && hop <= hops, RARC_E_INVALID, "rarc_khop_step: hop %d out of range (1 <= hop <= hops = %d)", hop, hops);
  const LvGraph g = lv_graph_carve(d_graph, n, m);
  RARC_REQUIRE(graph_bytes >= g.bytes, RARC_E_WORKSPACE, "rarc_khop_step: graph workspace of %zu bytes, %zu needed", graph_bytes, g.bytes);
  hipStream_t s = (hipStream_t)stream;
  KhopStepArgs p;
  p.row_ptr = g.row_ptr;
  p.adj = g.adj;
  p.prev = khop_level(ws, hop - 1);
  p.next = khop_level(ws, hop);
  p.seen = ws.seen;
  p.grew = ws.grew;
  p.n = n;
  p.W = W;
  p.nq = nq;
  RARC_HIP_CHECK(hipMemsetAsync(ws.grew, 0, 4, s));
  if (W > 2) khop_launch_step<4>(p, g, n, m, s);
  else if (W > 1) khop_launch_step<2>(p, g, n, m, s);
  else khop_launch_step<1>(p, g, n, m, s);
  RARC_HIP_CHECK(hipGetLastError());
  if (d_grew_out) RARC_HIP_CHECK(hipMemcpyAsync(d_grew_out, ws.grew, 4, hipMemcpyDeviceToDevice, s));
  return RARC_OK;
}

extern "C" int rarc_khop_step_typed(const void* d_graph, size_t graph_bytes, const void* d_types, size_t types_bytes, const uint32_t* d_filters,
                                    int64_t n, int64_t m, int nq, int hops, int hop, void* d_ws, size_t ws_bytes, uint32_t* d_grew_out,
                                    void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_graph && d_types && d_filters && d_ws, RARC_E_INVALID, "rarc_khop_step_typed: null pointer");
  RARC_REQUIRE(KHOP_ALIGNED(d_graph, 256), RARC_E_INVALID, "rarc_khop_step_typed: the graph is not 256-byte aligned");
  RARC_REQUIRE(KHOP_ALIGNED(d_types, 256), RARC_E_INVALID, "rarc_khop_step_typed: the typed adjacency is not 256-byte aligned");
  RARC_REQUIRE(KHOP_ALIGNED(d_filters, 4) && KHOP_ALIGNED(d_grew_out, 4), RARC_E_INVALID,
               "rarc_khop_step_typed: the filters or the grew word are not 4-byte aligned");
  KHOP_SHAPE_CHECKS("rarc_khop_step_typed");
  RARC_REQUIRE(hop >= 1 && hop <= hops, RARC_E_INVALID, "rarc_khop_step_typed: hop %d out of range (1 <= hop <= hops = %d)", hop, hops);
  const LvGraph g = lv_graph_carve(d_graph, n, m);
  RARC_REQUIRE(graph_bytes >= g.bytes, RARC_E_WORKSPACE, "rarc_khop_step_typed: graph workspace of %zu bytes, %zu needed", graph_bytes, g.bytes);
  const KhopTypes t = khop_types_carve(d_types, n, m);
  RARC_REQUIRE(types_bytes >= t.bytes, RARC_E_WORKSPACE, "rarc_khop_step_typed: typed adjacency of %zu bytes, %zu needed", types_bytes, t.bytes);
  hipStream_t s = (hipStream_t)stream;
  KhopStepArgs p;
  p.row_ptr = g.row_ptr;
  p.adj = t.adj;
  p.prev = khop_level(ws, hop - 1);
  p.next = khop_level(ws, hop);
  p.seen = ws.seen;
  p.grew = ws.grew;
  p.n = n;
  p.W = W;
  p.nq = nq;
  const KhopStepTypes ty = {t.mask, d_filters};
  RARC_HIP_CHECK(hipMemsetAsync(ws.grew, 0, 4, s));
  if (W > 2) khop_launch_step<4, true>(p, g, n, m, s, ty);
  else if (W > 1) khop_launch_step<2, true>(p, g, n, m, s, ty);
  else khop_launch_step<1, true>(p, g, n, m, s, ty);
  RARC_HIP_CHECK(hipGetLastError());
  if (d_grew_out) RARC_HIP_CHECK(hipMemcpyAsync(d_grew_out, ws.grew, 4, hipMemcpyDeviceToDevice, s));
  return RARC_OK;
}

// tile counts -> offsets and totals: the first two passes of the list, and all of the counts
static void khop_rank(const KhopWs& ws, size_t level_stride, int64_t n, int W, int H, int nq, hipStream_t s) {
  hipLaunchKernelGGL(khop_tile_count_kernel, dim3(lv_grid(khop_tiles(n) * H * W, 4, 16384)), dim3(256), 0, s, (const u64*)ws.level, level_stride, n,
                     W, H, ws.tiles);
  hipLaunchKernelGGL(khop_tile_scan_kernel, dim3((H * nq + 255) / 256), dim3(256), 0, s, khop_tiles(n), W, H, nq, ws.tiles, ws.totals);
}

extern "C" int rarc_khop_counts(int64_t n, int64_t m, int nq, int hops, void* d_ws, size_t ws_bytes, int32_t* d_out_counts, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_ws && d_out_counts, RARC_E_INVALID, "rarc_khop_counts: null pointer");
  RARC_REQUIRE(KHOP_ALIGNED(d_out_counts, 4), RARC_E_INVALID, "rarc_khop_counts: the counts are not 4-byte aligned");
  KHOP_SHAPE_CHECKS("rarc_khop_counts");
  hipStream_t s = (hipStream_t)stream;
  khop_rank(ws, level_stride, n, W, H, nq, s);
  RARC_HIP_CHECK(hipGetLastError());
  RARC_HIP_CHECK(hipMemcpyAsync(d_out_counts, ws.totals, (size_t)nq * H * 4, hipMemcpyDeviceToDevice, s));
  return RARC_OK;
}

extern "C" int rarc_khop_levels(int64_t n, int64_t m, int nq, int hops, const void* d_ws, size_t ws_bytes, uint8_t* d_out_levels, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_ws && d_out_levels, RARC_E_INVALID, "rarc_khop_levels: null pointer");
  KHOP_SHAPE_CHECKS("rarc_khop_levels");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(khop_levels_kernel, dim3(lv_grid(((n + 63) / 64) * W, 4, 16384)), dim3(256), 0, s, (const u64*)ws.level, level_stride, n, W, H,
                     nq, d_out_levels);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_khop_list(int64_t n, int64_t m, int nq, int hops, int max_vertices, void* d_ws, size_t ws_bytes, int64_t* d_out_ids,
                              int32_t* d_out_hops, int32_t* d_out_count, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_ws && d_out_ids && d_out_hops && d_out_count, RARC_E_INVALID, "rarc_khop_list: null pointer");
  RARC_REQUIRE(KHOP_ALIGNED(d_out_ids, 8) && KHOP_ALIGNED(d_out_hops, 4) && KHOP_ALIGNED(d_out_count, 4), RARC_E_INVALID,
               "rarc_khop_list: an output is not aligned to its element (ids 8 bytes, hops and counts 4)");
  KHOP_SHAPE_CHECKS("rarc_khop_list");
  RARC_REQUIRE(max_vertices >= 1, RARC_E_INVALID, "rarc_khop_list: max_vertices=%d out of range (1 <= max_vertices <= %d)", max_vertices,
               KHOP_MAX_VERTICES);
  RARC_REQUIRE(max_vertices <= KHOP_MAX_VERTICES, RARC_E_UNSUPPORTED,
               "rarc_khop_list: max_vertices=%d: a list holds at most %d vertices (rarc_khop_levels has no such limit)", max_vertices,
               KHOP_MAX_VERTICES);
  hipStream_t s = (hipStream_t)stream;
  RARC_HIP_CHECK(hipMemsetAsync(d_out_ids, 0xFF, (size_t)nq * max_vertices * 8, s));        // (-1, -1) past the count
  RARC_HIP_CHECK(hipMemsetAsync(d_out_hops, 0xFF, (size_t)nq * max_vertices * 4, s));
  khop_rank(ws, level_stride, n, W, H, nq, s);
  hipLaunchKernelGGL(khop_list_kernel<false>, dim3(lv_grid(khop_tiles(n) * W, 4, 16384)), dim3(256), 0, s, (const u64*)ws.level, level_stride, n, W, H,
                     nq, (const uint32_t*)ws.tiles, (const int32_t*)ws.totals, (uint32_t)max_vertices, d_out_ids, d_out_hops, d_out_count,
                     KhopRelations{nullptr, nullptr, 0});
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_khop_edges_limits(int* out2) {
  RARC_REQUIRE(out2, RARC_E_INVALID, "rarc_khop_edges_limits: null pointer");
  out2[0] = KHOP_MAX_EDGES;
  out2[1] = KHOP_TILE;
  return RARC_OK;
}

extern "C" size_t rarc_khop_edges_workspace_bytes(int64_t r, int nq, int hops) {
  if (!khop_rows_ok(r) || nq < 1 || nq > KHOP_MAX_B || hops < 0 || hops > KHOP_MAX_HOPS) return 0;
  return khop_edge_carve(nullptr, r, nq, hops).bytes;
}

// the arguments of rarc_khop_edges and rarc_khop_path_edges, which are the same: leaves `ws`, `ews`, W, H, level_stride and `listed`
#define KHOP_EDGE_CHECKS(NAME)                                                                                                           \
  const bool listed = d_out_ids || d_out_levels || d_out_count; /* all three, or the level counts alone */                               \
  RARC_REQUIRE(d_ws && d_rel && d_ews && d_out_level_counts && (!listed || (d_out_ids && d_out_levels && d_out_count)), RARC_E_INVALID,  \
               NAME ": null pointer");                                                                                                   \
  RARC_REQUIRE(KHOP_ALIGNED(d_rel, 8) && KHOP_ALIGNED(d_out_ids, 8) && KHOP_ALIGNED(d_out_levels, 4) && KHOP_ALIGNED(d_out_count, 4) &&  \
                   KHOP_ALIGNED(d_out_level_counts, 4),                                                                                  \
               RARC_E_INVALID, NAME ": an array is not aligned to its element (relations and ids 8 bytes, levels and counts 4)");        \
  KHOP_SHAPE_CHECKS(NAME);                                                                                                               \
  RARC_REQUIRE(khop_rows_ok(r), RARC_E_INVALID, NAME ": r=%lld relation rows out of range (1 <= r < 2^31 - 1)", (long long)r);           \
  RARC_REQUIRE(max_edges >= 1, RARC_E_INVALID, NAME ": max_edges=%d out of range (1 <= max_edges <= %d)", max_edges, KHOP_MAX_EDGES);    \
  RARC_REQUIRE(max_edges <= KHOP_MAX_EDGES, RARC_E_UNSUPPORTED,                                                                          \
               NAME ": max_edges=%d: a list holds at most %d relations (the level counts say how many there are)", max_edges,            \
               KHOP_MAX_EDGES);                                                                                                          \
  RARC_REQUIRE(KHOP_ALIGNED(d_ews, 256), RARC_E_INVALID, NAME ": the edge workspace is not 256-byte aligned");                           \
  const KhopEdgeWs ews = khop_edge_carve(d_ews, r, nq, hops);                                                                            \
  RARC_REQUIRE(ews_bytes >= ews.bytes, RARC_E_WORKSPACE, NAME ": edge workspace of %zu bytes, %zu needed", ews_bytes, ews.bytes)

// count / scan / write over the rows of the table, against the state in `ws`; PATHS: by the rule of the connecting paths
// TYPED: a row answers only the queries whose filter holds its type (`ty`)
template <bool PATHS, bool TYPED = false>
static int khop_edges_run(const KhopWs& ws, const KhopEdgeWs& ews, size_t level_stride, int64_t n, int nq, int W, int H, const int64_t* d_rel,
                          int64_t r, int max_edges, bool listed, int64_t* d_out_ids, int32_t* d_out_levels, int32_t* d_out_count,
                          int32_t* d_out_level_counts, hipStream_t s, const KhopRowTypes ty = {}) {
  const KhopEdgeBits src = {d_rel, ws.seen, ws.level, level_stride, r, n};
  const int64_t tiles = khop_tiles(r);
  if constexpr (TYPED)
    hipLaunchKernelGGL(khop_edge_count_typed_kernel<PATHS>, dim3(lv_grid(tiles * W, 4, 16384)), dim3(256), 0, s, src, W, H, nq, ews.tiles, ty);
  else hipLaunchKernelGGL(khop_edge_count_kernel<PATHS>, dim3(lv_grid(tiles * W, 4, 16384)), dim3(256), 0, s, src, W, H, ews.tiles);
  hipLaunchKernelGGL(khop_tile_scan_kernel, dim3((H * nq + 255) / 256), dim3(256), 0, s, tiles, W, H, nq, ews.tiles, ews.totals);
  if (listed) {
    RARC_HIP_CHECK(hipMemsetAsync(d_out_ids, 0xFF, (size_t)nq * max_edges * 8, s));            // (-1, -1) past the count
    RARC_HIP_CHECK(hipMemsetAsync(d_out_levels, 0xFF, (size_t)nq * max_edges * 4, s));
    if constexpr (TYPED)
      hipLaunchKernelGGL(khop_list_typed_kernel<PATHS>, dim3(lv_grid(tiles * W, 4, 16384)), dim3(256), 0, s, (const u64*)ws.level, level_stride, n,
                         W, H, nq, (const uint32_t*)ews.tiles, (const int32_t*)ews.totals, (uint32_t)max_edges, d_out_ids, d_out_levels,
                         d_out_count, KhopRelations{d_rel, ws.seen, r}, ty);
    else
      hipLaunchKernelGGL((khop_list_kernel<true, PATHS>), dim3(lv_grid(tiles * W, 4, 16384)), dim3(256), 0, s, (const u64*)ws.level, level_stride, n,
                         W, H, nq, (const uint32_t*)ews.tiles, (const int32_t*)ews.totals, (uint32_t)max_edges, d_out_ids, d_out_levels,
                         d_out_count, KhopRelations{d_rel, ws.seen, r});
  }
  RARC_HIP_CHECK(hipGetLastError());
  RARC_HIP_CHECK(hipMemcpyAsync(d_out_level_counts, ews.totals, (size_t)nq * H * 4, hipMemcpyDeviceToDevice, s));
  return RARC_OK;
}

extern "C" int rarc_khop_edges(int64_t n, int64_t m, int nq, int hops, const void* d_ws, size_t ws_bytes, const int64_t* d_rel, int64_t r,
                               int max_edges, void* d_ews, size_t ews_bytes, int64_t* d_out_ids, int32_t* d_out_levels, int32_t* d_out_count,
                               int32_t* d_out_level_counts, void* stream) {
  RARC_RANGE();
  KHOP_EDGE_CHECKS("rarc_khop_edges");
  return khop_edges_run<false>(ws, ews, level_stride, n, nq, W, H, d_rel, r, max_edges, listed, d_out_ids, d_out_levels, d_out_count,
                               d_out_level_counts, (hipStream_t)stream);
}

// what the typed forms add to KHOP_EDGE_CHECKS
#define KHOP_ROW_TYPE_CHECKS(NAME)                                                                                                        \
  RARC_REQUIRE(d_rel_types && d_filters, RARC_E_INVALID, NAME ": null pointer");                                                         \
  RARC_REQUIRE(KHOP_ALIGNED(d_rel_types, 4) && KHOP_ALIGNED(d_filters, 4), RARC_E_INVALID,                                               \
               NAME ": the row types or the filters are not 4-byte aligned");                                                            \
  RARC_REQUIRE(rel_masks == 0 || rel_masks == 1, RARC_E_INVALID, NAME ": rel_masks=%d out of range (0: a type id per row, 1: a mask)",   \
               rel_masks)

extern "C" int rarc_khop_edges_typed(int64_t n, int64_t m, int nq, int hops, const void* d_ws, size_t ws_bytes, const int64_t* d_rel, int64_t r,
                                     const int32_t* d_rel_types, int rel_masks, const uint32_t* d_filters, int max_edges, void* d_ews,
                                     size_t ews_bytes, int64_t* d_out_ids, int32_t* d_out_levels, int32_t* d_out_count,
                                     int32_t* d_out_level_counts, void* stream) {
  RARC_RANGE();
  KHOP_ROW_TYPE_CHECKS("rarc_khop_edges_typed");
  KHOP_EDGE_CHECKS("rarc_khop_edges_typed");
  return khop_edges_run<false, true>(ws, ews, level_stride, n, nq, W, H, d_rel, r, max_edges, listed, d_out_ids, d_out_levels, d_out_count,
                                     d_out_level_counts, (hipStream_t)stream, KhopRowTypes{d_rel_types, d_filters, rel_masks});
}

// ---- connecting paths: the entries -------------------------------------------------------------------------------------------------
extern "C" int rarc_khop_paths_limits(int* out3) {
  RARC_REQUIRE(out3, RARC_E_INVALID, "rarc_khop_paths_limits: null pointer");
  out3[0] = KHOP_MAX_HOPS;
  out3[1] = KHOP_MAX_B;
  out3[2] = KHOP_MAX_B;
  return RARC_OK;
}

extern "C" int rarc_khop_paths(int64_t n, int64_t m, int ns, int np, int max_length, const void* d_ws, size_t ws_bytes, const int32_t* d_pairs,
                               void* d_pws, size_t pws_bytes, int32_t* d_out_dist, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_ws && d_pairs && d_pws && d_out_dist, RARC_E_INVALID, "rarc_khop_paths: null pointer");
  RARC_REQUIRE(KHOP_ALIGNED(d_pairs, 4) && KHOP_ALIGNED(d_out_dist, 4), RARC_E_INVALID,
               "rarc_khop_paths: the pairs or the distances are not 4-byte aligned");
  RARC_REQUIRE(np >= 1 && np <= KHOP_MAX_B, RARC_E_INVALID, "rarc_khop_paths: %d pairs out of range (1 <= np <= %d per call)", np, KHOP_MAX_B);
  const int nq = ns, hops = max_length;                                // the traversal: ns columns stepped to max_length
  KHOP_SHAPE_CHECKS("rarc_khop_paths");
  RARC_REQUIRE(KHOP_ALIGNED(d_pws, 256), RARC_E_INVALID, "rarc_khop_paths: the path workspace is not 256-byte aligned");
  const KhopWs pws = khop_carve(d_pws, n, np, hops);
  RARC_REQUIRE(pws_bytes >= pws.bytes, RARC_E_WORKSPACE, "rarc_khop_paths: path workspace of %zu bytes, %zu needed", pws_bytes, pws.bytes);
  hipStream_t s = (hipStream_t)stream;
  RARC_HIP_CHECK(hipMemsetAsync(pws.grew, 0, KHOP_CTL_BYTES, s));
  RARC_HIP_CHECK(hipMemsetAsync(d_out_dist, 0xFF, (size_t)np * 4, s));                         // -1 until a vertex joins the pair
  hipLaunchKernelGGL(khop_path_dist_kernel, dim3(lv_grid(n, 256, 16384)), dim3(256), 0, s, (const u64*)ws.level, level_stride, n, W, H, ns, d_pairs,
                     np, (uint32_t*)d_out_dist);
  KhopPathArgs a;
  a.seen = ws.seen;
  a.level = ws.level;
  a.pseen = pws.seen;
  a.plevel = pws.level;
  a.pairs = d_pairs;
  a.dist = d_out_dist;
  a.level_stride = level_stride;
  a.plevel_stride = lv_align(pws.level_words * 8) / 8;
  a.n = n;
  a.W = W;
  a.PW = khop_words(np);
  a.H = H;
  a.ns = ns;
  a.np = np;
  hipLaunchKernelGGL(khop_path_mark_kernel, dim3(lv_grid(n, 4, 16384)), dim3(256), 0, s, a);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_khop_path_edges(int64_t n, int64_t m, int nq, int hops, const void* d_ws, size_t ws_bytes, const int64_t* d_rel, int64_t r,
                                    int max_edges, void* d_ews, size_t ews_bytes, int64_t* d_out_ids, int32_t* d_out_levels,
                                    int32_t* d_out_count, int32_t* d_out_level_counts, void* stream) {
  RARC_RANGE();
  KHOP_EDGE_CHECKS("rarc_khop_path_edges");
  return khop_edges_run<true>(ws, ews, level_stride, n, nq, W, H, d_rel, r, max_edges, listed, d_out_ids, d_out_levels, d_out_count,
                              d_out_level_counts, (hipStream_t)stream);
}

extern "C" int rarc_khop_path_edges_typed(int64_t n, int64_t m, int nq, int hops, const void* d_ws, size_t ws_bytes, const int64_t* d_rel,
                                          int64_t r, const int32_t* d_rel_types, int rel_masks, const uint32_t* d_filters, int max_edges,
                                          void* d_ews, size_t ews_bytes, int64_t* d_out_ids, int32_t* d_out_levels, int32_t* d_out_count,
                                          int32_t* d_out_level_counts, void* stream) {
  RARC_RANGE();
  KHOP_ROW_TYPE_CHECKS("rarc_khop_path_edges_typed");
  KHOP_EDGE_CHECKS("rarc_khop_path_edges_typed");
  return khop_edges_run<true, true>(ws, ews, level_stride, n, nq, W, H, d_rel, r, max_edges, listed, d_out_ids, d_out_levels, d_out_count,
                                    d_out_level_counts, (hipStream_t)stream, KhopRowTypes{d_rel_types, d_filters, rel_masks});
}

extern "C" int rarc_khop_chunks(int64_t n, int64_t m, int nq, int hops, const uint32_t* decay, const void* d_ws, size_t ws_bytes,
                                const int64_t* d_row_ptr, const int32_t* d_ent, const uint32_t* d_w, int64_t n_chunks, int64_t nnz,
                                const int32_t* d_split, int64_t n_split, void* d_cws, size_t cws_bytes, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(decay && d_ws && d_row_ptr && d_ent && d_w && d_cws && (d_split || n_split == 0), RARC_E_INVALID, "rarc_khop_chunks: null pointer");
  RARC_REQUIRE(KHOP_ALIGNED(d_row_ptr, 8) && KHOP_ALIGNED(d_ent, 4) && KHOP_ALIGNED(d_w, 4) && KHOP_ALIGNED(d_split, 4), RARC_E_INVALID,
               "rarc_khop_chunks: a mention array is not aligned to its element (row_ptr 8 bytes, entities, weights and the split list 4)");
  KHOP_SHAPE_CHECKS("rarc_khop_chunks");
  RARC_REQUIRE(n_chunks >= 1 && n_chunks < PPR_CHUNK_N_LIMIT, RARC_E_INVALID, "rarc_khop_chunks: n_chunks=%lld out of range (1 <= n_chunks < 2^31 - 1)",
               (long long)n_chunks);
  RARC_REQUIRE(KHOP_ALIGNED(d_cws, 256), RARC_E_INVALID, "rarc_khop_chunks: the chunk workspace is not 256-byte aligned");
  const PprChunkWs cws = ppr_chunk_carve(d_cws, n_chunks, nq);
  RARC_REQUIRE(cws_bytes >= cws.bytes, RARC_E_WORKSPACE, "rarc_khop_chunks: chunk workspace of %zu bytes, %zu needed", cws_bytes, cws.bytes);
  RARC_REQUIRE(nnz >= 1, RARC_E_INVALID, "rarc_khop_chunks: nnz=%lld mentions out of range (nnz >= 1)", (long long)nnz);
  RARC_REQUIRE(n_split >= 0 && n_split <= n_chunks, RARC_E_INVALID, "rarc_khop_chunks: %lld split chunks out of range (0 <= n_split <= n_chunks)",
               (long long)n_split);
  KhopChunkArgs a;
  for (int h = 0; h <= KHOP_MAX_HOPS; ++h) {                           // `decay` is a host array of hops + 1 words
    a.decay[h] = h < H ? decay[h] : 0u;
    RARC_REQUIRE(a.decay[h] <= KHOP_MAX_DECAY, RARC_E_INVALID, "rarc_khop_chunks: decay[%d]=%u out of range (0 <= decay <= 2^16 = %u)", h,
                 a.decay[h], KHOP_MAX_DECAY);
  }
  hipStream_t s = (hipStream_t)stream;
  a.row_ptr = d_row_ptr;
  a.ent = d_ent;
  a.w = d_w;
  a.level = ws.level;
  a.s = cws.s;
  a.level_stride = level_stride;
  a.n = n;
  a.n_chunks = n_chunks;
  a.nnz = nnz;
  a.W = W;
  a.H = H;
  a.nq = nq;
  hipLaunchKernelGGL(khop_chunks_kernel<false>, dim3(lv_grid(n_chunks * W, 4, 16384)), dim3(256), 0, s, a, (const int32_t*)nullptr, (int64_t)0);
  if (n_split > 0)
    hipLaunchKernelGGL(khop_chunks_kernel<true>, dim3(lv_grid(n_split * W, 1, 2048)), dim3(256), 0, s, a, d_split, n_split);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}
