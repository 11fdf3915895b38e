// merge.hip — entity merging: step 4 of the reference's entity de-duplication
// (encapsulation/database/graph_db/Base_Neo4j.py:714-890, _merge_clusters: pick the richest member of a cluster as the primary,
// move every relationship of the others onto it, DETACH DELETE the others).  The clusters are found on the device
// (csrc/louvain.hip) and the merged graph is queried there (csrc/ppr.hip, csrc/khop.hip); the kernels here contract the pair list,
// the mention CSR and the relation table in between, so nothing leaves HBM.
//
// The primitive is rarc_sort_reduce: sort 64-bit keys, merge equal keys, add their values — np.unique + bincount.  An LSD radix
// sort, 8 bits a pass, over ceil(key_bits / 8) passes; a pass is {per-tile histogram, scan of the histograms, scatter with ranks
// that are stable within the tile}.  Then {flag heads, scan, segmented sum into place}.  Every sum is an integer sum and every
// position comes from a scan: the answer is the same bits for any order of the input and from run to run.
//
// A tile is 2048 keys, a workgroup of 256 threads, 32 chunks of 64 keys: a wave ranks the keys of a chunk among themselves with
// ballots (rank = equal digits in lower lanes), the chunk's digit counts go to LDS [32][256], a scan down the chunks per digit
// makes them the chunk's base — so a key's place is (digit's global base of this tile) + (chunk's base) + (rank in chunk), in
// index order: stable.
//
// Every kernel takes its length twice: `cap`, what the host knows (grids and workspaces are sized by it), and `d_len`, a device
// word holding the real length <= cap, or null for "cap".  A compaction (pairs that fell inside an entity are left out) feeds the
// sort without the host reading a count in between.
#include "chunk_ws.h"       // lv_align / lv_grid, the limits on n and n_chunks, the bits of a mention weight

typedef unsigned long long u64;

constexpr int MG_TILE = 2048;                               // keys per tile: 256 threads x 8
constexpr int MG_CHUNKS = MG_TILE / 64;                     // 32 chunks of one wave's width
constexpr int MG_RADIX_BITS = 8;
constexpr int MG_BINS = 1 << MG_RADIX_BITS;
constexpr int MG_MAX_KEY_BITS = 62;
constexpr int64_t MG_COUNT_LIMIT = 1ll << 31;               // count < 2^31: every position fits uint32, count * 2^32 fits 64 bits
constexpr int MG_SPLIT_DEGREE = LV_DEG_WAVE;                // rarc_ppr_chunks_limits' split degree
constexpr size_t MG_CTL_BYTES = 256;
enum { MG_C_LEN = 0, MG_C_DISTINCT = 1, MG_C_MAX = 2, MG_C_DROPPED = 3, MG_C_DROPPED_W = 4, MG_C_BAD = 5, MG_C_SPLIT = 6, MG_C_WORDS = 8 };

static inline int64_t mg_tiles(int64_t n) { return (n + MG_TILE - 1) / MG_TILE; }
static inline int mg_passes(int key_bits) { return (key_bits + MG_RADIX_BITS - 1) / MG_RADIX_BITS; }
static inline int mg_bits(int64_t x) {                      // bits that hold every value of [0, x): at least 1
  int b = 1;
  while (b < 63 && (1ll << b) < x) ++b;
  return b;
}
__device__ __forceinline__ int64_t mg_len(const int64_t* d_len, int64_t cap) {
  if (!d_len) return cap;
  const int64_t l = *d_len;
  return l < 0 ? 0 : (l > cap ? cap : l);
}

// ---- block-wide helpers (256 threads) -------------------------------------------------------------------------------------------
// inclusive scan of one value per thread over the block (s: 256 words of LDS)
__device__ __forceinline__ u64 mg_block_scan(u64 x, u64* s) {
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

// ---- exclusive scan of n uint32 (tile sums, one block over the sums, tiles again); out[n] = the total ------------------------------
__global__ __launch_bounds__(256) void mg_scan_sums_kernel(const uint32_t* __restrict__ in, int64_t n, u64* __restrict__ bsum) {
  __shared__ u64 s[256];
  const int64_t base = (int64_t)blockIdx.x * MG_TILE + (int64_t)threadIdx.x * 8;
  u64 acc = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (base + j < n) acc += in[base + j];
  const u64 incl = mg_block_scan(acc, s);
  if (threadIdx.x == 255) bsum[blockIdx.x] = incl;
}
__global__ __launch_bounds__(256) void mg_scan_offsets_kernel(u64* bsum, int64_t nb) {
  __shared__ u64 s[256];
  u64 carry = 0;
  for (int64_t base = 0; base < nb; base += 256) {
    const int64_t i = base + threadIdx.x;
    const u64 x = i < nb ? bsum[i] : 0;
    const u64 incl = mg_block_scan(x, s);
    if (i < nb) bsum[i] = carry + incl - x;
    if (threadIdx.x == 255) s[0] = incl;
    __syncthreads();
    carry += s[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) bsum[nb] = carry;
}
// OUT: uint32_t (positions, totals below 2^31) or int64_t (a CSR's row_ptr); in and out may be the same array when OUT is uint32_t
// and the total is not asked for in place (each block reads its tile before it writes it)
template <typename OUT>
__global__ __launch_bounds__(256) void mg_scan_apply_kernel(const uint32_t* in, int64_t n, const u64* __restrict__ bsum, OUT* out, bool total,
                                                            int64_t* total_out) {
  __shared__ u64 s[256];
  const int64_t base = (int64_t)blockIdx.x * MG_TILE + (int64_t)threadIdx.x * 8;
  uint32_t x[8];
  u64 acc = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    x[j] = base + j < n ? in[base + j] : 0u;
    acc += x[j];
  }
  u64 run = bsum[blockIdx.x] + mg_block_scan(acc, s) - acc;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (base + j < n) out[base + j] = (OUT)run;
    run += x[j];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    if (total) out[n] = (OUT)bsum[gridDim.x];
    if (total_out) *total_out = (int64_t)bsum[gridDim.x];
  }
}
// n >= 1.  `total`: out has n + 1 slots and out[n] receives the sum; total_out: a device word that receives it too, or null
template <typename OUT>
static void mg_scan(const uint32_t* in, int64_t n, u64* bsum, OUT* out, bool total, int64_t* total_out, hipStream_t s) {
  const int64_t nb = mg_tiles(n);
  hipLaunchKernelGGL(mg_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, s, in, n, bsum);
  hipLaunchKernelGGL(mg_scan_offsets_kernel, dim3(1), dim3(256), 0, s, bsum, nb);
  hipLaunchKernelGGL(mg_scan_apply_kernel<OUT>, dim3((unsigned)nb), dim3(256), 0, s, in, n, (const u64*)bsum, out, total, total_out);
}

// ---- the radix sort ---------------------------------------------------------------------------------------------------------------
// hist[digit * tiles + tile] = the keys of the tile with that digit: digit-major, so one exclusive scan of the whole array is
// every (digit, tile)'s first position
__global__ __launch_bounds__(256) void mg_hist_kernel(const u64* __restrict__ keys, int64_t cap, const int64_t* __restrict__ d_len, int shift,
                                                      int64_t tiles, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_h[MG_BINS];
  const int64_t len = mg_len(d_len, cap);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = tile * MG_TILE;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t i = base + j * 256 + threadIdx.x;
      if (i < len) atomicAdd(&s_h[(uint32_t)(keys[i] >> shift) & (MG_BINS - 1)], 1u);
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * tiles + tile] = s_h[threadIdx.x];
    __syncthreads();
  }
}

// vals == nullptr: every value is 1
__global__ __launch_bounds__(256) void mg_scatter_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t cap,
                                                         const int64_t* __restrict__ d_len, int shift, int64_t tiles,
                                                         const uint32_t* __restrict__ offs, u64* __restrict__ out_keys,
                                                         uint32_t* __restrict__ out_vals) {
  __shared__ uint32_t s_cnt[MG_CHUNKS][MG_BINS];
  __shared__ uint32_t s_base[MG_BINS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t len = mg_len(d_len, cap);
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
    for (int c = 0; c < MG_CHUNKS; ++c) s_cnt[c][threadIdx.x] = 0;
    s_base[threadIdx.x] = offs[(int64_t)threadIdx.x * tiles + tile];
    __syncthreads();
    u64 k[8];
    uint32_t v[8], dg[8], rk[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {                                      // this wave's chunks: wave, wave + 4, ...
      const int c = j * 4 + wave;
      const int64_t i = tile * MG_TILE + c * 64 + lane;
      const bool valid = i < len;
      k[j] = valid ? keys[i] : 0ull;
      v[j] = valid ? (vals ? vals[i] : 1u) : 0u;
      dg[j] = (uint32_t)(k[j] >> shift) & (MG_BINS - 1);
      u64 same = __builtin_amdgcn_ballot_w64(valid);                   // the valid lanes of the chunk with this lane's digit
#pragma unroll
      for (int b = 0; b < MG_RADIX_BITS; ++b) {
        const u64 has = __builtin_amdgcn_ballot_w64(valid && ((dg[j] >> b) & 1u));
        same &= ((dg[j] >> b) & 1u) ? has : ~has;
      }
      rk[j] = (uint32_t)__builtin_popcountll(same & below);
      if (valid && rk[j] == 0) s_cnt[c][dg[j]] = (uint32_t)__builtin_popcountll(same);
    }
    __syncthreads();
    uint32_t run = 0;                                                  // thread d: digit d's counts down the chunks -> bases
#pragma unroll
    for (int c = 0; c < MG_CHUNKS; ++c) {
      const uint32_t x = s_cnt[c][threadIdx.x];
      s_cnt[c][threadIdx.x] = run;
      run += x;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = j * 4 + wave;
      const int64_t i = tile * MG_TILE + c * 64 + lane;
      if (i < len) {
        const int64_t at = (int64_t)s_base[dg[j]] + s_cnt[c][dg[j]] + rk[j];
        if (at < len) {                                                // (always, when offs is the scan of this pass's histogram)
          out_keys[at] = k[j];
          out_vals[at] = v[j];
        }
      }
    }
    __syncthreads();
  }
}

// ---- the reduction of equal keys -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mg_head_kernel(const u64* __restrict__ keys, int64_t cap, const int64_t* __restrict__ d_len,
                                                      uint32_t* __restrict__ flag) {
  const int64_t len = mg_len(d_len, cap);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += (int64_t)gridDim.x * 256)
    flag[i] = i < len && (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void mg_clear_kernel(u64* p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0;
}
// segment of element i = pos[i] + flag[i] - 1 (pos: the exclusive scan of the head flags).  A wave adds up each run of one
// segment among its lanes with shuffles; the first lane of a run adds the run to the segment's sum: integer adds, any order
__global__ __launch_bounds__(256) void mg_segsum_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t cap,
                                                        const int64_t* __restrict__ d_len, const uint32_t* __restrict__ flag,
                                                        const uint32_t* __restrict__ pos, u64* out_keys, u64* out_sums) {
  const int lane = threadIdx.x & 63;
  const int64_t len = mg_len(d_len, cap);
  const int64_t rounds = (len + (int64_t)gridDim.x * 256 - 1) / ((int64_t)gridDim.x * 256);
  for (int64_t r = 0; r < rounds; ++r) {                               // (every lane of a wave makes every round: the shuffles need them)
    const int64_t i = (r * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    const bool valid = i < len;
    const uint32_t f = valid ? flag[i] : 0u;
    const long long seg = valid ? (long long)pos[i] + f - 1 : -1;
    u64 sum = valid ? (u64)vals[i] : 0ull;
    if (valid && f) out_keys[seg] = keys[i];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u64 o = __shfl_down(sum, d, 64);
      const long long os = __shfl_down(seg, d, 64);
      if (lane + d < 64 && os == seg) sum += o;
    }
    const long long before = __shfl_up(seg, 1, 64);
    if (valid && seg >= 0 && (lane == 0 || before != seg)) atomicAdd(&out_sums[seg], sum);
  }
}
__global__ __launch_bounds__(256) void mg_max_kernel(const u64* __restrict__ sums, int64_t cap, const int64_t* __restrict__ d_distinct, u64* out_max) {
  const int64_t len = mg_len(d_distinct, cap);
  u64 mx = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) mx = sums[i] > mx ? sums[i] : mx;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 o = __shfl_down(mx, d, 64);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & 63) == 0 && mx) atomicMax(out_max, mx);
}

struct MgSortWs {
  int64_t* ctl;
  u64* key[2];
  uint32_t* val[2];
  uint32_t* hist;
  uint32_t* flag;
  uint32_t* pos;
  u64* bsum;
  size_t bytes;
};
static MgSortWs mg_sort_carve(const void* base, int64_t cap) {
  char* b = (char*)base;
  size_t o = 0;
  MgSortWs w;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  const int64_t tiles = mg_tiles(cap);
  w.ctl = (int64_t*)take(MG_CTL_BYTES);
  for (int i = 0; i < 2; ++i) w.key[i] = (u64*)take((size_t)cap * 8);
  for (int i = 0; i < 2; ++i) w.val[i] = (uint32_t*)take((size_t)cap * 4);
  w.hist = (uint32_t*)take((size_t)tiles * MG_BINS * 4);
  w.flag = (uint32_t*)take((size_t)cap * 4);
  w.pos = (uint32_t*)take((size_t)(cap + 1) * 4);
  const int64_t hist_blocks = mg_tiles(tiles * MG_BINS);
  w.bsum = (u64*)take((size_t)((hist_blocks > tiles ? hist_blocks : tiles) + 1) * 8);
  w.bytes = o;
  return w;
}

// keys / vals: `cap` slots of which the first *d_len (null: cap) are taken; they are only read.  out_keys, out_sums: cap slots.
// ctl[MG_C_DISTINCT] and ctl[MG_C_MAX] receive the number of distinct keys and the largest sum.  Launches only.
static void mg_sort_reduce(const u64* keys, const uint32_t* vals, int64_t cap, const int64_t* d_len, int key_bits, const MgSortWs& w,
                           u64* out_keys, u64* out_sums, hipStream_t s) {
  const int64_t tiles = mg_tiles(cap);
  const unsigned tile_grid = lv_grid(tiles, 1, 65536), flat_grid = lv_grid(cap, 256, 16384);
  const u64* src_k = keys;
  const uint32_t* src_v = vals;
  for (int p = 0; p < mg_passes(key_bits); ++p) {
    hipLaunchKernelGGL(mg_hist_kernel, dim3(tile_grid), dim3(256), 0, s, src_k, cap, d_len, p * MG_RADIX_BITS, tiles, w.hist);
    mg_scan<uint32_t>(w.hist, tiles * MG_BINS, w.bsum, w.hist, false, nullptr, s);
    hipLaunchKernelGGL(mg_scatter_kernel, dim3(tile_grid), dim3(256), 0, s, src_k, src_v, cap, d_len, p * MG_RADIX_BITS, tiles,
                       (const uint32_t*)w.hist, w.key[p & 1], w.val[p & 1]);
    src_k = w.key[p & 1];
    src_v = w.val[p & 1];
  }
  hipLaunchKernelGGL(mg_head_kernel, dim3(flat_grid), dim3(256), 0, s, src_k, cap, d_len, w.flag);
  mg_scan<uint32_t>(w.flag, cap, w.bsum, w.pos, true, &w.ctl[MG_C_DISTINCT], s);
  hipLaunchKernelGGL(mg_clear_kernel, dim3(flat_grid), dim3(256), 0, s, out_sums, cap);
  hipLaunchKernelGGL(mg_segsum_kernel, dim3(flat_grid), dim3(256), 0, s, src_k, src_v, cap, d_len, (const uint32_t*)w.flag,
                     (const uint32_t*)w.pos, out_keys, out_sums);
  hipLaunchKernelGGL(mg_max_kernel, dim3(flat_grid), dim3(256), 0, s, (const u64*)out_sums, cap, (const int64_t*)&w.ctl[MG_C_DISTINCT],
                     (u64*)&w.ctl[MG_C_MAX]);
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool mg_label_ok(int64_t c, int64_t n) { return c >= 0 && c < n; }

__global__ __launch_bounds__(256) void mg_plan_best_kernel(const int64_t* __restrict__ labels, const uint32_t* __restrict__ rich, int64_t n, u64* best) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    const int64_t c = labels[v];
    if (mg_label_ok(c, n)) atomicMax(&best[c], ((u64)(rich ? rich[v] : 0u) << 32) | (u64)(~(uint32_t)v));
  }
}
// a label outside [0, n): the vertex is a class of its own
__global__ __launch_bounds__(256) void mg_plan_primary_kernel(const int64_t* __restrict__ labels, int64_t n, const u64* __restrict__ best,
                                                              int64_t* __restrict__ primary, uint32_t* __restrict__ flag) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    const int64_t c = labels[v];
    int64_t p = mg_label_ok(c, n) ? (int64_t)(~(uint32_t)best[c]) : v;
    if (p < 0 || p >= n) p = v;                                        // (never: best[c] was raised by a member of c)
    primary[v] = p;
    flag[v] = p == v ? 1u : 0u;
  }
}
__global__ __launch_bounds__(256) void mg_plan_write_kernel(int64_t n, const int64_t* __restrict__ primary, const uint32_t* __restrict__ flag,
                                                            const uint32_t* __restrict__ pos, int64_t* __restrict__ new_id,
                                                            int64_t* __restrict__ kept, int64_t* __restrict__ removed) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    new_id[v] = pos[primary[v]];
    if (flag[v]) kept[pos[v]] = v;
    else removed[v - (int64_t)pos[v]] = v;                             // the non-primaries before v: v - (the primaries before v)
  }
}

struct MgPlanWs {
  u64* best;
  uint32_t* flag;
  uint32_t* pos;
  u64* bsum;
  size_t bytes;
};
static MgPlanWs mg_plan_carve(const void* base, int64_t n) {
  char* b = (char*)base;
  size_t o = 0;
  MgPlanWs w;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  w.best = (u64*)take((size_t)n * 8);
  w.flag = (uint32_t*)take((size_t)n * 4);
  w.pos = (uint32_t*)take((size_t)(n + 1) * 4);
  w.bsum = (u64*)take((size_t)(mg_tiles(n) + 1) * 8);
  w.bytes = o;
  return w;
}

// ---- pairs and mentions: map to packed keys, leave out what falls away, sort and reduce, unpack ---------------------------------------
// an id the map cannot take (outside [0, n), or mapped outside [0, n)) is counted as bad and left out: no index leaves its buffer
__device__ __forceinline__ int64_t mg_map(const int64_t* __restrict__ new_id, int64_t n, int64_t v) {
  if (v < 0 || v >= n) return -1;
  const int64_t x = new_id[v];
  return x >= 0 && x < n ? x : -1;
}
__device__ __forceinline__ void mg_count(bool mine, u64 weight, int64_t* counter, int64_t* weights) {
  const u64 mask = __builtin_amdgcn_ballot_w64(mine);
  if (!mask) return;
  u64 wsum = mine ? weight : 0ull;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) wsum += __shfl_down(wsum, d, 64);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd((u64*)counter, (u64)__builtin_popcountll(mask));
    if (weights) atomicAdd((u64*)weights, wsum);
  }
}

__global__ __launch_bounds__(256) void mg_pair_key_kernel(const int64_t* __restrict__ pairs, const uint32_t* __restrict__ w, int64_t m,
                                                          const int64_t* __restrict__ new_id, int64_t n, int lo_bits,
                                                          u64* __restrict__ keys, uint32_t* __restrict__ flag, int64_t* ctl) {
  const int64_t rounds = (m + (int64_t)gridDim.x * 256 - 1) / ((int64_t)gridDim.x * 256);
  for (int64_t r = 0; r < rounds; ++r) {
    const int64_t e = (r * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    const bool valid = e < m;
    const int64_t a = valid ? mg_map(new_id, n, pairs[2 * e]) : -1, b = valid ? mg_map(new_id, n, pairs[2 * e + 1]) : -1;
    const bool bad = valid && (a < 0 || b < 0), inside = valid && !bad && a == b, keep = valid && !bad && !inside;
    if (valid) {
      keys[e] = keep ? ((u64)(a < b ? a : b) << lo_bits) | (u64)(a < b ? b : a) : 0ull;
      flag[e] = keep ? 1u : 0u;
    }
    mg_count(inside, valid ? (u64)(w ? w[e] : 1u) : 0ull, &ctl[MG_C_DROPPED], &ctl[MG_C_DROPPED_W]);
    mg_count(bad, 0, &ctl[MG_C_BAD], nullptr);
  }
}
// the flagged (key, value) of slot e moves to slot pos[e]; w == nullptr: every value is 1
__global__ __launch_bounds__(256) void mg_compact_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ w, int64_t m,
                                                         const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                         u64* __restrict__ out_keys, uint32_t* __restrict__ out_vals) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256)
    if (flag[e]) {
      out_keys[pos[e]] = keys[e];
      out_vals[pos[e]] = w ? w[e] : 1u;
    }
}
__global__ __launch_bounds__(256) void mg_pair_unpack_kernel(const u64* __restrict__ keys, const u64* __restrict__ sums, int64_t cap,
                                                             const int64_t* __restrict__ d_len, int lo_bits, int64_t* __restrict__ out_pairs,
                                                             uint32_t* __restrict__ out_w) {
  const int64_t len = mg_len(d_len, cap);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) {
    out_pairs[2 * i] = (int64_t)(keys[i] >> lo_bits);
    out_pairs[2 * i + 1] = (int64_t)(keys[i] & ((1ull << lo_bits) - 1ull));
    out_w[i] = (uint32_t)sums[i];                                      // (the caller narrows: the largest sum is reported)
  }
}

// a wave per chunk; its mentions, clamped as rarc_ppr_chunks clamps them, become (chunk << bits(n) | new entity) in their own slots
__global__ __launch_bounds__(256) void mg_mention_key_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ ent,
                                                             const uint32_t* __restrict__ w, int64_t n_chunks, int64_t nnz,
                                                             const int64_t* __restrict__ new_id, int64_t n, int lo_bits,
                                                             u64* __restrict__ keys, uint32_t* __restrict__ flag, int64_t* ctl) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t c = (int64_t)blockIdx.x * 4 + wave; c < n_chunks; c += (int64_t)gridDim.x * 4) {
    int64_t r0 = row_ptr[c], r1 = row_ptr[c + 1];
    r0 = r0 < 0 ? 0 : (r0 > nnz ? nnz : r0);
    r1 = r1 < r0 ? r0 : (r1 > nnz ? nnz : r1);
    for (int64_t i0 = r0; i0 < r1; i0 += 64) {                         // (i0 is wave-uniform)
      const int64_t i = i0 + lane;
      const bool valid = i < r1;
      const int64_t e = valid ? mg_map(new_id, n, (int64_t)ent[i]) : -1;
      const bool keep = valid && e >= 0 && w[i] >= 1u;
      if (valid) {
        keys[i] = keep ? ((u64)c << lo_bits) | (u64)e : 0ull;
        flag[i] = keep ? 1u : 0u;
      }
      mg_count(valid && !keep, 0, &ctl[MG_C_BAD], nullptr);
    }
  }
}
// d_skip: a device word holding how many leading keys are left out (the ingest's placeholder key), or null for none
__global__ __launch_bounds__(256) void mg_mention_unpack_kernel(const u64* __restrict__ keys, const u64* __restrict__ sums, int64_t cap,
                                                                const int64_t* __restrict__ d_len, const int64_t* __restrict__ d_skip, int lo_bits,
                                                                int64_t n_chunks, int32_t* __restrict__ out_ent, uint32_t* __restrict__ out_w,
                                                                uint32_t* deg) {
  const int64_t skip = d_skip ? (*d_skip > 0 ? 1 : 0) : 0;
  int64_t len = mg_len(d_len, cap);
  len = len > cap - skip ? cap - skip : len;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) {
    const u64 key = keys[i + skip];
    const int64_t c = (int64_t)(key >> lo_bits);
    out_ent[i] = (int32_t)(key & ((1ull << lo_bits) - 1ull));
    out_w[i] = (uint32_t)sums[i + skip];
    if (c < n_chunks) atomicAdd(&deg[c], 1u);
  }
}
__global__ __launch_bounds__(256) void mg_split_flag_kernel(const uint32_t* __restrict__ deg, int64_t n_chunks, uint32_t* __restrict__ flag) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n_chunks; c += (int64_t)gridDim.x * 256)
    flag[c] = deg[c] > (uint32_t)MG_SPLIT_DEGREE ? 1u : 0u;
}
__global__ __launch_bounds__(256) void mg_split_write_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, int64_t n_chunks,
                                                             int32_t* __restrict__ out_split) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n_chunks; c += (int64_t)gridDim.x * 256)
    if (flag[c]) out_split[pos[c]] = (int32_t)c;
}

// cap slots of unsorted keys in front of the sort's own workspace, and for the mentions the per-chunk arrays behind it
struct MgMapWs {
  u64* raw_keys;
  u64* keys;
  uint32_t* vals;
  u64* red_keys;
  u64* red_sums;
  uint32_t* deg;
  uint32_t* cflag;
  uint32_t* cpos;
  u64* cbsum;
  MgSortWs sort;
  size_t bytes;
};
static MgMapWs mg_map_carve(const void* base, int64_t cap, int64_t n_chunks) {
  char* b = (char*)base;
  size_t o = 0;
  MgMapWs w;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  w.raw_keys = (u64*)take((size_t)cap * 8);
  w.keys = (u64*)take((size_t)cap * 8);
  w.vals = (uint32_t*)take((size_t)cap * 4);
  w.red_keys = (u64*)take((size_t)cap * 8);
  w.red_sums = (u64*)take((size_t)cap * 8);
  w.deg = (uint32_t*)take((size_t)n_chunks * 4);
  w.cflag = (uint32_t*)take((size_t)n_chunks * 4);
  w.cpos = (uint32_t*)take((size_t)(n_chunks + 1) * 4);
  w.cbsum = (u64*)take((size_t)(mg_tiles(n_chunks) + 1) * 8);
  w.sort = mg_sort_carve(b ? b + o : nullptr, cap);
  w.bytes = o + w.sort.bytes;
  return w;
}

// the reduced (chunk << lo_bits | entity) keys, ascending, become the CSR by chunk: entities and weights, the degrees (deg: zeroed by
// the caller), row_ptr and the list of the chunks of more than MG_SPLIT_DEGREE mentions, whose length goes to *d_split_count
static void mg_mention_rows(const u64* red_keys, const u64* red_sums, int64_t cap, const int64_t* d_len, const int64_t* d_skip, int lo_bits,
                            int64_t n_chunks, uint32_t* deg, uint32_t* cflag, uint32_t* cpos, u64* cbsum, int64_t* d_out_row_ptr,
                            int32_t* d_out_ent, uint32_t* d_out_w, int32_t* d_out_split, int64_t* d_split_count, hipStream_t s) {
  const unsigned grid = lv_grid(cap, 256, 16384), cgrid = lv_grid(n_chunks, 256, 16384);
  hipLaunchKernelGGL(mg_mention_unpack_kernel, dim3(grid), dim3(256), 0, s, red_keys, red_sums, cap, d_len, d_skip, lo_bits, n_chunks, d_out_ent,
                     d_out_w, deg);
  mg_scan<int64_t>(deg, n_chunks, cbsum, d_out_row_ptr, true, nullptr, s);
  hipLaunchKernelGGL(mg_split_flag_kernel, dim3(cgrid), dim3(256), 0, s, (const uint32_t*)deg, n_chunks, cflag);
  mg_scan<uint32_t>(cflag, n_chunks, cbsum, cpos, true, d_split_count, s);
  hipLaunchKernelGGL(mg_split_write_kernel, dim3(cgrid), dim3(256), 0, s, (const uint32_t*)cflag, (const uint32_t*)cpos, n_chunks, d_out_split);
}

// ---- relations: map, flag, scan, stable write -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mg_rel_flag_kernel(const int64_t* __restrict__ rel, int64_t r, const int64_t* __restrict__ new_id, int64_t n,
                                                          uint32_t* __restrict__ flag, int64_t* ctl) {
  const int64_t rounds = (r + (int64_t)gridDim.x * 256 - 1) / ((int64_t)gridDim.x * 256);
  for (int64_t k = 0; k < rounds; ++k) {
    const int64_t e = (k * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    const bool valid = e < r;
    const int64_t a0 = valid ? rel[2 * e] : -1, b0 = valid ? rel[2 * e + 1] : -1;
    const int64_t a = valid ? mg_map(new_id, n, a0) : -1, b = valid ? mg_map(new_id, n, b0) : -1;
    const bool bad = valid && (a < 0 || b < 0), inside = valid && !bad && a0 != b0 && a == b;
    if (valid) flag[e] = !bad && !inside ? 1u : 0u;
    mg_count(inside, 0, &ctl[MG_C_DROPPED], nullptr);
    mg_count(bad, 0, &ctl[MG_C_BAD], nullptr);
  }
}
__global__ __launch_bounds__(256) void mg_rel_write_kernel(const int64_t* __restrict__ rel, int64_t r, const int64_t* __restrict__ new_id,
                                                           const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                           int64_t* __restrict__ out_rel, int64_t* __restrict__ out_rows) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < r; e += (int64_t)gridDim.x * 256)
    if (flag[e]) {                                                     // (flagged: both ends were mapped inside [0, n))
      const int64_t at = pos[e];
      out_rel[2 * at] = new_id[rel[2 * e]];
      out_rel[2 * at + 1] = new_id[rel[2 * e + 1]];
      out_rows[at] = e;
    }
}

struct MgRelWs {
  int64_t* ctl;
  uint32_t* flag;
  uint32_t* pos;
  u64* bsum;
  size_t bytes;
};
static MgRelWs mg_rel_carve(const void* base, int64_t r) {
  char* b = (char*)base;
  size_t o = 0;
  MgRelWs w;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  w.ctl = (int64_t*)take(MG_CTL_BYTES);
  w.flag = (uint32_t*)take((size_t)r * 4);
  w.pos = (uint32_t*)take((size_t)(r + 1) * 4);
  w.bsum = (u64*)take((size_t)(mg_tiles(r) + 1) * 8);
  w.bytes = o;
  return w;
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define MG_ALIGNED(P, A) (((uintptr_t)(P) & (uintptr_t)((A)-1)) == 0)
static inline bool mg_count_ok(int64_t count) { return count >= 1 && count < MG_COUNT_LIMIT; }
static inline bool mg_n_ok(int64_t n) { return n >= 1 && n < LV_N_LIMIT; }

extern "C" int rarc_sort_reduce_limits(int* out4) {
  RARC_REQUIRE(out4, RARC_E_INVALID, "rarc_sort_reduce_limits: null pointer");
  out4[0] = MG_TILE;
  out4[1] = MG_RADIX_BITS;
  out4[2] = MG_MAX_KEY_BITS;
  out4[3] = 31;                                                        // count < 2^31
  return RARC_OK;
}

extern "C" size_t rarc_sort_reduce_workspace_bytes(int64_t count) {
  if (!mg_count_ok(count)) return 0;
  return mg_sort_carve(nullptr, count).bytes;
}

extern "C" int rarc_sort_reduce(const uint64_t* d_keys, const uint32_t* d_values, int64_t count, int key_bits, void* d_ws, size_t ws_bytes,
                                uint64_t* d_out_keys, uint64_t* d_out_sums, int64_t* d_out2, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_keys && d_ws && d_out_keys && d_out_sums && d_out2, RARC_E_INVALID, "rarc_sort_reduce: null pointer");
  RARC_REQUIRE(MG_ALIGNED(d_keys, 8) && MG_ALIGNED(d_values, 4) && MG_ALIGNED(d_out_keys, 8) && MG_ALIGNED(d_out_sums, 8) && MG_ALIGNED(d_out2, 8),
               RARC_E_INVALID, "rarc_sort_reduce: an array is not aligned to its element (keys, sums and the counts 8 bytes, values 4)");
  RARC_REQUIRE(mg_count_ok(count), RARC_E_INVALID, "rarc_sort_reduce: count=%lld out of range (1 <= count < 2^31)", (long long)count);
  RARC_REQUIRE(key_bits >= 1 && key_bits <= MG_MAX_KEY_BITS, RARC_E_INVALID, "rarc_sort_reduce: key_bits=%d out of range (1 <= key_bits <= %d)",
               key_bits, MG_MAX_KEY_BITS);
  RARC_REQUIRE(MG_ALIGNED(d_ws, 256), RARC_E_INVALID, "rarc_sort_reduce: the workspace is not 256-byte aligned");
  const MgSortWs w = mg_sort_carve(d_ws, count);
  RARC_REQUIRE(ws_bytes >= w.bytes, RARC_E_WORKSPACE, "rarc_sort_reduce: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  RARC_HIP_CHECK(hipMemsetAsync(w.ctl, 0, MG_CTL_BYTES, s));
  mg_sort_reduce((const u64*)d_keys, d_values, count, nullptr, key_bits, w, (u64*)d_out_keys, (u64*)d_out_sums, s);
  RARC_HIP_CHECK(hipGetLastError());
  RARC_HIP_CHECK(hipMemcpyAsync(d_out2, &w.ctl[MG_C_DISTINCT], 16, hipMemcpyDeviceToDevice, s));
  return RARC_OK;
}

extern "C" size_t rarc_merge_plan_workspace_bytes(int64_t n) {
  if (!mg_n_ok(n)) return 0;
  return mg_plan_carve(nullptr, n).bytes;
}

extern "C" int rarc_merge_plan(const int64_t* d_labels, const uint32_t* d_richness, int64_t n, void* d_ws, size_t ws_bytes, int64_t* d_primary,
                               int64_t* d_new_id, int64_t* d_kept, int64_t* d_removed, int64_t* d_out_count, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_labels && d_ws && d_primary && d_new_id && d_kept && d_removed && d_out_count, RARC_E_INVALID, "rarc_merge_plan: null pointer");
  RARC_REQUIRE(MG_ALIGNED(d_labels, 8) && MG_ALIGNED(d_richness, 4) && MG_ALIGNED(d_primary, 8) && MG_ALIGNED(d_new_id, 8) &&
                   MG_ALIGNED(d_kept, 8) && MG_ALIGNED(d_removed, 8) && MG_ALIGNED(d_out_count, 8),
               RARC_E_INVALID, "rarc_merge_plan: an array is not aligned to its element (richness 4 bytes, every other 8)");
  RARC_REQUIRE(mg_n_ok(n), RARC_E_INVALID, "rarc_merge_plan: n=%lld out of range (1 <= n < 2^31 - 1)", (long long)n);
  RARC_REQUIRE(MG_ALIGNED(d_ws, 256), RARC_E_INVALID, "rarc_merge_plan: the workspace is not 256-byte aligned");
  const MgPlanWs w = mg_plan_carve(d_ws, n);
  RARC_REQUIRE(ws_bytes >= w.bytes, RARC_E_WORKSPACE, "rarc_merge_plan: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = lv_grid(n, 256, 16384);
  RARC_HIP_CHECK(hipMemsetAsync(w.best, 0, (size_t)n * 8, s));
  hipLaunchKernelGGL(mg_plan_best_kernel, dim3(grid), dim3(256), 0, s, d_labels, d_richness, n, w.best);
  hipLaunchKernelGGL(mg_plan_primary_kernel, dim3(grid), dim3(256), 0, s, d_labels, n, (const u64*)w.best, d_primary, w.flag);
  mg_scan<uint32_t>(w.flag, n, w.bsum, w.pos, true, d_out_count, s);
  hipLaunchKernelGGL(mg_plan_write_kernel, dim3(grid), dim3(256), 0, s, n, (const int64_t*)d_primary, (const uint32_t*)w.flag,
                     (const uint32_t*)w.pos, d_new_id, d_kept, d_removed);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" size_t rarc_merge_pairs_workspace_bytes(int64_t m) {
  if (!mg_count_ok(m)) return 0;
  return mg_map_carve(nullptr, m, 1).bytes;
}

extern "C" int rarc_merge_pairs(const int64_t* d_pairs, const uint32_t* d_weights, int64_t m, const int64_t* d_new_id, int64_t n, void* d_ws,
                                size_t ws_bytes, int64_t* d_out_pairs, uint32_t* d_out_weights, int64_t* d_out5, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_pairs && d_new_id && d_ws && d_out_pairs && d_out_weights && d_out5, RARC_E_INVALID, "rarc_merge_pairs: null pointer");
  RARC_REQUIRE(MG_ALIGNED(d_pairs, 8) && MG_ALIGNED(d_weights, 4) && MG_ALIGNED(d_new_id, 8) && MG_ALIGNED(d_out_pairs, 8) &&
                   MG_ALIGNED(d_out_weights, 4) && MG_ALIGNED(d_out5, 8),
               RARC_E_INVALID, "rarc_merge_pairs: an array is not aligned to its element (weights 4 bytes, every other 8)");
  RARC_REQUIRE(mg_n_ok(n), RARC_E_INVALID, "rarc_merge_pairs: n=%lld out of range (1 <= n < 2^31 - 1)", (long long)n);
  RARC_REQUIRE(mg_count_ok(m), RARC_E_INVALID, "rarc_merge_pairs: m=%lld pairs out of range (1 <= m < 2^31)", (long long)m);
  RARC_REQUIRE(MG_ALIGNED(d_ws, 256), RARC_E_INVALID, "rarc_merge_pairs: the workspace is not 256-byte aligned");
  const MgMapWs w = mg_map_carve(d_ws, m, 1);
  RARC_REQUIRE(ws_bytes >= w.bytes, RARC_E_WORKSPACE, "rarc_merge_pairs: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  int64_t* ctl = w.sort.ctl;
  const int lo_bits = mg_bits(n);                                      // key = min << bits(n) | max: 2 bits(n) <= 62 bits
  const unsigned grid = lv_grid(m, 256, 16384);
  RARC_HIP_CHECK(hipMemsetAsync(ctl, 0, MG_CTL_BYTES, s));
  hipLaunchKernelGGL(mg_pair_key_kernel, dim3(grid), dim3(256), 0, s, d_pairs, d_weights, m, d_new_id, n, lo_bits, w.raw_keys, w.sort.flag, ctl);
  mg_scan<uint32_t>(w.sort.flag, m, w.sort.bsum, w.sort.pos, true, &ctl[MG_C_LEN], s);
  hipLaunchKernelGGL(mg_compact_kernel, dim3(grid), dim3(256), 0, s, (const u64*)w.raw_keys, d_weights, m, (const uint32_t*)w.sort.flag,
                     (const uint32_t*)w.sort.pos, w.keys, w.vals);
  mg_sort_reduce(w.keys, w.vals, m, &ctl[MG_C_LEN], 2 * lo_bits, w.sort, w.red_keys, w.red_sums, s);
  hipLaunchKernelGGL(mg_pair_unpack_kernel, dim3(grid), dim3(256), 0, s, (const u64*)w.red_keys, (const u64*)w.red_sums, m,
                     (const int64_t*)&ctl[MG_C_DISTINCT], lo_bits, d_out_pairs, d_out_weights);
  RARC_HIP_CHECK(hipGetLastError());
  RARC_HIP_CHECK(hipMemcpyAsync(d_out5, &ctl[MG_C_DISTINCT], 40, hipMemcpyDeviceToDevice, s));
  return RARC_OK;
}

extern "C" size_t rarc_merge_mentions_workspace_bytes(int64_t n_chunks, int64_t nnz) {
  if (!mg_count_ok(nnz) || n_chunks < 1 || n_chunks >= PPR_CHUNK_N_LIMIT) return 0;
  return mg_map_carve(nullptr, nnz, n_chunks).bytes;
}

extern "C" int rarc_merge_mentions(const int64_t* d_row_ptr, const int32_t* d_ent, const uint32_t* d_w, int64_t n_chunks, int64_t nnz,
                                   const int64_t* d_new_id, int64_t n, void* d_ws, size_t ws_bytes, int64_t* d_out_row_ptr, int32_t* d_out_ent,
                                   uint32_t* d_out_w, int32_t* d_out_split, int64_t* d_out6, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_row_ptr && d_ent && d_w && d_new_id && d_ws && d_out_row_ptr && d_out_ent && d_out_w && d_out_split && d_out6, RARC_E_INVALID,
               "rarc_merge_mentions: null pointer");
  RARC_REQUIRE(MG_ALIGNED(d_row_ptr, 8) && MG_ALIGNED(d_ent, 4) && MG_ALIGNED(d_w, 4) && MG_ALIGNED(d_new_id, 8) && MG_ALIGNED(d_out_row_ptr, 8) &&
                   MG_ALIGNED(d_out_ent, 4) && MG_ALIGNED(d_out_w, 4) && MG_ALIGNED(d_out_split, 4) && MG_ALIGNED(d_out6, 8),
               RARC_E_INVALID,
               "rarc_merge_mentions: an array is not aligned to its element (row_ptr, the map and the counts 8 bytes, every other 4)");
  RARC_REQUIRE(mg_n_ok(n), RARC_E_INVALID, "rarc_merge_mentions: n=%lld out of range (1 <= n < 2^31 - 1)", (long long)n);
  RARC_REQUIRE(n_chunks >= 1 && n_chunks < PPR_CHUNK_N_LIMIT, RARC_E_INVALID, "rarc_merge_mentions: n_chunks=%lld out of range (1 <= n_chunks < 2^31 - 1)",
               (long long)n_chunks);
  RARC_REQUIRE(mg_count_ok(nnz), RARC_E_INVALID, "rarc_merge_mentions: nnz=%lld mentions out of range (1 <= nnz < 2^31)", (long long)nnz);
  RARC_REQUIRE(MG_ALIGNED(d_ws, 256), RARC_E_INVALID, "rarc_merge_mentions: the workspace is not 256-byte aligned");
  const MgMapWs w = mg_map_carve(d_ws, nnz, n_chunks);
  RARC_REQUIRE(ws_bytes >= w.bytes, RARC_E_WORKSPACE, "rarc_merge_mentions: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  int64_t* ctl = w.sort.ctl;
  const int lo_bits = mg_bits(n);                                      // key = chunk << bits(n) | entity: at most 31 + 31 bits
  const unsigned grid = lv_grid(nnz, 256, 16384);
  RARC_HIP_CHECK(hipMemsetAsync(ctl, 0, MG_CTL_BYTES, s));
  RARC_HIP_CHECK(hipMemsetAsync(w.sort.flag, 0, (size_t)nnz * 4, s));             // (a slot no chunk's range covers carries nothing)
  RARC_HIP_CHECK(hipMemsetAsync(w.deg, 0, (size_t)n_chunks * 4, s));
  hipLaunchKernelGGL(mg_mention_key_kernel, dim3(lv_grid(n_chunks, 4, 16384)), dim3(256), 0, s, d_row_ptr, d_ent, d_w, n_chunks, nnz, d_new_id, n,
                     lo_bits, w.raw_keys, w.sort.flag, ctl);
  mg_scan<uint32_t>(w.sort.flag, nnz, w.sort.bsum, w.sort.pos, true, &ctl[MG_C_LEN], s);
  hipLaunchKernelGGL(mg_compact_kernel, dim3(grid), dim3(256), 0, s, (const u64*)w.raw_keys, d_w, nnz, (const uint32_t*)w.sort.flag,
                     (const uint32_t*)w.sort.pos, w.keys, w.vals);
  mg_sort_reduce(w.keys, w.vals, nnz, &ctl[MG_C_LEN], lo_bits + mg_bits(n_chunks), w.sort, w.red_keys, w.red_sums, s);
  mg_mention_rows(w.red_keys, w.red_sums, nnz, &ctl[MG_C_DISTINCT], nullptr, lo_bits, n_chunks, w.deg, w.cflag, w.cpos, w.cbsum, d_out_row_ptr,
                  d_out_ent, d_out_w, d_out_split, &ctl[MG_C_SPLIT], s);
  RARC_HIP_CHECK(hipGetLastError());
  RARC_HIP_CHECK(hipMemcpyAsync(d_out6, &ctl[MG_C_DISTINCT], 48, hipMemcpyDeviceToDevice, s));
  return RARC_OK;
}

extern "C" size_t rarc_merge_relations_workspace_bytes(int64_t r) {
  if (r < 1 || r >= LV_N_LIMIT) return 0;
  return mg_rel_carve(nullptr, r).bytes;
}

extern "C" int rarc_merge_relations(const int64_t* d_rel, int64_t r, const int64_t* d_new_id, int64_t n, void* d_ws, size_t ws_bytes,
                                    int64_t* d_out_rel, int64_t* d_out_rows, int64_t* d_out3, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_rel && d_new_id && d_ws && d_out_rel && d_out_rows && d_out3, RARC_E_INVALID, "rarc_merge_relations: null pointer");
  RARC_REQUIRE(MG_ALIGNED(d_rel, 8) && MG_ALIGNED(d_new_id, 8) && MG_ALIGNED(d_out_rel, 8) && MG_ALIGNED(d_out_rows, 8) && MG_ALIGNED(d_out3, 8),
               RARC_E_INVALID, "rarc_merge_relations: an array is not aligned to its element (8 bytes)");
  RARC_REQUIRE(mg_n_ok(n), RARC_E_INVALID, "rarc_merge_relations: n=%lld out of range (1 <= n < 2^31 - 1)", (long long)n);
  RARC_REQUIRE(r >= 1 && r < LV_N_LIMIT, RARC_E_INVALID, "rarc_merge_relations: r=%lld relation rows out of range (1 <= r < 2^31 - 1)", (long long)r);
  RARC_REQUIRE(MG_ALIGNED(d_ws, 256), RARC_E_INVALID, "rarc_merge_relations: the workspace is not 256-byte aligned");
  const MgRelWs w = mg_rel_carve(d_ws, r);
  RARC_REQUIRE(ws_bytes >= w.bytes, RARC_E_WORKSPACE, "rarc_merge_relations: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = lv_grid(r, 256, 16384);
  RARC_HIP_CHECK(hipMemsetAsync(w.ctl, 0, MG_CTL_BYTES, s));
  hipLaunchKernelGGL(mg_rel_flag_kernel, dim3(grid), dim3(256), 0, s, d_rel, r, d_new_id, n, w.flag, w.ctl);
  mg_scan<uint32_t>(w.flag, r, w.bsum, w.pos, true, &w.ctl[MG_C_LEN], s);
  hipLaunchKernelGGL(mg_rel_write_kernel, dim3(grid), dim3(256), 0, s, d_rel, r, d_new_id, (const uint32_t*)w.flag, (const uint32_t*)w.pos, d_out_rel,
                     d_out_rows);
  RARC_HIP_CHECK(hipGetLastError());
  RARC_HIP_CHECK(hipMemcpyAsync(d_out3, &w.ctl[MG_C_LEN], 8, hipMemcpyDeviceToDevice, s));
  RARC_HIP_CHECK(hipMemcpyAsync(d_out3 + 1, &w.ctl[MG_C_DROPPED], 8, hipMemcpyDeviceToDevice, s));
  RARC_HIP_CHECK(hipMemcpyAsync(d_out3 + 2, &w.ctl[MG_C_BAD], 8, hipMemcpyDeviceToDevice, s));
  return RARC_OK;
}

// ---- graph ingest: raw extraction rows, and a resident list to extend, become the unique sorted lists ----------------
// Every row — a base row or a new one — takes one slot of the sort.  A row the rule skips takes the key 0 with value 0 and mask 0:
// for pairs key 0 is (0, 0), which no edge has, so the writer leaves that one key out; for mentions key 0 is (chunk 0, entity 0),
// which a real mention may have — a skipped row adds 0 to its sum, and the key is left out only when its whole sum is 0 (a valid
// weight is >= 1).  Key 0 sorts first, so "left out" is one word: the writers start at slot `skip`.  No compaction, no cursor.
enum { IG_C_SKIP = 8, IG_C_KEPT = 9, IG_C_LARGEST = 10, IG_C_TOTAL = 11, IG_C_KIND0 = 12, IG_C_KIND1 = 13, IG_C_KIND2 = 14, IG_C_KIND3 = 15,
       IG_C_BASE = 16, IG_C_ROWS = 17 };
enum { IG_PAIRS = 0, IG_PAIRS_UNIT = 1, IG_MENTIONS = 2 };
constexpr int IG_TYPES = 32;

// slots [0, m0): the base rows (i < j, each once by contract; one outside it is counted as damaged); slots [m0, m0 + r): the new
// rows.  vals == nullptr: unit mode, the sort counts 1 a row; masks == nullptr: untyped
__global__ __launch_bounds__(256) void ig_pair_key_kernel(const int64_t* __restrict__ rows, const uint32_t* __restrict__ rw,
                                                          const int32_t* __restrict__ rt, int64_t r, const int64_t* __restrict__ base,
                                                          const uint32_t* __restrict__ bw, const uint32_t* __restrict__ bm, int64_t m0, int64_t n,
                                                          int lo_bits, u64* __restrict__ keys, uint32_t* __restrict__ vals,
                                                          uint32_t* __restrict__ masks, int64_t* ctl) {
  const int64_t cap = m0 + r;
  const int64_t rounds = (cap + (int64_t)gridDim.x * 256 - 1) / ((int64_t)gridDim.x * 256);
  for (int64_t k = 0; k < rounds; ++k) {                               // (every lane of a wave makes every round: mg_count shuffles)
    const int64_t i = (k * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    const bool valid = i < cap, is_base = valid && i < m0, is_new = valid && !is_base;
    int64_t a = -1, b = -1;
    uint32_t w = 1u, mask = 0u;
    int t = 0;
    if (is_base) {
      a = base[2 * i];
      b = base[2 * i + 1];
      if (bw) w = bw[i];
      if (bm) mask = bm[i];
    } else if (is_new) {
      const int64_t e = i - m0;
      a = rows[2 * e];
      b = rows[2 * e + 1];
      if (rw) w = rw[e];
      if (rt) t = rt[e];
      mask = (t >= 0 && t < IG_TYPES) ? 1u << t : 0u;
    }
    const bool in_range = a >= 0 && a < n && b >= 0 && b < n;
    const bool damaged = is_base && !(in_range && a < b && w != 0u);
    const bool k_range = is_new && !in_range;
    const bool k_loop = is_new && in_range && a == b;
    const bool k_weight = is_new && in_range && a != b && w == 0u;
    const bool k_type = is_new && in_range && a != b && w != 0u && (t < 0 || t >= IG_TYPES);
    const bool keep = valid && !damaged && !k_range && !k_loop && !k_weight && !k_type;
    if (valid) {
      keys[i] = keep ? ((u64)(a < b ? a : b) << lo_bits) | (u64)(a < b ? b : a) : 0ull;
      if (vals) vals[i] = keep ? w : 0u;
      if (masks) masks[i] = keep ? mask : 0u;
    }
    mg_count(k_range, 0, &ctl[IG_C_KIND0], nullptr);
    mg_count(k_loop, 0, &ctl[IG_C_KIND1], nullptr);
    mg_count(k_weight, 0, &ctl[IG_C_KIND2], nullptr);
    mg_count(k_type, 0, &ctl[IG_C_KIND3], nullptr);
    mg_count(damaged, 0, &ctl[IG_C_BASE], nullptr);
    mg_count(keep, (u64)w, &ctl[IG_C_ROWS], &ctl[IG_C_TOTAL]);
  }
}

// new (chunk, entity) rows into their slots (keys / vals point at the first of them); w == nullptr: 1 each
__global__ __launch_bounds__(256) void ig_mention_key_kernel(const int64_t* __restrict__ rows, const uint32_t* __restrict__ rw, int64_t r,
                                                             int64_t n_chunks, int64_t n_entities, int lo_bits, u64* __restrict__ keys,
                                                             uint32_t* __restrict__ vals, int64_t* ctl) {
  const int64_t rounds = (r + (int64_t)gridDim.x * 256 - 1) / ((int64_t)gridDim.x * 256);
  for (int64_t k = 0; k < rounds; ++k) {
    const int64_t i = (k * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    const bool valid = i < r;
    const int64_t c = valid ? rows[2 * i] : -1, e = valid ? rows[2 * i + 1] : -1;
    const uint32_t w = valid && rw ? rw[i] : 1u;
    const bool k_chunk = valid && (c < 0 || c >= n_chunks);
    const bool k_entity = valid && !k_chunk && (e < 0 || e >= n_entities);
    const bool k_weight = valid && !k_chunk && !k_entity && (w < 1u || w >= (1u << PPR_CHUNK_WEIGHT_BITS));
    const bool keep = valid && !k_chunk && !k_entity && !k_weight;
    if (valid) {
      keys[i] = keep ? ((u64)c << lo_bits) | (u64)e : 0ull;
      vals[i] = keep ? w : 0u;
    }
    mg_count(k_chunk, 0, &ctl[IG_C_KIND0], nullptr);
    mg_count(k_entity, 0, &ctl[IG_C_KIND1], nullptr);
    mg_count(k_weight, 0, &ctl[IG_C_KIND2], nullptr);
  }
}
// the base CSR into slots [0, nnz0), a wave per chunk, its ranges clamped as rarc_ppr_chunks clamps them (the slots no range
// covers were zeroed by the caller); an entry outside the rule is counted as damaged
__global__ __launch_bounds__(256) void ig_mention_base_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ ent,
                                                              const uint32_t* __restrict__ w, int64_t base_chunks, int64_t nnz0,
                                                              int64_t n_entities, int lo_bits, u64* __restrict__ keys,
                                                              uint32_t* __restrict__ vals, int64_t* ctl) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t c = (int64_t)blockIdx.x * 4 + wave; c < base_chunks; c += (int64_t)gridDim.x * 4) {
    int64_t r0 = row_ptr[c], r1 = row_ptr[c + 1];
    r0 = r0 < 0 ? 0 : (r0 > nnz0 ? nnz0 : r0);
    r1 = r1 < r0 ? r0 : (r1 > nnz0 ? nnz0 : r1);
    for (int64_t i0 = r0; i0 < r1; i0 += 64) {                         // (i0 is wave-uniform)
      const int64_t i = i0 + lane;
      const bool valid = i < r1;
      const int64_t e = valid ? (int64_t)ent[i] : -1;
      const uint32_t x = valid ? w[i] : 0u;
      const bool keep = valid && e >= 0 && e < n_entities && x >= 1u && x < (1u << PPR_CHUNK_WEIGHT_BITS);
      if (valid) {
        keys[i] = keep ? ((u64)c << lo_bits) | (u64)e : 0ull;
        vals[i] = keep ? x : 0u;
      }
      mg_count(valid && !keep, 0, &ctl[IG_C_BASE], nullptr);
    }
  }
}

// one thread, after the sort: whether the first key is the placeholder, what is kept, and the unit mode's own largest and total
__global__ void ig_finish_kernel(const u64* __restrict__ red_keys, const u64* __restrict__ red_sums, int64_t cap, int mode, int64_t* ctl) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t distinct = ctl[MG_C_DISTINCT];
  distinct = distinct < 0 ? 0 : (distinct > cap ? cap : distinct);
  const int64_t skip = distinct >= 1 && red_keys[0] == 0ull && (mode != IG_MENTIONS || red_sums[0] == 0ull) ? 1 : 0;
  const int64_t kept = distinct - skip;
  ctl[IG_C_SKIP] = skip;
  ctl[IG_C_KEPT] = kept;
  if (mode == IG_PAIRS_UNIT) {
    ctl[IG_C_LARGEST] = kept ? 1 : 0;
    ctl[IG_C_TOTAL] = kept;
  } else {
    ctl[IG_C_LARGEST] = ctl[MG_C_MAX];                                 // (the placeholder's sum is 0: it raises no maximum)
  }
}

// out_w == nullptr: not asked for; unit: every W is 1; out_masks: cleared here for the kept edges, ORed into by ig_mask_kernel
__global__ __launch_bounds__(256) void ig_pair_write_kernel(const u64* __restrict__ red_keys, const u64* __restrict__ red_sums, int64_t cap,
                                                            const int64_t* __restrict__ ctl, int lo_bits, bool unit,
                                                            int64_t* __restrict__ out_pairs, uint32_t* __restrict__ out_w,
                                                            uint32_t* __restrict__ out_masks) {
  const int64_t skip = ctl[IG_C_SKIP] > 0 ? 1 : 0;
  int64_t kept = ctl[IG_C_KEPT];
  kept = kept < 0 ? 0 : (kept > cap - skip ? cap - skip : kept);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < kept; i += (int64_t)gridDim.x * 256) {
    const u64 key = red_keys[i + skip];
    out_pairs[2 * i] = (int64_t)(key >> lo_bits);
    out_pairs[2 * i + 1] = (int64_t)(key & ((1ull << lo_bits) - 1ull));
    if (out_w) out_w[i] = unit ? 1u : (uint32_t)red_sums[i + skip];    // (the caller narrows: the largest sum is reported)
    if (out_masks) out_masks[i] = 0u;
  }
}
// every contributing row finds its pair among the kept keys (ascending: a binary search) and ORs its mask into that edge's word:
// integer ORs commute, so the word is the same bits for any order of the rows
__global__ __launch_bounds__(256) void ig_mask_kernel(const u64* __restrict__ raw_keys, const uint32_t* __restrict__ raw_masks, int64_t cap,
                                                      const u64* __restrict__ red_keys, const int64_t* __restrict__ ctl, uint32_t* out_masks) {
  const int64_t skip = ctl[IG_C_SKIP] > 0 ? 1 : 0;
  int64_t kept = ctl[IG_C_KEPT];
  kept = kept < 0 ? 0 : (kept > cap - skip ? cap - skip : kept);
  const u64* sorted = red_keys + skip;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += (int64_t)gridDim.x * 256) {
    const uint32_t mask = raw_masks[i];
    if (!mask) continue;
    const u64 key = raw_keys[i];
    int64_t lo = 0, hi = kept;                                         // the first slot whose key is >= key
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (sorted[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    if (lo < kept && sorted[lo] == key) atomicOr(&out_masks[lo], mask);
  }
}

struct IgWs {
  u64* raw_keys;
  uint32_t* raw_vals;
  uint32_t* raw_masks;
  u64* red_keys;
  u64* red_sums;
  uint32_t* deg;
  uint32_t* cflag;
  uint32_t* cpos;
  u64* cbsum;
  MgSortWs sort;
  size_t bytes;
};
// n_chunks == 0: the pairs' workspace, without the per-chunk arrays
static IgWs ig_carve(const void* base, int64_t cap, int64_t n_chunks) {
  char* b = (char*)base;
  size_t o = 0;
  IgWs w;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  w.raw_keys = (u64*)take((size_t)cap * 8);
  w.raw_vals = (uint32_t*)take((size_t)cap * 4);
  w.raw_masks = (uint32_t*)take((size_t)cap * 4);
  w.red_keys = (u64*)take((size_t)cap * 8);
  w.red_sums = (u64*)take((size_t)cap * 8);
  w.deg = (uint32_t*)take((size_t)n_chunks * 4);
  w.cflag = (uint32_t*)take((size_t)n_chunks * 4);
  w.cpos = (uint32_t*)take((size_t)(n_chunks + 1) * 4);
  w.cbsum = (u64*)take((size_t)(mg_tiles(n_chunks) + 1) * 8);
  w.sort = mg_sort_carve(b ? b + o : nullptr, cap);
  w.bytes = o + w.sort.bytes;
  return w;
}
static inline bool ig_counts_ok(int64_t base, int64_t r) { return base >= 0 && r >= 0 && base < MG_COUNT_LIMIT && r < MG_COUNT_LIMIT && mg_count_ok(base + r); }

extern "C" int rarc_ingest_limits(int* out4) {
  RARC_REQUIRE(out4, RARC_E_INVALID, "rarc_ingest_limits: null pointer");
  out4[0] = IG_TYPES;
  out4[1] = PPR_CHUNK_WEIGHT_BITS;
  out4[2] = MG_SPLIT_DEGREE;
  out4[3] = 31;                                                        // base + new rows < 2^31
  return RARC_OK;
}

extern "C" size_t rarc_ingest_pairs_workspace_bytes(int64_t m0, int64_t r) {
  if (!ig_counts_ok(m0, r)) return 0;
  return ig_carve(nullptr, m0 + r, 0).bytes;
}

extern "C" int rarc_ingest_pairs(const int64_t* d_rows, const uint32_t* d_row_weights, const int32_t* d_row_types, int64_t r,
                                 const int64_t* d_base_pairs, const uint32_t* d_base_weights, const uint32_t* d_base_masks, int64_t m0, int64_t n,
                                 void* d_ws, size_t ws_bytes, int64_t* d_out_pairs, uint32_t* d_out_weights, uint32_t* d_out_masks,
                                 int64_t* d_out8, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(ig_counts_ok(m0, r), RARC_E_INVALID, "rarc_ingest_pairs: m0=%lld base pairs and r=%lld rows out of range (1 <= m0 + r < 2^31)",
               (long long)m0, (long long)r);
  const bool typed = d_out_masks != nullptr, unit = !d_row_weights && !d_base_weights;
  RARC_REQUIRE(d_ws && d_out_pairs && d_out8 && (r == 0 || d_rows) && (m0 == 0 || d_base_pairs) && (unit || d_out_weights), RARC_E_INVALID,
               "rarc_ingest_pairs: null pointer");
  RARC_REQUIRE(typed ? (r == 0 || d_row_types) && (m0 == 0 || d_base_masks) : !d_row_types && !d_base_masks, RARC_E_INVALID,
               "rarc_ingest_pairs: typed and untyped inputs are mixed (d_out_masks asks for masks: then every side present carries types)");
  RARC_REQUIRE(MG_ALIGNED(d_rows, 8) && MG_ALIGNED(d_row_weights, 4) && MG_ALIGNED(d_row_types, 4) && MG_ALIGNED(d_base_pairs, 8) &&
                   MG_ALIGNED(d_base_weights, 4) && MG_ALIGNED(d_base_masks, 4) && MG_ALIGNED(d_out_pairs, 8) && MG_ALIGNED(d_out_weights, 4) &&
                   MG_ALIGNED(d_out_masks, 4) && MG_ALIGNED(d_out8, 8),
               RARC_E_INVALID, "rarc_ingest_pairs: an array is not aligned to its element (pairs, rows and the counts 8 bytes, every other 4)");
  RARC_REQUIRE(n >= 2 && n < LV_N_LIMIT, RARC_E_INVALID, "rarc_ingest_pairs: n=%lld out of range (2 <= n < 2^31 - 1)", (long long)n);
  RARC_REQUIRE(MG_ALIGNED(d_ws, 256), RARC_E_INVALID, "rarc_ingest_pairs: the workspace is not 256-byte aligned");
  const int64_t cap = m0 + r;
  const IgWs w = ig_carve(d_ws, cap, 0);
  RARC_REQUIRE(ws_bytes >= w.bytes, RARC_E_WORKSPACE, "rarc_ingest_pairs: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  int64_t* ctl = w.sort.ctl;
  const int lo_bits = mg_bits(n);                                      // key = min << bits(n) | max: 2 bits(n) <= 62 bits
  const unsigned grid = lv_grid(cap, 256, 16384);
  RARC_HIP_CHECK(hipMemsetAsync(ctl, 0, MG_CTL_BYTES, s));
  hipLaunchKernelGGL(ig_pair_key_kernel, dim3(grid), dim3(256), 0, s, d_rows, d_row_weights, d_row_types, r, d_base_pairs, d_base_weights,
                     d_base_masks, m0, n, lo_bits, w.raw_keys, unit ? (uint32_t*)nullptr : w.raw_vals, typed ? w.raw_masks : (uint32_t*)nullptr, ctl);
  mg_sort_reduce(w.raw_keys, unit ? (const uint32_t*)nullptr : w.raw_vals, cap, nullptr, 2 * lo_bits, w.sort, w.red_keys, w.red_sums, s);
  hipLaunchKernelGGL(ig_finish_kernel, dim3(1), dim3(64), 0, s, (const u64*)w.red_keys, (const u64*)w.red_sums, cap, unit ? IG_PAIRS_UNIT : IG_PAIRS,
                     ctl);
  hipLaunchKernelGGL(ig_pair_write_kernel, dim3(grid), dim3(256), 0, s, (const u64*)w.red_keys, (const u64*)w.red_sums, cap, (const int64_t*)ctl,
                     lo_bits, unit, d_out_pairs, d_out_weights, d_out_masks);
  if (typed)
    hipLaunchKernelGGL(ig_mask_kernel, dim3(grid), dim3(256), 0, s, (const u64*)w.raw_keys, (const uint32_t*)w.raw_masks, cap,
                       (const u64*)w.red_keys, (const int64_t*)ctl, d_out_masks);
  RARC_HIP_CHECK(hipGetLastError());
  RARC_HIP_CHECK(hipMemcpyAsync(d_out8, &ctl[IG_C_KEPT], 64, hipMemcpyDeviceToDevice, s));
  return RARC_OK;
}

extern "C" size_t rarc_ingest_mentions_workspace_bytes(int64_t n_chunks, int64_t nnz0, int64_t r) {
  if (!ig_counts_ok(nnz0, r) || n_chunks < 1 || n_chunks >= PPR_CHUNK_N_LIMIT) return 0;
  return ig_carve(nullptr, nnz0 + r, n_chunks).bytes;
}

extern "C" int rarc_ingest_mentions(const int64_t* d_rows, const uint32_t* d_row_weights, int64_t r, const int64_t* d_base_row_ptr,
                                    const int32_t* d_base_ent, const uint32_t* d_base_w, int64_t base_chunks, int64_t nnz0, int64_t n_chunks,
                                    int64_t n_entities, void* d_ws, size_t ws_bytes, int64_t* d_out_row_ptr, int32_t* d_out_ent, uint32_t* d_out_w,
                                    int32_t* d_out_split, int64_t* d_out8, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(ig_counts_ok(nnz0, r), RARC_E_INVALID, "rarc_ingest_mentions: nnz0=%lld base mentions and r=%lld rows out of range (1 <= nnz0 + r < 2^31)",
               (long long)nnz0, (long long)r);
  RARC_REQUIRE(d_ws && d_out_row_ptr && d_out_ent && d_out_w && d_out_split && d_out8 && (r == 0 || d_rows) &&
                   (nnz0 == 0 || (d_base_row_ptr && d_base_ent && d_base_w)),
               RARC_E_INVALID, "rarc_ingest_mentions: null pointer");
  RARC_REQUIRE(MG_ALIGNED(d_rows, 8) && MG_ALIGNED(d_row_weights, 4) && MG_ALIGNED(d_base_row_ptr, 8) && MG_ALIGNED(d_base_ent, 4) &&
                   MG_ALIGNED(d_base_w, 4) && MG_ALIGNED(d_out_row_ptr, 8) && MG_ALIGNED(d_out_ent, 4) && MG_ALIGNED(d_out_w, 4) &&
                   MG_ALIGNED(d_out_split, 4) && MG_ALIGNED(d_out8, 8),
               RARC_E_INVALID, "rarc_ingest_mentions: an array is not aligned to its element (rows, row_ptr and the counts 8 bytes, every other 4)");
  RARC_REQUIRE(mg_n_ok(n_entities), RARC_E_INVALID, "rarc_ingest_mentions: n_entities=%lld out of range (1 <= n_entities < 2^31 - 1)",
               (long long)n_entities);
  RARC_REQUIRE(n_chunks >= 1 && n_chunks < PPR_CHUNK_N_LIMIT, RARC_E_INVALID, "rarc_ingest_mentions: n_chunks=%lld out of range (1 <= n_chunks < 2^31 - 1)",
               (long long)n_chunks);
  RARC_REQUIRE(base_chunks >= (nnz0 ? 1 : 0) && base_chunks <= n_chunks, RARC_E_INVALID,
               "rarc_ingest_mentions: base_chunks=%lld out of range (the base's chunks are the first of the n_chunks=%lld)", (long long)base_chunks,
               (long long)n_chunks);
  RARC_REQUIRE(MG_ALIGNED(d_ws, 256), RARC_E_INVALID, "rarc_ingest_mentions: the workspace is not 256-byte aligned");
  const int64_t cap = nnz0 + r;
  const IgWs w = ig_carve(d_ws, cap, n_chunks);
  RARC_REQUIRE(ws_bytes >= w.bytes, RARC_E_WORKSPACE, "rarc_ingest_mentions: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  int64_t* ctl = w.sort.ctl;
  const int lo_bits = mg_bits(n_entities);                             // key = chunk << bits(n_entities) | entity: at most 31 + 31 bits
  RARC_HIP_CHECK(hipMemsetAsync(ctl, 0, MG_CTL_BYTES, s));
  RARC_HIP_CHECK(hipMemsetAsync(w.deg, 0, (size_t)n_chunks * 4, s));
  if (nnz0) {
    RARC_HIP_CHECK(hipMemsetAsync(w.raw_keys, 0, (size_t)nnz0 * 8, s));           // (a slot no chunk's range covers carries nothing)
    RARC_HIP_CHECK(hipMemsetAsync(w.raw_vals, 0, (size_t)nnz0 * 4, s));
    hipLaunchKernelGGL(ig_mention_base_kernel, dim3(lv_grid(base_chunks, 4, 16384)), dim3(256), 0, s, d_base_row_ptr, d_base_ent, d_base_w,
                       base_chunks, nnz0, n_entities, lo_bits, w.raw_keys, w.raw_vals, ctl);
  }
  if (r)
    hipLaunchKernelGGL(ig_mention_key_kernel, dim3(lv_grid(r, 256, 16384)), dim3(256), 0, s, d_rows, d_row_weights, r, n_chunks, n_entities, lo_bits,
                       w.raw_keys + nnz0, w.raw_vals + nnz0, ctl);
  mg_sort_reduce(w.raw_keys, w.raw_vals, cap, nullptr, lo_bits + mg_bits(n_chunks), w.sort, w.red_keys, w.red_sums, s);
  hipLaunchKernelGGL(ig_finish_kernel, dim3(1), dim3(64), 0, s, (const u64*)w.red_keys, (const u64*)w.red_sums, cap, (int)IG_MENTIONS, ctl);
  mg_mention_rows(w.red_keys, w.red_sums, cap, &ctl[IG_C_KEPT], &ctl[IG_C_SKIP], lo_bits, n_chunks, w.deg, w.cflag, w.cpos, w.cbsum, d_out_row_ptr,
                  d_out_ent, d_out_w, d_out_split, &ctl[IG_C_TOTAL], s);
  RARC_HIP_CHECK(hipGetLastError());
  RARC_HIP_CHECK(hipMemcpyAsync(d_out8, &ctl[IG_C_KEPT], 64, hipMemcpyDeviceToDevice, s));
  return RARC_OK;
}
