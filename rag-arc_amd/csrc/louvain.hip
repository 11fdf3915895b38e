// louvain.hip — Louvain communities of an undirected, unit-weight edge list: step 2 of the reference's entity
// de-duplication (encapsulation/database/graph_db/Base_Neo4j.py:646-658, gds.louvain.stream(graph, {maxIterations: 10}) over
// the SIMILAR edges step 1 wrote).  rarc_similar_pairs leaves those edges on the device; the kernels here cluster them there.
//
// GDS's Louvain is parallel and order-dependent.  This one is defined in integers (tests/louvain_ref.py restates it) and the
// answer depends neither on the order of the edge list nor on thread timing: a sweep is synchronous (every gain is taken
// against the labels at its start), every sum is an integer sum, and the target of a move is the maximum of (G, -label).
//
// What lives where.  A GRAPH blob holds one level: CSR in both directions (row_ptr, adj, adj_w, adj_src), self-loops, weighted
// degrees k, M2 = sum k and four lists of vertices bucketed by degree.  A STATE blob holds two label slots (comm, tot, size):
// a sweep reads slot `cur` and writes the other, so the host accepts a sweep by flipping `cur` and discards it by not doing so.
// The loops over sweeps and levels are the caller's: it reads {moved, Qn, movers with a target} after a sweep and {n_c, m_c} after an aggregate.
// Every weight of every level fits 32 bits: the total weight is conserved by aggregation and M2 = 2 m < 2^31.
//
// The sweep, per mover v: w_C = weight of v's edges into each neighbouring community C, then
// G(C) = M2 (w_C - w_A) - k_v (tot_C - (tot_A - k_v)).  By degree:
//   deg <= 8      eight lanes per vertex, one neighbour per lane; the lanes exchange (label, weight) with ds_bpermute
//   deg <= 64     a wave per vertex, the same way
//   deg <= 8192   a workgroup per vertex, an open-addressing table of (label, weight) in LDS (128 KB: 16384 slots)
//   beyond        a workgroup per vertex, the same table in global memory (one per resident workgroup)
#include "graph_csr.h"      // the GRAPH blob's layout, its degree classes and the limits on n and m
#include <limits.h>

constexpr uint32_t LV_LDS_SLOTS = 16384;                    // 2 * LV_DEG_LDS: load factor <= 1/2
constexpr size_t LV_LDS_BYTES = 64 + (size_t)LV_LDS_SLOTS * 8;
constexpr uint32_t LV_EMPTY = 0xffffffffu;                  // no label: labels are < n < 2^31
constexpr unsigned long long LV_EMPTY64 = ~0ull;
constexpr size_t LV_GLOBAL_TABLE_BUDGET = (size_t)64 << 20;
enum { LV_S_MOVED = 0, LV_S_IN = 1, LV_S_TOT2 = 2, LV_S_EDGES = 3, LV_S_TARGETS = 4, LV_S_WORDS = 8 };

// the global tables of the last bucket: one per resident workgroup, each holding twice the largest degree n and m allow
static inline unsigned long long lv_global_slots(int64_t n, int64_t m) {
  if (lv_max_degree(n, m) <= LV_DEG_LDS) return 0;
  unsigned long long s = 1024;
  while (s < 2ull * (unsigned long long)lv_max_degree(n, m)) s <<= 1;
  return s;
}
static inline int lv_global_blocks(int64_t n, int64_t m) {
  const unsigned long long s = lv_global_slots(n, m);
  if (!s) return 0;
  const size_t fit = LV_GLOBAL_TABLE_BUDGET / (size_t)(s * 8);
  return fit < 1 ? 1 : (fit > 32 ? 32 : (int)fit);
}
static inline unsigned long long lv_pair_slots(int64_t m) {
  unsigned long long s = 1024;
  while (s < 2ull * (unsigned long long)m) s <<= 1;
  return s;
}

struct LvState {
  int32_t* comm[2];
  uint32_t* tot[2];
  uint32_t* size[2];
  int64_t* scal;
  uint32_t* flag;
  int64_t* newid;
  int64_t* scan;
  char* table;          // the sweep's global tables, or the aggregate's pair table: never both at once
  size_t bytes;
};
static LvState lv_state_carve(const void* base, int64_t n, int64_t m) {
  char* b = (char*)base;
  size_t o = 0;
  LvState s;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  for (int i = 0; i < 2; ++i) s.comm[i] = (int32_t*)take((size_t)n * 4);
  for (int i = 0; i < 2; ++i) s.tot[i] = (uint32_t*)take((size_t)n * 4);
  for (int i = 0; i < 2; ++i) s.size[i] = (uint32_t*)take((size_t)n * 4);
  s.scal = (int64_t*)take(LV_S_WORDS * 8);
  s.flag = (uint32_t*)take((size_t)n * 4);
  s.newid = (int64_t*)take((size_t)(n + 1) * 8);
  s.scan = (int64_t*)take((size_t)(lv_scan_blocks(n) + 1) * 8);
  const size_t sweep_tables = (size_t)lv_global_blocks(n, m) * (size_t)lv_global_slots(n, m) * 8;
  const size_t pair_table = (size_t)lv_pair_slots(m) * 12;
  s.table = take(sweep_tables > pair_table ? sweep_tables : pair_table);
  s.bytes = o;
  return s;
}

// ---- block-wide helpers (256 threads) -------------------------------------------------------------------------------------------
__device__ __forceinline__ long long lv_wave_sum(long long x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
  return x;
}
// the sum of x over the block, valid in thread 0 (s_part: 4 words of LDS)
__device__ __forceinline__ long long lv_block_sum(long long x, long long* s_part) {
  x = lv_wave_sum(x);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = x;
  __syncthreads();
  const long long r = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
  __syncthreads();
  return r;
}
// append to a list with one atomic per wave: the position of this lane's item (mine), called by every lane of the wave
__device__ __forceinline__ long long lv_wave_append(bool mine, unsigned long long* counter) {
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(mine);
  if (!mask) return -1;
  const int lane = threadIdx.x & 63, leader = __builtin_ctzll(mask);
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(counter, (unsigned long long)__builtin_popcountll(mask));
  base = __shfl(base, leader, 64);
  return (long long)(base + (unsigned long long)__builtin_popcountll(mask & ((1ull << lane) - 1ull)));
}

// ---- exclusive scan of n uint32 into n + 1 int64 (out[n] = the total): tile sums, one block over the sums, tiles again -------------
__global__ __launch_bounds__(256) void lv_scan_sums_kernel(const uint32_t* __restrict__ in, int64_t n, int64_t* __restrict__ bsum) {
  __shared__ long long s_part[4];
  const int64_t base = (int64_t)blockIdx.x * LV_SCAN_TILE + (int64_t)threadIdx.x * 8;
  long long acc = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (base + j < n) acc += in[base + j];
  const long long r = lv_block_sum(acc, s_part);
  if (threadIdx.x == 0) bsum[blockIdx.x] = r;
}
// inclusive scan of one value per thread over the block (s: 256 words of LDS)
__device__ __forceinline__ long long lv_block_scan(long long x, long long* s) {
  s[threadIdx.x] = x;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const long long o = threadIdx.x >= (unsigned)d ? s[threadIdx.x - d] : 0;
    __syncthreads();
    s[threadIdx.x] += o;
    __syncthreads();
  }
  const long long r = s[threadIdx.x];
  __syncthreads();
  return r;
}
__global__ __launch_bounds__(256) void lv_scan_offsets_kernel(int64_t* bsum, int64_t nb) {
  __shared__ long long s[256];
  long long carry = 0;
  for (int64_t base = 0; base < nb; base += 256) {
    const int64_t i = base + threadIdx.x;
    const long long x = i < nb ? bsum[i] : 0;
    const long long incl = lv_block_scan(x, s);
    if (i < nb) bsum[i] = carry + incl - x;
    if (threadIdx.x == 255) s[0] = incl;
    __syncthreads();
    carry += s[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) bsum[nb] = carry;
}
__global__ __launch_bounds__(256) void lv_scan_apply_kernel(const uint32_t* __restrict__ in, int64_t n, const int64_t* __restrict__ bsum,
                                                            int64_t* __restrict__ out) {
  __shared__ long long s[256];
  const int64_t base = (int64_t)blockIdx.x * LV_SCAN_TILE + (int64_t)threadIdx.x * 8;
  uint32_t x[8];
  long long acc = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    x[j] = base + j < n ? in[base + j] : 0u;
    acc += x[j];
  }
  long long run = bsum[blockIdx.x] + lv_block_scan(acc, s) - acc;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (base + j < n) out[base + j] = run;
    run += x[j];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[n] = bsum[gridDim.x];
}
static int lv_scan(const uint32_t* in, int64_t n, int64_t* scratch, int64_t* out, hipStream_t s) {
  const int64_t nb = lv_scan_blocks(n);
  hipLaunchKernelGGL(lv_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, s, in, n, scratch);
  hipLaunchKernelGGL(lv_scan_offsets_kernel, dim3(1), dim3(256), 0, s, scratch, nb);
  hipLaunchKernelGGL(lv_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, s, in, n, (const int64_t*)scratch, out);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

// ---- the adjacency ------------------------------------------------------------------------------------------------------------
// an edge both passes skip alike (so a slot is written for exactly the edges that were counted): a pair outside 0 <= i < j < n
__device__ __forceinline__ bool lv_edge_ok(int64_t a, int64_t b, int64_t n) { return a >= 0 && a < b && b < n; }

__global__ __launch_bounds__(256) void lv_degree_kernel(const int64_t* __restrict__ pairs, const uint32_t* __restrict__ w, int64_t m, int64_t n,
                                                        uint32_t* cnt, uint32_t* k, int64_t* hdr) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256) {
    const int64_t a = pairs[2 * e], b = pairs[2 * e + 1];
    if (!lv_edge_ok(a, b, n)) {
      atomicAdd((unsigned long long*)&hdr[LV_H_BAD], 1ull);
      continue;
    }
    const uint32_t wt = w ? w[e] : 1u;
    atomicAdd(&cnt[a], 1u);
    atomicAdd(&cnt[b], 1u);
    atomicAdd(&k[a], wt);
    atomicAdd(&k[b], wt);
  }
}
__global__ __launch_bounds__(256) void lv_fill_kernel(const int64_t* __restrict__ pairs, const uint32_t* __restrict__ w, int64_t m, int64_t n,
                                                      const int64_t* __restrict__ row_ptr, uint32_t* cursor, int32_t* adj, uint32_t* adj_w,
                                                      int32_t* adj_src) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256) {
    const int64_t a = pairs[2 * e], b = pairs[2 * e + 1];
    if (!lv_edge_ok(a, b, n)) continue;
    const uint32_t wt = w ? w[e] : 1u;
    const int64_t pa = row_ptr[a] + atomicAdd(&cursor[a], 1u), pb = row_ptr[b] + atomicAdd(&cursor[b], 1u);
    if (pa < 2 * m) {
      adj[pa] = (int32_t)b;
      adj_w[pa] = wt;
      adj_src[pa] = (int32_t)a;
    }
    if (pb < 2 * m) {
      adj[pb] = (int32_t)a;
      adj_w[pb] = wt;
      adj_src[pb] = (int32_t)b;
    }
  }
}
// k_v gets its loop, M2 its sum, and every vertex with a neighbour joins the list of its degree class
__global__ __launch_bounds__(256) void lv_finish_kernel(int64_t n, const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ loops_in,
                                                        uint32_t* k, uint32_t* loop, int64_t* hdr, int32_t* l0, int32_t* l1, int32_t* l2,
                                                        int32_t* l3) {
  __shared__ long long s_part[4];
  int32_t* const lists[4] = {l0, l1, l2, l3};
  long long acc = 0;
  for (int64_t v0 = (int64_t)blockIdx.x * 256; v0 < n; v0 += (int64_t)gridDim.x * 256) {
    const int64_t v = v0 + threadIdx.x;
    int bucket = -1;
    if (v < n) {
      const int64_t deg = row_ptr[v + 1] - row_ptr[v];
      const uint32_t lp = loops_in ? loops_in[v] : 0u;
      const uint32_t kv = k[v] + 2u * lp;
      k[v] = kv;
      loop[v] = lp;
      acc += kv;
      bucket = deg == 0 ? -1 : deg <= LV_DEG_GROUP ? 0 : deg <= LV_DEG_WAVE ? 1 : deg <= LV_DEG_LDS ? 2 : 3;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const long long pos = lv_wave_append(bucket == b, (unsigned long long*)&hdr[LV_H_LIST + b]);
      if (bucket == b && pos < n) lists[b][pos] = (int32_t)v;
    }
  }
  const long long r = lv_block_sum(acc, s_part);
  if (threadIdx.x == 0 && r) atomicAdd((unsigned long long*)&hdr[LV_H_M2], (unsigned long long)r);
}

// ---- the sweep ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool lv_is_mover(uint32_t v, int t) { return (((v * 2654435761u) >> (16 + (t & 15))) & 1u) == 0u; }
// (G, label) order: the larger G, then the smaller label
__device__ __forceinline__ bool lv_better(long long g, int c, long long bg, int bc) { return g > bg || (g == bg && c < bc); }
__device__ __forceinline__ long long lv_gain(long long m2, long long w_c, long long w_a, long long k_v, long long tot_c, long long tot_a) {
  return m2 * (w_c - w_a) - k_v * (tot_c - (tot_a - k_v));
}
// the move itself: a target needs G > 0, and two singletons merge only towards the smaller label
__device__ __forceinline__ bool lv_decide(long long g, int target, int a, const uint32_t* __restrict__ size) {
  if (g <= 0) return false;
  return !(size[a] == 1u && size[target] == 1u && target > a);
}

struct LvSweepArgs {
  const int64_t* hdr;
  const int64_t* row_ptr;
  const int32_t* adj;
  const uint32_t* adj_w;
  const uint32_t* k;
  const int32_t* comm;
  const uint32_t* tot;
  const uint32_t* size;
  int32_t* comm_new;
  unsigned long long* moved;
  unsigned long long* targets;      // movers with a target (G > 0), moved or held back by the singleton rule
  int t;
};

// W lanes per vertex of at most W neighbours: lane j holds neighbour j's (label, weight), and every lane sums the weights of
// the lanes that share its label — w_C for its own C — and of those labelled A
template <int W, int BUCKET>
__global__ __launch_bounds__(256) void lv_sweep_group_kernel(const LvSweepArgs p, const int32_t* __restrict__ list) {
  constexpr int GPB = 256 / W;
  const long long m2 = p.hdr[LV_H_M2], n_list = p.hdr[LV_H_LIST + BUCKET];
  const int sub = threadIdx.x % W, grp = threadIdx.x / W;
  long long my_moved = 0, my_targets = 0;
  for (long long i0 = (long long)blockIdx.x * GPB; i0 < n_list; i0 += (long long)gridDim.x * GPB) {
    const long long i = i0 + grp;
    const int v = i < n_list ? list[i] : -1;
    const bool mover = v >= 0 && lv_is_mover((uint32_t)v, p.t);
    int a = -1, c = -1;
    uint32_t w = 0;
    if (mover) {
      a = p.comm[v];
      const int64_t r0 = p.row_ptr[v];
      const int deg = (int)(p.row_ptr[v + 1] - r0);
      if (sub < deg) {
        c = p.comm[p.adj[r0 + sub]];
        w = p.adj_w[r0 + sub];
      }
    }
    uint32_t w_c = 0, w_a = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int cj = __shfl(c, j, W);
      const uint32_t wj = (uint32_t)__shfl((int)w, j, W);
      w_c += cj == c ? wj : 0u;
      w_a += cj == a ? wj : 0u;
    }
    long long g = LLONG_MIN;
    int bc = INT_MAX;
    if (c >= 0 && c != a) {
      g = lv_gain(m2, w_c, w_a, p.k[v], p.tot[c], p.tot[a]);
      bc = c;
    }
#pragma unroll
    for (int d = W / 2; d >= 1; d >>= 1) {
      const long long og = __shfl_xor(g, d, W);
      const int oc = __shfl_xor(bc, d, W);
      if (lv_better(og, oc, g, bc)) {
        g = og;
        bc = oc;
      }
    }
    if (sub == 0 && mover && bc != INT_MAX && g > 0) {
      ++my_targets;
      if (lv_decide(g, bc, a, p.size)) {
        p.comm_new[v] = bc;
        ++my_moved;
      }
    }
  }
  my_moved = lv_wave_sum(my_moved);
  my_targets = lv_wave_sum(my_targets);
  if ((threadIdx.x & 63) == 0 && my_moved) atomicAdd(p.moved, (unsigned long long)my_moved);
  if ((threadIdx.x & 63) == 0 && my_targets) atomicAdd(p.targets, (unsigned long long)my_targets);
}

// table accesses: LDS behind the block's barriers, or global memory past the L1 (the adds are performed in L2)
template <bool GLOBAL>
__device__ __forceinline__ uint32_t lv_tab_load(const uint32_t* q) {
  if (GLOBAL) return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *q;
}
template <bool GLOBAL>
__device__ __forceinline__ void lv_tab_store(uint32_t* q, uint32_t x) {
  if (GLOBAL) __hip_atomic_store(q, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *q = x;
}

// a workgroup per vertex: (label -> weight) in an open-addressing table of 2^lg >= 2 deg slots, linear probing; the sums are
// integer atomics, so the table's content does not depend on who came first, and the choice below is a maximum of (G, -label)
template <bool GLOBAL, int BUCKET>
__global__ __launch_bounds__(256) void lv_sweep_hash_kernel(const LvSweepArgs p, const int32_t* __restrict__ list, uint32_t* gtab,
                                                            unsigned long long gslots) {
  extern __shared__ __attribute__((aligned(16))) char lv_smem[];
  long long* s_g = (long long*)lv_smem;            // [4]
  int* s_c = (int*)(lv_smem + 32);                 // [4]
  uint32_t* s_wa = (uint32_t*)(lv_smem + 48);
  uint32_t* keys = GLOBAL ? gtab + (size_t)blockIdx.x * 2 * gslots : (uint32_t*)(lv_smem + 64);
  uint32_t* vals = keys + (GLOBAL ? gslots : (unsigned long long)LV_LDS_SLOTS);
  const unsigned long long cap = GLOBAL ? gslots : (unsigned long long)LV_LDS_SLOTS;
  const long long m2 = p.hdr[LV_H_M2], n_list = p.hdr[LV_H_LIST + BUCKET];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (long long i = blockIdx.x; i < n_list; i += gridDim.x) {
    const int v = list[i];
    if (!lv_is_mover((uint32_t)v, p.t)) continue;                      // (block-uniform)
    const int64_t r0 = p.row_ptr[v], deg = p.row_ptr[v + 1] - r0;
    unsigned lg = 9;
    while ((1ull << lg) < 2ull * (unsigned long long)deg) ++lg;
    const unsigned long long slots = 1ull << lg, mask = slots - 1ull;
    if (slots > cap) continue;                                         // cannot happen: the lists are cut at the tables' sizes
    const int a = p.comm[v];
    for (unsigned long long s = threadIdx.x; s < slots; s += 256) {
      lv_tab_store<GLOBAL>(&keys[s], LV_EMPTY);
      lv_tab_store<GLOBAL>(&vals[s], 0u);
    }
    __syncthreads();
    for (int64_t e = threadIdx.x; e < deg; e += 256) {
      const uint32_t c = (uint32_t)p.comm[p.adj[r0 + e]], w = p.adj_w[r0 + e];
      unsigned long long h = (unsigned long long)((c * 2654435761u) >> (32 - lg)) & mask;
      for (unsigned long long probe = 0; probe < slots; ++probe) {
        const uint32_t prev = atomicCAS(&keys[h], LV_EMPTY, c);
        if (prev == LV_EMPTY || prev == c) {
          atomicAdd(&vals[h], w);
          break;
        }
        h = (h + 1ull) & mask;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t w_a = 0;
      unsigned long long h = (unsigned long long)(((uint32_t)a * 2654435761u) >> (32 - lg)) & mask;
      for (unsigned long long probe = 0; probe < slots; ++probe) {
        const uint32_t key = lv_tab_load<GLOBAL>(&keys[h]);
        if (key == (uint32_t)a) w_a = lv_tab_load<GLOBAL>(&vals[h]);
        if (key == (uint32_t)a || key == LV_EMPTY) break;
        h = (h + 1ull) & mask;
      }
      *s_wa = w_a;
    }
    __syncthreads();
    const long long w_a = *s_wa, k_v = p.k[v], tot_a = p.tot[a];
    long long g = LLONG_MIN;
    int bc = INT_MAX;
    for (unsigned long long s = threadIdx.x; s < slots; s += 256) {
      const uint32_t c = lv_tab_load<GLOBAL>(&keys[s]);
      if (c == LV_EMPTY || c == (uint32_t)a) continue;
      const long long gc = lv_gain(m2, lv_tab_load<GLOBAL>(&vals[s]), w_a, k_v, p.tot[c], tot_a);
      if (lv_better(gc, (int)c, g, bc)) {
        g = gc;
        bc = (int)c;
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const long long og = __shfl_xor(g, d, 64);
      const int oc = __shfl_xor(bc, d, 64);
      if (lv_better(og, oc, g, bc)) {
        g = og;
        bc = oc;
      }
    }
    if (lane == 0) {
      s_g[wave] = g;
      s_c[wave] = bc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int x = 1; x < 4; ++x)
        if (lv_better(s_g[x], s_c[x], g, bc)) {
          g = s_g[x];
          bc = s_c[x];
        }
      if (bc != INT_MAX && g > 0) {
        atomicAdd(p.targets, 1ull);
        if (lv_decide(g, bc, a, p.size)) {
          p.comm_new[v] = bc;
          atomicAdd(p.moved, 1ull);
        }
      }
    }
    __syncthreads();
  }
}

// ---- what a labelling is worth: tot_C, sizes, the weight inside, sum tot_C^2 -------------------------------------------------------
__global__ __launch_bounds__(256) void lv_tot_kernel(int64_t n, const int32_t* __restrict__ comm, const uint32_t* __restrict__ k,
                                                     const uint32_t* __restrict__ loop, uint32_t* tot, uint32_t* size, int64_t* scal) {
  __shared__ long long s_part[4];
  long long acc = 0;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    const int c = comm[v];
    atomicAdd(&tot[c], k[v]);
    atomicAdd(&size[c], 1u);
    acc += 2ll * loop[v];
  }
  const long long r = lv_block_sum(acc, s_part);
  if (threadIdx.x == 0 && r) atomicAdd((unsigned long long*)&scal[LV_S_IN], (unsigned long long)r);
}
// every non-loop edge is listed from both ends: the sum over the entries is twice the weight inside
__global__ __launch_bounds__(256) void lv_inside_kernel(int64_t entries, const int32_t* __restrict__ adj, const int32_t* __restrict__ adj_src,
                                                        const uint32_t* __restrict__ adj_w, const int32_t* __restrict__ comm, int64_t* scal) {
  __shared__ long long s_part[4];
  long long acc = 0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < entries; e += (int64_t)gridDim.x * 256)
    if (comm[adj[e]] == comm[adj_src[e]]) acc += adj_w[e];
  const long long r = lv_block_sum(acc, s_part);
  if (threadIdx.x == 0 && r) atomicAdd((unsigned long long*)&scal[LV_S_IN], (unsigned long long)r);
}
__global__ __launch_bounds__(256) void lv_tot2_kernel(int64_t n, const uint32_t* __restrict__ tot, int64_t* scal) {
  __shared__ long long s_part[4];
  long long acc = 0;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n; c += (int64_t)gridDim.x * 256) acc += (long long)tot[c] * (long long)tot[c];
  const long long r = lv_block_sum(acc, s_part);
  if (threadIdx.x == 0 && r) atomicAdd((unsigned long long*)&scal[LV_S_TOT2], (unsigned long long)r);
}
__global__ void lv_result_kernel(const int64_t* hdr, const int64_t* scal, int64_t* out) {
  out[0] = scal[LV_S_MOVED];
  out[1] = hdr[LV_H_M2] * scal[LV_S_IN] - scal[LV_S_TOT2];
  out[2] = scal[LV_S_TARGETS];
}
__global__ __launch_bounds__(256) void lv_identity_kernel(int64_t n, int32_t* comm) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) comm[v] = (int32_t)v;
}

// ---- after a level --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lv_flag_kernel(int64_t n, const uint32_t* __restrict__ size, uint32_t* flag) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n; c += (int64_t)gridDim.x * 256) flag[c] = size[c] ? 1u : 0u;
}
__global__ __launch_bounds__(256) void lv_compose_kernel(int64_t n0, int64_t* labels, int64_t n, const int32_t* __restrict__ comm,
                                                         const int64_t* __restrict__ newid) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n0; v += (int64_t)gridDim.x * 256) {
    const int64_t x = labels[v];
    if (x >= 0 && x < n) labels[v] = newid[comm[x]];
  }
}
__global__ __launch_bounds__(256) void lv_agg_loops_kernel(int64_t n, const int32_t* __restrict__ comm, const int64_t* __restrict__ newid,
                                                           const uint32_t* __restrict__ loop, uint32_t* out_loops) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256)
    if (loop[v]) atomicAdd(&out_loops[newid[comm[v]]], loop[v]);
}
// each edge once (from its smaller end): inside a community it adds to that community's loop, otherwise to the weight of the
// community pair, found in an open-addressing table keyed by (smaller id, larger id)
__global__ __launch_bounds__(256) void lv_agg_edges_kernel(int64_t entries, const int32_t* __restrict__ adj, const int32_t* __restrict__ adj_src,
                                                           const uint32_t* __restrict__ adj_w, const int32_t* __restrict__ comm,
                                                           const int64_t* __restrict__ newid, uint32_t* out_loops, unsigned long long* keys,
                                                           uint32_t* vals, unsigned lg) {
  const unsigned long long slots = 1ull << lg, mask = slots - 1ull;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < entries; e += (int64_t)gridDim.x * 256) {
    const int src = adj_src[e], dst = adj[e];
    if (src >= dst) continue;
    const unsigned long long a = (unsigned long long)newid[comm[src]], b = (unsigned long long)newid[comm[dst]];
    const uint32_t w = adj_w[e];
    if (a == b) {
      atomicAdd(&out_loops[a], w);
      continue;
    }
    const unsigned long long key = a < b ? (a << 32) | b : (b << 32) | a;
    unsigned long long h = ((key * 0x9E3779B97F4A7C15ull) >> (64 - lg)) & mask;
    for (unsigned long long probe = 0; probe < slots; ++probe) {
      const unsigned long long prev = atomicCAS(&keys[h], LV_EMPTY64, key);
      if (prev == LV_EMPTY64 || prev == key) {
        atomicAdd(&vals[h], w);
        break;
      }
      h = (h + 1ull) & mask;
    }
  }
}
__global__ __launch_bounds__(256) void lv_agg_compact_kernel(unsigned long long slots, const unsigned long long* __restrict__ keys,
                                                             const uint32_t* __restrict__ vals, int64_t cap, int64_t* out_pairs,
                                                             uint32_t* out_w, int64_t* scal) {
  for (unsigned long long s0 = (unsigned long long)blockIdx.x * 256; s0 < slots; s0 += (unsigned long long)gridDim.x * 256) {
    const unsigned long long s = s0 + threadIdx.x;
    const unsigned long long key = s < slots ? keys[s] : LV_EMPTY64;
    const long long pos = lv_wave_append(key != LV_EMPTY64, (unsigned long long*)&scal[LV_S_EDGES]);
    if (key != LV_EMPTY64 && pos < cap) {
      out_pairs[2 * pos] = (int64_t)(key >> 32);
      out_pairs[2 * pos + 1] = (int64_t)(key & 0xffffffffull);
      out_w[pos] = vals[s];
    }
  }
}
__global__ void lv_counts_kernel(const int64_t* newid, int64_t n, const int64_t* scal, int64_t* out) {
  out[0] = newid[n];
  out[1] = scal[LV_S_EDGES];
}
// the start of the atomicMin below: above every vertex index (n0 < 2^31 - 1), which no byte fill can say
__global__ __launch_bounds__(256) void lv_int_max_kernel(int64_t n0, int* minv) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n0; v += (int64_t)gridDim.x * 256) minv[v] = INT_MAX;
}
__global__ __launch_bounds__(256) void lv_min_kernel(int64_t n0, const int64_t* __restrict__ labels, int* minv) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n0; v += (int64_t)gridDim.x * 256) {
    const int64_t x = labels[v];
    if (x >= 0 && x < n0) atomicMin(&minv[x], (int)v);
  }
}
__global__ __launch_bounds__(256) void lv_relabel_kernel(int64_t n0, int64_t* labels, const int* __restrict__ minv) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n0; v += (int64_t)gridDim.x * 256) {
    const int64_t x = labels[v];
    if (x >= 0 && x < n0) labels[v] = minv[x];
  }
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------
extern "C" int rarc_louvain_limits(int* out4) {
  RARC_REQUIRE(out4, RARC_E_INVALID, "rarc_louvain_limits: null pointer");
  out4[0] = LV_DEG_GROUP;
  out4[1] = LV_DEG_WAVE;
  out4[2] = LV_DEG_LDS;
  out4[3] = (int)LV_LDS_SLOTS;
  return RARC_OK;
}

extern "C" size_t rarc_graph_csr_workspace_bytes(int64_t n, int64_t m) {
  if (!lv_shape_ok(n, m)) return 0;
  return lv_graph_carve(nullptr, n, m).bytes;
}

extern "C" int rarc_graph_csr(const int64_t* d_pairs, const uint32_t* d_weights, const uint32_t* d_loops, int64_t n, int64_t m,
                              void* d_graph, size_t graph_bytes, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_pairs && d_graph, RARC_E_INVALID, "rarc_graph_csr: null pointer");
  RARC_REQUIRE(lv_shape_ok(n, m), RARC_E_INVALID, "rarc_graph_csr: n=%lld m=%lld out of range (2 <= n < 2^31 - 1, 1 <= m < 2^30)",
               (long long)n, (long long)m);
  const LvGraph g = lv_graph_carve(d_graph, n, m);
  RARC_REQUIRE(graph_bytes >= g.bytes, RARC_E_WORKSPACE, "rarc_graph_csr: workspace of %zu bytes, %zu needed", graph_bytes, g.bytes);
  hipStream_t s = (hipStream_t)stream;
  RARC_HIP_CHECK(hipMemsetAsync(g.hdr, 0, LV_H_WORDS * 8, s));
  RARC_HIP_CHECK(hipMemsetAsync(g.k, 0, (size_t)n * 4, s));
  RARC_HIP_CHECK(hipMemsetAsync(g.cnt, 0, (size_t)n * 4, s));
  hipLaunchKernelGGL(lv_degree_kernel, dim3(lv_grid(m, 256, 4096)), dim3(256), 0, s, d_pairs, d_weights, m, n, g.cnt, g.k, g.hdr);
  if (int rc = lv_scan(g.cnt, n, g.scan, g.row_ptr, s)) return rc;
  RARC_HIP_CHECK(hipMemsetAsync(g.cnt, 0, (size_t)n * 4, s));
  hipLaunchKernelGGL(lv_fill_kernel, dim3(lv_grid(m, 256, 4096)), dim3(256), 0, s, d_pairs, d_weights, m, n, (const int64_t*)g.row_ptr,
                     g.cnt, g.adj, g.adj_w, g.adj_src);
  hipLaunchKernelGGL(lv_finish_kernel, dim3(lv_grid(n, 256, 2048)), dim3(256), 0, s, n, (const int64_t*)g.row_ptr, d_loops, g.k, g.loop,
                     g.hdr, g.list[0], g.list[1], g.list[2], g.list[3]);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" size_t rarc_louvain_workspace_bytes(int64_t n, int64_t m) {
  if (!lv_shape_ok(n, m)) return 0;
  return lv_state_carve(nullptr, n, m).bytes;
}

#define LV_COMMON_CHECKS(NAME)                                                                                                        \
  RARC_REQUIRE(lv_shape_ok(n, m), RARC_E_INVALID, NAME ": n=%lld m=%lld out of range (2 <= n < 2^31 - 1, 1 <= m < 2^30)", (long long)n, \
               (long long)m);                                                                                                         \
  const LvGraph g = lv_graph_carve(d_graph, n, m);                                                                                    \
  const LvState st = lv_state_carve(d_state, n, m);                                                                                   \
  RARC_REQUIRE(graph_bytes >= g.bytes, RARC_E_WORKSPACE, NAME ": graph workspace of %zu bytes, %zu needed", graph_bytes, g.bytes);    \
  RARC_REQUIRE(state_bytes >= st.bytes, RARC_E_WORKSPACE, NAME ": state workspace of %zu bytes, %zu needed", state_bytes, st.bytes)

// Qn of the labelling in slot `slot` -> d_out3 = {moved, Qn, movers with a target}; tot and size of the slot are rebuilt from its labels
static int lv_evaluate(const LvGraph& g, const LvState& st, int64_t n, int64_t m, int slot, int64_t* d_out3, hipStream_t s) {
  RARC_HIP_CHECK(hipMemsetAsync(st.tot[slot], 0, (size_t)n * 4, s));
  RARC_HIP_CHECK(hipMemsetAsync(st.size[slot], 0, (size_t)n * 4, s));
  hipLaunchKernelGGL(lv_tot_kernel, dim3(lv_grid(n, 256, 2048)), dim3(256), 0, s, n, (const int32_t*)st.comm[slot], (const uint32_t*)g.k,
                     (const uint32_t*)g.loop, st.tot[slot], st.size[slot], st.scal);
  hipLaunchKernelGGL(lv_inside_kernel, dim3(lv_grid(2 * m, 256, 4096)), dim3(256), 0, s, 2 * m, (const int32_t*)g.adj,
                     (const int32_t*)g.adj_src, (const uint32_t*)g.adj_w, (const int32_t*)st.comm[slot], st.scal);
  hipLaunchKernelGGL(lv_tot2_kernel, dim3(lv_grid(n, 256, 2048)), dim3(256), 0, s, n, (const uint32_t*)st.tot[slot], st.scal);
  hipLaunchKernelGGL(lv_result_kernel, dim3(1), dim3(1), 0, s, (const int64_t*)g.hdr, (const int64_t*)st.scal, d_out3);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_louvain_init(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, void* d_state, size_t state_bytes,
                                 int64_t* d_out3, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_graph && d_state && d_out3, RARC_E_INVALID, "rarc_louvain_init: null pointer");
  LV_COMMON_CHECKS("rarc_louvain_init");
  hipStream_t s = (hipStream_t)stream;
  RARC_HIP_CHECK(hipMemsetAsync(st.scal, 0, LV_S_WORDS * 8, s));
  hipLaunchKernelGGL(lv_identity_kernel, dim3(lv_grid(n, 256, 2048)), dim3(256), 0, s, n, st.comm[0]);
  return lv_evaluate(g, st, n, m, 0, d_out3, s);
}

extern "C" int rarc_louvain_sweep(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, void* d_state, size_t state_bytes, int cur,
                                  int sweep, int64_t* d_out3, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_graph && d_state && d_out3, RARC_E_INVALID, "rarc_louvain_sweep: null pointer");
  RARC_REQUIRE(sweep >= 0, RARC_E_INVALID, "rarc_louvain_sweep: sweep index %d is negative", sweep);
  RARC_REQUIRE(cur == 0 || cur == 1, RARC_E_INVALID, "rarc_louvain_sweep: slot %d is neither 0 nor 1", cur);
  LV_COMMON_CHECKS("rarc_louvain_sweep");
  hipStream_t s = (hipStream_t)stream;
  static RarcPerDevice attr_dev;
  size_t& attr = attr_dev.cur();
  if (!attr) {
    RARC_HIP_CHECK(hipFuncSetAttribute((const void*)lv_sweep_hash_kernel<false, 2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)LV_LDS_BYTES));
    attr = 1;
  }
  const int nxt = cur ^ 1;
  RARC_HIP_CHECK(hipMemsetAsync(st.scal, 0, LV_S_WORDS * 8, s));
  RARC_HIP_CHECK(hipMemcpyAsync(st.comm[nxt], st.comm[cur], (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  LvSweepArgs p;
  p.hdr = g.hdr;
  p.row_ptr = g.row_ptr;
  p.adj = g.adj;
  p.adj_w = g.adj_w;
  p.k = g.k;
  p.comm = st.comm[cur];
  p.tot = st.tot[cur];
  p.size = st.size[cur];
  p.comm_new = st.comm[nxt];
  p.moved = (unsigned long long*)&st.scal[LV_S_MOVED];
  p.targets = (unsigned long long*)&st.scal[LV_S_TARGETS];
  p.t = sweep;
  const int64_t dmax = lv_max_degree(n, m);          // no vertex of this graph has more neighbours: skip the lists that must be empty
  hipLaunchKernelGGL((lv_sweep_group_kernel<LV_DEG_GROUP, 0>), dim3(lv_grid(n, 256 / LV_DEG_GROUP, 4096)), dim3(256), 0, s, p,
                     (const int32_t*)g.list[0]);
  if (dmax > LV_DEG_GROUP)
    hipLaunchKernelGGL((lv_sweep_group_kernel<LV_DEG_WAVE, 1>), dim3(lv_grid(n, 256 / LV_DEG_WAVE, 4096)), dim3(256), 0, s, p,
                       (const int32_t*)g.list[1]);
  if (dmax > LV_DEG_WAVE)
    hipLaunchKernelGGL((lv_sweep_hash_kernel<false, 2>), dim3(lv_grid(n, 1, 512)), dim3(256), LV_LDS_BYTES, s, p, (const int32_t*)g.list[2],
                       (uint32_t*)nullptr, 0ull);
  if (dmax > LV_DEG_LDS)
    hipLaunchKernelGGL((lv_sweep_hash_kernel<true, 3>), dim3((unsigned)lv_global_blocks(n, m)), dim3(256), 64, s, p, (const int32_t*)g.list[3],
                       (uint32_t*)st.table, lv_global_slots(n, m));
  RARC_HIP_CHECK(hipGetLastError());
  return lv_evaluate(g, st, n, m, nxt, d_out3, s);
}

extern "C" int rarc_louvain_aggregate(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, void* d_state, size_t state_bytes,
                                      int cur, int64_t* d_labels, int64_t n0, int64_t* d_out_pairs, uint32_t* d_out_weights,
                                      uint32_t* d_out_loops, int64_t* d_out_counts, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_graph && d_state && d_labels && d_out_pairs && d_out_weights && d_out_loops && d_out_counts, RARC_E_INVALID,
               "rarc_louvain_aggregate: null pointer");
  RARC_REQUIRE(cur == 0 || cur == 1, RARC_E_INVALID, "rarc_louvain_aggregate: slot %d is neither 0 nor 1", cur);
  RARC_REQUIRE(n0 >= n && n0 < LV_N_LIMIT, RARC_E_INVALID, "rarc_louvain_aggregate: n0=%lld out of range (n <= n0 < 2^31 - 1)", (long long)n0);
  LV_COMMON_CHECKS("rarc_louvain_aggregate");
  hipStream_t s = (hipStream_t)stream;
  unsigned lg = 10;
  while ((1ull << lg) < lv_pair_slots(m)) ++lg;
  const unsigned long long slots = 1ull << lg;
  unsigned long long* keys = (unsigned long long*)st.table;
  uint32_t* vals = (uint32_t*)(st.table + slots * 8);
  RARC_HIP_CHECK(hipMemsetAsync(st.scal, 0, LV_S_WORDS * 8, s));
  RARC_HIP_CHECK(hipMemsetAsync(keys, 0xff, slots * 8, s));
  RARC_HIP_CHECK(hipMemsetAsync(vals, 0, slots * 4, s));
  RARC_HIP_CHECK(hipMemsetAsync(d_out_loops, 0, (size_t)n * 4, s));
  hipLaunchKernelGGL(lv_flag_kernel, dim3(lv_grid(n, 256, 2048)), dim3(256), 0, s, n, (const uint32_t*)st.size[cur], st.flag);
  if (int rc = lv_scan(st.flag, n, st.scan, st.newid, s)) return rc;
  hipLaunchKernelGGL(lv_compose_kernel, dim3(lv_grid(n0, 256, 2048)), dim3(256), 0, s, n0, d_labels, n, (const int32_t*)st.comm[cur],
                     (const int64_t*)st.newid);
  hipLaunchKernelGGL(lv_agg_loops_kernel, dim3(lv_grid(n, 256, 2048)), dim3(256), 0, s, n, (const int32_t*)st.comm[cur],
                     (const int64_t*)st.newid, (const uint32_t*)g.loop, d_out_loops);
  hipLaunchKernelGGL(lv_agg_edges_kernel, dim3(lv_grid(2 * m, 256, 4096)), dim3(256), 0, s, 2 * m, (const int32_t*)g.adj,
                     (const int32_t*)g.adj_src, (const uint32_t*)g.adj_w, (const int32_t*)st.comm[cur], (const int64_t*)st.newid, d_out_loops,
                     keys, vals, lg);
  hipLaunchKernelGGL(lv_agg_compact_kernel, dim3(lv_grid((int64_t)slots, 256, 4096)), dim3(256), 0, s, slots, (const unsigned long long*)keys,
                     (const uint32_t*)vals, m, d_out_pairs, d_out_weights, st.scal);
  hipLaunchKernelGGL(lv_counts_kernel, dim3(1), dim3(1), 0, s, (const int64_t*)st.newid, n, (const int64_t*)st.scal, d_out_counts);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" size_t rarc_louvain_labels_workspace_bytes(int64_t n0) {
  if (n0 < 1 || n0 >= LV_N_LIMIT) return 0;
  return lv_align((size_t)n0 * 4);
}

extern "C" int rarc_louvain_labels(int64_t* d_labels, int64_t n0, void* d_ws, size_t ws_bytes, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_labels && d_ws, RARC_E_INVALID, "rarc_louvain_labels: null pointer");
  RARC_REQUIRE(n0 >= 1 && n0 < LV_N_LIMIT, RARC_E_INVALID, "rarc_louvain_labels: n0=%lld out of range (1 <= n0 < 2^31 - 1)", (long long)n0);
  RARC_REQUIRE(ws_bytes >= lv_align((size_t)n0 * 4), RARC_E_WORKSPACE, "rarc_louvain_labels: workspace of %zu bytes, %zu needed", ws_bytes,
               lv_align((size_t)n0 * 4));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lv_int_max_kernel, dim3(lv_grid(n0, 256, 2048)), dim3(256), 0, s, n0, (int*)d_ws);
  hipLaunchKernelGGL(lv_min_kernel, dim3(lv_grid(n0, 256, 2048)), dim3(256), 0, s, n0, (const int64_t*)d_labels, (int*)d_ws);
  hipLaunchKernelGGL(lv_relabel_kernel, dim3(lv_grid(n0, 256, 2048)), dim3(256), 0, s, n0, d_labels, (const int*)d_ws);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}
