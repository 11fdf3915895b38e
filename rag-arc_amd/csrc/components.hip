// components.hip — connected components of the GRAPH blob rarc_graph_csr wrote: which vertices are joined at all,
// how many pieces the graph has and how large they are — what a graph store answers with gds.wcc.
//
// The rule (tests/components_ref.py restates it in Python): a parent word p[v] per vertex, p[v] = v at first.  A round starts from
// a star forest (every p[v] is a root, p[p[v]] == p[v]) and
//   hook   for every adjacency entry (u, v) with ru = p[u], rv = p[v] AS THEY STOOD AT THE START OF THE ROUND and rv < ru:
//          p[ru] = min(p[ru], rv).  After it p[r] is the smallest root among the trees next to r's tree, r itself included: a min
//          over a set, the same for any order of the edges and any timing of the threads
//   jump   every vertex follows p to its root and stores it.  A hook points at a smaller index only: no cycle, and a root is
//          written by nobody in this pass
//   the changed word tells whether any hook lowered a parent; the first round that lowers none ends the run.
// label(v) = p[v] is then the smallest vertex of v's component (the convention of rarc_louvain_labels).  The whole state after
// every round is a function of the graph alone, so the number of rounds is part of the answer.  A tree that is no local minimum
// among its neighbouring trees hooks; one that is either has a neighbour hooked into it or sees only smaller roots in the next
// round and hooks then: the trees that still have an outside edge at least halve over two rounds, 2 ceil(log2 n) +
// CC_ROUND_SLACK rounds are enough for any graph (the last finds nothing to do), and ceil(log2 n) + CC_ROUND_SLACK for every
// graph of the tests (DESIGN §4.13j has the argument and what a search over small graphs found).
//
// "As they stood at the start" is two arrays: the hook reads `p`, which nobody writes in that launch, and lowers `q`, a copy of
// it, with one integer atomicMin a vertex — the entries of a vertex are folded to their minimum in registers first.  The jump
// reads `q` and leaves the root in both.  It is pointer doubling on the vertex's own word, q[v] = q[q[v]] until q[v] is a root:
// a thread writes no word but its own, and a word another thread reads while it shrinks names an ancestor before and after, so
// the root found does not depend on what a reader saw.  Ancestors have smaller indices and are visited earlier or at the same
// time: a chain of hooks of any length is walked in about log2 of its length steps, not one step a link.
//
// The hook takes the degree classes of the blob (graph_csr.h): up to LV_DEG_GROUP = 8 neighbours 8 lanes a vertex, one entry a
// lane; up to LV_DEG_WAVE = 64 a quarter wave a vertex, four vertices a wave, up to four entries a lane; above that a workgroup
// a vertex (list 2, and list 3 above LV_DEG_LDS = 8192), joined by wave reductions and four words of LDS.  A vertex without
// neighbours is in no list and is read by nobody.
//
// The finish counts the members of every root (one atomic add per wave and distinct root), numbers the roots in ascending
// order (flag, scan, scatter, as rarc_louvain_aggregate numbers communities), and finds the largest component as the maximum
// of size << 32 | ~root: ties go to the smaller label.
//
// The workspace is {largest key u64 | components i64} | p i32 [n] | q i32 [n] | sizes by root u32 [n] | rank of a root i32 [n] |
// tile sums i64 [tiles + 1].
#include "graph_csr.h"

constexpr int CC_ROUND_SLACK = 2;                           // the additive constant of the round bounds
#ifndef CC_MID_LANES_BUILD                                  // (-DCC_MID_LANES_BUILD=64: a wave per vertex, for tools/components_bench.py --trace)
#define CC_MID_LANES_BUILD 16
#endif
constexpr int CC_MID_LANES = CC_MID_LANES_BUILD;            // lanes that share a vertex of 9 .. 64 neighbours
static_assert(CC_MID_LANES == 8 || CC_MID_LANES == 16 || CC_MID_LANES == 32 || CC_MID_LANES == 64, "a power of two that divides a wave");
constexpr int CC_NONE = 0x7fffffff;                         // no parent: parents are < n < 2^31 - 1
constexpr size_t CC_CTL_BYTES = 256;
constexpr int CC_VERTEX_BLOCKS = 4096;                      // workgroups of a thread-per-vertex launch: 2^20 vertices a pass

typedef unsigned long long u64;

struct CcWs {
  u64* key;                                                 // size << 32 | ~root of the largest component
  int64_t* count;                                           // the number of components
  int32_t* p;
  int32_t* q;
  uint32_t* size;                                           // [root]
  int32_t* rank;                                            // [root]
  int64_t* scan;
  size_t bytes;
};
static CcWs cc_carve(const void* base, int64_t n) {
  char* b = (char*)base;
  size_t o = 0;
  CcWs w;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  char* ctl = take(CC_CTL_BYTES);
  w.key = (u64*)ctl;
  w.count = (int64_t*)(ctl + 8);
  w.p = (int32_t*)take((size_t)n * 4);
  w.q = (int32_t*)take((size_t)n * 4);
  w.size = (uint32_t*)take((size_t)n * 4);
  w.rank = (int32_t*)take((size_t)n * 4);
  w.scan = (int64_t*)take((size_t)(lv_scan_blocks(n) + 1) * 8);
  w.bytes = o;
  return w;
}

// ---- init ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cc_init_kernel(int64_t n, int32_t* p, int32_t* q) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    p[v] = (int32_t)v;
    q[v] = (int32_t)v;
  }
}

// ---- the hook -----------------------------------------------------------------------------------------------------------------------
struct CcHookArgs {
  const int64_t* hdr;
  const int64_t* row_ptr;
  const int32_t* adj;
  const int32_t* p;                                         // the parents at the start of the round: only read
  int32_t* q;                                               // a copy of them: only lowered
  int32_t* changed;
  int64_t n;
  int64_t entries;                                          // 2 m
};

__device__ __forceinline__ int64_t cc_list_count(const CcHookArgs& a, int bucket) {
  const int64_t c = a.hdr[LV_H_LIST + bucket];
  return c < 0 ? 0 : (c > a.n ? a.n : c);
}
// the parent of the neighbour in entry e, CC_NONE for an entry that names no vertex
__device__ __forceinline__ int cc_parent_of_entry(const CcHookArgs& a, int64_t e) {
  const int32_t u = a.adj[e];
  return (uint32_t)u < (uint64_t)a.n ? a.p[u] : CC_NONE;
}

// W lanes per vertex of list BUCKET, lane j entries j, j + W, ..; the lanes are joined by shuffle-mins and lane 0 hooks
template <int W, int BUCKET>
__global__ __launch_bounds__(256) void cc_hook_group_kernel(const CcHookArgs a, const int32_t* __restrict__ list) {
  constexpr int GPB = 256 / W;
  const int64_t n_list = cc_list_count(a, BUCKET);
  const int sub = threadIdx.x % W, grp = threadIdx.x / W;
  bool changed = false;
  for (int64_t i0 = (int64_t)blockIdx.x * GPB; i0 < n_list; i0 += (int64_t)gridDim.x * GPB) {     // (workgroup-uniform)
    const int64_t i = i0 + grp;
    int64_t v = i < n_list ? (int64_t)list[i] : -1;
    v = v < a.n ? v : -1;
    int mn = CC_NONE;
    if (v >= 0) {
      int64_t r0 = a.row_ptr[v], r1 = a.row_ptr[v + 1];
      r0 = r0 < 0 ? 0 : (r0 > a.entries ? a.entries : r0);
      r1 = r1 < r0 ? r0 : (r1 > a.entries ? a.entries : r1);
      for (int64_t e = r0 + sub; e < r1; e += W) {
        const int rv = cc_parent_of_entry(a, e);
        mn = rv < mn ? rv : mn;
      }
    }
#pragma unroll
    for (int d = W / 2; d >= 1; d >>= 1) {
      const int o = __shfl_xor(mn, d, W);
      mn = o < mn ? o : mn;
    }
    if (sub == 0 && v >= 0) {
      const int ru = a.p[v];
      if (mn < ru && (uint32_t)ru < (uint64_t)a.n) {                     // (ru names a vertex unless nobody initialised the workspace)
        atomicMin(&a.q[ru], mn);
        changed = true;
      }
    }
  }
  if (__builtin_amdgcn_ballot_w64(changed) && (threadIdx.x & 63) == 0) atomicOr(a.changed, 1);
}

// a workgroup per vertex of list `bucket`: 256 entries a pass, the waves joined in LDS, thread 0 hooks
__global__ __launch_bounds__(256) void cc_hook_block_kernel(const CcHookArgs a, const int32_t* __restrict__ list, int bucket) {
  __shared__ int s_min[4];
  const int64_t n_list = cc_list_count(a, bucket);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool changed = false;
  for (int64_t i = blockIdx.x; i < n_list; i += gridDim.x) {                                        // (workgroup-uniform)
    const int64_t v = list[i];
    if (v < 0 || v >= a.n) continue;
    int64_t r0 = a.row_ptr[v], r1 = a.row_ptr[v + 1];
    r0 = r0 < 0 ? 0 : (r0 > a.entries ? a.entries : r0);
    r1 = r1 < r0 ? r0 : (r1 > a.entries ? a.entries : r1);
    int mn = CC_NONE;
#pragma unroll 4
    for (int64_t e = r0 + threadIdx.x; e < r1; e += 256) {
      const int rv = cc_parent_of_entry(a, e);
      mn = rv < mn ? rv : mn;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const int o = __shfl_xor(mn, d, 64);
      mn = o < mn ? o : mn;
    }
    if (lane == 0) s_min[wave] = mn;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m01 = s_min[0] < s_min[1] ? s_min[0] : s_min[1], m23 = s_min[2] < s_min[3] ? s_min[2] : s_min[3];
      mn = m01 < m23 ? m01 : m23;
      const int ru = a.p[v];
      if (mn < ru && (uint32_t)ru < (uint64_t)a.n) {                     // (ru names a vertex unless nobody initialised the workspace)
        atomicMin(&a.q[ru], mn);
        changed = true;
      }
    }
    __syncthreads();
  }
  if (changed) atomicOr(a.changed, 1);
}

// ---- the jump -----------------------------------------------------------------------------------------------------------------------
// a thread per vertex, in ascending order: q[v] = q[q[v]] until q[v] is a root, then p[v] = q[v].  Only v's thread writes q[v]
// and p[v]; the words of other vertices it reads name an ancestor of theirs whenever they are read.  The answer does not
// depend on how fresh such a word is, the number of steps does: the words go through agent-scope accesses, past the L1 of the
// compute unit and visible to every XCD, so that the doubling of one thread shortens the walk of the others
__global__ __launch_bounds__(256) void cc_jump_kernel(int64_t n, int32_t* p, int32_t* q) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    int a = q[v];                                                      // (written by the hook launch or by this thread: a plain load)
    for (;;) {
      if ((uint32_t)a >= (uint64_t)n) break;                           // (no vertex: a workspace nobody initialised)
      const int b = __hip_atomic_load(&q[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (b == a) break;
      __hip_atomic_store(&q[v], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      a = b;
    }
    p[v] = a;
  }
}

// ---- the finish ---------------------------------------------------------------------------------------------------------------------
// labels[v] = p[v], and size[r] = the vertices whose root is r: the lanes of a wave that share a root add once
__global__ __launch_bounds__(256) void cc_count_kernel(int64_t n, const int32_t* __restrict__ p, int64_t* __restrict__ labels, uint32_t* size) {
  const int lane = threadIdx.x & 63;
  for (int64_t v0 = (int64_t)blockIdx.x * 256; v0 < n; v0 += (int64_t)gridDim.x * 256) {           // (workgroup-uniform)
    const int64_t v = v0 + threadIdx.x;
    int r = -1;
    if (v < n) {
      r = p[v];
      labels[v] = (int64_t)r;
    }
    bool todo = (uint32_t)r < (uint64_t)n;
    for (u64 left = __builtin_amdgcn_ballot_w64(todo); left; left = __builtin_amdgcn_ballot_w64(todo)) {     // (wave-uniform)
      const int leader = __builtin_ctzll(left);
      const int lr = __shfl(r, leader, 64);
      const u64 same = __builtin_amdgcn_ballot_w64(todo && r == lr);
      if (lane == leader) atomicAdd(&size[lr], (uint32_t)__builtin_popcountll(same));
      todo = todo && r != lr;
    }
  }
}

// the roots of a tile of LV_SCAN_TILE vertices
__global__ __launch_bounds__(256) void cc_scan_sums_kernel(const int32_t* __restrict__ p, int64_t n, int64_t* __restrict__ bsum) {
  __shared__ int s_part[4];
  const int64_t base = (int64_t)blockIdx.x * LV_SCAN_TILE + (int64_t)threadIdx.x * 8;
  int acc = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (base + j < n) acc += p[base + j] == (int32_t)(base + j) ? 1 : 0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = (int64_t)((s_part[0] + s_part[1]) + (s_part[2] + s_part[3]));
}
// inclusive scan of one value per thread over the block (s: 256 words of LDS)
__device__ __forceinline__ long long cc_block_scan(long long x, long long* s) {
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
// one workgroup: the tile sums become exclusive offsets, bsum[nb] their total
__global__ __launch_bounds__(256) void cc_scan_offsets_kernel(int64_t* bsum, int64_t nb) {
  __shared__ long long s[256];
  long long carry = 0;
  for (int64_t base = 0; base < nb; base += 256) {
    const int64_t i = base + threadIdx.x;
    const long long x = i < nb ? bsum[i] : 0;
    const long long incl = cc_block_scan(x, s);
    if (i < nb) bsum[i] = carry + incl - x;
    if (threadIdx.x == 255) s[0] = incl;
    __syncthreads();
    carry += s[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) bsum[nb] = carry;
}
// the tiles again: a root learns its rank among the roots, its size goes to sizes[rank], and the largest (size, ~root) is kept
__global__ __launch_bounds__(256) void cc_scan_apply_kernel(const int32_t* __restrict__ p, int64_t n, const int64_t* __restrict__ bsum,
                                                            const uint32_t* __restrict__ size, int32_t* __restrict__ rank,
                                                            int64_t* __restrict__ sizes, u64* key_out, int64_t* count_out) {
  __shared__ long long s[256];
  const int64_t base = (int64_t)blockIdx.x * LV_SCAN_TILE + (int64_t)threadIdx.x * 8;
  bool root[8];
  int acc = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    root[j] = base + j < n && p[base + j] == (int32_t)(base + j);
    acc += root[j] ? 1 : 0;
  }
  long long run = bsum[blockIdx.x] + cc_block_scan(acc, s) - acc;
  u64 key = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (root[j]) {
      const uint32_t sz = size[base + j];
      rank[base + j] = (int32_t)run;
      if (sizes) sizes[run] = (int64_t)sz;
      const u64 k = (u64)sz << 32 | (u64)(0xffffffffu - (uint32_t)(base + j));
      key = k > key ? k : key;
      ++run;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 o = (u64)__shfl_xor((long long)key, d, 64);
    key = o > key ? o : key;
  }
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = (long long)key;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) key = (u64)s[w] > key ? (u64)s[w] : key;
    if (key) atomicMax(key_out, key);
    if (blockIdx.x == gridDim.x - 1) *count_out = bsum[gridDim.x];
  }
}
// dense[v] = the rank of v's root; the first thread writes {components, largest size, label of the largest}
__global__ __launch_bounds__(256) void cc_dense_kernel(int64_t n, const int32_t* __restrict__ p, const int32_t* __restrict__ rank,
                                                       int32_t* __restrict__ dense, const u64* __restrict__ key, const int64_t* __restrict__ count,
                                                       int64_t* out3) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const u64 k = *key;
    out3[0] = *count;
    out3[1] = (int64_t)(k >> 32);
    out3[2] = (int64_t)(0xffffffffu - (uint32_t)k);
  }
  if (!dense) return;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    const int r = p[v];
    dense[v] = (uint32_t)r < (uint64_t)n ? rank[r] : -1;
  }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" int rarc_components_limits(int* out4) {
  RARC_REQUIRE(out4, RARC_E_INVALID, "rarc_components_limits: null pointer");
  out4[0] = LV_DEG_GROUP;
  out4[1] = LV_DEG_WAVE;
  out4[2] = LV_DEG_LDS;
  out4[3] = CC_ROUND_SLACK;
  return RARC_OK;
}

extern "C" size_t rarc_components_workspace_bytes(int64_t n, int64_t m) {
  if (!lv_shape_ok(n, m)) return 0;
  return cc_carve(nullptr, n).bytes;
}

#define CC_ALIGNED(P, A) (((uintptr_t)(P) & (uintptr_t)((A)-1)) == 0)
#define CC_SHAPE_CHECKS(NAME)                                                                                                          \
  RARC_REQUIRE(lv_shape_ok(n, m), RARC_E_INVALID, NAME ": n=%lld m=%lld out of range (2 <= n < 2^31 - 1, 1 <= m < 2^30)", (long long)n, \
               (long long)m);                                                                                                          \
  RARC_REQUIRE(CC_ALIGNED(d_ws, 256), RARC_E_INVALID, NAME ": the workspace is not 256-byte aligned");                                  \
  const CcWs ws = cc_carve(d_ws, n);                                                                                                   \
  RARC_REQUIRE(ws_bytes >= ws.bytes, RARC_E_WORKSPACE, NAME ": workspace of %zu bytes, %zu needed", ws_bytes, ws.bytes)

extern "C" int rarc_components_init(int64_t n, int64_t m, void* d_ws, size_t ws_bytes, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_ws, RARC_E_INVALID, "rarc_components_init: null pointer");
  CC_SHAPE_CHECKS("rarc_components_init");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_init_kernel, dim3(lv_grid(n, 256, CC_VERTEX_BLOCKS)), dim3(256), 0, s, n, ws.p, ws.q);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_components_round(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, void* d_ws, size_t ws_bytes,
                                     int32_t* d_changed, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_graph && d_ws && d_changed, RARC_E_INVALID, "rarc_components_round: null pointer");
  RARC_REQUIRE(CC_ALIGNED(d_graph, 256), RARC_E_INVALID, "rarc_components_round: the graph is not 256-byte aligned");
  RARC_REQUIRE(CC_ALIGNED(d_changed, 4), RARC_E_INVALID, "rarc_components_round: the changed word is not 4-byte aligned");
  CC_SHAPE_CHECKS("rarc_components_round");
  const LvGraph g = lv_graph_carve(d_graph, n, m);
  RARC_REQUIRE(graph_bytes >= g.bytes, RARC_E_WORKSPACE, "rarc_components_round: graph workspace of %zu bytes, %zu needed", graph_bytes, g.bytes);
  hipStream_t s = (hipStream_t)stream;
  CcHookArgs a;
  a.hdr = g.hdr;
  a.row_ptr = g.row_ptr;
  a.adj = g.adj;
  a.p = ws.p;
  a.q = ws.q;
  a.changed = d_changed;
  a.n = n;
  a.entries = 2 * m;
  RARC_HIP_CHECK(hipMemsetAsync(d_changed, 0, 4, s));
  // a list of degree class c holds at most 2 m / (its smallest degree) vertices, and none where no vertex can have that degree
  const int64_t dmax = lv_max_degree(n, m);
  auto at_most = [&](int64_t least_degree) { const int64_t c = 2 * m / least_degree; return c < n ? c : n; };
  hipLaunchKernelGGL((cc_hook_group_kernel<LV_DEG_GROUP, 0>), dim3(lv_grid(n, 256 / LV_DEG_GROUP, 8192)), dim3(256), 0, s, a,
                     (const int32_t*)g.list[0]);
  if (dmax > LV_DEG_GROUP)
    hipLaunchKernelGGL((cc_hook_group_kernel<CC_MID_LANES, 1>), dim3(lv_grid(at_most(LV_DEG_GROUP + 1), 256 / CC_MID_LANES, 8192)), dim3(256), 0, s,
                       a, (const int32_t*)g.list[1]);
  if (dmax > LV_DEG_WAVE)
    hipLaunchKernelGGL(cc_hook_block_kernel, dim3(lv_grid(at_most(LV_DEG_WAVE + 1), 1, 2048)), dim3(256), 0, s, a, (const int32_t*)g.list[2], 2);
  if (dmax > LV_DEG_LDS)
    hipLaunchKernelGGL(cc_hook_block_kernel, dim3(lv_grid(at_most(LV_DEG_LDS + 1), 1, 2048)), dim3(256), 0, s, a, (const int32_t*)g.list[3], 3);
  hipLaunchKernelGGL(cc_jump_kernel, dim3(lv_grid(n, 256, CC_VERTEX_BLOCKS)), dim3(256), 0, s, n, ws.p, ws.q);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_components_finish(int64_t n, int64_t m, void* d_ws, size_t ws_bytes, int64_t* d_labels, int32_t* d_dense, int64_t* d_sizes,
                                      int64_t* d_out3, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_ws && d_labels && d_out3, RARC_E_INVALID, "rarc_components_finish: null pointer");
  RARC_REQUIRE(CC_ALIGNED(d_labels, 8) && CC_ALIGNED(d_dense, 4) && CC_ALIGNED(d_sizes, 8) && CC_ALIGNED(d_out3, 8), RARC_E_INVALID,
               "rarc_components_finish: an output is not aligned to its element (labels, sizes and out3 8 bytes, dense 4)");
  CC_SHAPE_CHECKS("rarc_components_finish");
  hipStream_t s = (hipStream_t)stream;
  const unsigned tiles = (unsigned)lv_scan_blocks(n);
  RARC_HIP_CHECK(hipMemsetAsync(ws.key, 0, CC_CTL_BYTES, s));
  RARC_HIP_CHECK(hipMemsetAsync(ws.size, 0, (size_t)n * 4, s));
  hipLaunchKernelGGL(cc_count_kernel, dim3(lv_grid(n, 256, CC_VERTEX_BLOCKS)), dim3(256), 0, s, n, (const int32_t*)ws.p, d_labels, ws.size);
  hipLaunchKernelGGL(cc_scan_sums_kernel, dim3(tiles), dim3(256), 0, s, (const int32_t*)ws.p, n, ws.scan);
  hipLaunchKernelGGL(cc_scan_offsets_kernel, dim3(1), dim3(256), 0, s, ws.scan, (int64_t)tiles);
  hipLaunchKernelGGL(cc_scan_apply_kernel, dim3(tiles), dim3(256), 0, s, (const int32_t*)ws.p, n, (const int64_t*)ws.scan, (const uint32_t*)ws.size,
                     ws.rank, d_sizes, ws.key, ws.count);
  hipLaunchKernelGGL(cc_dense_kernel, dim3(d_dense ? lv_grid(n, 256, CC_VERTEX_BLOCKS) : 1u), dim3(256), 0, s, n, (const int32_t*)ws.p, (const int32_t*)ws.rank,
                     d_dense, (const u64*)ws.key, (const int64_t*)ws.count, d_out3);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}
