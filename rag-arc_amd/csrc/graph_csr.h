// graph_csr.h — the layout of the GRAPH blob rarc_graph_csr writes (csrc/louvain.hip), shared with the kernels that only read
// it (csrc/ppr.hip): one adjacency format, carved the same way by whoever holds the pointer.
#pragma once
#include "rarc_common.h"

constexpr int LV_DEG_GROUP = 8;
constexpr int LV_DEG_WAVE = 64;
constexpr int LV_DEG_LDS = 8192;
constexpr int64_t LV_N_LIMIT = 0x7fffffffll;                // n < 2^31 - 1
constexpr int64_t LV_M_LIMIT = 1ll << 30;                   // m < 2^30: M2 < 2^31, every product below fits int64
constexpr int LV_SCAN_TILE = 2048;                          // 256 threads x 8 items
enum { LV_H_M2 = 0, LV_H_LIST = 1, LV_H_BAD = 5, LV_H_WORDS = 32 };

static inline size_t lv_align(size_t b) { return (b + 255) & ~(size_t)255; }
static inline int64_t lv_scan_blocks(int64_t n) { return (n + LV_SCAN_TILE - 1) / LV_SCAN_TILE; }
static inline bool lv_shape_ok(int64_t n, int64_t m) { return n >= 2 && n < LV_N_LIMIT && m >= 1 && m < LV_M_LIMIT; }
static inline int64_t lv_max_degree(int64_t n, int64_t m) { return n - 1 < m ? n - 1 : m; }
static inline unsigned lv_grid(int64_t items, int per_block, int cap) {
  int64_t b = (items + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

struct LvGraph {
  int64_t* hdr;
  int64_t* row_ptr;
  uint32_t *k, *loop, *cnt;
  int32_t* adj;
  uint32_t* adj_w;
  int32_t* adj_src;
  int32_t* list[4];
  int64_t* scan;
  size_t bytes;
};
static inline LvGraph lv_graph_carve(const void* base, int64_t n, int64_t m) {
  char* b = (char*)base;
  size_t o = 0;
  LvGraph g;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  g.hdr = (int64_t*)take(LV_H_WORDS * 8);
  g.row_ptr = (int64_t*)take((size_t)(n + 1) * 8);
  g.k = (uint32_t*)take((size_t)n * 4);
  g.loop = (uint32_t*)take((size_t)n * 4);
  g.cnt = (uint32_t*)take((size_t)n * 4);
  g.adj = (int32_t*)take((size_t)m * 8);
  g.adj_w = (uint32_t*)take((size_t)m * 8);
  g.adj_src = (int32_t*)take((size_t)m * 8);
  for (int i = 0; i < 4; ++i) g.list[i] = (int32_t*)take((size_t)n * 4);
  g.scan = (int64_t*)take((size_t)(lv_scan_blocks(n) + 1) * 8);
  g.bytes = o;
  return g;
}
