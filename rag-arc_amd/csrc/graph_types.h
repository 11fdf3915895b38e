// graph_types.h — the layout of the typed adjacency rarc_graph_types and rarc_graph_types_weighted write (csrc/khop.hip), shared
// with the kernels that only read it (csrc/ppr.hip): t_adj int32 [2m] | t_mask uint32 [2m] | cursor uint32 [n] | bad u32, and
// behind them, in the weighted form only, t_w uint32 [2m].  The unweighted blob is a prefix of the
// weighted one: `bytes` is the size of the first, `weighted_bytes` of the second.
#pragma once
#include "graph_csr.h"

struct KhopTypes {
  int32_t* adj;
  uint32_t* mask;
  uint32_t* cursor;
  uint32_t* bad;
  uint32_t* w;                                              // (past `bytes`: only a blob of `weighted_bytes` holds it)
  size_t bytes;
  size_t weighted_bytes;
};
static inline KhopTypes khop_types_carve(const void* base, int64_t n, int64_t m) {
  char* b = (char*)base;
  size_t o = 0;
  KhopTypes t;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  t.adj = (int32_t*)take((size_t)m * 8);
  t.mask = (uint32_t*)take((size_t)m * 8);
  t.cursor = (uint32_t*)take((size_t)n * 4);
  t.bad = (uint32_t*)take(4);
  t.bytes = o;
  t.w = (uint32_t*)take((size_t)m * 8);
  t.weighted_bytes = o;
  return t;
}
