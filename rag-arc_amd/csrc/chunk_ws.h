// chunk_ws.h — the layout of the chunk workspace (rarc_ppr_chunks_workspace_bytes), shared by whoever writes the chunk state S
// (csrc/ppr.hip from the PPR mass, csrc/khop.hip from the hop levels) and by the kernels of csrc/ppr.hip that transpose, key
// and rank it: {positive counts u32 [256]} | S u64 [n_chunks][B] | keys u64 [B][n_chunks].
#pragma once
#include "graph_csr.h"

constexpr int PPR_MAX_B = 256;
constexpr int PPR_CHUNK_WEIGHT_BITS = 12;
constexpr int64_t PPR_CHUNK_N_LIMIT = LV_N_LIMIT;             // n_chunks < 2^31 - 1: a chunk id is an int32 in the split list
constexpr size_t PPR_CHUNK_CTL_BYTES = 1024;                // positive u32 [256]

struct PprChunkWs {
  uint32_t* positive;
  unsigned long long* s;
  unsigned long long* keys;
  size_t bytes;
};
static inline bool ppr_chunk_shape_ok(int64_t n_chunks, int nq) { return n_chunks >= 1 && n_chunks < PPR_CHUNK_N_LIMIT && nq >= 1 && nq <= PPR_MAX_B; }
static inline PprChunkWs ppr_chunk_carve(const void* base, int64_t n_chunks, int nq) {
  char* b = (char*)base;
  size_t o = 0;
  PprChunkWs w;
  auto take = [&](size_t bytes) { char* p = b + o; o += lv_align(bytes); return p; };
  w.positive = (uint32_t*)take(PPR_CHUNK_CTL_BYTES);
  const size_t state = (size_t)n_chunks * (size_t)nq * 8;
  w.s = (unsigned long long*)take(state);
  w.keys = (unsigned long long*)take(state);
  w.bytes = o;
  return w;
}
