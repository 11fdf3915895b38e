// canon_topk.h — the device functions that make an answer out of candidate rows, shared by wide.hip (the finalize of the
// chunked-GEMM search) and subset.hip (the search over a list of rows): the canonical fp32 score of a stored row by eight
// lanes, the radix select of the k-th largest key, and the k best keys of a list in exact order.  One copy of each, so the two
// searches cannot drift apart: ids and score bits of both are the oracle's.
#pragma once
#include "rarc_common.h"

// k-th largest 32-bit value among n words read through `at(i)` by the whole block: four rounds of an 8-bit radix
// histogram in LDS.  Returns the value (every thread); n >= k >= 1.
template <typename At>
__device__ uint32_t wide_kth_largest_u32(At at, uint32_t n, uint32_t k, uint32_t* s_hist, uint32_t* s_pick) {
  uint32_t prefix = 0, mask = 0, need = k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) s_hist[i] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      const uint32_t v = at(i);
      if ((v & mask) == prefix) atomicAdd(&s_hist[(v >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 64) {      // the bin holding the need-th largest, by one wave (a serial walk of the 256 counters by one
      uint32_t above = 0;        //  thread was 7 us a round — 28 of the 40 us a tighten took)
      int b = rarc_wave_find_from_top(s_hist, 256, need, &above);
      if (b < 0) { b = 0; above = 0; }           // (n >= need: cannot happen)
      if (threadIdx.x == 0) {
        s_pick[0] = (uint32_t)b;
        s_pick[1] = need - above;
      }
    }
    __syncthreads();
    prefix |= s_pick[0] << shift;
    mask |= 255u << shift;
    need = s_pick[1];
    __syncthreads();
  }
  return prefix;
}

// canonical fp32 scores of QT queries with one stored row, by 8 lanes: lane j runs chain j (elements 8m + j, m ascending) of
// every query, the tree of rarc_canon_tree joins them — the same arithmetic, in the same order, as canon_dot_f16 / oracle
// canon_dot.  The row is fetched once for all QT queries.
// fp16 rows: the group fetches 128 contiguous bytes per step (lane j the 16 bytes of elements 8(8b + j) .. + 7) and passes them
// through its 128 bytes of LDS, from which lane j picks element j of each of the eight pieces in ascending order — one
// 16-byte load per 64 elements and lane instead of eight 2-byte ones (the finalize was 100 us of a 490 us search of 100,000
// rows, 2 ms of 13 at k = 2000: all of it these loads).  A wave's LDS operations execute in order, so the lanes of a group
// (always inside one wave) see each other's writes without a barrier.  q: the queries (fp32, query t at q + t * q_stride; in
// LDS wherever a block scores many rows).
template <bool F32ROWS, int QT>
__device__ __forceinline__ void wide_canon_dot8n(const float* q, int q_stride, const void* __restrict__ rows, size_t row, int d_pad,
                                                 int j, uint4* stage, float (&out)[QT]) {
  float a[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) a[t] = 0.f;
  if (F32ROWS) {
    const float* r = (const float*)rows + row * (size_t)d_pad;
    for (int m = j; m < d_pad; m += 8) {
      const float x = r[m];
#pragma unroll
      for (int t = 0; t < QT; ++t) a[t] = __builtin_fmaf(q[t * q_stride + m], x, a[t]);
    }
  } else {
    const uint4* r = (const uint4*)((const half_t*)rows + row * (size_t)d_pad) + j;
    const half_t* sh = (const half_t*)stage + j;
    const int nblk = d_pad >> 6;                    // 64 elements per step (d_pad is a multiple of 64)
    uint4 v0 = r[0], v1 = nblk > 1 ? r[8] : v0;     // two steps in flight
    for (int b = 0; b < nblk; ++b) {
      const uint4 vn = b + 2 < nblk ? r[(b + 2) * 8] : v1;
      stage[j] = v0;
      asm volatile("" ::: "memory");
      const float* qb = q + 64 * b + j;
#pragma unroll
      for (int mm = 0; mm < 8; ++mm) {
        const float x = (float)sh[8 * mm];
#pragma unroll
        for (int t = 0; t < QT; ++t) a[t] = __builtin_fmaf(qb[t * q_stride + 8 * mm], x, a[t]);
      }
      asm volatile("" ::: "memory");
      v0 = v1;
      v1 = vn;
    }
  }
  // ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7)): lanes j and j ^ 4, then j ^ 2, then j ^ 1
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    float s = a[t];
    s = s + __shfl_xor(s, 4, 8);
    s = s + __shfl_xor(s, 2, 8);
    s = s + __shfl_xor(s, 1, 8);
    out[t] = s;
  }
}

// one query (the finalize of the wide search; a gather when the rows come from a list)
template <bool F32ROWS>
__device__ __forceinline__ float wide_canon_dot8(const float* q, const void* __restrict__ rows, size_t row, int d_pad, int j,
                                                 uint4* stage) {
  float s[1];
  wide_canon_dot8n<F32ROWS, 1>(q, 0, rows, row, d_pad, j, stage, s);
  return s[0];
}

// metric "l2": the key of a row from its canonical inner product with the query — dist = max(0, (qn + xn) - 2 ip), ranked as
// 0 - dist.  2 ip is exact and the subtraction rounds once: contracted into an FMA or not, the same bits.  0 - dist: +0 stays
// +0 (one key for distance zero), every other distance changes sign exactly.
__device__ __forceinline__ float wide_l2_neg_dist(float qn, float xn, float ip) {
  const float dd = (qn + xn) - 2.0f * ip;
  return 0.f - (dd > 0.f ? dd : 0.f);
}

// The kk = min(k, c) largest of the 64-bit keys keys[0 .. c) (score, then ~row = id ascending) into s_top[0 .. pow2), pow2 the
// power of two >= kk, zeros — below every real key — behind them; in exact descending order when `sort`.  Whole block; s_cnt:
// two words of LDS.  Radix select on the high word, then on the low word among the keys that share it, then a bitonic sort.
__device__ __forceinline__ void wide_topk_keys(const uint64_t* keys, uint32_t c, uint32_t kk, uint32_t pow2, uint64_t* s_top,
                                               uint32_t* s_hist, uint32_t* s_pick, uint32_t* s_cnt, bool sort) {
  for (uint32_t i = threadIdx.x; i < pow2; i += blockDim.x) s_top[i] = 0;
  if (threadIdx.x == 0) { s_cnt[0] = 0; s_cnt[1] = 0; }
  __syncthreads();
  if (kk == 0) return;
  const uint32_t hi = wide_kth_largest_u32([&](uint32_t i) { return (uint32_t)(keys[i] >> 32); }, c, kk, s_hist, s_pick);
  // how many keys lie strictly above `hi` in the high word; the rest of the k come from the ties on it, by low word
  uint32_t mine = 0;
  for (uint32_t i = threadIdx.x; i < c; i += blockDim.x) mine += ((uint32_t)(keys[i] >> 32) > hi);
  if (mine) atomicAdd(&s_cnt[1], mine);
  __syncthreads();
  const uint32_t need_lo = kk - s_cnt[1];   // >= 1
  // (the low word is ~row: larger = smaller id; ties on the high word are few except for duplicate rows)
  const uint32_t lo = wide_kth_largest_u32(
      [&](uint32_t i) { return (uint32_t)(keys[i] >> 32) == hi ? (uint32_t)keys[i] : 0u; }, c, need_lo, s_hist, s_pick);
  const uint64_t kth = ((uint64_t)hi << 32) | lo;
  for (uint32_t i = threadIdx.x; i < c; i += blockDim.x)
    if (keys[i] >= kth) {
      const uint32_t pos = atomicAdd(&s_cnt[0], 1u);
      if (pos < pow2) s_top[pos] = keys[i];
    }
  __syncthreads();
  if (!sort) return;
  // exact order: bitonic sort, descending (the zeros pad to the power of two)
  for (uint32_t kb = 2; kb <= pow2; kb <<= 1)
    for (uint32_t jb = kb >> 1; jb > 0; jb >>= 1) {
      for (uint32_t i = threadIdx.x; i < pow2; i += blockDim.x) {
        const uint32_t ixj = i ^ jb;
        if (ixj > i) {
          const uint64_t a = s_top[i], b = s_top[ixj];
          const bool desc = (i & kb) == 0;
          if (desc ? a < b : a > b) { s_top[i] = b; s_top[ixj] = a; }
        }
      }
      __syncthreads();
    }
}

// A query's answer from its sorted keys: (id_base + row, score) for the kk real entries, (-1, -inf) behind them; metric "l2"
// writes the distances (+inf behind the real entries).
template <bool L2>
__device__ __forceinline__ void wide_write_topk(const uint64_t* s_top, uint32_t kk, uint32_t k, int64_t id_base, int64_t* out_ids,
                                                float* out_scores) {
  for (uint32_t i = threadIdx.x; i < k; i += blockDim.x) {
    const bool have = i < kk;
    const uint64_t key = have ? s_top[i] : 0;
    out_ids[i] = have ? id_base + (int64_t)rarc_candrow(key) : -1;
    out_scores[i] = L2 ? (have ? 0.f - rarc_candscore(key) : INFINITY) : (have ? rarc_candscore(key) : -INFINITY);
  }
}
