// pairs_common.h — what the two embedding self-joins share (pairs.hip: all pairs with cosine >= threshold; knn.hip: every
// row's top-K cosine neighbours): the workspace both carve (fp16 image, float64 inverse norms, per-column thresholds and
// nomination lists), the bound on the approximate cosine, the fixed-order wave sum and the exact float64 cosine of a pair.
// One copy of each, so the score of a pair is the same bits whichever of the two computed it.
#pragma once
#include "rarc_common.h"

constexpr int PAIRS_COLS = 4096;     // columns per GEMM launch (16 tiles wide: with >= 16 row tiles the chip is full)

struct PairsWs {
  uint16_t* image;       // [n_pad][d_pad] fp16, rows normalised, zero padded
  double* inv_norm;      // [n_pad]
  float* thr;            // [PAIRS_COLS]
  uint32_t* count;       // [PAIRS_COLS]
  uint32_t* status;      // [PAIRS_COLS]
  unsigned long long* cand;   // [PAIRS_COLS][cap]
};
static inline size_t a256(size_t v) { return (v + 255) & ~(size_t)255; }
static inline int64_t pad256(int64_t n) { return (n + 255) / 256 * 256; }
static inline int pairs_d_pad(int d) { return (d + 63) / 64 * 64 < 256 ? 256 : (d + 63) / 64 * 64; }
static inline size_t pairs_ws_bytes(int64_t n, int d_pad, int64_t cap) {
  const int64_t n_pad = pad256(n);
  return a256((size_t)n_pad * d_pad * 2) + a256((size_t)n_pad * 8) + 3 * a256((size_t)PAIRS_COLS * 4) +
         a256((size_t)PAIRS_COLS * (size_t)cap * 8) + 256;
}
static inline PairsWs pairs_carve(void* base, int64_t n, int d_pad) {
  const int64_t n_pad = pad256(n);
  char* b = (char*)(((uintptr_t)base + 255) & ~(uintptr_t)255);
  PairsWs w;
  w.image = (uint16_t*)b;    b += a256((size_t)n_pad * d_pad * 2);
  w.inv_norm = (double*)b;   b += a256((size_t)n_pad * 8);
  w.thr = (float*)b;         b += a256((size_t)PAIRS_COLS * 4);
  w.count = (uint32_t*)b;    b += a256((size_t)PAIRS_COLS * 4);
  w.status = (uint32_t*)b;   b += a256((size_t)PAIRS_COLS * 4);
  w.cand = (unsigned long long*)b;
  return w;
}

// |fp32-accumulated x16·y16 - x·y| for unit vectors x, y rounded to fp16 elementwise: each factor is off by 2^-11 relative
// (or 2^-25 absolute under the normal range), the products' sum by d_pad·2^-24 at most (fp32 accumulation, MFMA order unknown).
static inline float pairs_eps(int d_pad) { return 0.0009765625f + (float)d_pad * 1.1920928955078125e-07f + 1e-6f; }

// pairs.hip: rows -> the fp16 image of the normalised rows + the float64 inverse norms (pairs_prepare_kernel), n_pad rows
int rarc_pairs_prepare(const float* d_rows, int64_t ld, int64_t n_rows, int d, int d_pad, uint16_t* image, double* inv_norm,
                       hipStream_t s);
// pairs.hip: thr[q] = t for the columns col0 + q < n_rows (+inf for padding columns: they never nominate), count = status = 0
int rarc_pairs_reset(const PairsWs& w, float t, int64_t col0, int64_t n_rows, hipStream_t s);

// sum over a wave in a FIXED order (lane l holds the partial of elements l, l + 64, ...): a tree over the lane index, so the
// exact score of a pair does not depend on where it was computed
__device__ __forceinline__ double pairs_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The exact cosine of rows x and y by one wave (every lane returns it): float64 dot product of the fp32 rows in the fixed order
// above, times the two float64 inverse norms.  inv_lo is the inverse norm of the row with the SMALLER index: the two products
// round in that order wherever the pair is scored (the dot product itself is symmetric: a product of doubles commutes).
__device__ __forceinline__ double pairs_exact_cos(const float* __restrict__ x, const float* __restrict__ y, int d, int lane,
                                                  double inv_lo, double inv_hi) {
  double acc = 0.0;
  for (int m = lane; m < d; m += 64) acc += (double)x[m] * (double)y[m];
  acc = pairs_wave_sum(acc);
  return acc * inv_lo * inv_hi;
}
