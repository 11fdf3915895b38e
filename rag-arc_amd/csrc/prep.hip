// prep.hip — row-wise kernels either side of the scan:
//   rarc_l2norm_rows_f32   faiss.normalize_L2            (VectorStore_Faiss.py:150-154)
//   rarc_ingest_f16        normalise + index.add as fp16 (VectorStore_Faiss.py:178, :199-202)
//   rarc_prep_queries      np.array([q]).astype(f32) + normalise (VectorStore_Faiss.py:258-259)
//   rarc_cosine_matrix_f32 / rarc_adjacent_cosine_distance_f32   the chunker's float64 cosines (spliter.py:307-371)
//   rarc_synth_rows_*      deterministic synthetic data (bench / property tests)
//
// All reductions use the canonical 8-lane order: lane j of an 8-lane group owns elements
// 8m+j (m ascending, one fma per element), then tree ((a0+a4)+(a2+a6))+((a1+a5)+(a3+a7)).
// oracle/rarc_oracle.c uses the same order, so normalised rows are bit-identical.
// HBM-bound streaming kernels: 8 rows per wave, 32 contiguous bytes per row per step.
#include "rarc_common.h"

__device__ __forceinline__ float group8_tree_f32(float acc, int lane) {
  const int base = lane & ~7;
  float a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = __shfl(acc, base + j, 64);
  return rarc_canon_tree(a);
}
__device__ __forceinline__ double group8_tree_f64(double acc, int lane) {
  const int base = lane & ~7;
  double a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = __shfl(acc, base + j, 64);
  return ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7]));
}

// inv norm exactly as faiss: (float)(1.0 / sqrtf(nr)), evaluated in double like the C expression.
// sqrtf is taken as (float)sqrt((double)nr): correctly rounded (53 >= 2*24+2 makes the double
// rounding innocuous), whereas HIP's __fsqrt_rn is the 1-ulp native v_sqrt_f32.
__device__ __forceinline__ float inv_norm(float nr) { return (float)(1.0 / (double)(float)sqrt((double)nr)); }

__global__ __launch_bounds__(256) void rarc_l2norm_kernel(const float* in, int64_t ld_in, float* out,
                                                          int64_t ld_out, int64_t n_rows, int d) {
  const int lane = threadIdx.x & 63, j = threadIdx.x & 7;
  const int64_t rows_per_block = blockDim.x / 8;
  for (int64_t r0 = (int64_t)blockIdx.x * rows_per_block; r0 < n_rows; r0 += (int64_t)gridDim.x * rows_per_block) {
    const int64_t r = r0 + threadIdx.x / 8;
    const bool live = r < n_rows;
    const float* x = in + (live ? r : 0) * ld_in;
    float acc = 0.f;
    if (live)
      for (int m = j; m < d; m += 8) acc = __builtin_fmaf(x[m], x[m], acc);
    const float nr = group8_tree_f32(acc, lane);
    if (live) {
      float* y = out + r * ld_out;
      if (nr > 0.f) {
        const float inv = inv_norm(nr);
        for (int m = j; m < d; m += 8) y[m] = x[m] * inv;
      } else if (y != x) {
        for (int m = j; m < d; m += 8) y[m] = x[m];
      }
    }
  }
}

// Cosine similarity of row pairs in float64 (the chunker's distances, core/file_management/chunker/spliter.py:307-371:
// np.dot(X, Y.T) / np.outer(|X|, |Y|) on float64 arrays, non-finite quotients -> 0).  One wave per (i, j) pair: lane l
// owns elements l, l+64, ... (products of fp32 values are exact in fp64, one rounding per add), then a butterfly
// over lane distances 32, 16, ..., 1.  `adjacent`: pairs (i, i+1) of X only and the value written is 1 - similarity.
__global__ __launch_bounds__(256) void rarc_cosine_pairs_kernel(const float* x, int64_t ldx, int nx, const float* y,
                                                                int64_t ldy, int ny, int d, int adjacent, double* out) {
  const int lane = threadIdx.x & 63;
  const int64_t n_pairs = adjacent ? (int64_t)nx - 1 : (int64_t)nx * ny;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < n_pairs; p += (int64_t)gridDim.x * 4) {
    const int64_t i = adjacent ? p : p / ny, j = adjacent ? p + 1 : p % ny;
    const float* a = x + i * ldx;
    const float* b = adjacent ? x + j * ldx : y + j * ldy;
    double dot = 0.0, na = 0.0, nb = 0.0;
    for (int m = lane; m < d; m += 64) {
      const double av = (double)a[m], bv = (double)b[m];
      dot = __builtin_fma(av, bv, dot);
      na = __builtin_fma(av, av, na);
      nb = __builtin_fma(bv, bv, nb);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      dot += __shfl_xor(dot, off, 64);
      na += __shfl_xor(na, off, 64);
      nb += __shfl_xor(nb, off, 64);
    }
    if (lane == 0) {
      double sim = dot / (sqrt(na) * sqrt(nb));
      if (!(sim - sim == 0.0)) sim = 0.0;  // NaN or +-inf (a zero row): the reference zeroes those entries
      out[p] = adjacent ? 1.0 - sim : sim;
    }
  }
}

__global__ __launch_bounds__(256) void rarc_ingest_kernel(const float* in, int64_t ld_in, half_t* out,
                                                          int d_pad, float* row_norm2, int64_t n_rows,
                                                          int d, int normalize) {
  const int lane = threadIdx.x & 63, j = threadIdx.x & 7;
  const int64_t rows_per_block = blockDim.x / 8;
  for (int64_t r0 = (int64_t)blockIdx.x * rows_per_block; r0 < n_rows; r0 += (int64_t)gridDim.x * rows_per_block) {
    const int64_t r = r0 + threadIdx.x / 8;
    const bool live = r < n_rows;
    const float* x = in + (live ? r : 0) * ld_in;
    float acc = 0.f;
    if (live && normalize)
      for (int m = j; m < d; m += 8) acc = __builtin_fmaf(x[m], x[m], acc);
    const float nr = group8_tree_f32(acc, lane);
    const float inv = (normalize && nr > 0.f) ? inv_norm(nr) : 1.f;
    float acc2 = 0.f;
    if (live) {
      half_t* y = out + r * d_pad;
      for (int m = j; m < d_pad; m += 8) {
        half_t hv = (half_t)0.f;
        if (m < d) hv = (half_t)((normalize && nr > 0.f) ? x[m] * inv : x[m]);
        y[m] = hv;
        const float f = (float)hv;
        acc2 = __builtin_fmaf(f, f, acc2);
      }
    }
    const float n2 = group8_tree_f32(acc2, lane);
    if (live && row_norm2 && j == 0) row_norm2[r] = n2;
  }
}

// fp32 storage (the reference's own: VectorStore_Faiss.py:170,199-202 keeps fp32): the normalised fp32 row is
// stored as is (zero padded) and an fp16 image of it feeds the scan kernels; norm2 is that of the fp32 row.
__global__ __launch_bounds__(256) void rarc_ingest_f32_kernel(const float* in, int64_t ld_in, float* out32, half_t* out16,
                                                              int d_pad, float* row_norm2, int64_t n_rows, int d,
                                                              int normalize) {
  const int lane = threadIdx.x & 63, j = threadIdx.x & 7;
  const int64_t rows_per_block = blockDim.x / 8;
  for (int64_t r0 = (int64_t)blockIdx.x * rows_per_block; r0 < n_rows; r0 += (int64_t)gridDim.x * rows_per_block) {
    const int64_t r = r0 + threadIdx.x / 8;
    const bool live = r < n_rows;
    const float* x = in + (live ? r : 0) * ld_in;
    float acc = 0.f;
    if (live && normalize)
      for (int m = j; m < d; m += 8) acc = __builtin_fmaf(x[m], x[m], acc);
    const float nr = group8_tree_f32(acc, lane);
    const float inv = (normalize && nr > 0.f) ? inv_norm(nr) : 1.f;
    float acc2 = 0.f;
    if (live) {
      for (int m = j; m < d_pad; m += 8) {
        float v = 0.f;
        if (m < d) v = (normalize && nr > 0.f) ? x[m] * inv : x[m];
        out32[r * d_pad + m] = v;
        out16[r * d_pad + m] = (half_t)v;
        acc2 = __builtin_fmaf(v, v, acc2);
      }
    }
    const float n2 = group8_tree_f32(acc2, lane);
    if (live && row_norm2 && j == 0) row_norm2[r] = n2;
  }
}

// fp8 (e4m3fn + per-row scale) form of the ingest: same normalisation, then scale = max|x| / 448 and
// byte = encode(x / scale).  8 lanes per row; bit-identical to oracle_ingest_f8.
__device__ __forceinline__ float group8_max_f32(float v, int lane) {
  const int base = lane & ~7;
  float m = v;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, __shfl(v, base + j, 64));
  return m;
}
__global__ __launch_bounds__(256) void rarc_ingest_f8_kernel(const float* in, int64_t ld_in, uint8_t* out, int d_pad,
                                                             float* row_scale, float* row_norm2, int64_t n_rows,
                                                             int d, int normalize) {
  const int lane = threadIdx.x & 63, j = threadIdx.x & 7;
  const int64_t rows_per_block = blockDim.x / 8;
  for (int64_t r0 = (int64_t)blockIdx.x * rows_per_block; r0 < n_rows; r0 += (int64_t)gridDim.x * rows_per_block) {
    const int64_t r = r0 + threadIdx.x / 8;
    const bool live = r < n_rows;
    const float* x = in + (live ? r : 0) * ld_in;
    float acc = 0.f;
    if (live && normalize)
      for (int m = j; m < d; m += 8) acc = __builtin_fmaf(x[m], x[m], acc);
    const float nr = group8_tree_f32(acc, lane);
    const bool sc = normalize && nr > 0.f;
    const float inv = sc ? inv_norm(nr) : 1.f;
    float mx = 0.f;
    if (live)
      for (int m = j; m < d; m += 8) mx = fmaxf(mx, __builtin_fabsf(sc ? x[m] * inv : x[m]));
    mx = group8_max_f32(mx, lane);
    const float scale = (mx > 0.f && mx < INFINITY) ? mx / 448.0f : 1.0f;
    float acc2 = 0.f;
    if (live) {
      uint8_t* y = out + r * d_pad;
      for (int m = j; m < d_pad; m += 8) {
        uint8_t b = 0;
        if (m < d) b = rarc_f8_encode((sc ? x[m] * inv : x[m]) / scale);
        y[m] = b;
        float f4[4];
        rarc_f8x4_to_f32((uint32_t)b, f4);
        acc2 = __builtin_fmaf(f4[0], f4[0], acc2);
      }
    }
    const float n2 = group8_tree_f32(acc2, lane);
    if (live && j == 0) {
      row_scale[r] = scale;
      if (row_norm2) row_norm2[r] = (scale * scale) * n2;
    }
  }
}

// One block per query slot (all RARC_MAX_QUERIES rows are written; padding rows are zero).  Only the
// squared-norm has a prescribed order (8 lanes run the canonical chains out of LDS); scaling, the
// fp16 / int8 copies and the error-bound sums are order-free and use the whole block.
constexpr int PREP_MAX_D = 4096;   // (rows beyond 1024 padded dimensions take the wide path, wide.hip)
__global__ __launch_bounds__(256) void rarc_prep_queries_kernel(const float* in, int64_t ld_in, int nq, int d,
                                                                int d_pad, int normalize, float corpus_max_norm,
                                                                const float* qmeta, float* q32, half_t* q16,
                                                                int8_t* q8, float* eps, float* eps8, float* qinv,
                                                                float* hq, float* floor, uint32_t* status_zero,
                                                                uint32_t* flag_host) {
  __shared__ float row[PREP_MAX_D];
  if (blockIdx.x == 0) {   // the search's status words start at zero (rarc_search_batch: no fill launch in front of the batch)
    if (status_zero)
      for (int i = threadIdx.x; i <= RARC_MAX_QUERIES; i += 256) status_zero[i] = 0u;
    if (flag_host && threadIdx.x == 0) __hip_atomic_store(flag_host, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __shared__ float s_nr;
  __shared__ uint32_t s_amax;
  __shared__ double s_red[4][4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int r = blockIdx.x;
  const bool live = r < nq;
  for (int m = tid; m < d_pad; m += 256) row[m] = (live && m < d) ? in[(size_t)r * ld_in + m] : 0.f;
  if (tid == 0) s_amax = 0;
  __syncthreads();
  if (tid < 64) {
    float acc = 0.f;
    if (tid < 8 && live && normalize)
      for (int m = tid; m < d; m += 8) acc = __builtin_fmaf(row[m], row[m], acc);
    const float nr = group8_tree_f32(acc, lane);
    if (tid == 0) s_nr = nr;
  }
  __syncthreads();
  const float nr = s_nr;
  const bool scale = live && normalize && nr > 0.f;
  const float inv = scale ? inv_norm(nr) : 1.f;
  double dn = 0.0, qn = 0.0;
  uint32_t am = 0;
  for (int m = tid; m < d_pad; m += 256) {
    const float v = scale ? row[m] * inv : row[m];
    row[m] = v;  // each thread rewrites only the elements it owns
    const half_t hv = (half_t)v;
    q32[(size_t)r * d_pad + m] = v;
    q16[(size_t)r * d_pad + m] = hv;
    const double df = (double)v - (double)(float)hv;
    dn += df * df;
    qn += (double)v * (double)v;
    const uint32_t a = __float_as_uint(v) & 0x7fffffffu;
    am = a > am ? a : am;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t x = __shfl_xor(am, o, 64);
    am = x > am ? x : am;
  }
  if (lane == 0) atomicMax(&s_amax, am);
  __syncthreads();
  // int8 image for the prefilter: q8 = rint(v * s_q), s_q = 127 / max|v|; the scan dequantises with
  // the fp32 number qi = 1/s_q, so the quantised query is DEFINED as q8 * qi and the residual below
  // is taken against exactly that
  const float mx = __uint_as_float(s_amax);
  float sq, qi;
  rarc_query_scale8(mx, &sq, &qi);
  double rn = 0.0, hn = 0.0;
  for (int m = tid; m < d_pad; m += 256) {
    const float v = row[m];
    float t = __builtin_rintf(v * sq);
    t = t > 127.f ? 127.f : (t < -127.f ? -127.f : t);
    if (q8) q8[(size_t)r * d_pad + m] = (int8_t)(int)t;
    const double qh = (double)t * (double)qi;
    const double df = (double)v - qh;
    rn += df * df;
    hn += qh * qh;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    dn += __shfl_xor(dn, o, 64);
    qn += __shfl_xor(qn, o, 64);
    rn += __shfl_xor(rn, o, 64);
    hn += __shfl_xor(hn, o, 64);
  }
  if (lane == 0) { s_red[tid >> 6][0] = dn; s_red[tid >> 6][1] = qn; s_red[tid >> 6][2] = rn; s_red[tid >> 6][3] = hn; }
  __syncthreads();
  if (tid == 0) {
    dn = (s_red[0][0] + s_red[1][0]) + (s_red[2][0] + s_red[3][0]);
    qn = (s_red[0][1] + s_red[1][1]) + (s_red[2][1] + s_red[3][1]);
    rn = (s_red[0][2] + s_red[1][2]) + (s_red[2][2] + s_red[3][2]);
    hn = (s_red[0][3] + s_red[1][3]) + (s_red[2][3] + s_red[3][3]);
    // fp16 MFMA scores (seed pass): |approx - canonical| <= ||q32 - q16||·||d|| + fp32 accumulation
    const double acc_err = 8.0 * (double)d_pad * 5.9604644775390625e-08;  // 8·d·2^-24
    // fp32 storage: the scans read an fp16 image of rows whose canonical score is taken on the fp32 originals;
    // qmeta[1] = rho bounds ||d32 - d16|| over all rows, so either approximate scorer is off by ||q||·rho more
    const double rho_err = (qmeta ? (double)qmeta[1] : 0.0) * sqrt(qn) * 1.0001;
    const double e = (sqrt(dn) + acc_err * sqrt(qn)) * (double)corpus_max_norm * 1.01 + rho_err + 1e-30;
    eps[r] = live ? (float)e * 1.0001f : 0.f;
    // int8 prefilter (quant.hip): |<q,d> - approx| <= ||q^||·R + ||q - q^||·max||d||, plus the fp32
    // rounding of the canonical score and of the dequantisation
    if (eps8 && qinv) {
      const double R = qmeta ? (double)qmeta[0] : 0.0;
      const double e8 = (sqrt(hn) * R * 1.0001 + sqrt(rn) * (double)corpus_max_norm) * 1.0001 +
                        (acc_err + 1e-6) * sqrt(qn) * (double)corpus_max_norm + rho_err + 1e-30;
      eps8[r] = live ? (float)e8 * 1.0001f : 0.f;
      qinv[r] = qi;
      // inside tile t the first term is ||q^||·R_t: the scan raises the query's threshold there by hq·(R − R_t),
      // with hq rounded DOWN so that the reduced bound still dominates ||q^||·R_t·1.0001 + the rest
      if (hq) hq[r] = live ? (float)(sqrt(hn) * 0.9999) : 0.f;
      if (floor) floor[r] = -INFINITY;  // nothing known about the k-th best score yet
    }
  }
}

// ---- synthetic rows ---------------------------------------------------------------------------
// v(seed,row,col) ~ N(0,1): counter hash -> 52-bit uniform p -> Phi^-1(p) (Wichura AS 241, PPND16) -> the
// integer rint(z * 2^20).  Only exactly rounded double operations in a fixed order (the log is the explicit
// series below; the file is compiled with -ffp-contract=off), so oracle/rarc_oracle.c:synth_val produces
// the same integers bit for bit.
__host__ __device__ static inline uint64_t synth_mix(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__device__ static inline double synth_log(double x) {  // ln x, x normal and positive
  uint64_t u = (uint64_t)__double_as_longlong(x);
  int e = (int)((u >> 52) & 0x7ff) - 1023;
  u = (u & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
  double m = __longlong_as_double((long long)u);
  if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
  const double s = (m - 1.0) / (m + 1.0), z = s * s;
  double t = 1.0 / 27.0;
  t = t * z + 1.0 / 25.0;
  t = t * z + 1.0 / 23.0;
  t = t * z + 1.0 / 21.0;
  t = t * z + 1.0 / 19.0;
  t = t * z + 1.0 / 17.0;
  t = t * z + 1.0 / 15.0;
  t = t * z + 1.0 / 13.0;
  t = t * z + 1.0 / 11.0;
  t = t * z + 1.0 / 9.0;
  t = t * z + 1.0 / 7.0;
  t = t * z + 1.0 / 5.0;
  t = t * z + 1.0 / 3.0;
  t = t * z + 1.0;
  return (double)e * 0.6931471805599453 + (s + s) * t;
}
__device__ static inline double synth_ppnd(double p) {
  const double q = p - 0.5;
  if (q >= -0.425 && q <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                            4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                         1.3314166789178437745e+2) * r + 3.3871328727963666080e0);
    const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                            2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                         4.2313330701600911252e+1) * r + 1.0);
    return q * num / den;
  }
  double r = q < 0.0 ? p : 1.0 - p;
  r = sqrt(-synth_log(r));
  double v;
  if (r <= 5.0) {
    r = r - 1.6;
    const double num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                            1.27045825245236838258e0) * r + 3.64784832476320460504e0) * r + 5.76949722146069140550e0) * r +
                         4.63033784615654529590e0) * r + 1.42343711074968357734e0);
    const double den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                            1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e0) * r +
                         2.05319162663775882187e0) * r + 1.0);
    v = num / den;
  } else {
    r = r - 5.0;
    const double num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                            2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e0) * r +
                         5.46378491116411436990e0) * r + 6.65790464350110377720e0);
    const double den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                            7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                         5.99832206555887937690e-1) * r + 1.0);
    v = num / den;
  }
  return q < 0.0 ? -v : v;
}
__device__ static inline int32_t synth_val(uint64_t seed, uint64_t row, uint32_t col) {
  const uint64_t h = synth_mix(synth_mix(seed ^ (row * 0xd1342543de82ef95ull)) + col);
  const double p = ((double)(h >> 12) + 0.5) * 2.220446049250313e-16;  // (i + 1/2) * 2^-52, exact
  return (int32_t)rint(synth_ppnd(p) * 1048576.0);
}

template <bool F16>
__global__ __launch_bounds__(256) void rarc_synth_kernel(void* out, int64_t ld_out, int d_fill, int d,
                                                         int64_t first_row, int64_t n_rows, uint64_t seed) {
  // one wave per row: exact integer sum of squares (order free), fp64 scale, one rounding to f32
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / 64);
  for (int64_t r = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; r < n_rows; r += waves) {
    const uint64_t row = (uint64_t)(first_row + r);
    uint64_t ss = 0;
    for (int c = lane; c < d; c += 64) {
      const int64_t v = synth_val(seed, row, (uint32_t)c);
      ss += (uint64_t)(v * v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const double scale = (ss > 0) ? 1.0 / sqrt((double)ss) : 0.0;
    for (int c = lane; c < d_fill; c += 64) {
      float f = 0.f;
      if (c < d) f = (float)((double)synth_val(seed, row, (uint32_t)c) * scale);
      if (F16) ((half_t*)out)[r * ld_out + c] = (half_t)f;
      else ((float*)out)[r * ld_out + c] = f;
    }
  }
}

static int grid_for(int64_t units, int per_block, int cap = 4096) {
  int64_t g = (units + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

extern "C" int rarc_l2norm_rows_f32(const float* d_in, int64_t ld_in, float* d_out, int64_t ld_out,
                                    int64_t n_rows, int d, void* stream) {
  RARC_REQUIRE(d_in && d_out && d > 0 && n_rows >= 0, RARC_E_INVALID, "rarc_l2norm_rows_f32: bad arguments");
  if (n_rows == 0) return RARC_OK;
  hipLaunchKernelGGL(rarc_l2norm_kernel, dim3(grid_for(n_rows, 32)), dim3(256), 0, (hipStream_t)stream,
                     d_in, ld_in, d_out, ld_out, n_rows, d);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_cosine_matrix_f32(const float* d_x, int64_t ld_x, int nx, const float* d_y, int64_t ld_y, int ny,
                                      int d, double* d_out, void* stream) {
  RARC_REQUIRE(d_x && d_y && d_out && d > 0 && nx >= 0 && ny >= 0 && ld_x >= d && ld_y >= d, RARC_E_INVALID,
               "rarc_cosine_matrix_f32: bad arguments");
  if (nx == 0 || ny == 0) return RARC_OK;
  hipLaunchKernelGGL(rarc_cosine_pairs_kernel, dim3(grid_for((int64_t)nx * ny, 4)), dim3(256), 0, (hipStream_t)stream,
                     d_x, ld_x, nx, d_y, ld_y, ny, d, 0, d_out);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_adjacent_cosine_distance_f32(const float* d_x, int64_t ld_x, int n_rows, int d, double* d_out,
                                                 void* stream) {
  RARC_REQUIRE(d_x && d_out && d > 0 && n_rows >= 0 && ld_x >= d, RARC_E_INVALID,
               "rarc_adjacent_cosine_distance_f32: bad arguments");
  if (n_rows < 2) return RARC_OK;
  hipLaunchKernelGGL(rarc_cosine_pairs_kernel, dim3(grid_for(n_rows - 1, 4)), dim3(256), 0, (hipStream_t)stream, d_x,
                     ld_x, n_rows, d_x, ld_x, n_rows, d, 1, d_out);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_ingest_f16(const float* d_in, int64_t ld_in, uint16_t* d_corpus_f16, int d_pad,
                               float* d_row_norm2, int64_t n_rows, int d, int normalize, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_in && d_corpus_f16 && d > 0 && d_pad >= d && d_pad % 8 == 0 && n_rows >= 0, RARC_E_INVALID,
               "rarc_ingest_f16: bad arguments");
  if (n_rows == 0) return RARC_OK;
  hipLaunchKernelGGL(rarc_ingest_kernel, dim3(grid_for(n_rows, 32)), dim3(256), 0, (hipStream_t)stream, d_in,
                     ld_in, (half_t*)d_corpus_f16, d_pad, d_row_norm2, n_rows, d, normalize);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_ingest_f32(const float* d_in, int64_t ld_in, float* d_corpus_f32, uint16_t* d_image_f16, int d_pad,
                               float* d_row_norm2, int64_t n_rows, int d, int normalize, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_in && d_corpus_f32 && d_image_f16 && d > 0 && d_pad >= d && d_pad % 8 == 0 && n_rows >= 0,
               RARC_E_INVALID, "rarc_ingest_f32: bad arguments");
  if (n_rows == 0) return RARC_OK;
  hipLaunchKernelGGL(rarc_ingest_f32_kernel, dim3(grid_for(n_rows, 32)), dim3(256), 0, (hipStream_t)stream, d_in,
                     ld_in, d_corpus_f32, (half_t*)d_image_f16, d_pad, d_row_norm2, n_rows, d, normalize);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_padded_dim_f8(int d) {
  return d <= 0 ? 0 : ((d + RARC_DIM_ALIGN_F8 - 1) / RARC_DIM_ALIGN_F8) * RARC_DIM_ALIGN_F8;
}

extern "C" int rarc_ingest_f8(const float* d_in, int64_t ld_in, uint8_t* d_corpus_f8, int d_pad, float* d_row_scale,
                              float* d_row_norm2, int64_t n_rows, int d, int normalize, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_in && d_corpus_f8 && d_row_scale && d > 0 && d_pad >= d && d_pad % RARC_DIM_ALIGN_F8 == 0 &&
                   n_rows >= 0,
               RARC_E_INVALID, "rarc_ingest_f8: bad arguments");
  if (n_rows == 0) return RARC_OK;
  hipLaunchKernelGGL(rarc_ingest_f8_kernel, dim3(grid_for(n_rows, 32)), dim3(256), 0, (hipStream_t)stream, d_in,
                     ld_in, d_corpus_f8, d_pad, d_row_scale, d_row_norm2, n_rows, d, normalize);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" size_t rarc_query_block_bytes(int d_pad) { return d_pad > 0 ? rarc_qb_bytes(d_pad) : 0; }

extern "C" int rarc_prep_queries(const float* d_in, int64_t ld_in, int nq, int d, int d_pad, int normalize,
                                 float corpus_max_norm, const float* d_qmeta, void* d_qblock, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_in && d_qblock && ((uintptr_t)d_qblock % 256) == 0 && d > 0 && d_pad >= d &&
                   d_pad % RARC_DIM_ALIGN == 0 && d_pad <= PREP_MAX_D && nq >= 0 && nq <= RARC_MAX_QUERIES,
               RARC_E_INVALID, "rarc_prep_queries: bad arguments (nq=%d d=%d d_pad=%d)", nq, d, d_pad);
  const RarcQb qb = rarc_qb_carve(d_qblock, d_pad);
  hipLaunchKernelGGL(rarc_prep_queries_kernel, dim3(RARC_MAX_QUERIES), dim3(256), 0, (hipStream_t)stream,
                     d_in, ld_in, nq, d, d_pad, normalize, corpus_max_norm, d_qmeta, qb.q32, (half_t*)qb.q16,
                     qb.q8, qb.eps16, qb.eps8, qb.qinv, qb.hq, qb.floor, rarc_launch_extras().status_zero,
                     rarc_launch_extras().flag_host);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

// Host-only view of the scale the kernel above takes for a query whose largest prepared magnitude is mx: touches no device
extern "C" int rarc_debug_query_scale8(float mx, float* sq, float* qi) {
  RARC_REQUIRE(sq && qi, RARC_E_INVALID, "rarc_debug_query_scale8: null pointer");
  rarc_query_scale8(mx, sq, qi);
  return RARC_OK;
}

// floor[q] = the k-th entry of a previous (possibly incomplete) answer for query q: canonical scores of real rows,
// so the k-th best of them bounds the true k-th best from below (entries with id < 0 carry no information)
__global__ void rarc_set_floor_kernel(const int64_t* ids, const float* scores, int k, int nq, float* floor) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < nq) floor[q] = ids[(size_t)q * k + k - 1] >= 0 ? scores[(size_t)q * k + k - 1] : -INFINITY;
}
extern "C" int rarc_qblock_set_floor(void* d_qblock, int d_pad, const int64_t* d_prev_ids, const float* d_prev_scores,
                                     int k, int nq, void* stream) {
  RARC_REQUIRE(d_qblock && d_prev_ids && d_prev_scores && d_pad > 0 && d_pad % RARC_DIM_ALIGN == 0 && k >= 1 && nq >= 0 &&
                   nq <= RARC_MAX_QUERIES,
               RARC_E_INVALID, "rarc_qblock_set_floor: bad arguments");
  if (nq == 0) return RARC_OK;
  const RarcQb qb = rarc_qb_carve(d_qblock, d_pad);
  hipLaunchKernelGGL(rarc_set_floor_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, d_prev_ids, d_prev_scores, k, nq,
                     qb.floor);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_synth_rows_f16(uint16_t* d_out_f16, int d_pad, int d, int64_t first_row, int64_t n_rows,
                                   uint64_t seed, void* stream) {
  RARC_REQUIRE(d_out_f16 && d > 0 && d_pad >= d && n_rows >= 0, RARC_E_INVALID, "rarc_synth_rows_f16: bad arguments");
  if (n_rows == 0) return RARC_OK;
  hipLaunchKernelGGL(rarc_synth_kernel<true>, dim3(grid_for(n_rows, 4, 8192)), dim3(256), 0, (hipStream_t)stream,
                     (void*)d_out_f16, (int64_t)d_pad, d_pad, d, first_row, n_rows, seed);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}

extern "C" int rarc_synth_rows_f32(float* d_out_f32, int64_t ld_out, int d, int64_t first_row, int64_t n_rows,
                                   uint64_t seed, void* stream) {
  RARC_REQUIRE(d_out_f32 && d > 0 && ld_out >= d && n_rows >= 0, RARC_E_INVALID, "rarc_synth_rows_f32: bad arguments");
  if (n_rows == 0) return RARC_OK;
  hipLaunchKernelGGL(rarc_synth_kernel<false>, dim3(grid_for(n_rows, 4, 8192)), dim3(256), 0, (hipStream_t)stream,
                     (void*)d_out_f32, ld_out, d, d, first_row, n_rows, seed);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}


// ---- measurement helper: the read ceiling of this part's HBM (rarc.h: rarc_stream_read) ----------------------------------
// One persistent workgroup of 512 threads per CU (the scan's shape), every lane keeps eight 16-byte loads in flight over a
// grid-strided sweep; the xor of everything read goes to d_sink so that nothing is optimised away.
typedef uint32_t sr_u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(512) void rarc_stream_read_kernel(const sr_u32x4* __restrict__ src, size_t n16, unsigned long long* sink) {
  const size_t stride = (size_t)gridDim.x * 512;
  size_t i = (size_t)blockIdx.x * 512 + threadIdx.x;
  sr_u32x4 acc = {0, 0, 0, 0};
  for (; i + 7 * stride < n16; i += 8 * stride) {
    sr_u32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(src + i + u * stride);
#pragma unroll
    for (int u = 0; u < 8; ++u) acc ^= v[u];
  }
  for (; i < n16; i += stride) acc ^= __builtin_nontemporal_load(src + i);
  const unsigned long long w = ((unsigned long long)(acc.x ^ acc.z) << 32) | (acc.y ^ acc.w);
  if (w == 0x9e3779b97f4a7c15ull) atomicXor(sink, w);   // (practically never: the data decides; keeps the loads alive)
}

extern "C" int rarc_stream_read(const void* d_src, size_t n_bytes, void* d_sink, void* stream) {
  RARC_REQUIRE(d_src && d_sink && ((uintptr_t)d_src % 16) == 0, RARC_E_INVALID, "rarc_stream_read: bad arguments");
  if (n_bytes < 16) return RARC_OK;
  int dev = 0, cus = 256;
  RARC_HIP_CHECK(hipGetDevice(&dev));
  RARC_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  hipLaunchKernelGGL(rarc_stream_read_kernel, dim3(cus), dim3(512), 0, (hipStream_t)stream, (const sr_u32x4*)d_src, n_bytes / 16,
                     (unsigned long long*)d_sink);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}
