// l2.hip — the per-row side array of metric "l2": xn[r] = canonical fp32 dot(x_r, x_r) of the STORED rows (the fp16-rounded row of
// fp16 storage, the fp32 row of fp32 storage) — the same eight FMA chains + tree as every score of this library, so
// that wide.hip's finalize can form dist = max(0, (qn + xn) - 2 ip) from three canonical numbers.  Derived data: the engine
// recomputes it for appended rows, from the first hole after a removal, and for all rows after a load; no file holds it.
//
// Eight lanes per row, lane j runs chain j (elements 8m + j, m ascending).  fp16 rows: the group fetches 128 contiguous bytes
// per step (lane j the 16 bytes of elements 8(8b + j) .. + 7) and passes them through its 128 bytes of LDS, from which lane j
// picks element j of each of the eight pieces in ascending order (as canon_topk.h's wide_canon_dot8; a wave's LDS operations
// execute in order, and a group sits inside one wave).  fp32 rows go the same way, 32 elements per step.  One read of the rows
// in 128-byte pieces, 4 bytes written per row (the measured rate is in DESIGN 4.10b).
#include "rarc_common.h"

namespace {
template <bool F32ROWS>
__global__ __launch_bounds__(256) void row_sqnorms_kernel(const void* __restrict__ rows, int64_t n_rows, int d_pad, int64_t first_row,
                                                          float* __restrict__ xn) {
  __shared__ uint4 s_stage[256];
  const int j = threadIdx.x & 7;
  uint4* stage = s_stage + (threadIdx.x & ~7);
  const int64_t groups = (int64_t)gridDim.x * 32;
  // (whole groups of 32 rows per step: the lanes of a group stay together through the shuffles; rows past the end are read
  //  as the last row and not written)
  for (int64_t r0 = first_row + (int64_t)blockIdx.x * 32; r0 < n_rows; r0 += groups) {
    const int64_t r = r0 + (threadIdx.x >> 3);
    const bool live = r < n_rows;
    const size_t row = (size_t)(live ? r : n_rows - 1);
    float a = 0.f;
    if (F32ROWS) {
      // 32 elements per step: lane j fetches the 16 bytes of elements 4j .. 4j + 3 (128 contiguous bytes per group), then
      // picks elements 8 mm + j, mm = 0 .. 3, from the group's LDS — the same staging as the fp16 rows
      const uint4* x = (const uint4*)((const float*)rows + row * (size_t)d_pad) + j;
      const float* sf = (const float*)stage + j;
      const int nblk = d_pad >> 5;                    // (d_pad is a multiple of 32)
      uint4 v0 = x[0], v1 = nblk > 1 ? x[8] : v0;     // two steps in flight
      for (int b = 0; b < nblk; ++b) {
        const uint4 vn = b + 2 < nblk ? x[(b + 2) * 8] : v1;
        stage[j] = v0;
        asm volatile("" ::: "memory");
#pragma unroll
        for (int mm = 0; mm < 4; ++mm) {
          const float e = sf[8 * mm];
          a = __builtin_fmaf(e, e, a);
        }
        asm volatile("" ::: "memory");
        v0 = v1;
        v1 = vn;
      }
    } else {
      const uint4* x = (const uint4*)((const half_t*)rows + row * (size_t)d_pad) + j;
      const half_t* sh = (const half_t*)stage + j;
      const int nblk = d_pad >> 6;                    // 64 elements per step (d_pad is a multiple of 64)
      uint4 v0 = x[0], v1 = nblk > 1 ? x[8] : v0;     // two steps in flight
      for (int b = 0; b < nblk; ++b) {
        const uint4 vn = b + 2 < nblk ? x[(b + 2) * 8] : v1;
        stage[j] = v0;
        asm volatile("" ::: "memory");
#pragma unroll
        for (int mm = 0; mm < 8; ++mm) {
          const float e = (float)sh[8 * mm];
          a = __builtin_fmaf(e, e, a);
        }
        asm volatile("" ::: "memory");
        v0 = v1;
        v1 = vn;
      }
    }
    // ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7)): rarc_canon_tree over the lanes of the group
    a = a + __shfl_xor(a, 4, 8);
    a = a + __shfl_xor(a, 2, 8);
    a = a + __shfl_xor(a, 1, 8);
    if (live && j == 0) xn[r] = a;
  }
}
}  // namespace

// d_xn[r] = canonical dot(row r, row r) for r in [first_row, n_rows).  fmt 0: fp16 rows [n_rows][d_pad]; fmt 2: fp32 rows.
extern "C" int rarc_row_sqnorms(const void* d_rows, int fmt, int64_t n_rows, int d_pad, int64_t first_row, float* d_xn, void* stream) {
  RARC_RANGE();
  RARC_REQUIRE(d_rows && d_xn, RARC_E_INVALID, "rarc_row_sqnorms: null pointer");
  RARC_REQUIRE(fmt == 0 || fmt == 2, RARC_E_INVALID, "rarc_row_sqnorms: fmt 0 (fp16 rows) or 2 (fp32 rows), got %d", fmt);
  RARC_REQUIRE(d_pad > 0 && d_pad % RARC_DIM_ALIGN == 0 && d_pad <= 4096, RARC_E_UNSUPPORTED,
               "rarc_row_sqnorms: padded dim %d unsupported (multiple of %d, <= 4096)", d_pad, RARC_DIM_ALIGN);
  RARC_REQUIRE(n_rows >= 0 && first_row >= 0 && first_row <= n_rows, RARC_E_INVALID,
               "rarc_row_sqnorms: need 0 <= first_row <= n_rows (first_row=%lld n_rows=%lld)", (long long)first_row, (long long)n_rows);
  if (first_row == n_rows) return RARC_OK;
  const int64_t blocks = (n_rows - first_row + 31) / 32;
  const int grid = (int)(blocks < 16384 ? blocks : 16384);
  hipStream_t s = (hipStream_t)stream;
  if (fmt == 2)
    hipLaunchKernelGGL(row_sqnorms_kernel<true>, dim3(grid), dim3(256), 0, s, d_rows, n_rows, d_pad, first_row, d_xn);
  else
    hipLaunchKernelGGL(row_sqnorms_kernel<false>, dim3(grid), dim3(256), 0, s, d_rows, n_rows, d_pad, first_row, d_xn);
  RARC_HIP_CHECK(hipGetLastError());
  return RARC_OK;
}
