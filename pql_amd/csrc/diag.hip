// Unit diagnostics of one post-ELU activation matrix (pqlk_unit_stats): the law is written out in include/pqlk.h.  Read-only on h.
// Column sums over the rows in the chunk-then-fold pattern of k_ln_bwd_sums_wide / k_ln_fold (pql_amd/csrc/ln.hip): a block sums 64
// columns over one chunk of rows, its four waves taking every fourth row; one block then folds the chunks in index order, the columns
// in a fixed order, and decides the dormant units.  No float atomics: the same input gives the same bits.
#include "pqlk_common.h"

// Launch 1, grid (ceil(cols / 64), chunks).  part[(chunk * 2 + 0) * cols + c] = sum over the chunk's rows of |h[r, c]|,
// part[(chunk * 2 + 1) * cols + c] = of the ELU slope s(h[r, c]).  Columns >= cols are never read.
__global__ __launch_bounds__(256) void k_unit_sums(const float* __restrict__ h, int64_t ld, int64_t rows, int cols, float* __restrict__ part) {
  __shared__ float sh[2][4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  float s1 = 0.f, s2 = 0.f;
  if (c < cols) {
    const int64_t rows_per = (rows + gridDim.y - 1) / gridDim.y;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per, r1 = min(rows, r0 + rows_per);
    for (int64_t r = r0 + rl; r < r1; r += 4) {
      const float x = h[r * ld + c];
      s1 += fabsf(x);
      s2 += x > 0.f ? 1.f : x + 1.f;   // ELU'(z) from y = ELU(z), as in ln.hip
    }
  }
  sh[0][rl][cl] = s1; sh[1][rl][cl] = s2;
  __syncthreads();
  if (rl == 0 && c < cols) {
    part[((int64_t)blockIdx.y * 2 + 0) * cols + c] = (sh[0][0][cl] + sh[0][1][cl]) + (sh[0][2][cl] + sh[0][3][cl]);
    part[((int64_t)blockIdx.y * 2 + 1) * cols + c] = (sh[1][0][cl] + sh[1][1][cl]) + (sh[1][2][cl] + sh[1][3][cl]);
  }
}

// sum of one value per thread over the block: the xor butterfly per wave, then the four waves as (w0 + w1) + (w2 + w3); every thread
// gets the result
__device__ __forceinline__ float unit_block_sum(float v, float (&shw)[4]) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) shw[threadIdx.x >> 6] = v;
  __syncthreads();
  return (shw[0] + shw[1]) + (shw[2] + shw[3]);
}

// Launch 2, one block.  Thread t owns columns t, t + 256, ...: per column the chunks in index order -> a_c (kept in a_out for the
// second pass) and the column's slope sum; the thread's columns in increasing c; then unit_block_sum.
__global__ __launch_bounds__(256) void k_unit_fold(const float* __restrict__ part, int chunks, int64_t rows, int cols, float tau,
                                                   float* __restrict__ a_out, float* __restrict__ out) {
  __shared__ float shw[4];
  float sa = 0.f, ss = 0.f;
  for (int c = threadIdx.x; c < cols; c += 256) {
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < chunks; ++k) {
      s1 += part[((int64_t)k * 2 + 0) * cols + c];
      s2 += part[((int64_t)k * 2 + 1) * cols + c];
    }
    const float a = s1 / (float)rows;
    a_out[c] = a;
    sa += a;
    ss += s2;
  }
  const float A = unit_block_sum(sa, shw) / (float)cols;
  const float S = unit_block_sum(ss, shw);
  const float thr = tau * A;
  float n = 0.f;   // (a count below 2^24: exact in fp32 in any order)
  for (int c = threadIdx.x; c < cols; c += 256) n += a_out[c] <= thr ? 1.f : 0.f;   // (the thread's own stores)
  n = unit_block_sum(n, shw);
  if (threadIdx.x == 0) {
    out[0] = n / (float)cols;
    out[1] = A;
    out[2] = S / ((float)rows * (float)cols);
  }
}

static int unit_chunks(int64_t rows) { return (int)(rows < PQLK_UNIT_CHUNKS ? rows : PQLK_UNIT_CHUNKS); }

extern "C" int64_t pqlk_unit_stats_scratch_floats(int32_t cols) { return cols > 0 ? (int64_t)(2 * PQLK_UNIT_CHUNKS + 1) * cols : 0; }

extern "C" int pqlk_unit_stats(const float* h, int64_t ld, int64_t rows, int32_t cols, float tau, float* out, float* scratch,
                               pqlk_stream_t stream) {
  PQLK_REQUIRE(h && out && scratch, PQLK_E_NULL);
  PQLK_REQUIRE(rows > 0 && cols > 0 && ld >= cols, PQLK_E_SHAPE);
  PQLK_REQUIRE(tau >= 0.f && tau < 1.f, PQLK_E_SHAPE);   // (false for a NaN)
  const int chunks = unit_chunks(rows);
  hipLaunchKernelGGL(k_unit_sums, dim3((unsigned)((cols + 63) / 64), (unsigned)chunks), dim3(256), 0, pqlk_s(stream), h, ld, rows, (int)cols,
                     scratch);
  PQLK_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_unit_fold, dim3(1), dim3(256), 0, pqlk_s(stream), scratch, chunks, rows, (int)cols, tau,
                     scratch + (int64_t)2 * PQLK_UNIT_CHUNKS * cols, out);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}
