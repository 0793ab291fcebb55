// Temporally correlated exploration noise (algo.noise.color = ar1 | pink): the state update of R AR(1) processes per action element
// and the noised, clamped action, in ONE launch.  The law is stated with pqlk_action_noise_colored in include/pqlk.h; every written
// operation below is one fp32 rounding (no contraction), so a CPU model that rounds after every operation gives the same bits.
//
// One thread per (row, col) element, consecutive threads on consecutive columns: state[e, k, :] and draw[e, k*A : (k+1)*A] share the
// flat index (e * R + k) * A + a, so both are read (and the state written) coalesced, like act and out.  The octave loop carries
// only the running sum; no LDS, no atomics.  Latency-bound (a few MB at most): nothing here is tuned beyond that.
#include "pqlk_common.h"

#pragma clang fp contract(off)

#define NOISE_THREADS 256
#define NOISE_MAX_BLOCKS 4096   // grid cap: past 4096 * 256 elements a thread takes a second one (grid-stride loop)

__global__ __launch_bounds__(NOISE_THREADS) void k_action_noise_colored(
    const float* __restrict__ act, const float* __restrict__ draw, const float* __restrict__ std_rows, float std_scalar,
    const float* __restrict__ rho, const float* __restrict__ coef, int groups, int R, long long env_offset,
    const uint8_t* __restrict__ fresh, float* __restrict__ state, long long total, int cols, float w, float lo, float hi,
    float* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * NOISE_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * NOISE_THREADS) {
    const long long e = i / cols;
    const int a = (int)(i - e * cols);
    const int g = (int)((env_offset + e) % groups);
    const bool first = fresh[e] != 0;
    const float* __restrict__ r = rho + (long long)g * R;
    const float* __restrict__ c = coef + (long long)g * R;
    const long long base = e * R * cols + a;   // (e, 0, a) of state, (e, a) of draw
    float n = 0.f;
    for (int k = 0; k < R; ++k) {
      const long long j = base + (long long)k * cols;
      const float eps = draw[j];
      const float s = first ? eps : (r[k] * state[j]) + (c[k] * eps);
      state[j] = s;
      n = k == 0 ? s : n + s;
    }
    n = n * w;
    const float sigma = std_rows ? std_rows[e] : std_scalar;
    const float noise = n * sigma;
    out[i] = fminf(fmaxf(act[i] + noise, lo), hi);
  }
}

extern "C" int pqlk_action_noise_colored(const float* act, const float* draw, const float* std_rows, float std_scalar, const float* rho,
                                         const float* coef, int32_t groups, int32_t octaves, int64_t env_offset, const uint8_t* fresh,
                                         float* state, int64_t rows, int32_t cols, float w, float lo, float hi, float* out,
                                         pqlk_stream_t stream) {
  PQLK_REQUIRE(act && draw && rho && coef && fresh && state && out, PQLK_E_NULL);
  PQLK_REQUIRE(rows > 0 && cols > 0 && octaves >= 1 && octaves <= PQLK_NOISE_MAX_OCTAVES && groups >= 1 && env_offset >= 0 && lo <= hi,
               PQLK_E_SHAPE);
  const long long total = rows * (long long)cols;
  // out may not alias state: a thread's state rows are read after another thread's out element would have been written
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)total * sizeof(float);
  const uintptr_t s0 = (uintptr_t)state, s1 = s0 + (uintptr_t)total * (uintptr_t)octaves * sizeof(float);
  PQLK_REQUIRE(o1 <= s0 || s1 <= o0, PQLK_E_RANGE);
  long long blocks = (total + NOISE_THREADS - 1) / NOISE_THREADS;
  if (blocks > NOISE_MAX_BLOCKS) blocks = NOISE_MAX_BLOCKS;
  hipLaunchKernelGGL(k_action_noise_colored, dim3((unsigned)blocks), dim3(NOISE_THREADS), 0, pqlk_s(stream), act, draw, std_rows,
                     std_scalar, rho, coef, (int)groups, (int)octaves, (long long)env_offset, fresh, state, total, cols, w, lo, hi, out);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}
