// PointMass vectorised environment step in ONE launch (not a reference component: the learnable task of
// pql_amd/envs/pointmass.py, whose `_step_torch` is the definition and costs ~40 elementwise / masked torch launches).
//
//   phase 1, one thread per env: clamp the action, integrate (v, x) in place, reduce the squared distance and the
//            action cost over the A columns IN INDEX ORDER, form reward / done / truncated, and reset a finished env
//            (episode index + 1, start state from the counter-based uniform of envhash.h);
//   phase 2, the block together: the O-wide next_obs rows [x | v | g | 0 ...] of the block's envs, written with
//            coalesced 16-byte stores where O % 4 == 0 (scalar stores otherwise).
//
// No atomics, no transcendental functions, and no contraction: every operation rounds once to fp32 exactly like the
// separate torch ops, so every output is bit-equal to the definition.
#include "envhash.h"

#pragma clang fp contract(off)

#define PM_BLOCK 256
#define PM_STREAM_X 11u
#define PM_STREAM_G 12u

// column c of the observation row of env e: [x | v | g | 0 ... 0]
__device__ __forceinline__ float pm_obs_elem(const float* x, const float* v, const float* g, int64_t e, int A, int c) {
  if (c < A) return x[e * A + c];
  if (c < 2 * A) return v[e * A + (c - A)];
  if (c < 3 * A) return g[e * A + (c - 2 * A)];
  return 0.f;
}

template <bool VEC>
__global__ __launch_bounds__(PM_BLOCK) void k_pointmass_step(int64_t n, int O, int A, uint32_t seed, uint32_t env0, int ep_len,
                                                             float inv_a, const float* __restrict__ action, float* x, float* v,
                                                             float* g, int32_t* k, int32_t* ep, float* __restrict__ next_obs,
                                                             float* __restrict__ reward, uint8_t* __restrict__ done,
                                                             uint8_t* __restrict__ truncated) {
  const int64_t tiles = (n + PM_BLOCK - 1) / PM_BLOCK;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // (block-uniform: every thread meets the barrier)
    const int64_t base = tile * PM_BLOCK;
    const int64_t e = base + threadIdx.x;
    if (e < n) {
      const float* ae = action + e * A;
      float *xe = x + e * A, *ve = v + e * A, *ge = g + e * A;
      float d2 = 0.f, a2 = 0.f;
      bool oob = false;
      for (int j = 0; j < A; ++j) {
        float a = ae[j];
        a = a < -1.f ? -1.f : (a > 1.f ? 1.f : a);
        const float vn = 0.8f * ve[j] + 0.2f * a;
        const float xn = xe[j] + 0.25f * vn;
        const float df = xn - ge[j];
        d2 = d2 + df * df;
        a2 = a2 + a * a;
        oob = oob || fabsf(xn) > 1.5f;
        ve[j] = vn;
        xe[j] = xn;
      }
      d2 = d2 * inv_a;
      a2 = a2 * inv_a;
      const int kn = k[e] + 1;
      const bool trunc = kn >= ep_len && !oob;
      const bool fin = oob || trunc;
      reward[e] = (-d2 - 0.01f * a2) - (oob ? 1.f : 0.f);
      done[e] = fin ? 1 : 0;
      truncated[e] = trunc ? 1 : 0;
      if (fin) {
        const uint32_t epn = (uint32_t)ep[e] + 1u, env = env0 + (uint32_t)e;
        const uint32_t kx = uni_key(env, seed, epn, PM_STREAM_X), kg = uni_key(env, seed, epn, PM_STREAM_G);
        for (int j = 0; j < A; ++j) {
          xe[j] = 2.0f * uni_col(kx, (uint32_t)j) - 1.0f;
          ge[j] = 2.0f * uni_col(kg, (uint32_t)j) - 1.0f;
          ve[j] = 0.f;
        }
        ep[e] = (int32_t)epn;
        k[e] = 0;
      } else {
        k[e] = kn;
      }
    }
    __syncthreads();   // the block's new state is in place: phase 2 reads rows written by other lanes
    const int64_t rest = n - base;
    const int rows = rest < PM_BLOCK ? (int)rest : PM_BLOCK;
    if (VEC) {
      const int O4 = O >> 2;
      float4* out = reinterpret_cast<float4*>(next_obs + base * O);
      for (int i = threadIdx.x; i < rows * O4; i += PM_BLOCK) {
        const int r = i / O4, c = (i - r * O4) * 4;
        const int64_t er = base + r;
        out[i] = make_float4(pm_obs_elem(x, v, g, er, A, c), pm_obs_elem(x, v, g, er, A, c + 1),
                             pm_obs_elem(x, v, g, er, A, c + 2), pm_obs_elem(x, v, g, er, A, c + 3));
      }
    } else {
      float* out = next_obs + base * O;
      for (int i = threadIdx.x; i < rows * O; i += PM_BLOCK) {
        const int r = i / O;
        out[i] = pm_obs_elem(x, v, g, base + r, A, i - r * O);
      }
    }
  }
}

extern "C" int pqlk_pointmass_step(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                                   int32_t episode_length, const float* action, float* x, float* v, float* g, int32_t* k,
                                   int32_t* ep, float* next_obs, float* reward, uint8_t* done, uint8_t* truncated,
                                   pqlk_stream_t stream) {
  PQLK_REQUIRE(action && x && v && g && k && ep && next_obs && reward && done && truncated, PQLK_E_NULL);
  PQLK_REQUIRE(n > 0 && act_dim > 0 && obs_dim >= 3 * (int64_t)act_dim, PQLK_E_SHAPE);
  PQLK_REQUIRE((int64_t)PM_BLOCK * obs_dim <= INT32_MAX, PQLK_E_SHAPE);   // phase 2 indexes a block's rows with 32-bit ints
  int64_t blocks = (n + PM_BLOCK - 1) / PM_BLOCK;
  if (blocks > 65535) blocks = 65535;
  const float inv_a = 1.0f / (float)act_dim;
  const dim3 grid((unsigned)blocks), block(PM_BLOCK);
  if ((obs_dim & 3) == 0 && pqlk_aligned16(next_obs))
    hipLaunchKernelGGL(k_pointmass_step<true>, grid, block, 0, pqlk_s(stream), n, (int)obs_dim, (int)act_dim, seed, env_offset,
                       (int)episode_length, inv_a, action, x, v, g, k, ep, next_obs, reward, done, truncated);
  else
    hipLaunchKernelGGL(k_pointmass_step<false>, grid, block, 0, pqlk_s(stream), n, (int)obs_dim, (int)act_dim, seed, env_offset,
                       (int)episode_length, inv_a, action, x, v, g, k, ep, next_obs, reward, done, truncated);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}
