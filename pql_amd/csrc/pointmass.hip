// PointMass vectorised environment step in ONE launch (not a reference component: the learnable task of
// pql_amd/envs/pointmass.py, whose `_step_torch` is the definition and costs ~40 elementwise / masked torch launches).
// The launch itself -- tiles, counters, done / truncated, the reset of finished envs, the next_obs rows -- is the shared
// `k_task_step` of taskstep.h; this file is the task:
//
//   advance: clamp the action, integrate (v, x) in place, reduce the squared distance and the action cost over the A columns
//            IN INDEX ORDER, form the reward; terminal = some |x'_j| > 1.5; info channels (dist2, oob) = the reward's own mean
//            squared distance and 1.0 / 0.0 for the terminal;
//   reset:   x, g from the counter-based uniform of envhash.h, v = 0;
//   obs:     [x | v | g | 0 ...].
//
// No atomics, no transcendental functions, and no contraction: every operation rounds once to fp32 exactly like the
// separate torch ops, so every output is bit-equal to the definition.
#include "taskstep.h"

#pragma clang fp contract(off)

#define PM_STREAM_X 11u
#define PM_STREAM_G 12u

struct PointMassTask {
  float *x, *v, *g;
  static constexpr int N_INFO = 2;   // dist2, oob (PointMassVecEnv.info_keys)

  __device__ __forceinline__ float advance(int64_t e, int A, const float* ae, float inv_a, bool& terminal, float* inf) const {
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
    terminal = oob;
    inf[0] = d2;
    inf[1] = oob ? 1.f : 0.f;
    return (-d2 - 0.01f * a2) - (oob ? 1.f : 0.f);
  }

  __device__ __forceinline__ void reset(int64_t e, int A, uint32_t env, uint32_t seed, uint32_t epn) const {
    float *xe = x + e * A, *ve = v + e * A, *ge = g + e * A;
    const uint32_t kx = uni_key(env, seed, epn, PM_STREAM_X), kg = uni_key(env, seed, epn, PM_STREAM_G);
    for (int j = 0; j < A; ++j) {
      xe[j] = 2.0f * uni_col(kx, (uint32_t)j) - 1.0f;
      ge[j] = 2.0f * uni_col(kg, (uint32_t)j) - 1.0f;
      ve[j] = 0.f;
    }
  }

  __device__ __forceinline__ float obs(int64_t e, int A, int c) const {
    if (c < A) return x[e * A + c];
    if (c < 2 * A) return v[e * A + (c - A)];
    if (c < 3 * A) return g[e * A + (c - 2 * A)];
    return 0.f;
  }
};

extern "C" int pqlk_pointmass_step(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                                   int32_t episode_length, const float* action, float* x, float* v, float* g, int32_t* k,
                                   int32_t* ep, float* next_obs, float* reward, uint8_t* done, uint8_t* truncated,
                                   pqlk_stream_t stream) {
  return launch_task_step<PointMassTask, false>(n, obs_dim, act_dim, seed, env_offset, episode_length, action, x, v, g, k, ep, next_obs,
                                                reward, done, truncated, nullptr, stream);
}

extern "C" int pqlk_pointmass_step_info(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                                        int32_t episode_length, const float* action, float* x, float* v, float* g, int32_t* k,
                                        int32_t* ep, float* next_obs, float* reward, uint8_t* done, uint8_t* truncated, float* info,
                                        pqlk_stream_t stream) {
  return launch_task_step<PointMassTask, true>(n, obs_dim, act_dim, seed, env_offset, episode_length, action, x, v, g, k, ep, next_obs,
                                               reward, done, truncated, info, stream);
}
