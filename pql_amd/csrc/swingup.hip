// SwingUp vectorised environment step in ONE launch (not a reference component: the nonlinear learnable task of
// pql_amd/envs/swingup.py, whose `_step_torch` is the definition and costs ~200 elementwise torch launches).
// A independent torque-limited pendulums per env, held as (cos, sin) of the angle from upright and the angular velocity.
// The launch itself -- tiles, counters, done / truncated, the reset of finished envs, the next_obs rows -- is the shared
// `k_task_step` of taskstep.h; this file is the task:
//
//   advance: clamp the action, integrate (w, then the rotation of (c, s) by 0.05 w') in place, reduce the cost over the A joints
//            IN INDEX ORDER, form the reward; no terminal (the speed is clamped instead), so every done is a time limit; info
//            channels (upright, effort) = the means over the joints of c' and of a^2, both summed in index order;
//   reset:   (c, s) = four rotations of hanging by a draw from the counter-based uniform of envhash.h, w another draw;
//   obs:     [c | s | 0.125 w | 0 ...].
//
// The rotation (rot.h) is a polynomial followed by one Newton step back to the unit circle: no transcendental function, no division,
// no square root.  No atomics and no contraction: every operation rounds once to fp32 exactly like the separate torch ops,
// so every output is bit-equal to the definition.
#include "taskstep.h"
#include "rot.h"

#pragma clang fp contract(off)

#define SU_STREAM_TH 13u
#define SU_STREAM_W 14u

struct SwingUpTask {
  float *c, *s, *w;
  static constexpr int N_INFO = 2;   // upright, effort (SwingUpVecEnv.info_keys)

  __device__ __forceinline__ float advance(int64_t e, int A, const float* ae, float inv_a, bool& terminal, float* inf) const {
    float *ce = c + e * A, *se = s + e * A, *we = w + e * A;
    float cost = 0.f, up = 0.f, eff = 0.f;
    for (int j = 0; j < A; ++j) {
      float a = ae[j];
      a = a < -1.f ? -1.f : (a > 1.f ? 1.f : a);
      float cj = ce[j], sj = se[j];
      float wn = we[j] + 0.05f * (15.0f * sj + 6.0f * a);
      wn = wn < -8.f ? -8.f : (wn > 8.f ? 8.f : wn);
      task_rot(cj, sj, 0.05f * wn);
      const float cost_j = ((1.0f - cj) + 0.01f * (wn * wn)) + 0.01f * (a * a);
      cost = j == 0 ? cost_j : cost + cost_j;
      up = j == 0 ? cj : up + cj;
      eff = j == 0 ? a * a : eff + a * a;
      we[j] = wn;
      ce[j] = cj;
      se[j] = sj;
    }
    terminal = false;
    inf[0] = up * inv_a;
    inf[1] = eff * inv_a;
    return -(0.05f * (cost * inv_a));
  }

  __device__ __forceinline__ void reset(int64_t e, int A, uint32_t env, uint32_t seed, uint32_t epn) const {
    float *ce = c + e * A, *se = s + e * A, *we = w + e * A;
    const uint32_t kt = uni_key(env, seed, epn, SU_STREAM_TH), kw = uni_key(env, seed, epn, SU_STREAM_W);
    for (int j = 0; j < A; ++j) {
      const float d = 0.5f * (2.0f * uni_col(kt, (uint32_t)j) - 1.0f);
      float cj = -1.f, sj = 0.f;   // hanging; four rotations by d: up to +-2 rad away from it
      task_rot(cj, sj, d);
      task_rot(cj, sj, d);
      task_rot(cj, sj, d);
      task_rot(cj, sj, d);
      ce[j] = cj;
      se[j] = sj;
      we[j] = 2.0f * uni_col(kw, (uint32_t)j) - 1.0f;
    }
  }

  __device__ __forceinline__ float obs(int64_t e, int A, int col) const {
    if (col < A) return c[e * A + col];
    if (col < 2 * A) return s[e * A + (col - A)];
    if (col < 3 * A) return 0.125f * w[e * A + (col - 2 * A)];
    return 0.f;
  }
};

extern "C" int pqlk_swingup_step(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                                 int32_t episode_length, const float* action, float* c, float* s, float* w, int32_t* k,
                                 int32_t* ep, float* next_obs, float* reward, uint8_t* done, uint8_t* truncated,
                                 pqlk_stream_t stream) {
  return launch_task_step<SwingUpTask, false>(n, obs_dim, act_dim, seed, env_offset, episode_length, action, c, s, w, k, ep, next_obs,
                                              reward, done, truncated, nullptr, stream);
}

extern "C" int pqlk_swingup_step_info(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                                      int32_t episode_length, const float* action, float* c, float* s, float* w, int32_t* k,
                                      int32_t* ep, float* next_obs, float* reward, uint8_t* done, uint8_t* truncated, float* info,
                                      pqlk_stream_t stream) {
  return launch_task_step<SwingUpTask, true>(n, obs_dim, act_dim, seed, env_offset, episode_length, action, c, s, w, k, ep, next_obs,
                                             reward, done, truncated, info, stream);
}
