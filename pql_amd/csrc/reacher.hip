// Reacher vectorised environment step in ONE launch (not a reference component: the coupled learnable task of
// pql_amd/envs/reacher.py, whose `_step_torch` is the definition).  A planar arm of A links of length 1 / A per env, joint j
// held as (cos, sin) of its angle relative to link j - 1 (joint 0: to the world x axis) and its angular velocity; the tip has to
// reach the fixed point (0.6, 0).  The joint dynamics are per joint; the reward and two observation columns go through the forward
// kinematics of the whole chain, so every joint's best action depends on all the others.  The launch itself is the shared
// `k_task_step` of taskstep.h; this file is the task:
//
//   advance: clamp the action, integrate (w, then the rotation of (c, s) by 0.05 w') in place with the two effort sums IN INDEX
//            ORDER, then the chain over the new state (`reacher_tip`), the cost and the reward; no terminal, so every done is a
//            time limit; info channels (tip_dist2, effort, reached) = d2, the mean of a^2, and 1.0 where d2 < 0.01;
//   reset:   (c, s) = six rotations of (1, 0) by a draw from the counter-based uniform of envhash.h, w another draw;
//   obs:     [c | s | 0.25 w | ex | ey | 0 ...]: the two tip columns run `reacher_tip` on the state in place (after a reset: the
//            new episode's), the very operations of advance, so they are bit-equal to the definition's as well.
//
// No transcendental function, no division, no square root, no atomics and no contraction: every operation rounds once to fp32
// exactly like the separate torch ops, so every output is bit-equal to the definition.
#include "taskstep.h"
#include "rot.h"

#pragma clang fp contract(off)

#define RE_STREAM_TH 15u
#define RE_STREAM_W 16u

// Tip error of the chain held in ce[0 .. A), se[0 .. A): (C, S) = direction of link j (the angle sum, by the addition theorems, both
// from the old C, S), the tip = the sum of the directions in index order times the link length 1 / A, minus the goal (0.6, 0).
__device__ __forceinline__ void reacher_link(float& C, float& S, float& x, float& y, float cj, float sj) {
  const float Cn = C * cj - S * sj;
  const float Sn = S * cj + C * sj;
  C = Cn;
  S = Sn;
  x = x + C;
  y = y + S;
}

// (The chain is serial in its arithmetic only: four joints' loads are issued together, so a lane waits for memory once per four
// links and not once per link -- in phase 2 a whole wave waits for its few tip lanes.)
__device__ __forceinline__ void reacher_tip(const float* ce, const float* se, int A, float inv_a, float& ex, float& ey) {
  float C = ce[0], S = se[0];
  float x = C, y = S;
  int j = 1;
  for (; j + 4 <= A; j += 4) {
    const float c0 = ce[j], c1 = ce[j + 1], c2 = ce[j + 2], c3 = ce[j + 3];
    const float s0 = se[j], s1 = se[j + 1], s2 = se[j + 2], s3 = se[j + 3];
    reacher_link(C, S, x, y, c0, s0);
    reacher_link(C, S, x, y, c1, s1);
    reacher_link(C, S, x, y, c2, s2);
    reacher_link(C, S, x, y, c3, s3);
  }
  for (; j < A; ++j) reacher_link(C, S, x, y, ce[j], se[j]);
  ex = x * inv_a - 0.6f;
  ey = y * inv_a;
}

struct ReacherTask {
  float *c, *s, *w;
  static constexpr int N_INFO = 3;   // tip_dist2, effort, reached (ReacherVecEnv.info_keys)

  __device__ __forceinline__ float advance(int64_t e, int A, const float* ae, float inv_a, bool& terminal, float* inf) const {
    float *ce = c + e * A, *se = s + e * A, *we = w + e * A;
    float w2 = 0.f, eff = 0.f;
    for (int j = 0; j < A; ++j) {
      float a = ae[j];
      a = a < -1.f ? -1.f : (a > 1.f ? 1.f : a);
      float cj = ce[j], sj = se[j];
      float wn = 0.9f * we[j] + 0.3f * a;
      wn = wn < -3.f ? -3.f : (wn > 3.f ? 3.f : wn);
      task_rot(cj, sj, 0.05f * wn);
      w2 = j == 0 ? wn * wn : w2 + wn * wn;
      eff = j == 0 ? a * a : eff + a * a;
      we[j] = wn;
      ce[j] = cj;
      se[j] = sj;
    }
    float ex, ey;
    reacher_tip(ce, se, A, inv_a, ex, ey);   // (this thread's own stores, read back)
    const float d2 = ex * ex + ey * ey;
    eff = eff * inv_a;
    const float cost = (d2 + 0.01f * (w2 * inv_a)) + 0.01f * eff;
    terminal = false;
    inf[0] = d2;
    inf[1] = eff;
    inf[2] = d2 < 0.01f ? 1.f : 0.f;
    return -(0.05f * cost);
  }

  __device__ __forceinline__ void reset(int64_t e, int A, uint32_t env, uint32_t seed, uint32_t epn) const {
    float *ce = c + e * A, *se = s + e * A, *we = w + e * A;
    const uint32_t kt = uni_key(env, seed, epn, RE_STREAM_TH), kw = uni_key(env, seed, epn, RE_STREAM_W);
    for (int j = 0; j < A; ++j) {
      const float d = 0.5f * (2.0f * uni_col(kt, (uint32_t)j) - 1.0f);
      float cj = 1.f, sj = 0.f;   // straight on; six rotations by d: up to +-3 rad
      for (int r = 0; r < 6; ++r) task_rot(cj, sj, d);
      ce[j] = cj;
      se[j] = sj;
      we[j] = 0.5f * (2.0f * uni_col(kw, (uint32_t)j) - 1.0f);
    }
  }

  __device__ __forceinline__ float obs(int64_t e, int A, int col) const {
    if (col < A) return c[e * A + col];
    if (col < 2 * A) return s[e * A + (col - A)];
    if (col < 3 * A) return 0.25f * w[e * A + (col - 2 * A)];
    if (col > 3 * A + 1) return 0.f;
    float ex, ey;
    reacher_tip(c + e * A, s + e * A, A, 1.0f / (float)A, ex, ey);
    return col == 3 * A ? ex : ey;
  }
};

extern "C" int pqlk_reacher_step(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                                 int32_t episode_length, const float* action, float* c, float* s, float* w, int32_t* k,
                                 int32_t* ep, float* next_obs, float* reward, uint8_t* done, uint8_t* truncated,
                                 pqlk_stream_t stream) {
  PQLK_REQUIRE(obs_dim >= 3 * (int64_t)act_dim + 2, PQLK_E_SHAPE);
  return launch_task_step<ReacherTask, false>(n, obs_dim, act_dim, seed, env_offset, episode_length, action, c, s, w, k, ep, next_obs,
                                              reward, done, truncated, nullptr, stream);
}

extern "C" int pqlk_reacher_step_info(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                                      int32_t episode_length, const float* action, float* c, float* s, float* w, int32_t* k,
                                      int32_t* ep, float* next_obs, float* reward, uint8_t* done, uint8_t* truncated, float* info,
                                      pqlk_stream_t stream) {
  PQLK_REQUIRE(obs_dim >= 3 * (int64_t)act_dim + 2, PQLK_E_SHAPE);
  return launch_task_step<ReacherTask, true>(n, obs_dim, act_dim, seed, env_offset, episode_length, action, c, s, w, k, ep, next_obs,
                                             reward, done, truncated, info, stream);
}
