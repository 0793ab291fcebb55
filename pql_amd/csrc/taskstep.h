// One-launch step of a hash-reset task (pointmass.hip, swingup.hip; the Python side is `HashResetVecEnv`,
// pql_amd/envs/base.py): everything but the task itself, written once.
//
//   phase 1, one thread per env: the task advances the env in place and hands back reward, terminal and its info channels; the step
//            count, done / truncated and, for a finished env, the episode index + 1 and the task's reset from the counter-based
//            uniform.  INFO: the channels of the step just taken (before the reset) go to the channel-major (N_INFO, N) block
//            `info`, row stride N, one coalesced store per channel;
//   phase 2, the block together: the O-wide next_obs rows of the block's envs, column by column from the task, written with
//            coalesced 16-byte stores where O % 4 == 0 (scalar stores otherwise).
//
// A task is a struct of its three (N, A) state pointers, in the order of the entry point's arguments, with the constant N_INFO
// (its number of info channels, in the order of the env class's `info_keys`) and three `__device__ __forceinline__` members:
//
//   float advance(int64_t e, int A, const float* ae, float inv_a, bool& terminal, float* inf) const
//       one step of env e under the action row ae (not yet clamped): the per-joint loop in index order, the state written in
//       place; returns the reward, sets terminal (a task without terminals sets the constant false, and the time limit alone
//       ends its episodes) and inf[0 .. N_INFO) (registers: a launch without INFO drops them, and what it computes is untouched);
//   void reset(int64_t e, int A, uint32_t env, uint32_t seed, uint32_t epn) const
//       the start state of episode epn of the global env id `env`, from uni_key / uni_col (envhash.h);
//   float obs(int64_t e, int A, int col) const
//       column col of env e's observation row (0 past the task's 3 A columns).
//
// Bit-equality with the torch definitions needs every written operation to round once.  A template takes its floating-point
// options where it is DEFINED, so the pragma stands here as well as in the task files (whose structs stay below their own).
#pragma once
#include "envhash.h"

#pragma clang fp contract(off)

#define TASK_BLOCK 256

template <class Task, bool VEC, bool INFO>
__global__ __launch_bounds__(TASK_BLOCK) void k_task_step(int64_t n, int O, int A, uint32_t seed, uint32_t env0, int ep_len,
                                                          float inv_a, const float* __restrict__ action, Task task, int32_t* k,
                                                          int32_t* ep, float* __restrict__ next_obs, float* __restrict__ reward,
                                                          uint8_t* __restrict__ done, uint8_t* __restrict__ truncated,
                                                          float* __restrict__ info) {
  const int64_t tiles = (n + TASK_BLOCK - 1) / TASK_BLOCK;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // (block-uniform: every thread meets the barrier)
    const int64_t base = tile * TASK_BLOCK;
    const int64_t e = base + threadIdx.x;
    if (e < n) {
      bool terminal;
      float inf[Task::N_INFO];
      const float r = task.advance(e, A, action + e * A, inv_a, terminal, inf);
      const int kn = k[e] + 1;
      const bool trunc = kn >= ep_len && !terminal;
      const bool fin = terminal || trunc;
      reward[e] = r;
      done[e] = fin ? 1 : 0;
      truncated[e] = trunc ? 1 : 0;
      if (INFO) {
#pragma unroll
        for (int c = 0; c < Task::N_INFO; ++c) info[c * n + e] = inf[c];
      }
      if (fin) {
        const uint32_t epn = (uint32_t)ep[e] + 1u;
        task.reset(e, A, env0 + (uint32_t)e, seed, epn);
        ep[e] = (int32_t)epn;
        k[e] = 0;
      } else {
        k[e] = kn;
      }
    }
    __syncthreads();   // the block's new state is in place: phase 2 reads rows written by other lanes
    const int64_t rest = n - base;
    const int rows = rest < TASK_BLOCK ? (int)rest : TASK_BLOCK;
    if (VEC) {
      const int O4 = O >> 2;
      float4* out = reinterpret_cast<float4*>(next_obs + base * O);
      for (int i = threadIdx.x; i < rows * O4; i += TASK_BLOCK) {
        const int r = i / O4, c = (i - r * O4) * 4;
        const int64_t er = base + r;
        out[i] = make_float4(task.obs(er, A, c), task.obs(er, A, c + 1), task.obs(er, A, c + 2), task.obs(er, A, c + 3));
      }
    } else {
      float* out = next_obs + base * O;
      for (int i = threadIdx.x; i < rows * O; i += TASK_BLOCK) {
        const int r = i / O;
        out[i] = task.obs(base + r, A, i - r * O);
      }
    }
  }
}

// The body of a task's `extern "C"` entry points (include/pqlk.h: pqlk_pointmass_step, pqlk_swingup_step and their `_info` forms).
template <class Task, bool INFO>
int launch_task_step(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset, int32_t episode_length,
                     const float* action, float* s0, float* s1, float* s2, int32_t* k, int32_t* ep, float* next_obs, float* reward,
                     uint8_t* done, uint8_t* truncated, float* info, pqlk_stream_t stream) {
  PQLK_REQUIRE(action && s0 && s1 && s2 && k && ep && next_obs && reward && done && truncated && (info || !INFO), PQLK_E_NULL);
  PQLK_REQUIRE(n > 0 && act_dim > 0 && obs_dim >= 3 * (int64_t)act_dim, PQLK_E_SHAPE);
  PQLK_REQUIRE((int64_t)TASK_BLOCK * obs_dim <= INT32_MAX, PQLK_E_SHAPE);   // phase 2 indexes a block's rows with 32-bit ints
  int64_t blocks = (n + TASK_BLOCK - 1) / TASK_BLOCK;
  if (blocks > 65535) blocks = 65535;
  const float inv_a = 1.0f / (float)act_dim;
  const dim3 grid((unsigned)blocks), block(TASK_BLOCK);
  const Task task{s0, s1, s2};
  if ((obs_dim & 3) == 0 && pqlk_aligned16(next_obs))
    hipLaunchKernelGGL((k_task_step<Task, true, INFO>), grid, block, 0, pqlk_s(stream), n, (int)obs_dim, (int)act_dim, seed, env_offset,
                       (int)episode_length, inv_a, action, task, k, ep, next_obs, reward, done, truncated, info);
  else
    hipLaunchKernelGGL((k_task_step<Task, false, INFO>), grid, block, 0, pqlk_s(stream), n, (int)obs_dim, (int)act_dim, seed, env_offset,
                       (int)episode_length, inv_a, action, task, k, ep, next_obs, reward, done, truncated, info);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}
