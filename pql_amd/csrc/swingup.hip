// SwingUp vectorised environment step in ONE launch (not a reference component: the nonlinear learnable task of
// pql_amd/envs/swingup.py, whose `_step_torch` is the definition and costs ~200 elementwise torch launches).
// A independent torque-limited pendulums per env, held as (cos, sin) of the angle from upright and the angular velocity.
//
//   phase 1, one thread per env: clamp the action, integrate (w, then the rotation of (c, s) by 0.05 w') in place, reduce the
//            cost over the A joints IN INDEX ORDER, form reward / done / truncated, and reset a finished env
//            (episode index + 1, start state from the counter-based uniform of envhash.h);
//   phase 2, the block together: the O-wide next_obs rows [c | s | 0.125 w | 0 ...] of the block's envs, written with
//            coalesced 16-byte stores where O % 4 == 0 (scalar stores otherwise).
//
// The rotation is a polynomial followed by one Newton step back to the unit circle: no transcendental function, no division,
// no square root.  No atomics and no contraction: every operation rounds once to fp32 exactly like the separate torch ops,
// so every output is bit-equal to the definition.
#include "envhash.h"

#pragma clang fp contract(off)

#define SU_BLOCK 256
#define SU_STREAM_TH 13u
#define SU_STREAM_W 14u

// (c, s) rotated by the angle d, |d| <= 0.5: cos d and sin d to degree 4 / 5, then m = 1.5 - 0.5 |.|^2 pulls the result back
// to the unit circle.  The operation order is the one of `_rot` in pql_amd/envs/swingup.py.
__device__ __forceinline__ void su_rot(float& c, float& s, float d) {
  const float d2 = d * d;
  const float cd = 1.0f - d2 * (0.5f - d2 * 0.041666668f);
  const float sd = d * (1.0f - d2 * (0.16666667f - d2 * 0.008333334f));
  const float cn = c * cd - s * sd;
  const float sn = s * cd + c * sd;
  const float m = 1.5f - 0.5f * (cn * cn + sn * sn);
  c = cn * m;
  s = sn * m;
}

// column col of the observation row of env e: [c | s | 0.125 w | 0 ... 0]
__device__ __forceinline__ float su_obs_elem(const float* c, const float* s, const float* w, int64_t e, int A, int col) {
  if (col < A) return c[e * A + col];
  if (col < 2 * A) return s[e * A + (col - A)];
  if (col < 3 * A) return 0.125f * w[e * A + (col - 2 * A)];
  return 0.f;
}

template <bool VEC>
__global__ __launch_bounds__(SU_BLOCK) void k_swingup_step(int64_t n, int O, int A, uint32_t seed, uint32_t env0, int ep_len,
                                                           float inv_a, const float* __restrict__ action, float* c, float* s,
                                                           float* w, int32_t* k, int32_t* ep, float* __restrict__ next_obs,
                                                           float* __restrict__ reward, uint8_t* __restrict__ done,
                                                           uint8_t* __restrict__ truncated) {
  const int64_t tiles = (n + SU_BLOCK - 1) / SU_BLOCK;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // (block-uniform: every thread meets the barrier)
    const int64_t base = tile * SU_BLOCK;
    const int64_t e = base + threadIdx.x;
    if (e < n) {
      const float* ae = action + e * A;
      float *ce = c + e * A, *se = s + e * A, *we = w + e * A;
      float cost = 0.f;
      for (int j = 0; j < A; ++j) {
        float a = ae[j];
        a = a < -1.f ? -1.f : (a > 1.f ? 1.f : a);
        float cj = ce[j], sj = se[j];
        float wn = we[j] + 0.05f * (15.0f * sj + 6.0f * a);
        wn = wn < -8.f ? -8.f : (wn > 8.f ? 8.f : wn);
        su_rot(cj, sj, 0.05f * wn);
        const float cost_j = ((1.0f - cj) + 0.01f * (wn * wn)) + 0.01f * (a * a);
        cost = j == 0 ? cost_j : cost + cost_j;
        we[j] = wn;
        ce[j] = cj;
        se[j] = sj;
      }
      const int kn = k[e] + 1;
      const bool trunc = kn >= ep_len;   // no terminals: the speed is clamped instead
      reward[e] = -(0.05f * (cost * inv_a));
      done[e] = trunc ? 1 : 0;
      truncated[e] = trunc ? 1 : 0;
      if (trunc) {
        const uint32_t epn = (uint32_t)ep[e] + 1u, env = env0 + (uint32_t)e;
        const uint32_t kt = uni_key(env, seed, epn, SU_STREAM_TH), kw = uni_key(env, seed, epn, SU_STREAM_W);
        for (int j = 0; j < A; ++j) {
          const float d = 0.5f * (2.0f * uni_col(kt, (uint32_t)j) - 1.0f);
          float cj = -1.f, sj = 0.f;   // hanging; four rotations by d: up to +-2 rad away from it
          su_rot(cj, sj, d);
          su_rot(cj, sj, d);
          su_rot(cj, sj, d);
          su_rot(cj, sj, d);
          ce[j] = cj;
          se[j] = sj;
          we[j] = 2.0f * uni_col(kw, (uint32_t)j) - 1.0f;
        }
        ep[e] = (int32_t)epn;
        k[e] = 0;
      } else {
        k[e] = kn;
      }
    }
    __syncthreads();   // the block's new state is in place: phase 2 reads rows written by other lanes
    const int64_t rest = n - base;
    const int rows = rest < SU_BLOCK ? (int)rest : SU_BLOCK;
    if (VEC) {
      const int O4 = O >> 2;
      float4* out = reinterpret_cast<float4*>(next_obs + base * O);
      for (int i = threadIdx.x; i < rows * O4; i += SU_BLOCK) {
        const int r = i / O4, col = (i - r * O4) * 4;
        const int64_t er = base + r;
        out[i] = make_float4(su_obs_elem(c, s, w, er, A, col), su_obs_elem(c, s, w, er, A, col + 1),
                             su_obs_elem(c, s, w, er, A, col + 2), su_obs_elem(c, s, w, er, A, col + 3));
      }
    } else {
      float* out = next_obs + base * O;
      for (int i = threadIdx.x; i < rows * O; i += SU_BLOCK) {
        const int r = i / O;
        out[i] = su_obs_elem(c, s, w, base + r, A, i - r * O);
      }
    }
  }
}

extern "C" int pqlk_swingup_step(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                                 int32_t episode_length, const float* action, float* c, float* s, float* w, int32_t* k,
                                 int32_t* ep, float* next_obs, float* reward, uint8_t* done, uint8_t* truncated,
                                 pqlk_stream_t stream) {
  PQLK_REQUIRE(action && c && s && w && k && ep && next_obs && reward && done && truncated, PQLK_E_NULL);
  PQLK_REQUIRE(n > 0 && act_dim > 0 && obs_dim >= 3 * (int64_t)act_dim, PQLK_E_SHAPE);
  PQLK_REQUIRE((int64_t)SU_BLOCK * obs_dim <= INT32_MAX, PQLK_E_SHAPE);   // phase 2 indexes a block's rows with 32-bit ints
  int64_t blocks = (n + SU_BLOCK - 1) / SU_BLOCK;
  if (blocks > 65535) blocks = 65535;
  const float inv_a = 1.0f / (float)act_dim;
  const dim3 grid((unsigned)blocks), block(SU_BLOCK);
  if ((obs_dim & 3) == 0 && pqlk_aligned16(next_obs))
    hipLaunchKernelGGL(k_swingup_step<true>, grid, block, 0, pqlk_s(stream), n, (int)obs_dim, (int)act_dim, seed, env_offset,
                       (int)episode_length, inv_a, action, c, s, w, k, ep, next_obs, reward, done, truncated);
  else
    hipLaunchKernelGGL(k_swingup_step<false>, grid, block, 0, pqlk_s(stream), n, (int)obs_dim, (int)act_dim, seed, env_offset,
                       (int)episode_length, inv_a, action, c, s, w, k, ep, next_obs, reward, done, truncated);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}
