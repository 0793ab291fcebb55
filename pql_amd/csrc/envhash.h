// Counter-based uniform shared by the env-step kernels (synth.hip, and through taskstep.h the hash-reset tasks
// pointmass.hip and swingup.hip): a pure function of (global env id, seed, counter, stream, column), so data-parallel
// shards reproduce slices of the global env.  Same constants as `_hash32` / `_uniform` of pql_amd/envs/base.py.
// A new hash-reset task is a task struct for `k_task_step` (taskstep.h says what it has to supply), its own stream
// numbers for uni_key, and an `extern "C"` entry point that calls `launch_task_step`.
#pragma once
#include "pqlk_common.h"

__device__ __forceinline__ uint32_t hash32(uint32_t x) {
  x = (x ^ (x >> 16)) * 0x7FEB352Du;
  x = (x ^ (x >> 15)) * 0x846CA68Bu;
  return x ^ (x >> 16);
}

__device__ __forceinline__ uint32_t uni_key(uint32_t env, uint32_t seed, uint32_t t, uint32_t stream) {
  return hash32(env * 0x9E3779B1u + seed * 0x85EBCA77u + t * 0xC2B2AE3Du + stream * 0x27D4EB2Fu);
}

__device__ __forceinline__ float uni_col(uint32_t key, uint32_t col) {
  const uint32_t h = hash32(key * 0x165667B1u + col * 0x9E3779B1u + 0x5BD1E995u);
  return ((float)h + 0.5f) * (1.0f / 4294967296.0f);
}

__device__ __forceinline__ float uni(uint32_t env, uint32_t seed, uint32_t t, uint32_t stream, uint32_t col) {
  return uni_col(uni_key(env, seed, t, stream), col);
}
