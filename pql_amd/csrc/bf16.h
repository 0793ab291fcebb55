// fp32 -> bf16 as every bf16-MFMA forward rounds it (fwd_bf16.hip, fwd_ln_bf16.hip, fwd_bro_bf16.hip; the "bf16 law" of include/pqlk.h).
#pragma once
#include "pqlk_common.h"

// round to nearest even, ties included; NaN stays a (quiet) NaN, overflow goes to +-inf
__device__ __forceinline__ unsigned bf16_rne(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
__device__ __forceinline__ unsigned bf16_pack2(float lo, float hi) { return bf16_rne(lo) | (bf16_rne(hi) << 16); }
__device__ __forceinline__ float bf16_round(float f) { return __uint_as_float(bf16_rne(f) << 16); }   // the fp32 value of bf16(f)
