// The LayerNorm row routine of include/pqlk.h's law, shared by the row kernels of ln.hip and the whole-stack forward of fwd_ln.hip:
// one wavefront holds a row in registers (VPL values per lane), sums it as per-lane partials in register order followed by the
// 64-lane xor butterfly of wave_sum, and every written operation is one fp32 rounding (-ffp-contract=off).
#pragma once
#include "pqlk_common.h"

__device__ __forceinline__ float ln_elu(float x) { return x > 0.f ? x : expm1f(x); }   // nn.ELU(alpha=1)

// register slot i of lane `lane` <-> column: VEC: chunks of V consecutive columns, chunk k of a lane at (k * 64 + lane) * V;
// scalar: column i * 64 + lane
template <int VPL, bool VEC>
struct LnMap {
  static constexpr int V = VEC ? (VPL == 2 ? 2 : 4) : 1;
  static constexpr int NCH = VPL / V;
  __device__ static __forceinline__ int col(int i, int lane) { return ((i / V) * 64 + lane) * V + (i % V); }
};

// p[0, cols) -> v, slots past cols = 0 (nothing past cols is read)
template <int VPL, bool VEC>
__device__ __forceinline__ void ln_load(const float* __restrict__ p, int cols, int lane, float (&v)[VPL]) {
  using M = LnMap<VPL, VEC>;
#pragma unroll
  for (int k = 0; k < M::NCH; ++k) {
    const int c0 = (k * 64 + lane) * M::V;
    if (M::V == 4 && c0 + 4 <= cols) {
      const float4 t = *reinterpret_cast<const float4*>(p + c0);
      v[k * M::V + 0] = t.x; v[k * M::V + 1 % M::V] = t.y; v[k * M::V + 2 % M::V] = t.z; v[k * M::V + 3 % M::V] = t.w;
    } else if (M::V == 2 && c0 + 2 <= cols) {
      const float2 t = *reinterpret_cast<const float2*>(p + c0);
      v[k * M::V + 0] = t.x; v[k * M::V + 1 % M::V] = t.y;
    } else {
#pragma unroll
      for (int e = 0; e < M::V; ++e) v[k * M::V + e] = c0 + e < cols ? p[c0 + e] : 0.f;
    }
  }
}

// v -> p[0, cols); nothing past cols is written
template <int VPL, bool VEC>
__device__ __forceinline__ void ln_store(float* __restrict__ p, int cols, int lane, const float (&v)[VPL]) {
  using M = LnMap<VPL, VEC>;
#pragma unroll
  for (int k = 0; k < M::NCH; ++k) {
    const int c0 = (k * 64 + lane) * M::V;
    if (M::V == 4 && c0 + 4 <= cols) {
      *reinterpret_cast<float4*>(p + c0) = make_float4(v[k * M::V + 0], v[k * M::V + 1 % M::V], v[k * M::V + 2 % M::V], v[k * M::V + 3 % M::V]);
    } else if (M::V == 2 && c0 + 2 <= cols) {
      *reinterpret_cast<float2*>(p + c0) = make_float2(v[k * M::V + 0], v[k * M::V + 1 % M::V]);
    } else {
#pragma unroll
      for (int e = 0; e < M::V; ++e)
        if (c0 + e < cols) p[c0 + e] = v[k * M::V + e];
    }
  }
}

// The law's statistics of the row held in `float v[VPL]` (slots past cols hold 0), in the scope it is written in: declares mu = mean
// and rs = rstd and leaves v_j = z_j - mean (0 past cols).  Needs M = LnMap<VPL, VEC>, cols, lane, n = (float)cols and eps there.
// (A macro, not a function: as a function the row kernels of ln.hip come out with their additions' operands swapped -- the same
// bits, but tools/kernel_resources.py --same holds those kernels to their instructions.)
#define LN_ROW_CENTER(v)                                          \
  float s = 0.f;                                                  \
  _Pragma("unroll") for (int i = 0; i < VPL; ++i) s += v[i];      \
  const float mu = wave_sum(s) / n;                               \
  float q = 0.f;                                                  \
  _Pragma("unroll") for (int i = 0; i < VPL; ++i) {               \
    const float d = M::col(i, lane) < cols ? v[i] - mu : 0.f;     \
    v[i] = d;                                                     \
    q += d * d;                                                   \
  }                                                               \
  const float var = wave_sum(q) / n;                              \
  const float rs = 1.0f / sqrtf(var + eps);
