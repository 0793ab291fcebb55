// LayerNorm + ELU for the LayerNorm twin critic (DoubleQLayerNorm: `Linear -> LayerNorm -> ELU` blocks on DDPG / SAC).  The Linear
// parts run on the fp32-MFMA GEMMs (a one-layer PqlMlpDesc); what is here is the row-wise normalise + activate pass, its backward
// and the column sums the backward needs for dgamma / dbeta.  The law is written op by op in include/pqlk.h; every written
// operation is one fp32 rounding (the library is built with -ffp-contract=off, division and sqrtf are correctly rounded).
//
// Shape: one wavefront per row, four rows per 256-thread block, the row held in registers (VPL values per lane: 2 / 4 / 8 / 16 for
// cols <= 128 / 256 / 512 / 1024, ragged widths masked); wider rows take a strided path that re-reads the row.  16-byte (8-byte at
// VPL = 2) accesses when every pointer is 16-B aligned and ld % 4 == 0, scalar ones otherwise.  Row sums: per-lane partials in
// register order, then the xor butterfly of wave_sum (every lane ends with the same bits).  No float atomics anywhere.
//
// Dropout (DroQ, DoubleQDropoutLayerNorm): the pqlk_drop_ln_elu_* entries run the SAME row bodies on u = keep ? z * s : 0 with the
// keep mask regenerated from Philox4x32-10 in registers (the mask law of include/pqlk.h): no mask tensor, no extra pass.  Every row
// kernel below ends in a parameter pack `D... dr` that is either empty (the plain kernel: the signature, the instructions and the
// bits of pqlk_ln_elu_* are what they were, every `if constexpr (DROP)` is compiled out) or one LnDrop (the dropout sibling).
//
// Skip connection (BroNet, DoubleQBroNet): pqlk_ln_res_forward / pqlk_ln_sum_backward run the same row bodies again, the pack now
// one LnRes (forward: no ELU, y = res + LN(z)) or one LnSum (backward: the incoming gradient is dy + dy2, handed on as dsum; the ELU
// factor only where y is given).  The skip and the second addend are loaded a chunk at a time where they are used, not held as a row.
#include <type_traits>

#include "pqlk_common.h"

// Philox4x32-10 (Salmon et al. 2011), ten rounds written out: counter (c0, c1, c2, c3), key (k0, k1) -> one block of four words
__device__ __forceinline__ uint4 ln_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}

// the mask law's host-made constants: key = seed, counter words 2 / 3 = tag, thr = floor(p * 2^32), s = 1 / (1 - p)
struct LnDrop {
  uint32_t k0, k1, t0, t1, thr;
  float s;
};

// the LnDrop of a kernel's trailing pack (an empty pack: the plain kernel, which never reads it)
__device__ __forceinline__ LnDrop ln_drop_of() { return LnDrop{}; }
__device__ __forceinline__ LnDrop ln_drop_of(const LnDrop& d) { return d; }

// the skip connection's extra operands (include/pqlk.h): the forward's res; the backward's second addend and where the sum goes
struct LnRes {
  const float* res;
};
struct LnSum {
  const float* dy2;   // NULL: one addend
  float* dsum;        // NULL: the sum is not handed on
};
__device__ __forceinline__ LnRes ln_res_of(const LnRes& r) { return r; }
__device__ __forceinline__ LnSum ln_sum_of(const LnSum& a) { return a; }

// whether a kernel's trailing pack is one T
template <typename T, typename... D>
inline constexpr bool ln_has = (std::is_same_v<T, D> || ...);

// word (c & 3) of a block (selects on values: an indexed uint4 would be promoted to LDS)
__device__ __forceinline__ uint32_t ln_word(uint4 b, int c) {
  const uint32_t lo = (c & 1) ? b.y : b.x, hi = (c & 1) ? b.w : b.z;
  return (c & 2) ? hi : lo;
}

// keep(r, c) of one element: one Philox block per call (the scalar layout, the strided wide path)
__device__ __forceinline__ bool ln_keep1(const LnDrop& d, uint32_t r, int c) {
  return ln_word(ln_philox(d.k0, d.k1, (uint32_t)c >> 2, r, d.t0, d.t1), c) >= d.thr;
}

__device__ __forceinline__ float ln_elu(float x) { return x > 0.f ? x : expm1f(x); }   // nn.ELU(alpha=1)

#define LN_WAVES 4             // rows in flight per block
#define LN_MAX_REG_COLS 1024   // widest row held in registers

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

// chunk k of a lane alone -> v: register slots [k * V, (k + 1) * V) of ln_load<VPL, VEC>.  A chunk is the whole of a one-chunk row
// map that starts 64 * V columns per chunk further on
template <int VPL, bool VEC>
__device__ __forceinline__ void ln_load_chunk(const float* __restrict__ p, int cols, int lane, int k, float (&v)[LnMap<VPL, VEC>::V]) {
  constexpr int V = LnMap<VPL, VEC>::V;
  ln_load<V, VEC>(p + k * 64 * V, cols - k * 64 * V, lane, v);
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

// bit i = keep of register slot i of row r (slots past cols: 0; they hold 0.f anyway).  VEC: a lane's chunk lies in ONE Philox block
// (V = 4: the whole block; V = 2: its lower or upper half), generated once per chunk; scalar: one block per element.
template <int VPL, bool VEC>
__device__ __forceinline__ unsigned ln_keep_bits(const LnDrop& d, uint32_t r, int cols, int lane) {
  using M = LnMap<VPL, VEC>;
  unsigned km = 0;
  if (VEC) {
#pragma unroll
    for (int k = 0; k < M::NCH; ++k) {
      const int c0 = (k * 64 + lane) * M::V;
      if (c0 < cols) {
        const uint4 b = ln_philox(d.k0, d.k1, (uint32_t)c0 >> 2, r, d.t0, d.t1);
#pragma unroll
        for (int e = 0; e < M::V; ++e) km |= (unsigned)(ln_word(b, c0 + e) >= d.thr) << (k * M::V + e);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = i * 64 + lane;
      if (c < cols) km |= (unsigned)ln_keep1(d, r, c) << i;
    }
  }
  return km;
}

template <int VPL, bool VEC, typename... D>
__global__ __launch_bounds__(256) void k_ln_elu_fwd(const float* __restrict__ z, int64_t ld, int64_t m, int cols,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                    float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, D... dr) {
  using M = LnMap<VPL, VEC>;
  constexpr bool DROP = ln_has<LnDrop, D...>, RES = ln_has<LnRes, D...>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float ga[VPL], be[VPL];
  ln_load<VPL, VEC>(gamma, cols, lane, ga);
  ln_load<VPL, VEC>(beta, cols, lane, be);
  const float n = (float)cols;
  for (int64_t r = (int64_t)blockIdx.x * LN_WAVES + wave; r < m; r += (int64_t)gridDim.x * LN_WAVES) {
    float v[VPL];
    ln_load<VPL, VEC>(z + r * ld, cols, lane, v);
    if constexpr (DROP) {   // u = keep ? z * s : 0
      const LnDrop d = ln_drop_of(dr...);
      const unsigned km = ln_keep_bits<VPL, VEC>(d, (uint32_t)r, cols, lane);
#pragma unroll
      for (int i = 0; i < VPL; ++i) v[i] = (km >> i) & 1u ? v[i] * d.s : 0.f;
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) s += v[i];
    const float mu = wave_sum(s) / n;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const float d = M::col(i, lane) < cols ? v[i] - mu : 0.f;
      v[i] = d;
      q += d * d;
    }
    const float var = wave_sum(q) / n;
    const float rs = 1.0f / sqrtf(var + eps);
    if constexpr (!RES) {
#pragma unroll
      for (int i = 0; i < VPL; ++i) v[i] = ln_elu(v[i] * rs * ga[i] + be[i]);
    } else {   // no activation; y = res + t, the skip loaded chunk by chunk
      const float* rr = ln_res_of(dr...).res + r * ld;
#pragma unroll
      for (int k = 0; k < M::NCH; ++k) {
        float sk[M::V];
        ln_load_chunk<VPL, VEC>(rr, cols, lane, k, sk);
#pragma unroll
        for (int e = 0; e < M::V; ++e) v[k * M::V + e] = sk[e] + (v[k * M::V + e] * rs * ga[k * M::V + e] + be[k * M::V + e]);
      }
    }
    ln_store<VPL, VEC>(y + r * ld, cols, lane, v);
    if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
  }
}

// element (r, c) of u (one LnDrop) or of z (none) from the loaded z: the strided paths re-read the row and, with it, re-form the
// mask, one block per element
__device__ __forceinline__ float ln_u(float zv, uint32_t, int) { return zv; }
__device__ __forceinline__ float ln_u(float zv, uint32_t, int, const LnRes&) { return zv; }
__device__ __forceinline__ float ln_u(float zv, uint32_t, int, const LnSum&) { return zv; }
__device__ __forceinline__ float ln_u(float zv, uint32_t r, int c, const LnDrop& d) { return ln_keep1(d, r, c) ? zv * d.s : 0.f; }

// rows wider than LN_MAX_REG_COLS: the same law with the row re-read from memory (sum, squared deviations, output)
template <typename... D>
__global__ __launch_bounds__(256) void k_ln_elu_fwd_wide(const float* __restrict__ z, int64_t ld, int64_t m, int cols,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                         float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd,
                                                         D... dr) {
  constexpr bool RES = ln_has<LnRes, D...>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float n = (float)cols;
  for (int64_t r = (int64_t)blockIdx.x * LN_WAVES + wave; r < m; r += (int64_t)gridDim.x * LN_WAVES) {
    const float* zr = z + r * ld;
    float* yr = y + r * ld;
    float s = 0.f;
    for (int c = lane; c < cols; c += 64) s += ln_u(zr[c], (uint32_t)r, c, dr...);
    const float mu = wave_sum(s) / n;
    float q = 0.f;
    for (int c = lane; c < cols; c += 64) { const float d = ln_u(zr[c], (uint32_t)r, c, dr...) - mu; q += d * d; }
    const float var = wave_sum(q) / n;
    const float rs = 1.0f / sqrtf(var + eps);
    if constexpr (!RES) {
      for (int c = lane; c < cols; c += 64) yr[c] = ln_elu((ln_u(zr[c], (uint32_t)r, c, dr...) - mu) * rs * gamma[c] + beta[c]);
    } else {
      const float* rr = ln_res_of(dr...).res + r * ld;
      for (int c = lane; c < cols; c += 64) yr[c] = rr[c] + ((zr[c] - mu) * rs * gamma[c] + beta[c]);
    }
    if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
  }
}

// Backward, one wave per row.  PARAMS: each wave also accumulates its rows' g and g * xhat per column in registers; the block
// folds its waves through LDS in wave order and writes one partial row: part[(blockIdx.x * 2 + {0: dbeta, 1: dgamma}) * cols + c].
// DROP: xhat is re-formed from u = keep ? z * s : 0 (the mask regenerated, never stored), the law gives du, dz = keep ? du * s : 0.
template <int VPL, bool VEC, bool PARAMS, typename... D>
__global__ __launch_bounds__(256) void k_ln_elu_bwd(const float* dy, const float* __restrict__ y, const float* __restrict__ z,
                                                    int64_t ld, int64_t m, int cols, const float* __restrict__ mean,
                                                    const float* __restrict__ rstd, const float* __restrict__ gamma, float* dz,
                                                    float* __restrict__ part, D... dr) {
  using M = LnMap<VPL, VEC>;
  constexpr bool DROP = ln_has<LnDrop, D...>, SUM = ln_has<LnSum, D...>;
  __shared__ float sh[PARAMS ? 2 * LN_WAVES * VPL * 64 : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float ga[VPL], accb[VPL], accg[VPL];
  ln_load<VPL, VEC>(gamma, cols, lane, ga);
#pragma unroll
  for (int i = 0; i < VPL; ++i) accb[i] = accg[i] = 0.f;
  const float n = (float)cols;
  for (int64_t r = (int64_t)blockIdx.x * LN_WAVES + wave; r < m; r += (int64_t)gridDim.x * LN_WAVES) {
    const float mu = mean[r], rs = rstd[r];
    float h[VPL], xh[VPL], yv[VPL];
    ln_load<VPL, VEC>(dy + r * ld, cols, lane, h);
    [[maybe_unused]] bool act = true;   // whether an ELU stands behind the norm (SUM: only where y is given)
    if constexpr (SUM) {   // h = g0 = dy + dy2, the second addend chunk by chunk; handed on as dsum before anything else is written
      const LnSum a = ln_sum_of(dr...);
      act = y != nullptr;
      if (a.dy2) {
#pragma unroll
        for (int k = 0; k < M::NCH; ++k) {
          float t[M::V];
          ln_load_chunk<VPL, VEC>(a.dy2 + r * ld, cols, lane, k, t);
#pragma unroll
          for (int e = 0; e < M::V; ++e) h[k * M::V + e] = h[k * M::V + e] + t[e];
        }
      }
      if (a.dsum) ln_store<VPL, VEC>(a.dsum + r * ld, cols, lane, h);
      if (act) ln_load<VPL, VEC>(y + r * ld, cols, lane, yv);
    } else {
      ln_load<VPL, VEC>(y + r * ld, cols, lane, yv);
    }
    ln_load<VPL, VEC>(z + r * ld, cols, lane, xh);
    [[maybe_unused]] unsigned km = 0;
    if constexpr (DROP) {
      const LnDrop d = ln_drop_of(dr...);
      km = ln_keep_bits<VPL, VEC>(d, (uint32_t)r, cols, lane);
#pragma unroll
      for (int i = 0; i < VPL; ++i) xh[i] = (km >> i) & 1u ? xh[i] * d.s : 0.f;
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const bool in = M::col(i, lane) < cols;
      float g;
      if constexpr (SUM) g = in ? (act ? h[i] * (yv[i] > 0.f ? 1.f : yv[i] + 1.f) : h[i]) : 0.f;
      else g = in ? h[i] * (yv[i] > 0.f ? 1.f : yv[i] + 1.f) : 0.f;
      const float x = in ? (xh[i] - mu) * rs : 0.f;
      const float hh = g * ga[i];
      if (PARAMS) { accb[i] += g; accg[i] += g * x; }
      s1 += hh;
      s2 += hh * x;
      h[i] = hh; xh[i] = x;
    }
    const float c1 = wave_sum(s1) / n, c2 = wave_sum(s2) / n;
#pragma unroll
    for (int i = 0; i < VPL; ++i) h[i] = rs * (h[i] - c1 - xh[i] * c2);
    if constexpr (DROP) {
      const float sc = ln_drop_of(dr...).s;
#pragma unroll
      for (int i = 0; i < VPL; ++i) h[i] = (km >> i) & 1u ? h[i] * sc : 0.f;
    }
    ln_store<VPL, VEC>(dz + r * ld, cols, lane, h);
  }
  if (PARAMS) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      sh[(0 * LN_WAVES + wave) * (VPL * 64) + i * 64 + lane] = accb[i];
      sh[(1 * LN_WAVES + wave) * (VPL * 64) + i * 64 + lane] = accg[i];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 2 * VPL * 64; idx += 256) {
      const int which = idx / (VPL * 64), slot = idx % (VPL * 64);
      const int c = M::col(slot / 64, slot % 64);
      if (c < cols) {
        const float* s = sh + which * LN_WAVES * (VPL * 64) + slot;
        float t = s[0];
#pragma unroll
        for (int w = 1; w < LN_WAVES; ++w) t += s[w * (VPL * 64)];
        part[((int64_t)blockIdx.x * 2 + which) * cols + c] = t;
      }
    }
  }
}


// the summed-gradient backward's g0 = dy (+ dy2) and g = g0 (* ELU' from y, where y is given) of element i = r * ld + c
__device__ __forceinline__ float ln_elu_slope(float y) { return y > 0.f ? 1.f : y + 1.f; }
__device__ __forceinline__ float ln_g0(const float* dy, int64_t i, const LnSum& a) { return a.dy2 ? dy[i] + a.dy2[i] : dy[i]; }
__device__ __forceinline__ float ln_g(const float* dy, const float* y, int64_t i, const LnSum& a) {
  const float g0 = ln_g0(dy, i, a);
  return y ? g0 * ln_elu_slope(y[i]) : g0;
}

// wide rows: dz with the row re-read (dy fully read before dz, which may alias it, is written: the sums need all of it first,
// and every element is then read and written by the same lane)
template <typename... D>
__global__ __launch_bounds__(256) void k_ln_elu_bwd_wide(const float* dy, const float* __restrict__ y, const float* __restrict__ z,
                                                         int64_t ld, int64_t m, int cols, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ gamma, float* dz,
                                                         D... dr) {
  constexpr bool DROP = ln_has<LnDrop, D...>, SUM = ln_has<LnSum, D...>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float n = (float)cols;
  for (int64_t r = (int64_t)blockIdx.x * LN_WAVES + wave; r < m; r += (int64_t)gridDim.x * LN_WAVES) {
    const float mu = mean[r], rs = rstd[r];
    const float *dyr = dy + r * ld, *yr = y + r * ld, *zr = z + r * ld;
    float* o = dz + r * ld;
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < cols; c += 64) {
      float hh;
      if constexpr (SUM) {
        hh = ln_g(dy, y, r * ld + c, dr...) * gamma[c];
      } else {
        const float yy = yr[c];
        hh = dyr[c] * (yy > 0.f ? 1.f : yy + 1.f) * gamma[c];
      }
      s1 += hh;
      s2 += hh * ((ln_u(zr[c], (uint32_t)r, c, dr...) - mu) * rs);
    }
    const float c1 = wave_sum(s1) / n, c2 = wave_sum(s2) / n;
    for (int c = lane; c < cols; c += 64) {
      float hh;
      if constexpr (SUM) {   // dy and dy2 at c are read here, by the lane that then writes dsum and dz at c
        const LnSum a = ln_sum_of(dr...);
        const float g0 = ln_g0(dy, r * ld + c, a);
        hh = (y ? g0 * ln_elu_slope(yr[c]) : g0) * gamma[c];
        if (a.dsum) a.dsum[r * ld + c] = g0;
      } else {
        const float yy = yr[c];
        hh = dyr[c] * (yy > 0.f ? 1.f : yy + 1.f) * gamma[c];
      }
      if constexpr (!DROP) {
        o[c] = rs * (hh - c1 - ((zr[c] - mu) * rs) * c2);
      } else {
        const LnDrop d = ln_drop_of(dr...);
        const bool keep = ln_keep1(d, (uint32_t)r, c);
        const float u = keep ? zr[c] * d.s : 0.f;
        const float du = rs * (hh - c1 - ((u - mu) * rs) * c2);
        o[c] = keep ? du * d.s : 0.f;
      }
    }
  }
}

// wide rows: the column sums of g and g * xhat over a chunk of rows, down the columns like k_bn_bwd_sums -> the same partial layout
template <typename... D>
__global__ __launch_bounds__(256) void k_ln_bwd_sums_wide(const float* __restrict__ dy, const float* __restrict__ y,
                                                          const float* __restrict__ z, int64_t ld, int64_t m, int cols,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          float* __restrict__ part, D... dr) {
  __shared__ float sh[2][4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  float s1 = 0.f, s2 = 0.f;
  if (c < cols) {
    const int64_t rows_per = (m + gridDim.y - 1) / gridDim.y;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per, r1 = min(m, r0 + rows_per);
    for (int64_t r = r0 + rl; r < r1; r += 4) {
      float g;
      if constexpr (ln_has<LnSum, D...>) {
        g = ln_g(dy, y, r * ld + c, dr...);
      } else {
        const float yy = y[r * ld + c];
        g = dy[r * ld + c] * (yy > 0.f ? 1.f : yy + 1.f);
      }
      s1 += g;
      s2 += g * ((ln_u(z[r * ld + c], (uint32_t)r, c, dr...) - mean[r]) * rstd[r]);
    }
  }
  sh[0][rl][cl] = s1; sh[1][rl][cl] = s2;
  __syncthreads();
  if (rl == 0 && c < cols) {
    part[((int64_t)blockIdx.y * 2 + 0) * cols + c] = (sh[0][0][cl] + sh[0][1][cl]) + (sh[0][2][cl] + sh[0][3][cl]);
    part[((int64_t)blockIdx.y * 2 + 1) * cols + c] = (sh[1][0][cl] + sh[1][1][cl]) + (sh[1][2][cl] + sh[1][3][cl]);
  }
}


// fold the chunk partials in index order: 16 columns x 16 groups of consecutive chunks per block, the groups then in group order.
// blockIdx.y: 0 -> dbeta, 1 -> dgamma
#define LN_FOLD_GROUPS 16
__global__ __launch_bounds__(256) void k_ln_fold(const float* __restrict__ part, int chunks, int cols, float* __restrict__ dgamma,
                                                 float* __restrict__ dbeta) {
  __shared__ float sh[LN_FOLD_GROUPS][16];
  const int cl = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl, which = blockIdx.y;
  float* out = which ? dgamma : dbeta;
  if (!out) return;   // (uniform over the block)
  const int per = (chunks + LN_FOLD_GROUPS - 1) / LN_FOLD_GROUPS;
  const int k0 = g * per, k1 = min(chunks, k0 + per);
  float s = 0.f;
  if (c < cols)
    for (int k = k0; k < k1; ++k) s += part[((int64_t)k * 2 + which) * cols + c];
  sh[g][cl] = s;
  __syncthreads();
  if (g == 0 && c < cols) {
    float t = sh[0][cl];
#pragma unroll
    for (int j = 1; j < LN_FOLD_GROUPS; ++j) t += sh[j][cl];
    out[c] = t;
  }
}

static inline unsigned ln_blocks(int64_t m, int64_t cap) {
  const int64_t nb = (m + LN_WAVES - 1) / LN_WAVES;
  return (unsigned)(nb < cap ? nb : cap);
}

// whether the pack's own pointers allow 16-byte accesses
static inline bool ln_pack_aligned16() { return true; }
static inline bool ln_pack_aligned16(const LnDrop&) { return true; }
static inline bool ln_pack_aligned16(const LnRes& r) { return pqlk_aligned16(r.res); }
static inline bool ln_pack_aligned16(const LnSum& a) { return pqlk_aligned16(a.dy2) && pqlk_aligned16(a.dsum); }   // (NULL counts as aligned)

// `D... dr` below: nothing (the plain kernels), one LnDrop (their dropout siblings), or one LnRes (forward) / LnSum (backward) of the
// skip connection, handed on behind the kernels' arguments
template <int VPL, typename... D>
static void ln_launch_fwd(bool vec, unsigned grid, hipStream_t s, const float* z, int64_t ld, int64_t m, int cols, const float* gamma,
                          const float* beta, float eps, float* y, float* mean, float* rstd, D... dr) {
  if (vec)
    k_ln_elu_fwd<VPL, true><<<dim3(grid), dim3(256), 0, s>>>(z, ld, m, cols, gamma, beta, eps, y, mean, rstd, dr...);
  else
    k_ln_elu_fwd<VPL, false><<<dim3(grid), dim3(256), 0, s>>>(z, ld, m, cols, gamma, beta, eps, y, mean, rstd, dr...);
}

template <int VPL, typename... D>
static void ln_launch_bwd(bool vec, bool params, unsigned grid, hipStream_t s, const float* dy, const float* y, const float* z, int64_t ld,
                          int64_t m, int cols, const float* mean, const float* rstd, const float* gamma, float* dz, float* part, D... dr) {
  if (vec && params)
    k_ln_elu_bwd<VPL, true, true><<<dim3(grid), dim3(256), 0, s>>>(dy, y, z, ld, m, cols, mean, rstd, gamma, dz, part, dr...);
  else if (vec)
    k_ln_elu_bwd<VPL, true, false><<<dim3(grid), dim3(256), 0, s>>>(dy, y, z, ld, m, cols, mean, rstd, gamma, dz, part, dr...);
  else if (params)
    k_ln_elu_bwd<VPL, false, true><<<dim3(grid), dim3(256), 0, s>>>(dy, y, z, ld, m, cols, mean, rstd, gamma, dz, part, dr...);
  else
    k_ln_elu_bwd<VPL, false, false><<<dim3(grid), dim3(256), 0, s>>>(dy, y, z, ld, m, cols, mean, rstd, gamma, dz, part, dr...);
}

extern "C" int64_t pqlk_ln_scratch_floats(int32_t cols) { return cols > 0 ? (int64_t)2 * PQLK_LN_CHUNKS * cols : 0; }

// the one forward / backward dispatch of the plain and the dropout entries
template <typename... D>
static int ln_forward(const float* z, int64_t ld, int64_t m, int32_t cols, const float* gamma, const float* beta, float eps, float* y,
                      float* mean, float* rstd, pqlk_stream_t stream, D... dr) {
  PQLK_REQUIRE(z && gamma && beta && y && mean && rstd, PQLK_E_NULL);
  PQLK_REQUIRE(m > 0 && cols > 0 && ld >= cols, PQLK_E_SHAPE);
  const unsigned grid = ln_blocks(m, PQLK_LN_ROW_BLOCKS);
  const bool vec = pqlk_aligned16(z) && pqlk_aligned16(y) && pqlk_aligned16(gamma) && pqlk_aligned16(beta) && ld % 4 == 0 &&
                   ln_pack_aligned16(dr...);
  hipStream_t s = pqlk_s(stream);
  if (cols <= 128) ln_launch_fwd<2>(vec, grid, s, z, ld, m, (int)cols, gamma, beta, eps, y, mean, rstd, dr...);
  else if (cols <= 256) ln_launch_fwd<4>(vec, grid, s, z, ld, m, (int)cols, gamma, beta, eps, y, mean, rstd, dr...);
  else if (cols <= 512) ln_launch_fwd<8>(vec, grid, s, z, ld, m, (int)cols, gamma, beta, eps, y, mean, rstd, dr...);
  else if (cols <= LN_MAX_REG_COLS) ln_launch_fwd<16>(vec, grid, s, z, ld, m, (int)cols, gamma, beta, eps, y, mean, rstd, dr...);
  else k_ln_elu_fwd_wide<<<dim3(grid), dim3(256), 0, s>>>(z, ld, m, (int)cols, gamma, beta, eps, y, mean, rstd, dr...);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

template <typename... D>
static int ln_backward(const float* dy, const float* y, const float* z, int64_t ld, int64_t m, int32_t cols, const float* mean,
                       const float* rstd, const float* gamma, float* dz, float* dgamma, float* dbeta, float* scratch,
                       pqlk_stream_t stream, D... dr) {
  const bool params = dgamma || dbeta;
  PQLK_REQUIRE(dy && (y || ln_has<LnSum, D...>) && z && mean && rstd && gamma && dz && (scratch || !params), PQLK_E_NULL);
  PQLK_REQUIRE(m > 0 && cols > 0 && ld >= cols, PQLK_E_SHAPE);
  hipStream_t s = pqlk_s(stream);
  const int c = (int)cols;
  int chunks;
  if (cols <= LN_MAX_REG_COLS) {
    const unsigned grid = ln_blocks(m, params ? PQLK_LN_CHUNKS : PQLK_LN_ROW_BLOCKS);
    const bool vec = pqlk_aligned16(dy) && pqlk_aligned16(y) && pqlk_aligned16(z) && pqlk_aligned16(gamma) && pqlk_aligned16(dz) && ld % 4 == 0 &&
                     ln_pack_aligned16(dr...);
    if (cols <= 128) ln_launch_bwd<2>(vec, params, grid, s, dy, y, z, ld, m, c, mean, rstd, gamma, dz, scratch, dr...);
    else if (cols <= 256) ln_launch_bwd<4>(vec, params, grid, s, dy, y, z, ld, m, c, mean, rstd, gamma, dz, scratch, dr...);
    else if (cols <= 512) ln_launch_bwd<8>(vec, params, grid, s, dy, y, z, ld, m, c, mean, rstd, gamma, dz, scratch, dr...);
    else ln_launch_bwd<16>(vec, params, grid, s, dy, y, z, ld, m, c, mean, rstd, gamma, dz, scratch, dr...);
    PQLK_LAUNCH_CHECK();
    chunks = (int)grid;
  } else {
    chunks = (int)(m < PQLK_LN_CHUNKS ? m : PQLK_LN_CHUNKS);
    if (params) {   // before dz, which may alias dy, is written
      k_ln_bwd_sums_wide<<<dim3((unsigned)((cols + 63) / 64), (unsigned)chunks), dim3(256), 0, s>>>(dy, y, z, ld, m, c, mean, rstd, scratch,
                                                                                                    dr...);
      PQLK_LAUNCH_CHECK();
    }
    k_ln_elu_bwd_wide<<<dim3(ln_blocks(m, PQLK_LN_ROW_BLOCKS)), dim3(256), 0, s>>>(dy, y, z, ld, m, c, mean, rstd, gamma, dz, dr...);
    PQLK_LAUNCH_CHECK();
  }
  if (params) {
    hipLaunchKernelGGL(k_ln_fold, dim3((unsigned)((cols + 15) / 16), 2), dim3(256), 0, s, scratch, chunks, c, dgamma, dbeta);
    PQLK_LAUNCH_CHECK();
  }
  return PQLK_OK;
}

extern "C" int pqlk_ln_elu_forward(const float* z, int64_t ld, int64_t m, int32_t cols, const float* gamma, const float* beta, float eps,
                                   float* y, float* mean, float* rstd, pqlk_stream_t stream) {
  return ln_forward(z, ld, m, cols, gamma, beta, eps, y, mean, rstd, stream);
}

extern "C" int pqlk_ln_elu_backward(const float* dy, const float* y, const float* z, int64_t ld, int64_t m, int32_t cols, const float* mean,
                                    const float* rstd, const float* gamma, float* dz, float* dgamma, float* dbeta, float* scratch,
                                    pqlk_stream_t stream) {
  return ln_backward(dy, y, z, ld, m, cols, mean, rstd, gamma, dz, dgamma, dbeta, scratch, stream);
}

// ---- skip-connection entries (the residual LayerNorm critic)
extern "C" int pqlk_ln_res_forward(const float* z, int64_t ld, int64_t m, int32_t cols, const float* gamma, const float* beta, float eps,
                                   const float* res, float* y, float* mean, float* rstd, pqlk_stream_t stream) {
  PQLK_REQUIRE(res, PQLK_E_NULL);
  return ln_forward(z, ld, m, cols, gamma, beta, eps, y, mean, rstd, stream, LnRes{res});
}

extern "C" int pqlk_ln_sum_backward(const float* dy, const float* dy2, const float* y, const float* z, int64_t ld, int64_t m, int32_t cols,
                                    const float* mean, const float* rstd, const float* gamma, float* dsum, float* dz, float* dgamma,
                                    float* dbeta, float* scratch, pqlk_stream_t stream) {
  return ln_backward(dy, y, z, ld, m, cols, mean, rstd, gamma, dz, dgamma, dbeta, scratch, stream, LnSum{dy2, dsum});
}

// ---- dropout entries: the mask law's constants are made here, on the host (include/pqlk.h)
static bool ln_drop_make(float p, uint64_t seed, uint64_t tag, int64_t m, LnDrop* d) {
  if (!(p >= 0.f && p < 1.f) || m > (int64_t)1 << 32) return false;   // (a NaN p fails the first test)
  d->k0 = (uint32_t)seed; d->k1 = (uint32_t)(seed >> 32);
  d->t0 = (uint32_t)tag; d->t1 = (uint32_t)(tag >> 32);
  d->thr = (uint32_t)floor((double)p * 4294967296.0);
  const float q = 1.0f - p;
  d->s = 1.0f / q;
  return true;
}

// keep(r, c) as bytes: one thread per Philox block = four consecutive columns of a row
__global__ __launch_bounds__(256) void k_drop_mask(LnDrop dr, int64_t m, int cols, uint8_t* __restrict__ keep, int64_t ld_keep) {
  const int64_t per_row = (cols + 3) / 4, total = m * per_row;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / per_row;
    const int c0 = (int)(i % per_row) * 4;
    const uint4 b = ln_philox(dr.k0, dr.k1, (uint32_t)c0 >> 2, (uint32_t)r, dr.t0, dr.t1);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c0 + e < cols) keep[r * ld_keep + c0 + e] = ln_word(b, e) >= dr.thr;
  }
}

extern "C" int pqlk_drop_mask(uint64_t seed, uint64_t tag, float p, int64_t m, int32_t cols, uint8_t* keep, int64_t ld_keep,
                              pqlk_stream_t stream) {
  PQLK_REQUIRE(keep, PQLK_E_NULL);
  LnDrop d;
  PQLK_REQUIRE(m > 0 && cols > 0 && ld_keep >= cols && ln_drop_make(p, seed, tag, m, &d), PQLK_E_SHAPE);
  const int64_t nb = (m * (((int64_t)cols + 3) / 4) + 255) / 256;
  hipLaunchKernelGGL(k_drop_mask, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(256), 0, pqlk_s(stream), d, m, (int)cols, keep, ld_keep);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

extern "C" int pqlk_drop_ln_elu_forward(const float* z, int64_t ld, int64_t m, int32_t cols, const float* gamma, const float* beta,
                                        float eps, float p, uint64_t seed, uint64_t tag, float* y, float* mean, float* rstd,
                                        pqlk_stream_t stream) {
  LnDrop d;
  PQLK_REQUIRE(ln_drop_make(p, seed, tag, m, &d), PQLK_E_SHAPE);
  return ln_forward(z, ld, m, cols, gamma, beta, eps, y, mean, rstd, stream, d);
}

extern "C" int pqlk_drop_ln_elu_backward(const float* dy, const float* y, const float* z, int64_t ld, int64_t m, int32_t cols,
                                         const float* mean, const float* rstd, const float* gamma, float p, uint64_t seed, uint64_t tag,
                                         float* dz, float* dgamma, float* dbeta, float* scratch, pqlk_stream_t stream) {
  LnDrop d;
  PQLK_REQUIRE(ln_drop_make(p, seed, tag, m, &d), PQLK_E_SHAPE);
  return ln_backward(dy, y, z, ld, m, cols, mean, rstd, gamma, dz, dgamma, dbeta, scratch, stream, d);
}

