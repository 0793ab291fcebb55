// The mask law of include/pqlk.h ("The mask law") as device code, shared by the dropout row kernels of ln.hip and the dropout forms
// of the whole-stack forwards (fwd_ln.hip, fwd_ln_bf16.hip): Philox4x32-10, the host-made constants of one mask, and keep(r, c) in
// the shapes the kernels hold a row in.  A kernel that ends in a parameter pack `D... dr` reads its LnDrop through ln_drop_of(dr...);
// with an empty pack nothing of this file reaches its instructions.
#pragma once
#include <type_traits>

#include "lnrow.h"

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

// u = keep ? z * s : 0 of the four consecutive, 4-aligned columns c0 .. c0 + 3 of row r: the whole of one Philox block
__device__ __forceinline__ float4 ln_drop4(const LnDrop& d, uint32_t r, int c0, float4 z) {
  const uint4 b = ln_philox(d.k0, d.k1, (uint32_t)c0 >> 2, r, d.t0, d.t1);
  return make_float4(b.x >= d.thr ? z.x * d.s : 0.f, b.y >= d.thr ? z.y * d.s : 0.f, b.z >= d.thr ? z.z * d.s : 0.f,
                     b.w >= d.thr ? z.w * d.s : 0.f);
}

// ---- host side: the mask law's constants of (p, seed, tag) for a matrix of m rows; false: p < 0, p >= 1, a NaN p (it fails the
// first test) or m > 2^32 (r is one counter word)
static inline bool ln_drop_make(float p, uint64_t seed, uint64_t tag, int64_t m, LnDrop* d) {
  if (!(p >= 0.f && p < 1.f) || m > (int64_t)1 << 32) return false;
  d->k0 = (uint32_t)seed; d->k1 = (uint32_t)(seed >> 32);
  d->t0 = (uint32_t)tag; d->t1 = (uint32_t)(tag >> 32);
  d->thr = (uint32_t)floor((double)p * 4294967296.0);
  const float q = 1.0f - p;
  d->s = 1.0f / q;
  return true;
}

// the whole-stack forwards' mask constants: one tag_base for the launch, tag of (net, layer) = tag_base | (net << 4) | layer, so the
// low 5 bits of tag_base must be clear and the stack may have at most 2 nets and 16 hidden layers
static inline bool ln_drop_make_stack(float p, uint64_t seed, uint64_t tag_base, int64_t m, int n_nets, int hidden, LnDrop* d) {
  return (tag_base & 31u) == 0 && n_nets <= 2 && hidden <= 16 && ln_drop_make(p, seed, tag_base, m, d);
}
__device__ __forceinline__ LnDrop ln_drop_at(LnDrop d, int net, int layer) {
  d.t0 |= (uint32_t)((net << 4) | layer);
  return d;
}
