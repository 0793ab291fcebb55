// Loss kernels: TD target + twin MSE, C51 softmax/projection/BCE, HL-Gauss cross-entropy, DPG actor loss, quantile Huber losses.
// Reference: pql/algo/pql_v_learner.py:80-108, pql/utils/distl_util.py:4-20, pql/algo/pql_p_learner.py:55-57,
// pql/models/mlp.py:256-263.  Each kernel writes the gradient w.r.t. the critic's last-layer output
// (padded (2,B,ld) layout expected by pqlk_mlp_backward) and deterministic per-block loss partials.
#include "pqlk_common.h"

#define LOSS_MAX_BLOCKS 1024

// sum `n` partials in fixed order with one block -> out[0] = scale * sum  (strided per-thread sums -> xor-shuffle tree per wave
// -> the four waves in order: the order in which k_adamw folds the same partials when the loss rides in its launch)
__global__ __launch_bounds__(256) void k_sum_partials(const float* __restrict__ part, int n, float scale,
                                                      float* __restrict__ out, const int32_t* __restrict__ slot_dev,
                                                      int ring_len) {
  __shared__ float shw[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) shw[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[slot_dev ? (slot_dev[0] % ring_len) : 0] = ((shw[0] + shw[1]) + (shw[2] + shw[3])) * scale;
}

__device__ __forceinline__ float block_sum_256(float v) {
  __shared__ float shw[4];
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) shw[threadIdx.x >> 6] = v;
  __syncthreads();
  return (shw[0] + shw[1]) + (shw[2] + shw[3]);
}

// blocks of a loss kernel = per-block partials it leaves in `scratch` (k = 1: scalar heads, one row per thread; k > 1: one wave per row)
static int loss_blocks(int64_t b, int32_t k) {
  const int64_t blocks = k <= 1 ? (b + 255) / 256 : (b + 3) / 4;
  return (int)(blocks < LOSS_MAX_BLOCKS ? blocks : LOSS_MAX_BLOCKS);
}
extern "C" int32_t pqlk_loss_parts(int64_t b, int32_t k) { return loss_blocks(b, k); }

// tail of every loss entry point: scale * (sum of the partials) -> the loss ring; without a ring the partials stay in
// scratch[0, pqlk_loss_parts(b, k)) and pqlk_adamw_polyak_fused folds them
static int fold_partials(const float* scratch, int blocks, float scale, float* loss_out, const int32_t* slot_dev, int32_t ring_len,
                         pqlk_stream_t stream) {
  if (!loss_out) return PQLK_OK;
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, pqlk_s(stream), scratch, blocks, scale, loss_out, slot_dev, (int)ring_len);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

// ------------------------------------------------------------------------------------------------
// PER: the importance weight wh = w[i] / wmax[0] of prioritized replay on each sample (and |TD| out, the new priority).  The plain
// instance never touches w, wmax or abs_td; with every w and wmax 1.0 the multiplications by wh change no bit.
template <bool PER>
__global__ __launch_bounds__(256) void k_td_mse(const float* __restrict__ q, const float* __restrict__ qt, int64_t ld,
                                                const float* __restrict__ rew, const float* __restrict__ done,
                                                float gamma_n, int64_t b, float* __restrict__ dy, float* __restrict__ part,
                                                const float* __restrict__ w, const float* __restrict__ wmax,
                                                float* __restrict__ abs_td) {
  const float two_over_b = 2.0f / (float)b;
  float wm = 1.f;
  if constexpr (PER) wm = wmax[0];
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < b; i += (int64_t)gridDim.x * 256) {
    const float t1 = qt[i * ld], t2 = qt[(b + i) * ld];
    const float tq = fminf(t1, t2);
    const float y = rew[i] + ((1.f - done[i]) * gamma_n) * tq;  // r + (1-d)*gamma^n*minQ'  (:105)
    const float d1 = q[i * ld] - y, d2 = q[(b + i) * ld] - y;
    float sq = d1 * d1 + d2 * d2, g = two_over_b;
    if constexpr (PER) {
      const float wh = w[i] / wm;
      sq = wh * sq;
      g = two_over_b * wh;
    }
    acc += sq;
    dy[i * ld] = g * d1;
    dy[(b + i) * ld] = g * d2;
    if constexpr (PER) abs_td[i] = fmaxf(fabsf(d1), fabsf(d2));
  }
  const float s = block_sum_256(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

template <bool PER>
static int td_mse_impl(const float* q, const float* qt, int64_t ld, const float* rew, const float* done, float gamma_n, int64_t b,
                       float* dy, float* loss_out, const int32_t* slot_dev, int32_t ring_len, float* scratch, const float* w,
                       const float* wmax, float* abs_td_out, pqlk_stream_t stream) {
  PQLK_REQUIRE(q && qt && rew && done && dy && scratch, PQLK_E_NULL);
  PQLK_REQUIRE(!PER || (w && wmax && abs_td_out), PQLK_E_NULL);
  PQLK_REQUIRE(!slot_dev || ring_len > 0, PQLK_E_SHAPE);
  PQLK_REQUIRE(b > 0, PQLK_E_SHAPE);
  PQLK_REQUIRE(ld >= 32 && ld % 32 == 0, PQLK_E_ALIGN);
  const int blocks = loss_blocks(b, 1);
  hipLaunchKernelGGL(k_td_mse<PER>, dim3(blocks), dim3(256), 0, pqlk_s(stream), q, qt, ld, rew, done, gamma_n, b, dy, scratch, w, wmax,
                     abs_td_out);
  PQLK_LAUNCH_CHECK();
  return fold_partials(scratch, blocks, 1.0f / (float)b, loss_out, slot_dev, ring_len, stream);
}

extern "C" int pqlk_td_mse_loss(const float* q, const float* qt, int64_t ld, const float* rew, const float* done,
                                float gamma_n, int64_t b, float* dy, float* loss_out, const int32_t* slot_dev,
                                int32_t ring_len, float* scratch, pqlk_stream_t stream) {
  return td_mse_impl<false>(q, qt, ld, rew, done, gamma_n, b, dy, loss_out, slot_dev, ring_len, scratch, nullptr, nullptr, nullptr,
                            stream);
}

extern "C" int pqlk_td_mse_loss_per(const float* q, const float* qt, int64_t ld, const float* rew, const float* done,
                                    float gamma_n, int64_t b, float* dy, float* loss_out, const int32_t* slot_dev,
                                    int32_t ring_len, float* scratch, const float* w, const float* wmax, float* abs_td_out,
                                    pqlk_stream_t stream) {
  return td_mse_impl<true>(q, qt, ld, rew, done, gamma_n, b, dy, loss_out, slot_dev, ring_len, scratch, w, wmax, abs_td_out, stream);
}

// ------------------------------------------------------------------------------------------------
// C51 with 2 ... PQLK_C51_MAX_ATOMS atoms.  One wave per batch row and four rows per block; a lane holds atoms lane + 64 j,
// j < NJ = ceil(K / 64): coalesced row reads (NJ = 1, K <= 64: lane k <-> atom k).  Softmax, E[z] and the softmax backward's dot
// product reduce over the lane's own atoms first, then with wave_max / wave_sum.  The lane's own reduction starts from -inf / 0.f
// at every NJ: against starting from atom j = 0 that can move the sign of a zero sum, and only of one whose 64 lanes all hold -0
// (DESIGN 10 f16 shows that no input with a finite non-zero support gets there).
template <int NJ>
__device__ __forceinline__ void load_row(const float* __restrict__ row, int K, int lane, float (&x)[NJ]) {
#pragma unroll
  for (int j = 0; j < NJ; ++j) x[j] = lane + 64 * j < K ? row[lane + 64 * j] : 0.f;
}

// one row of dy: columns [0, K) <- v, pad columns [K, ld) <- 0
template <int NJ>
__device__ __forceinline__ void store_dy_row(float* __restrict__ row, int64_t ld, int K, int lane, const float (&v)[NJ]) {
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < ld) row[c] = c < K ? v[j] : 0.f;
  }
  for (int64_t c = 64 * NJ + lane; c < ld; c += 64) row[c] = 0.f;
}

// softmax over the K values a wave holds as x[j] <-> atom lane + 64 j (x[j] is ignored where the atom is >= K)
template <int NJ>
__device__ __forceinline__ void wave_softmax(float (&x)[NJ], int K, int lane) {
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (lane + 64 * j < K) m = fmaxf(m, x[j]);
  m = wave_max(m);
#pragma unroll
  for (int j = 0; j < NJ; ++j) x[j] = lane + 64 * j < K ? expf(x[j] - m) : 0.f;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) s += x[j];
  s = wave_sum(s);
#pragma unroll
  for (int j = 0; j < NJ; ++j) x[j] = x[j] / s;
}

// sum over a row of a[j] * b[j]
template <int NJ>
__device__ __forceinline__ float wave_dot(const float (&a)[NJ], const float (&b)[NJ]) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) s += a[j] * b[j];
  return wave_sum(s);
}

// Projection.  Atom a of a row with pmf value p deposits w_lo into bin lo and w_up into bin up:
struct C51Deposit {
  int lo, up;
  float w_lo, w_up;
};
__device__ __forceinline__ C51Deposit c51_deposit(float p, float zk, float r, float d, float gamma_n, float v_min, float v_max,
                                                  float dz, int K) {
  float tz = r + ((1.f - d) * gamma_n) * zk;
  tz = fminf(fmaxf(tz, v_min), v_max);
  const float bpos = (tz - v_min) / dz;
  int lo = (int)floorf(bpos), up = (int)ceilf(bpos);
  if (up > 0 && lo == up) lo -= 1;
  if (lo < K - 1 && lo == up) up += 1;
  return {lo, up, p * ((float)up - bpos), p * (bpos - (float)lo)};
}

// K <= 64: one row's pmf p (lane k) -> projected pmf (lane j) by cross-lane shuffles.  Deposits are accumulated per bin
// in atom order, all lower-neighbour deposits first, then all upper ones: the order of the reference's
// two sequential index_add_ passes (distl_util.py:18-19), so the result is deterministic.
template <int KMAX>
__device__ __forceinline__ float project_row(float p, float zk, float r, float d, float gamma_n, float v_min, float v_max,
                                             float dz, int K, int lane) {
  const C51Deposit a = c51_deposit(p, zk, r, d, gamma_n, v_min, v_max, dz, K);
  float out = 0.f;
#pragma unroll
  for (int kk = 0; kk < KMAX; ++kk) {
    if (kk < K) {
      const int l2 = __shfl(a.lo, kk, 64);
      const float w2 = __shfl(a.w_lo, kk, 64);
      if (l2 == lane) out += w2;
    }
  }
#pragma unroll
  for (int kk = 0; kk < KMAX; ++kk) {
    if (kk < K) {
      const int u2 = __shfl(a.up, kk, 64);
      const float w2 = __shfl(a.w_up, kk, 64);
      if (u2 == lane) out += w2;
    }
  }
  return out;
}

// K > 64.  The wave writes the deposits of its K atoms into its own 4 KiB LDS image.  lo and up are non-decreasing in the atom
// index (precondition in pqlk.h), so the atoms that deposit into bin j are a contiguous range: the lane that owns the bin finds the
// first atom with lo >= j by binary search, walks while lo == j, then does the same for up -- all lower-neighbour deposits in atom
// order, then all upper ones, a plain left-to-right fp32 sum: the order of project_row and of the reference's two index_add_
// passes.  O(K) LDS reads per bin at worst (a terminal row: one bin collects every atom), O(log K) typically.  lo / up are only ever
// COMPARED, never used as an address: a non-finite reward can drop mass, as in project_row, but cannot index outside the image.
//
// The image belongs to one wave and the row loop's trip count differs between the waves of a block (ragged last trip; B < 4 leaves
// waves idle): no __syncthreads() inside that loop.  A wave's LDS accesses execute in order; wave_lds_fence() keeps the compiler
// from reordering them.
struct C51Image {
  int lo[PQLK_C51_MAX_ATOMS];
  float w_lo[PQLK_C51_MAX_ATOMS];
  int up[PQLK_C51_MAX_ATOMS];
  float w_up[PQLK_C51_MAX_ATOMS];
};
static_assert(sizeof(C51Image) == 4096 && PQLK_C51_MAX_ATOMS == 256, "first_ge's step and the launch table assume 256");

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// number of leading entries of the non-decreasing v[0, K) that are < bin (= index of the first one >= bin, or K)
__device__ __forceinline__ int first_ge(const int* v, int K, int bin) {
  int pos = 0;
#pragma unroll
  for (int s = PQLK_C51_MAX_ATOMS; s > 0; s >>= 1) {
    const int e = pos + s;
    const int x = v[min(e, PQLK_C51_MAX_ATOMS) - 1];   // (read inside the image whatever e is; used only when e <= K)
    if (e <= K && x < bin) pos = e;
  }
  return pos;
}

// the projection of the kernels below: pmf p -> projected pmf out, both as load_row holds a row.  NJ == 1 never touches img (the
// compiler then drops the kernel's image: tests/test_host_cpu.py holds the LDS sizes)
template <int NJ>
__device__ __forceinline__ void project(const float (&p)[NJ], const float (&zk)[NJ], float r, float d, float gamma_n, float v_min,
                                        float v_max, float dz, int K, int lane, C51Image& img, float (&out)[NJ]) {
  if constexpr (NJ == 1) {
    out[0] = project_row<64>(p[0], zk[0], r, d, gamma_n, v_min, v_max, dz, K, lane);
  } else {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int a = lane + 64 * j;
      if (a < K) {
        const C51Deposit dep = c51_deposit(p[j], zk[j], r, d, gamma_n, v_min, v_max, dz, K);
        img.lo[a] = dep.lo;
        img.w_lo[a] = dep.w_lo;
        img.up[a] = dep.up;
        img.w_up[a] = dep.w_up;
      }
    }
    wave_lds_fence();
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int bin = lane + 64 * j;
      float o = 0.f;
      if (bin < K) {
        for (int a = first_ge(img.lo, K, bin); a < K && img.lo[a] == bin; ++a) o += img.w_lo[a];
        for (int a = first_ge(img.up, K, bin); a < K && img.up[a] == bin; ++a) o += img.w_up[a];
      }
      out[j] = o;
    }
    wave_lds_fence();   // the next projection's writes stay behind these reads
  }
}

template <int NJ>
__global__ __launch_bounds__(256) void k_c51_project(const float* __restrict__ p, const float* __restrict__ rew,
                                                     const float* __restrict__ done, const float* __restrict__ support,
                                                     float gamma_n, float v_min, float v_max, float dz, int K, int64_t b,
                                                     float* __restrict__ out) {
  __shared__ C51Image image[4];
  C51Image& img = image[threadIdx.x >> 6];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  float zk[NJ], pv[NJ], o[NJ];
  load_row<NJ>(support, K, lane, zk);
  for (int64_t i = wave; i < b; i += nw) {
    load_row<NJ>(p + i * K, K, lane, pv);
    project<NJ>(pv, zk, rew[i], done[i], gamma_n, v_min, v_max, dz, K, lane, img, o);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (lane + 64 * j < K) out[i * K + lane + 64 * j] = o[j];
  }
}

template <int NJ>
__global__ __launch_bounds__(256) void k_c51_bce(const float* __restrict__ logits, const float* __restrict__ logits_t,
                                                 int64_t ld, int K, const float* __restrict__ rew,
                                                 const float* __restrict__ done, const float* __restrict__ support,
                                                 float gamma_n, float v_min, float v_max, float dz, int64_t b,
                                                 float* __restrict__ dy, float* __restrict__ proj_out,
                                                 float* __restrict__ part) {
  __shared__ C51Image image[4];
  C51Image& img = image[threadIdx.x >> 6];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const float inv_numel = 1.0f / ((float)b * (float)K);
  float zk[NJ];
  load_row<NJ>(support, K, lane, zk);
  float acc = 0.f;
  for (int64_t i = wave; i < b; i += nw) {
    const float r = rew[i], d = done[i];
    // target pmf: min of the two projected target distributions (pql_v_learner.py:83-102)
    float pt[NJ], t[NJ], pr[NJ];
    load_row<NJ>(logits_t + i * ld, K, lane, pt);
    wave_softmax<NJ>(pt, K, lane);
    project<NJ>(pt, zk, r, d, gamma_n, v_min, v_max, dz, K, lane, img, t);
    load_row<NJ>(logits_t + (b + i) * ld, K, lane, pt);
    wave_softmax<NJ>(pt, K, lane);
    project<NJ>(pt, zk, r, d, gamma_n, v_min, v_max, dz, K, lane, img, pr);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      t[j] = fminf(t[j], pr[j]);
      if (proj_out && lane + 64 * j < K) proj_out[i * K + lane + 64 * j] = t[j];
    }
#pragma unroll
    for (int net = 0; net < 2; ++net) {
      const int64_t row = (int64_t)net * b + i;
      float pc[NJ], gp[NJ];
      load_row<NJ>(logits + row * ld, K, lane, pc);
      wave_softmax<NJ>(pc, K, lane);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float le = 0.f;
        gp[j] = 0.f;
        if (lane + 64 * j < K) {
          // F.binary_cross_entropy: (t-1)*max(log(1-p),-100) - t*max(log(p),-100); grad (p-t)/max((1-p)p,1e-12)
          le = (t[j] - 1.f) * fmaxf(logf(1.f - pc[j]), -100.f) - t[j] * fmaxf(logf(pc[j]), -100.f);
          gp[j] = (pc[j] - t[j]) / fmaxf((1.f - pc[j]) * pc[j], 1e-12f) * inv_numel;
        }
        acc += le;
      }
      const float dot = wave_dot<NJ>(gp, pc);
#pragma unroll
      for (int j = 0; j < NJ; ++j) gp[j] = (gp[j] - dot) * pc[j];  // softmax backward (pc is 0 past K)
      store_dy_row<NJ>(dy + row * ld, ld, K, lane, gp);
    }
  }
  const float s = block_sum_256(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// launch KERNEL<ceil(k / 64)> for 2 <= k <= PQLK_C51_MAX_ATOMS
#define C51_LAUNCH(KERNEL, k, blocks, stream, ...)                                                                    \
  do {                                                                                                                \
    const int nj__ = ((int)(k) + 63) / 64;                                                                            \
    if (nj__ == 1) hipLaunchKernelGGL(KERNEL<1>, dim3(blocks), dim3(256), 0, pqlk_s(stream), __VA_ARGS__);            \
    else if (nj__ == 2) hipLaunchKernelGGL(KERNEL<2>, dim3(blocks), dim3(256), 0, pqlk_s(stream), __VA_ARGS__);       \
    else if (nj__ == 3) hipLaunchKernelGGL(KERNEL<3>, dim3(blocks), dim3(256), 0, pqlk_s(stream), __VA_ARGS__);       \
    else hipLaunchKernelGGL(KERNEL<4>, dim3(blocks), dim3(256), 0, pqlk_s(stream), __VA_ARGS__);                      \
  } while (0)

extern "C" int pqlk_c51_project(const float* p, const float* rew, const float* done, const float* support, float gamma_n,
                                float v_min, float v_max, int32_t k, int64_t b, float* out, pqlk_stream_t stream) {
  PQLK_REQUIRE(p && rew && done && support && out, PQLK_E_NULL);
  PQLK_REQUIRE(b > 0 && k >= 2, PQLK_E_SHAPE);
  PQLK_REQUIRE(k <= PQLK_C51_MAX_ATOMS, PQLK_E_UNSUPPORTED);
  const float dz = (float)(((double)v_max - (double)v_min) / (double)(k - 1));
  int blocks = (int)((b + 3) / 4);
  if (blocks > 4096) blocks = 4096;
  C51_LAUNCH(k_c51_project, k, blocks, stream, p, rew, done, support, gamma_n, v_min, v_max, dz, (int)k, b, out);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

extern "C" int pqlk_c51_bce_loss(const float* logits, const float* logits_t, int64_t ld, int32_t k, const float* rew,
                                 const float* done, const float* support, float gamma_n, float v_min, float v_max,
                                 int64_t b, float* dy, float* loss_out, const int32_t* slot_dev, int32_t ring_len,
                                 float* proj_out, float* scratch, pqlk_stream_t stream) {
  PQLK_REQUIRE(logits && logits_t && rew && done && support && dy && scratch, PQLK_E_NULL);
  PQLK_REQUIRE(!slot_dev || ring_len > 0, PQLK_E_SHAPE);
  PQLK_REQUIRE(b > 0 && k >= 2, PQLK_E_SHAPE);
  PQLK_REQUIRE(k <= PQLK_C51_MAX_ATOMS, PQLK_E_UNSUPPORTED);
  PQLK_REQUIRE(ld % 32 == 0 && ld >= k, PQLK_E_ALIGN);
  const float dz = (float)(((double)v_max - (double)v_min) / (double)(k - 1));
  const int blocks = loss_blocks(b, k);
  C51_LAUNCH(k_c51_bce, k, blocks, stream, logits, logits_t, ld, (int)k, rew, done, support, gamma_n, v_min, v_max, dz, b, dy,
             proj_out, scratch);
  PQLK_LAUNCH_CHECK();
  return fold_partials(scratch, blocks, 1.0f / ((float)b * (float)k), loss_out, slot_dev, ring_len, stream);
}

// ------------------------------------------------------------------------------------------------
// HL-Gauss (Farebrother et al. 2024) on the categorical head: the law is written out in include/pqlk.h.  Geometry of k_c51_bce
// without its image: the scalar TD target y of k_td_mse, formed from the target nets' expectations, is spread over the K bins as
// a Gaussian histogram that each lane evaluates for its own atoms (no cross-lane sum in the target), and the logits are trained
// with a soft-target cross-entropy.  The bin edges depend on the support alone and stay in registers over the row loop.
__device__ __forceinline__ float hl_cdf(float u) { return u >= 4.f ? 1.f : (u <= -4.f ? -1.f : erff(u)); }

template <int NJ, bool PER>
__global__ __launch_bounds__(256) void k_hlgauss_ce(const float* __restrict__ logits, const float* __restrict__ logits_t,
                                                    int64_t ld, int K, const float* __restrict__ rew,
                                                    const float* __restrict__ done, const float* __restrict__ support,
                                                    float gamma_n, float v_min, float v_max, float dz, float inv, int64_t b,
                                                    float* __restrict__ dy, float* __restrict__ target_out,
                                                    float* __restrict__ part, const float* __restrict__ w,
                                                    const float* __restrict__ wmax, float* __restrict__ abs_td) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const float inv_b = 1.0f / (float)b;
  float wm = 1.f;
  if constexpr (PER) wm = wmax[0];
  float zk[NJ], e_lo[NJ], e_hi[NJ];
  load_row<NJ>(support, K, lane, zk);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {   // the edges of bin k = lane + 64 j: e_k and e_{k + 1}
    e_lo[j] = v_min + ((float)(lane + 64 * j) - 0.5f) * dz;
    e_hi[j] = v_min + ((float)(lane + 64 * j + 1) - 0.5f) * dz;
  }
  const float e_first = v_min + (0.f - 0.5f) * dz, e_last = v_min + ((float)K - 0.5f) * dz;
  float acc = 0.f;
  for (int64_t i = wave; i < b; i += nw) {
    const float r = rew[i], d = done[i];
    float x0[NJ], x1[NJ], pt[NJ];
    load_row<NJ>(logits + i * ld, K, lane, x0);
    load_row<NJ>(logits + (b + i) * ld, K, lane, x1);
    // y = clamp(r + (1 - d) gamma^n min_i E_i[z]) -- k_td_mse's target on the target nets' expectations (k_dpg_dist's E[z])
    bool odd = !(fabsf(r) < INFINITY) || !(fabsf(d) < INFINITY);
    load_row<NJ>(logits_t + i * ld, K, lane, pt);
#pragma unroll
    for (int j = 0; j < NJ; ++j) odd |= !(fabsf(pt[j]) < INFINITY) || !(fabsf(x0[j]) < INFINITY) || !(fabsf(x1[j]) < INFINITY);
    wave_softmax<NJ>(pt, K, lane);
    const float q0 = wave_dot<NJ>(pt, zk);
    load_row<NJ>(logits_t + (b + i) * ld, K, lane, pt);
#pragma unroll
    for (int j = 0; j < NJ; ++j) odd |= !(fabsf(pt[j]) < INFINITY);
    wave_softmax<NJ>(pt, K, lane);
    const float q1 = wave_dot<NJ>(pt, zk);
    float y = r + ((1.f - d) * gamma_n) * fminf(q0, q1);
    y = fminf(fmaxf(y, v_min), v_max);
    if (__ballot(odd) != 0) y = NAN;   // a row with a non-finite input: every output of the row, and the loss, is NaN
    // target pmf: the mass of N(y, sigma^2) between the edges of each bin, over its mass on the whole support
    const float c_first = hl_cdf((e_first - y) * inv), c_last = hl_cdf((e_last - y) * inv);
    const float norm = c_last - c_first;
    float t[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      t[j] = (hl_cdf((e_hi[j] - y) * inv) - hl_cdf((e_lo[j] - y) * inv)) / norm;
      if (lane + 64 * j >= K) t[j] = 0.f;
      else if (target_out) target_out[i * K + lane + 64 * j] = t[j];
    }
    float wh = 1.f, g = inv_b, td = 0.f;
    if constexpr (PER) {
      wh = w[i] / wm;
      g = wh * inv_b;
    }
    float lrow = 0.f;
#pragma unroll
    for (int net = 0; net < 2; ++net) {
      float(&x)[NJ] = net == 0 ? x0 : x1;
      float p[NJ];
      // log-sum-exp and softmax in wave_softmax's reduction order
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (lane + 64 * j < K) m = fmaxf(m, x[j]);
      m = wave_max(m);
#pragma unroll
      for (int j = 0; j < NJ; ++j) p[j] = lane + 64 * j < K ? expf(x[j] - m) : 0.f;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) s += p[j];
      s = wave_sum(s);
      const float lse = m + logf(s);
      float le = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        p[j] = p[j] / s;
        le += t[j] == 0.f ? 0.f : t[j] * (lse - x[j]);   // (t is 0 past K)
      }
      lrow += wave_sum(le);
      if constexpr (PER) td = fmaxf(td, fabsf(wave_dot<NJ>(p, zk) - y));
#pragma unroll
      for (int j = 0; j < NJ; ++j) p[j] = g * (p[j] - t[j]);
      store_dy_row<NJ>(dy + ((int64_t)net * b + i) * ld, ld, K, lane, p);
    }
    if constexpr (PER) {
      lrow = wh * lrow;
      if (lane == 0) abs_td[i] = y != y ? y : td;   // (fmaxf drops a NaN: the row's |TD| is NaN with its y)
    }
    if (lane == 0) acc += lrow;
  }
  const float s = block_sum_256(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
template <int NJ>
static constexpr auto k_hlgauss_plain = &k_hlgauss_ce<NJ, false>;   // (C51_LAUNCH names its kernel with one argument)
template <int NJ>
static constexpr auto k_hlgauss_weighted = &k_hlgauss_ce<NJ, true>;

template <bool PER>
static int hlgauss_impl(const float* logits, const float* logits_t, int64_t ld, int32_t k, const float* rew, const float* done,
                        const float* support, float gamma_n, float v_min, float v_max, float sigma_ratio, int64_t b, float* dy,
                        float* loss_out, const int32_t* slot_dev, int32_t ring_len, float* target_out, float* scratch, const float* w,
                        const float* wmax, float* abs_td_out, pqlk_stream_t stream) {
  PQLK_REQUIRE(logits && logits_t && rew && done && support && dy && scratch, PQLK_E_NULL);
  PQLK_REQUIRE(!PER || (w && wmax && abs_td_out), PQLK_E_NULL);
  PQLK_REQUIRE(!slot_dev || ring_len > 0, PQLK_E_SHAPE);
  PQLK_REQUIRE(b > 0 && k >= 2 && sigma_ratio > 0.f && v_max > v_min, PQLK_E_SHAPE);
  PQLK_REQUIRE(k <= PQLK_C51_MAX_ATOMS, PQLK_E_UNSUPPORTED);
  PQLK_REQUIRE(ld % 32 == 0 && ld >= k, PQLK_E_ALIGN);
  const float dz = (float)(((double)v_max - (double)v_min) / (double)(k - 1));
  const float inv = (float)(1.0 / ((double)sigma_ratio * (double)dz * sqrt(2.0)));
  const int blocks = loss_blocks(b, k);
  if constexpr (PER)
    C51_LAUNCH(k_hlgauss_weighted, k, blocks, stream, logits, logits_t, ld, (int)k, rew, done, support, gamma_n, v_min, v_max, dz, inv,
               b, dy, target_out, scratch, w, wmax, abs_td_out);
  else
    C51_LAUNCH(k_hlgauss_plain, k, blocks, stream, logits, logits_t, ld, (int)k, rew, done, support, gamma_n, v_min, v_max, dz, inv, b,
               dy, target_out, scratch, w, wmax, abs_td_out);
  PQLK_LAUNCH_CHECK();
  return fold_partials(scratch, blocks, 1.0f / (float)b, loss_out, slot_dev, ring_len, stream);
}

extern "C" int pqlk_hlgauss_ce_loss(const float* logits, const float* logits_t, int64_t ld, int32_t k, const float* rew,
                                    const float* done, const float* support, float gamma_n, float v_min, float v_max,
                                    float sigma_ratio, int64_t b, float* dy, float* loss_out, const int32_t* slot_dev,
                                    int32_t ring_len, float* target_out, float* scratch, pqlk_stream_t stream) {
  return hlgauss_impl<false>(logits, logits_t, ld, k, rew, done, support, gamma_n, v_min, v_max, sigma_ratio, b, dy, loss_out, slot_dev,
                             ring_len, target_out, scratch, nullptr, nullptr, nullptr, stream);
}

extern "C" int pqlk_hlgauss_ce_loss_per(const float* logits, const float* logits_t, int64_t ld, int32_t k, const float* rew,
                                        const float* done, const float* support, float gamma_n, float v_min, float v_max,
                                        float sigma_ratio, int64_t b, float* dy, float* loss_out, const int32_t* slot_dev,
                                        int32_t ring_len, float* target_out, float* scratch, const float* w, const float* wmax,
                                        float* abs_td_out, pqlk_stream_t stream) {
  return hlgauss_impl<true>(logits, logits_t, ld, k, rew, done, support, gamma_n, v_min, v_max, sigma_ratio, b, dy, loss_out, slot_dev,
                            ring_len, target_out, scratch, w, wmax, abs_td_out, stream);
}

__global__ __launch_bounds__(256) void k_dpg_scalar(const float* __restrict__ q, int64_t ld, int64_t b,
                                                    float* __restrict__ dy, float* __restrict__ part,
                                                    uint8_t* __restrict__ owner) {
  const float g = -1.0f / (float)b;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < b; i += (int64_t)gridDim.x * 256) {
    const float a = q[i * ld], c = q[(b + i) * ld];
    acc += fminf(a, c);
    const float g1 = a < c ? g : (a == c ? 0.5f * g : 0.f);
    const float g2 = c < a ? g : (a == c ? 0.5f * g : 0.f);
    dy[i * ld] = g1;
    dy[(b + i) * ld] = g2;
    if (owner) owner[i] = (uint8_t)((a <= c ? 1 : 0) | (c <= a ? 2 : 0));   // which net(s) the gradient reaches (minnet.h)
  }
  const float s = block_sum_256(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

template <int NJ>
__global__ __launch_bounds__(256) void k_dpg_dist(const float* __restrict__ logits, int64_t ld, int K,
                                                  const float* __restrict__ support, int64_t b, float* __restrict__ dy,
                                                  float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const float g = -1.0f / (float)b;
  float zk[NJ];
  load_row<NJ>(support, K, lane, zk);
  float acc = 0.f;
  for (int64_t i = wave; i < b; i += nw) {
    float p1[NJ], p2[NJ];
    load_row<NJ>(logits + i * ld, K, lane, p1);
    load_row<NJ>(logits + (b + i) * ld, K, lane, p2);
    wave_softmax<NJ>(p1, K, lane);
    wave_softmax<NJ>(p2, K, lane);
    const float q1 = wave_dot<NJ>(p1, zk), q2 = wave_dot<NJ>(p2, zk);  // E[z] (mlp.py:258-259)
    if (lane == 0) acc += fminf(q1, q2);
    const float g1 = q1 < q2 ? g : (q1 == q2 ? 0.5f * g : 0.f);
    const float g2 = q2 < q1 ? g : (q1 == q2 ? 0.5f * g : 0.f);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {   // dQ/dlogit_k = p_k (z_k - Q)
      p1[j] = g1 * p1[j] * (zk[j] - q1);
      p2[j] = g2 * p2[j] * (zk[j] - q2);
    }
    store_dy_row<NJ>(dy + i * ld, ld, K, lane, p1);
    store_dy_row<NJ>(dy + (b + i) * ld, ld, K, lane, p2);
  }
  const float s = block_sum_256(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

static int dpg_loss_impl(const float* q, int64_t ld, int32_t k, const float* support, int64_t b, float* dy,
                         float* loss_out, const int32_t* slot_dev, int32_t ring_len, float* scratch, uint8_t* owner,
                         pqlk_stream_t stream) {
  PQLK_REQUIRE(q && dy && scratch, PQLK_E_NULL);
  PQLK_REQUIRE(!slot_dev || ring_len > 0, PQLK_E_SHAPE);
  PQLK_REQUIRE(b > 0 && k >= 1, PQLK_E_SHAPE);
  PQLK_REQUIRE(k <= PQLK_C51_MAX_ATOMS, PQLK_E_UNSUPPORTED);
  PQLK_REQUIRE(ld % 32 == 0 && ld >= k, PQLK_E_ALIGN);
  PQLK_REQUIRE(k == 1 || support, PQLK_E_NULL);
  const int blocks = loss_blocks(b, k);
  if (k == 1)
    hipLaunchKernelGGL(k_dpg_scalar, dim3(blocks), dim3(256), 0, pqlk_s(stream), q, ld, b, dy, scratch, owner);
  else
    C51_LAUNCH(k_dpg_dist, k, blocks, stream, q, ld, (int)k, support, b, dy, scratch);
  PQLK_LAUNCH_CHECK();
  return fold_partials(scratch, blocks, -1.0f / (float)b, loss_out, slot_dev, ring_len, stream);
}

extern "C" int pqlk_dpg_loss(const float* q, int64_t ld, int32_t k, const float* support, int64_t b, float* dy,
                             float* loss_out, const int32_t* slot_dev, int32_t ring_len, float* scratch,
                             pqlk_stream_t stream) {
  return dpg_loss_impl(q, ld, k, support, b, dy, loss_out, slot_dev, ring_len, scratch, nullptr, stream);
}

// Same; for scalar heads (k == 1) additionally owner[m] = bit 0: the gradient of min(Q1, Q2) reaches net 0, bit 1: net 1
// (both on an exact tie) -- the input of pqlk_dpg_critic_backward's partition.  owner is not written when k > 1.
extern "C" int pqlk_dpg_loss_owner(const float* q, int64_t ld, int32_t k, const float* support, int64_t b, float* dy,
                                   float* loss_out, const int32_t* slot_dev, int32_t ring_len, float* scratch,
                                   uint8_t* owner, pqlk_stream_t stream) {
  return dpg_loss_impl(q, ld, k, support, b, dy, loss_out, slot_dev, ring_len, scratch, owner, stream);
}

// ------------------------------------------------------------------------------------------------
// Quantile regression (QR-DQN, Dabney et al. 2018) on twin critics: the law is written out in include/pqlk.h.  The reference has
// no such critic.  Geometry of the C51 kernels: one wave per batch row, four rows per block, a row loop above LOSS_MAX_BLOCKS;
// lane j holds quantile j of both nets (N <= 64), lanes >= N hold zeros and store the pad columns.  The target quantile T_k
// lives in lane k; the k loop fetches it with a wave-uniform lane read (v_readlane: no LDS, no cross-lane traffic).
//
// Reduction order (what the tests' bounds count):
//   S_i, the means of abs_td : wave_sum, the xor butterfly of pqlk_common.h (offsets 32 ... 1) over the 64 lanes;
//   dy[i, b, j]             : one chain over k = 0 ... N-1 in lane j, then / kappa, * 1/(B N), (* wh), negated;
//   loss                    : per lane and net one chain over k; (l0 + l1) / kappa (* wh) joins the lane's accumulator, one add
//                             per row of the wave's row loop; then block_sum_256 (butterfly, then the four waves as
//                             (w0 + w1) + (w2 + w3)) -> part[block]; then k_sum_partials / the optimiser's fold.
__device__ __forceinline__ float lane_read(float v, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

// one (j, k) pair of one net: u = T_k - theta_j -> the gradient chain g and the loss chain l of lane j
__device__ __forceinline__ void qr_term(float u, float tau, float kappa, float& g, float& l) {
  const float wgt = fabsf(tau - (u < 0.f ? 1.f : 0.f));
  const float a = fabsf(u);
  const float h = a <= kappa ? 0.5f * (u * u) : kappa * (a - 0.5f * kappa);
  g += wgt * fminf(fmaxf(u, -kappa), kappa);
  l += wgt * h;
}

// the four guarded loads of a row: lane j < N holds quantile j of both nets (th) and of both target nets (t), the other lanes zeros
struct QrRow {
  float th0, th1, t0, t1;
};
__device__ __forceinline__ QrRow qr_load_row(const float* __restrict__ theta, const float* __restrict__ theta_t, int64_t ld, int64_t b,
                                             int64_t i, int lane, bool on) {
  return {on ? theta[i * ld + lane] : 0.f, on ? theta[(b + i) * ld + lane] : 0.f, on ? theta_t[i * ld + lane] : 0.f,
          on ? theta_t[(b + i) * ld + lane] : 0.f};
}

// Tail of a row of either Huber kernel, from the lane's chains g0, g1 (gradient) and l0, l1 (loss) of the two nets: / kappa, the
// row's scale 1 / (B * target atoms), (* wh), the loss into the lane's accumulator, the negated gradient and the pad columns -> dy,
// and with PER the row's new priority |mt - mean_j theta_j| of either net, the larger (mt: the mean of the row's targets, formed by
// the caller; the plain instances never read it, w or abs_td).
template <bool PER>
__device__ __forceinline__ void huber_row_epilogue(float g0, float g1, float l0, float l1, float kappa, float scale, float mt, float th0,
                                                   float th1, bool on, int lane, int N, int64_t i, int64_t b, int64_t ld,
                                                   float* __restrict__ dy, float& acc, const float* __restrict__ w, float wm,
                                                   float* __restrict__ abs_td) {
  float row = (l0 + l1) / kappa;
  float v0[1] = {(g0 / kappa) * scale}, v1[1] = {(g1 / kappa) * scale};
  if constexpr (PER) {
    const float wh = w[i] / wm;
    row = wh * row;
    v0[0] = wh * v0[0];
    v1[0] = wh * v1[0];
  }
  if (on) acc += row;
  v0[0] = -v0[0];
  v1[0] = -v1[0];
  store_dy_row<1>(dy + i * ld, ld, N, lane, v0);
  store_dy_row<1>(dy + (b + i) * ld, ld, N, lane, v1);
  if constexpr (PER) {
    const float inv_n = 1.0f / (float)N;
    const float m0 = wave_sum(th0) * inv_n, m1 = wave_sum(th1) * inv_n;
    if (lane == 0) abs_td[i] = fmaxf(fabsf(mt - m0), fabsf(mt - m1));
  }
}

template <bool PER>
__global__ __launch_bounds__(256) void k_qr_huber(const float* __restrict__ theta, const float* __restrict__ theta_t, int64_t ld,
                                                  int N, const float* __restrict__ rew, const float* __restrict__ done,
                                                  float gamma_n, float kappa, int64_t b, float* __restrict__ dy,
                                                  float* __restrict__ part, const float* __restrict__ w,
                                                  const float* __restrict__ wmax, float* __restrict__ abs_td) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const float inv_bn = 1.0f / ((float)b * (float)N);
  const float tau = (float)(2 * lane + 1) / (float)(2 * N);
  const bool on = lane < N;
  float wm = 1.f;
  if constexpr (PER) wm = wmax[0];
  float acc = 0.f;
  for (int64_t i = wave; i < b; i += nw) {
    const float r = rew[i], d = done[i];
    const auto [th0, th1, t0, t1] = qr_load_row(theta, theta_t, ld, b, i, lane, on);
    const float s0 = wave_sum(t0), s1 = wave_sum(t1);
    const float ts = s1 < s0 ? t1 : t0;                 // clipped double-Q on the means: one net per row, a tie takes net 0
    const float T = r + ((1.f - d) * gamma_n) * ts;     // lane k: T_k (k_td_mse's operation order)
    float g0 = 0.f, g1 = 0.f, l0 = 0.f, l1 = 0.f;
    for (int k = 0; k < N; ++k) {
      const float tk = lane_read(T, k);
      qr_term(tk - th0, tau, kappa, g0, l0);
      qr_term(tk - th1, tau, kappa, g1, l1);
    }
    float mt = 0.f;                                     // mean_k T_k
    if constexpr (PER) mt = wave_sum(on ? T : 0.f) * (1.0f / (float)N);
    huber_row_epilogue<PER>(g0, g1, l0, l1, kappa, inv_bn, mt, th0, th1, on, lane, N, i, b, ld, dy, acc, w, wm, abs_td);
  }
  const float s = block_sum_256(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------------
// Truncated pooled targets (TQC, Kuznetsov et al. 2020) on the same heads: the law is written out in include/pqlk.h.  k_qr_huber's
// geometry; lane k holds quantile k of both nets and of BOTH target nets, i.e. the pooled atoms p = k (net 0) and p = N + k (net 1).
// Rank by counting, no sort and no LDS: over a wave-uniform loop of 2 N lane reads every lane counts the pooled atoms that precede
// its two (smaller, or equal with a smaller pool index); atom p is kept iff that count is below M = 2 (N - drop).  The two keep
// bits become two wave-wide ballots (SGPR pairs); the main loop walks their set bits in increasing p -- dropped atoms cost nothing
// -- and fetches T_p with a lane read, as k_qr_huber does.
//
// Reduction order: k_qr_huber's with "kept p in increasing p" in place of "k = 0 ... N-1" (chains of M terms) and 1 / (B M) in place
// of 1 / (B N); the mean of the kept targets is wave_sum over lanes of ((keep_0 ? T_0 : 0) + (keep_1 ? T_1 : 0)) times 1.0f / (float)M.
//
// SOFT (the maximum-entropy target of the TQC agent, "Soft truncated target" in include/pqlk.h): every atom of row b is lowered by
// s_b = expf(log_alpha[0]) * logp[b] (k_sac_entropy_shift's expression) before it is scaled: T_p = r + c * (z_p - s_b).  alpha is
// read once per wave, logp[b] is a wave-uniform load beside rew[b] and done[b].  The ranks stay on the raw z_p: one shift for the
// whole row cannot change their order in real arithmetic, and ranking before it keeps rounding from making or breaking a tie.  The
// plain instances never touch logp or log_alpha and compile to the code they were.
template <bool PER, bool SOFT>
__global__ __launch_bounds__(256) void k_tqc_huber(const float* __restrict__ theta, const float* __restrict__ theta_t, int64_t ld,
                                                   int N, int drop, const float* __restrict__ rew, const float* __restrict__ done,
                                                   float gamma_n, float kappa, int64_t b, float* __restrict__ dy,
                                                   float* __restrict__ part, const float* __restrict__ w,
                                                   const float* __restrict__ wmax, float* __restrict__ abs_td,
                                                   const float* __restrict__ logp, const float* __restrict__ log_alpha) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const int M = 2 * (N - drop);
  const float inv_bm = 1.0f / ((float)b * (float)M);
  const float tau = (float)(2 * lane + 1) / (float)(2 * N);
  const bool on = lane < N;
  float wm = 1.f;
  if constexpr (PER) wm = wmax[0];
  float alpha = 0.f;
  if constexpr (SOFT) alpha = expf(log_alpha[0]);
  float acc = 0.f;
  for (int64_t i = wave; i < b; i += nw) {
    const float r = rew[i], d = done[i];
    float sh = 0.f;
    if constexpr (SOFT) sh = alpha * logp[i];            // s_b: one product
    const auto [th0, th1, t0, t1] = qr_load_row(theta, theta_t, ld, b, i, lane, on);
    // ranks of this lane's atoms p = lane (z = t0) and p = N + lane (z = t1) among the 2 N pooled raw target quantiles
    int c0 = 0, c1 = 0;
    for (int q = 0; q < N; ++q) {
      const float a0 = lane_read(t0, q), a1 = lane_read(t1, q);       // pool indices q and N + q
      c0 += (a0 < t0 || (a0 == t0 && q < lane)) ? 1 : 0;
      c0 += a1 < t0 ? 1 : 0;                                           // (N + q > lane: an equal atom of net 1 comes after)
      c1 += a0 <= t1 ? 1 : 0;                                          // (q < N + lane: an equal atom of net 0 comes before)
      c1 += (a1 < t1 || (a1 == t1 && q < lane)) ? 1 : 0;
    }
    const bool keep0 = on && c0 < M, keep1 = on && c1 < M;
    const unsigned long long m0 = __ballot(keep0), m1 = __ballot(keep1);
    const float c = (1.f - d) * gamma_n;
    float T0, T1;                                        // lane k: T_k and T_{N + k} (k_td_mse's operation order)
    if constexpr (SOFT) {
      T0 = r + c * (t0 - sh);                            // subtract, multiply, add: each step rounds
      T1 = r + c * (t1 - sh);
    } else {
      T0 = r + c * t0;
      T1 = r + c * t1;
    }
    float g0 = 0.f, g1 = 0.f, l0 = 0.f, l1 = 0.f;
    for (unsigned long long m = m0; m; m &= m - 1) {     // kept atoms of net 0, increasing p
      const float tp = lane_read(T0, __builtin_ctzll(m));
      qr_term(tp - th0, tau, kappa, g0, l0);
      qr_term(tp - th1, tau, kappa, g1, l1);
    }
    for (unsigned long long m = m1; m; m &= m - 1) {     // then those of net 1
      const float tp = lane_read(T1, __builtin_ctzll(m));
      qr_term(tp - th0, tau, kappa, g0, l0);
      qr_term(tp - th1, tau, kappa, g1, l1);
    }
    float mt = 0.f;                                      // mean of the kept T_p
    if constexpr (PER) mt = wave_sum((keep0 ? T0 : 0.f) + (keep1 ? T1 : 0.f)) * (1.0f / (float)M);
    huber_row_epilogue<PER>(g0, g1, l0, l1, kappa, inv_bm, mt, th0, th1, on, lane, N, i, b, ld, dy, acc, w, wm, abs_td);
  }
  const float s = block_sum_256(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// Behind the six Huber entries.  POOLED: the truncated pooled law (k_tqc_huber; drop is checked, the loss's divisor is the kept atoms
// M = 2 (n - drop)); otherwise one whole target net per row (k_qr_huber; drop, logp and log_alpha are not looked at, the divisor is n).
template <bool PER, bool POOLED, bool SOFT>
static int huber_impl(const float* theta, const float* theta_t, int64_t ld, int32_t n, int32_t drop, const float* rew, const float* done,
                      float gamma_n, float kappa, int64_t b, float* dy, float* loss_out, const int32_t* slot_dev, int32_t ring_len,
                      float* scratch, const float* w, const float* wmax, float* abs_td_out, const float* logp, const float* log_alpha,
                      pqlk_stream_t stream) {
  static_assert(POOLED || !SOFT, "the soft target is a law of the pooled atoms");
  PQLK_REQUIRE(theta && theta_t && rew && done && dy && scratch, PQLK_E_NULL);
  PQLK_REQUIRE(!PER || (w && wmax && abs_td_out), PQLK_E_NULL);
  PQLK_REQUIRE(!SOFT || (logp && log_alpha), PQLK_E_NULL);
  PQLK_REQUIRE(!slot_dev || ring_len > 0, PQLK_E_SHAPE);
  PQLK_REQUIRE(b > 0 && kappa > 0.f, PQLK_E_SHAPE);
  PQLK_REQUIRE(n >= 2 && n <= PQLK_QR_MAX_QUANTILES, PQLK_E_UNSUPPORTED);
  PQLK_REQUIRE(!POOLED || (drop >= 0 && drop < n), PQLK_E_SHAPE);
  PQLK_REQUIRE(ld % 32 == 0 && ld >= n, PQLK_E_ALIGN);
  const int blocks = loss_blocks(b, n);
  if constexpr (POOLED)
    hipLaunchKernelGGL((k_tqc_huber<PER, SOFT>), dim3(blocks), dim3(256), 0, pqlk_s(stream), theta, theta_t, ld, (int)n, (int)drop, rew, done,
                       gamma_n, kappa, b, dy, scratch, w, wmax, abs_td_out, logp, log_alpha);
  else
    hipLaunchKernelGGL(k_qr_huber<PER>, dim3(blocks), dim3(256), 0, pqlk_s(stream), theta, theta_t, ld, (int)n, rew, done, gamma_n, kappa, b,
                       dy, scratch, w, wmax, abs_td_out);
  PQLK_LAUNCH_CHECK();
  return fold_partials(scratch, blocks, 1.0f / ((float)b * (float)(POOLED ? 2 * (n - drop) : n)), loss_out, slot_dev, ring_len, stream);
}

extern "C" int pqlk_qr_huber_loss(const float* theta, const float* theta_t, int64_t ld, int32_t n, const float* rew,
                                  const float* done, float gamma_n, float kappa, int64_t b, float* dy, float* loss_out,
                                  const int32_t* slot_dev, int32_t ring_len, float* scratch, pqlk_stream_t stream) {
  return huber_impl<false, false, false>(theta, theta_t, ld, n, 0, rew, done, gamma_n, kappa, b, dy, loss_out, slot_dev, ring_len, scratch,
                                         nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int pqlk_qr_huber_loss_per(const float* theta, const float* theta_t, int64_t ld, int32_t n, const float* rew,
                                      const float* done, float gamma_n, float kappa, int64_t b, float* dy, float* loss_out,
                                      const int32_t* slot_dev, int32_t ring_len, float* scratch, const float* w, const float* wmax,
                                      float* abs_td_out, pqlk_stream_t stream) {
  return huber_impl<true, false, false>(theta, theta_t, ld, n, 0, rew, done, gamma_n, kappa, b, dy, loss_out, slot_dev, ring_len, scratch, w,
                                        wmax, abs_td_out, nullptr, nullptr, stream);
}

extern "C" int pqlk_tqc_huber_loss(const float* theta, const float* theta_t, int64_t ld, int32_t n, const float* rew,
                                   const float* done, float gamma_n, float kappa, int64_t b, float* dy, float* loss_out,
                                   const int32_t* slot_dev, int32_t ring_len, float* scratch, int32_t drop, pqlk_stream_t stream) {
  return huber_impl<false, true, false>(theta, theta_t, ld, n, drop, rew, done, gamma_n, kappa, b, dy, loss_out, slot_dev, ring_len, scratch,
                                        nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int pqlk_tqc_huber_loss_per(const float* theta, const float* theta_t, int64_t ld, int32_t n, const float* rew,
                                       const float* done, float gamma_n, float kappa, int64_t b, float* dy, float* loss_out,
                                       const int32_t* slot_dev, int32_t ring_len, float* scratch, const float* w, const float* wmax,
                                       float* abs_td_out, int32_t drop, pqlk_stream_t stream) {
  return huber_impl<true, true, false>(theta, theta_t, ld, n, drop, rew, done, gamma_n, kappa, b, dy, loss_out, slot_dev, ring_len, scratch, w,
                                       wmax, abs_td_out, nullptr, nullptr, stream);
}

extern "C" int pqlk_tqc_huber_loss_soft(const float* theta, const float* theta_t, int64_t ld, int32_t n, const float* rew,
                                        const float* done, float gamma_n, float kappa, int64_t b, float* dy, float* loss_out,
                                        const int32_t* slot_dev, int32_t ring_len, float* scratch, const float* logp,
                                        const float* log_alpha, int32_t drop, pqlk_stream_t stream) {
  return huber_impl<false, true, true>(theta, theta_t, ld, n, drop, rew, done, gamma_n, kappa, b, dy, loss_out, slot_dev, ring_len, scratch,
                                       nullptr, nullptr, nullptr, logp, log_alpha, stream);
}

extern "C" int pqlk_tqc_huber_loss_soft_per(const float* theta, const float* theta_t, int64_t ld, int32_t n, const float* rew,
                                            const float* done, float gamma_n, float kappa, int64_t b, float* dy, float* loss_out,
                                            const int32_t* slot_dev, int32_t ring_len, float* scratch, const float* w,
                                            const float* wmax, float* abs_td_out, const float* logp, const float* log_alpha,
                                            int32_t drop, pqlk_stream_t stream) {
  return huber_impl<true, true, true>(theta, theta_t, ld, n, drop, rew, done, gamma_n, kappa, b, dy, loss_out, slot_dev, ring_len, scratch, w,
                                      wmax, abs_td_out, logp, log_alpha, stream);
}

// DPG on the quantile heads, one wave per row.  The min law (MEAN false): Q_i = (sum_j theta[i, b, j]) * (1 / N) (wave_sum),
// L = -mean_b min(Q_0, Q_1); every quantile of the smaller net gets -1 / (B N), on a tie both nets half of it (torch.min's backward,
// k_dpg_scalar).  The mean-of-critics objective of the TQC agent (MEAN true, "Mean-of-critics actor objective" in include/pqlk.h):
// Qbar_b = wave_sum(th0 + th1) * (1 / (2 N)), L = -mean_b Qbar_b; every quantile of both nets gets -1 / (B 2 N), whatever the
// values (no min, no tie).  Lane 0 carries the row's min / Qbar_b into the block's partial; the fold scale is -1 / B.
template <bool MEAN>
__device__ __forceinline__ void dpg_quantile_rows(const float* __restrict__ theta, int64_t ld, int N, int64_t b, float* __restrict__ dy,
                                                  float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const int D = MEAN ? 2 * N : N;                        // atoms a row's Q is the mean of
  const float g = -(1.0f / ((float)b * (float)D));
  const float inv_d = 1.0f / (float)D;
  float acc = 0.f;
  for (int64_t i = wave; i < b; i += nw) {
    float th0[1], th1[1];
    load_row<1>(theta + i * ld, N, lane, th0);
    load_row<1>(theta + (b + i) * ld, N, lane, th1);
    float g0 = g, g1 = g;
    if constexpr (MEAN) {
      const float qbar = wave_sum(th0[0] + th1[0]) * inv_d;
      if (lane == 0) acc += qbar;
    } else {
      const float q0 = wave_sum(th0[0]) * inv_d, q1 = wave_sum(th1[0]) * inv_d;
      if (lane == 0) acc += fminf(q0, q1);
      g0 = q0 < q1 ? g : (q0 == q1 ? 0.5f * g : 0.f);
      g1 = q1 < q0 ? g : (q0 == q1 ? 0.5f * g : 0.f);
    }
    const float v0[1] = {g0}, v1[1] = {g1};
    store_dy_row<1>(dy + i * ld, ld, N, lane, v0);
    store_dy_row<1>(dy + (b + i) * ld, ld, N, lane, v1);
  }
  const float s = block_sum_256(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_dpg_quantile(const float* __restrict__ theta, int64_t ld, int N, int64_t b,
                                                      float* __restrict__ dy, float* __restrict__ part) {
  dpg_quantile_rows<false>(theta, ld, N, b, dy, part);
}

__global__ __launch_bounds__(256) void k_dpg_quantile_mean(const float* __restrict__ theta, int64_t ld, int N, int64_t b,
                                                           float* __restrict__ dy, float* __restrict__ part) {
  dpg_quantile_rows<true>(theta, ld, N, b, dy, part);
}

static int dpg_quantile_impl(bool mean, const float* theta, int64_t ld, int32_t n, int64_t b, float* dy, float* loss_out,
                             const int32_t* slot_dev, int32_t ring_len, float* scratch, pqlk_stream_t stream) {
  PQLK_REQUIRE(theta && dy && scratch, PQLK_E_NULL);
  PQLK_REQUIRE(!slot_dev || ring_len > 0, PQLK_E_SHAPE);
  PQLK_REQUIRE(b > 0, PQLK_E_SHAPE);
  PQLK_REQUIRE(n >= 2 && n <= PQLK_QR_MAX_QUANTILES, PQLK_E_UNSUPPORTED);
  PQLK_REQUIRE(ld % 32 == 0 && ld >= n, PQLK_E_ALIGN);
  const int blocks = loss_blocks(b, n);
  hipLaunchKernelGGL(mean ? k_dpg_quantile_mean : k_dpg_quantile, dim3(blocks), dim3(256), 0, pqlk_s(stream), theta, ld, (int)n, b, dy,
                     scratch);
  PQLK_LAUNCH_CHECK();
  return fold_partials(scratch, blocks, -1.0f / (float)b, loss_out, slot_dev, ring_len, stream);
}

extern "C" int pqlk_dpg_loss_quantile(const float* theta, int64_t ld, int32_t n, int64_t b, float* dy, float* loss_out,
                                      const int32_t* slot_dev, int32_t ring_len, float* scratch, pqlk_stream_t stream) {
  return dpg_quantile_impl(false, theta, ld, n, b, dy, loss_out, slot_dev, ring_len, scratch, stream);
}

extern "C" int pqlk_dpg_loss_quantile_mean(const float* theta, int64_t ld, int32_t n, int64_t b, float* dy, float* loss_out,
                                           const int32_t* slot_dev, int32_t ring_len, float* scratch, pqlk_stream_t stream) {
  return dpg_quantile_impl(true, theta, ld, n, b, dy, loss_out, slot_dev, ring_len, scratch, stream);
}

// ------------------------------------------------------------------------------------------------
// Critic diagnostics (pqlk_critic_stats): the law is written out in include/pqlk.h.  No gradient, no loss: PQLK_CRITIC_STATS
// reductions over the rows of the twin heads' row values V_1, V_2 and the scalar TD target y.  Geometry of the loss kernels above --
// k_td_mse's on the scalar head (one row per thread), k_dpg_dist's on the wider ones (one wave per row, load_row / wave_softmax /
// wave_dot: the categorical row value is the E[z] of k_dpg_dist and k_hlgauss_ce, bit for bit) -- with PQLK_CRITIC_STATS partials per
// block in place of one: part[j * gridDim.x + block].  Statistic j joins its operands with stat_join: + (the sums and the count),
// fminf (j = 2) or fmaxf (j = 3, 7).  A second launch of one block folds the partials in a fixed order.  No float atomics.
struct CriticAcc {
  float v[PQLK_CRITIC_STATS];
};
__device__ __forceinline__ constexpr int stat_op(int j) { return j == 2 ? 1 : ((j == 3 || j == 7) ? 2 : 0); }
__device__ __forceinline__ constexpr float stat_identity(int j) { return stat_op(j) == 0 ? 0.f : (stat_op(j) == 1 ? INFINITY : -INFINITY); }
__device__ __forceinline__ float stat_join(int j, float a, float b) {
  return stat_op(j) == 0 ? a + b : (stat_op(j) == 1 ? fminf(a, b) : fmaxf(a, b));
}
__device__ __forceinline__ void stat_reset(CriticAcc& a) {
#pragma unroll
  for (int j = 0; j < PQLK_CRITIC_STATS; ++j) a.v[j] = stat_identity(j);
}
__device__ __forceinline__ bool stat_finite(float x) { return fabsf(x) < INFINITY; }

// one row joins the accumulator.  y_raw: the target before the categorical head's clamp (the other heads: y itself)
__device__ __forceinline__ void stat_row(CriticAcc& a, float v1, float v2, float y, float y_raw) {
  const float td = fmaxf(fabsf(v1 - y), fabsf(v2 - y));   // (k_td_mse's and k_hlgauss_ce's |TD|)
  const float row[PQLK_CRITIC_STATS] = {v1, v2, fminf(v1, v2), fmaxf(v1, v2), y, (v1 + v2) * 0.5f - y, td, td, fabsf(v1 - v2),
                                        (stat_finite(v1) && stat_finite(v2) && stat_finite(y_raw)) ? 0.f : 1.f};
#pragma unroll
  for (int j = 0; j < PQLK_CRITIC_STATS; ++j) a.v[j] = stat_join(j, a.v[j], row[j]);
}

__device__ __forceinline__ float stat_wave(int j, float v) {   // the xor butterfly of wave_sum under statistic j's join
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = stat_join(j, v, __shfl_xor(v, o, 64));
  return v;
}

// the block's partials from what each wave holds (UNIFORM: every lane of a wave already holds the wave's value)
template <bool UNIFORM>
__device__ __forceinline__ void stat_block_store(CriticAcc& a, float* __restrict__ part) {
  __shared__ float shw[4][PQLK_CRITIC_STATS];
#pragma unroll
  for (int j = 0; j < PQLK_CRITIC_STATS; ++j) {
    if constexpr (!UNIFORM) a.v[j] = stat_wave(j, a.v[j]);
    if ((threadIdx.x & 63) == 0) shw[threadIdx.x >> 6][j] = a.v[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < PQLK_CRITIC_STATS; ++j)
      part[(int64_t)j * gridDim.x + blockIdx.x] = stat_join(j, stat_join(j, shw[0][j], shw[1][j]), stat_join(j, shw[2][j], shw[3][j]));
  }
}

__global__ __launch_bounds__(256) void k_critic_stats_scalar(const float* __restrict__ q, const float* __restrict__ qt, int64_t ld,
                                                             const float* __restrict__ rew, const float* __restrict__ done,
                                                             float gamma_n, int64_t b, float* __restrict__ part) {
  CriticAcc a;
  stat_reset(a);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < b; i += (int64_t)gridDim.x * 256) {
    const float tq = fminf(qt[i * ld], qt[(b + i) * ld]);
    const float y = rew[i] + ((1.f - done[i]) * gamma_n) * tq;   // k_td_mse's target, op for op
    stat_row(a, q[i * ld], q[(b + i) * ld], y, y);
  }
  stat_block_store<false>(a, part);
}

// CAT: the categorical head (NJ = ceil(K / 64); V = E[z] of the softmax, y clamped); otherwise the quantile head (NJ = 1; V = the
// mean of the K quantile locations, wave_sum * (1.0f / (float)K) as in dpg_quantile_rows)
template <int NJ, bool CAT>
__global__ __launch_bounds__(256) void k_critic_stats_rows(const float* __restrict__ q, const float* __restrict__ qt, int64_t ld, int K,
                                                           const float* __restrict__ support, float v_min, float v_max,
                                                           const float* __restrict__ rew, const float* __restrict__ done,
                                                           float gamma_n, int64_t b, float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const float inv_k = 1.0f / (float)K;
  float zk[NJ];
  if constexpr (CAT) load_row<NJ>(support, K, lane, zk);
  CriticAcc a;
  stat_reset(a);
  for (int64_t i = wave; i < b; i += nw) {
    float v[4];   // V_1, V_2, V'_1, V'_2
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      float x[NJ];
      load_row<NJ>((n < 2 ? q : qt) + ((int64_t)(n & 1) * b + i) * ld, K, lane, x);
      if constexpr (CAT) {
        wave_softmax<NJ>(x, K, lane);
        v[n] = wave_dot<NJ>(x, zk);
      } else {
        v[n] = wave_sum(x[0]) * inv_k;
      }
    }
    const float y_raw = rew[i] + ((1.f - done[i]) * gamma_n) * fminf(v[2], v[3]);
    float y = y_raw;
    if constexpr (CAT) y = y_raw != y_raw ? y_raw : fminf(fmaxf(y_raw, v_min), v_max);   // (the clamp would turn a NaN into v_min)
    stat_row(a, v[0], v[1], y, y_raw);
  }
  stat_block_store<true>(a, part);
}
template <int NJ>
static constexpr auto k_critic_stats_cat = &k_critic_stats_rows<NJ, true>;   // (C51_LAUNCH names its kernel with one argument)

// part[j * n + block] -> out[j]: per thread a chain over its blocks (block t, t + 256, ...), the butterfly, the four waves in order;
// the sums (not the count) times inv_b
__global__ __launch_bounds__(256) void k_critic_stats_fold(const float* __restrict__ part, int n, float inv_b, float* __restrict__ out) {
  __shared__ float shw[4][PQLK_CRITIC_STATS];
#pragma unroll
  for (int j = 0; j < PQLK_CRITIC_STATS; ++j) {
    float v = stat_identity(j);
    for (int i = threadIdx.x; i < n; i += 256) v = stat_join(j, v, part[(int64_t)j * n + i]);
    v = stat_wave(j, v);
    if ((threadIdx.x & 63) == 0) shw[threadIdx.x >> 6][j] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < PQLK_CRITIC_STATS; ++j) {
      const float r = stat_join(j, stat_join(j, shw[0][j], shw[1][j]), stat_join(j, shw[2][j], shw[3][j]));
      out[j] = (stat_op(j) == 0 && j != PQLK_CRITIC_STATS - 1) ? r * inv_b : r;
    }
  }
}

extern "C" int64_t pqlk_critic_stats_scratch_floats(int64_t b, int32_t k) {
  return b > 0 && k >= 1 ? (int64_t)PQLK_CRITIC_STATS * loss_blocks(b, k) : 0;
}

extern "C" int pqlk_critic_stats(const float* q, const float* qt, int64_t ld, int32_t head, int32_t k, const float* z_atoms, float v_min,
                                 float v_max, const float* rew, const float* done, float gamma_n, int64_t b, float* out, float* scratch,
                                 pqlk_stream_t stream) {
  PQLK_REQUIRE(q && qt && rew && done && out && scratch, PQLK_E_NULL);
  PQLK_REQUIRE(head == PQLK_HEAD_SCALAR || head == PQLK_HEAD_CATEGORICAL || head == PQLK_HEAD_QUANTILE, PQLK_E_UNSUPPORTED);
  PQLK_REQUIRE(head != PQLK_HEAD_CATEGORICAL || z_atoms, PQLK_E_NULL);
  PQLK_REQUIRE(b > 0, PQLK_E_SHAPE);
  if (head == PQLK_HEAD_SCALAR) PQLK_REQUIRE(k == 1, PQLK_E_SHAPE);
  else PQLK_REQUIRE(k >= 2, PQLK_E_SHAPE);
  PQLK_REQUIRE(k <= (head == PQLK_HEAD_QUANTILE ? PQLK_QR_MAX_QUANTILES : PQLK_C51_MAX_ATOMS), PQLK_E_UNSUPPORTED);
  PQLK_REQUIRE(head != PQLK_HEAD_CATEGORICAL || v_max > v_min, PQLK_E_SHAPE);
  PQLK_REQUIRE(ld >= 32 && ld % 32 == 0 && ld >= k, PQLK_E_ALIGN);
  const int blocks = loss_blocks(b, k);
  if (head == PQLK_HEAD_SCALAR)
    hipLaunchKernelGGL(k_critic_stats_scalar, dim3(blocks), dim3(256), 0, pqlk_s(stream), q, qt, ld, rew, done, gamma_n, b, scratch);
  else if (head == PQLK_HEAD_QUANTILE)
    hipLaunchKernelGGL((k_critic_stats_rows<1, false>), dim3(blocks), dim3(256), 0, pqlk_s(stream), q, qt, ld, (int)k, z_atoms, v_min, v_max,
                       rew, done, gamma_n, b, scratch);
  else
    C51_LAUNCH(k_critic_stats_cat, k, blocks, stream, q, qt, ld, (int)k, z_atoms, v_min, v_max, rew, done, gamma_n, b, scratch);
  PQLK_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_critic_stats_fold, dim3(1), dim3(256), 0, pqlk_s(stream), scratch, blocks, 1.0f / (float)b, out);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}
