// Prioritized experience replay on a device sum tree (include/pqlk.h, "Prioritized experience replay").
//
// Layout.  One flat fp32 buffer: level 0 = one leaf per ring row (priority^alpha, 0 for a row never written), level l + 1 = the
// sums of 64 consecutive nodes of level l, until a level has at most 64 nodes.  Each level is padded with zeros to a multiple of
// 64 floats, so a wave always loads a node's 64 children with one coalesced 256-B access and needs no bounds test; pads are
// never written.  The total is the sum of the top level, formed by whoever needs it.
//
// Order of sums.  One wave owns one node.  Lane j holds child j; the sum is `wave_sum` of pqlk_common.h, an xor butterfly over
// the offsets 32, 16, 8, 4, 2, 1.  After the round with offset o every lane holds the sum of the lanes that differ from it only in
// the bits >= o ... written out for lane 0:
//     r32[j] = c[j] + c[j ^ 32]                       (j in 0..63)
//     r16[j] = r32[j] + r32[j ^ 16]
//     ...
//     sum    = r2[0] + r2[1],  r2[j] = r4[j] + r4[j ^ 2]
// i.e. a balanced binary tree whose leaves pair child j with child j + 32 first.  fp32 addition is commutative, so both lanes
// of a pair compute the same bits and all 64 lanes end with the same value; lane 0 stores it.  A node's value therefore depends
// on its 64 children alone: the upper levels are a pure function of the leaves, however they were reached (insert, update,
// rebuild), and a node recomputed by several waves receives identical bits from each.
//
// Order of the prefix (sampling).  Hillis-Steele over the 64 lanes: for d = 1, 2, 4, 8, 16, 32, lane j >= d adds the value lane
// j - d held before the round.  Lane j's inclusive prefix is a fixed expression in c[0..j]; the prefixes of different lanes
// associate differently, so they need not be monotone in the last bit: the choice below never relies on that.
//
// No float atomic add anywhere.  The two atomics are integer maxima on the bit patterns of non-negative floats (their order
// is the floats' order), whose result does not depend on the order of the threads.
#include "pqlk_common.h"

#define PER_MAX_LEVELS 8   // 64^8 rows

struct PerGeom {
  int levels;
  int64_t n[PER_MAX_LEVELS];     // nodes of level l
  int64_t off[PER_MAX_LEVELS];   // first float of level l
  int64_t floats;
};

static PerGeom per_geom(int64_t capacity) {
  PerGeom g = {};
  if (capacity <= 0) return g;
  int64_t n = capacity, off = 0;
  for (;;) {
    g.n[g.levels] = n;
    g.off[g.levels] = off;
    off += pqlk_round_up(n, 64);
    g.levels++;
    if (n <= 64 || g.levels == PER_MAX_LEVELS) break;
    n = (n + 63) / 64;
  }
  g.floats = off;
  return g;
}

extern "C" int32_t pqlk_per_levels(int64_t capacity) { return per_geom(capacity).levels; }
extern "C" int64_t pqlk_per_tree_floats(int64_t capacity) { return per_geom(capacity).floats; }

// x ^ e as include/pqlk.h defines it
__device__ __forceinline__ float per_pow(float x, float e) {
  if (e == 0.f) return 1.f;
  if (e == 1.f) return x;
  if (e == -1.f) return 1.0f / x;
  if (e == 0.5f) return sqrtf(x);
  return powf(x, e);
}

__device__ __forceinline__ float wave_prefix_incl(float v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

// total mass: every lane of the calling wave gets the sum of the (zero-padded) top level
__device__ __forceinline__ float per_total(const float* __restrict__ top, int lane) { return wave_sum(top[lane]); }

// ------------------------------------------------------------------------------------------------ maintenance
__global__ __launch_bounds__(256) void k_per_fill(float* __restrict__ leaf, const float* __restrict__ pmax, int64_t m, float alpha) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < m) leaf[i] = per_pow(pmax[0], alpha);
}

// one wave per node: parent[first + w] = sum of child[(first + w) * 64 + lane]
__global__ __launch_bounds__(256) void k_per_nodes(const float* __restrict__ child, float* __restrict__ parent, int64_t first,
                                                   int64_t count) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= count) return;   // (whole waves leave: the butterfly below always runs with 64 lanes)
  const int64_t node = first + w;
  const float s = wave_sum(child[node * 64 + lane]);
  if (lane == 0) parent[node] = s;
}

// one wave per sample: the sample's ancestor at `shift` / 6 levels above the leaves
__global__ __launch_bounds__(256) void k_per_nodes_of(const float* __restrict__ child, float* __restrict__ parent,
                                                      const int64_t* __restrict__ idx, int64_t b, int64_t capacity, int shift) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= b) return;
  const int64_t r = idx[w];
  if (r < 0 || r >= capacity) return;   // (wave-uniform)
  const int64_t node = r >> shift;
  const float s = wave_sum(child[node * 64 + lane]);
  if (lane == 0) parent[node] = s;
}

__global__ __launch_bounds__(256) void k_per_clear(float* __restrict__ leaf, const int64_t* __restrict__ idx, int64_t b,
                                                   int64_t capacity) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= b) return;
  const int64_t r = idx[i];
  if (r >= 0 && r < capacity) leaf[r] = 0.f;
}

__global__ __launch_bounds__(256) void k_per_raise(float* __restrict__ leaf, float* __restrict__ pmax, const int64_t* __restrict__ idx,
                                                   const float* __restrict__ abs_td, int64_t b, int64_t capacity, float eps,
                                                   float alpha) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float p = 0.f;
  if (i < b) {
    const int64_t r = idx[i];
    if (r >= 0 && r < capacity) {
      p = abs_td[i] + eps;
      atomicMax(reinterpret_cast<unsigned int*>(leaf + r), __float_as_uint(per_pow(p, alpha)));
    }
  }
  p = wave_max(p);
  if ((threadIdx.x & 63) == 0 && p > 0.f) atomicMax(reinterpret_cast<unsigned int*>(pmax), __float_as_uint(p));
}

static inline int per_wave_blocks(int64_t waves) { return (int)((waves + 3) / 4); }

// ancestors of the leaf range [lo, hi], one launch per level
static int per_range_up(float* tree, const PerGeom& g, int64_t lo, int64_t hi, hipStream_t st) {
  for (int l = 1; l < g.levels; ++l) {
    lo >>= 6; hi >>= 6;
    const int64_t count = hi - lo + 1;
    hipLaunchKernelGGL(k_per_nodes, dim3(per_wave_blocks(count)), dim3(256), 0, st, tree + g.off[l - 1], tree + g.off[l], lo, count);
    PQLK_LAUNCH_CHECK();
  }
  return PQLK_OK;
}

extern "C" int pqlk_per_insert(float* tree, int64_t capacity, const float* pmax, int64_t dst_start, int64_t m, float alpha,
                               pqlk_stream_t stream) {
  PQLK_REQUIRE(tree && pmax, PQLK_E_NULL);
  PQLK_REQUIRE(capacity > 0 && m > 0, PQLK_E_SHAPE);
  PQLK_REQUIRE(dst_start >= 0 && dst_start <= capacity - m, PQLK_E_RANGE);
  const PerGeom g = per_geom(capacity);
  hipLaunchKernelGGL(k_per_fill, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, pqlk_s(stream), tree + dst_start, pmax, m, alpha);
  PQLK_LAUNCH_CHECK();
  return per_range_up(tree, g, dst_start, dst_start + m - 1, pqlk_s(stream));
}

extern "C" int pqlk_per_rebuild(float* tree, int64_t capacity, pqlk_stream_t stream) {
  PQLK_REQUIRE(tree, PQLK_E_NULL);
  PQLK_REQUIRE(capacity > 0, PQLK_E_SHAPE);
  return per_range_up(tree, per_geom(capacity), 0, capacity - 1, pqlk_s(stream));
}

extern "C" int pqlk_per_update(float* tree, int64_t capacity, float* pmax, const int64_t* idx, const float* abs_td, int64_t b,
                               float eps, float alpha, pqlk_stream_t stream) {
  PQLK_REQUIRE(tree && pmax && idx && abs_td, PQLK_E_NULL);
  PQLK_REQUIRE(capacity > 0 && b > 0, PQLK_E_SHAPE);
  const PerGeom g = per_geom(capacity);
  hipStream_t st = pqlk_s(stream);
  const unsigned blocks = (unsigned)((b + 255) / 256);
  hipLaunchKernelGGL(k_per_clear, dim3(blocks), dim3(256), 0, st, tree, idx, b, capacity);
  PQLK_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_per_raise, dim3(blocks), dim3(256), 0, st, tree, pmax, idx, abs_td, b, capacity, eps, alpha);
  PQLK_LAUNCH_CHECK();
  for (int l = 1; l < g.levels; ++l) {
    if (g.n[l] <= b) {   // fewer nodes than samples: the whole level (the same bits, fewer waves)
      hipLaunchKernelGGL(k_per_nodes, dim3(per_wave_blocks(g.n[l])), dim3(256), 0, st, tree + g.off[l - 1], tree + g.off[l], (int64_t)0,
                         g.n[l]);
    } else {
      hipLaunchKernelGGL(k_per_nodes_of, dim3(per_wave_blocks(b)), dim3(256), 0, st, tree + g.off[l - 1], tree + g.off[l], idx, b,
                         capacity, 6 * l);
    }
    PQLK_LAUNCH_CHECK();
  }
  return PQLK_OK;
}

// ------------------------------------------------------------------------------------------------ sampling and weights
// One wave's walk from the top level to a leaf: at each level the first child with a non-zero value whose inclusive prefix
// exceeds the residual (else the last non-zero child).  -> the row, and in every lane that row's leaf value.
__device__ __forceinline__ int64_t per_walk(const float* __restrict__ tree, const PerGeom& g, float resid, int lane, float* leaf) {
  int64_t node = 0;   // the node whose children are being looked at (at the top level: the virtual root)
  float c = 0.f;
  for (int l = g.levels - 1; l >= 0; --l) {
    c = tree[g.off[l] + node * 64 + lane];
    const float incl = wave_prefix_incl(c, lane);
    const unsigned long long nonzero = __ballot(c != 0.f);
    const unsigned long long over = __ballot(incl > resid) & nonzero;
    int j = 0;   // (an all-zero node: an empty tree.  Child 0 of a real node is a real node, so the walk stays in bounds)
    if (over) j = __ffsll((long long)over) - 1;
    else if (nonzero) j = 63 - __clzll((long long)nonzero);
    const float below = __shfl_up(incl, 1, 64);   // lane j - 1's inclusive prefix = lane j's exclusive one
    resid -= __shfl(lane > 0 ? below : 0.f, j, 64);
    node = node * 64 + j;
    if (node >= g.n[l]) node = g.n[l] - 1;   // (cannot happen while the pads are zero; keeps a corrupted buffer from leading out of it)
  }
  *leaf = __shfl(c, (int)(node & 63), 64);   // level 0's children are the leaves: lane (node mod 64) holds leaf[node]
  return node;
}

// importance weight of a row with leaf value `leaf` = priority^alpha: (N P(i))^-beta
__device__ __forceinline__ float per_weight(float n_valid, float leaf, float total, float beta) {
  return per_pow((n_valid * leaf) / total, -beta);
}

__global__ __launch_bounds__(256) void k_per_sample(const float* __restrict__ tree, PerGeom g, const float* __restrict__ u, int64_t b,
                                                    int64_t* __restrict__ idx_out) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= b) return;
  const float total = per_total(tree + g.off[g.levels - 1], lane);
  const float seg = total / (float)b;
  float leaf;
  const int64_t node = per_walk(tree, g, ((float)k + u[k]) * seg, lane, &leaf);
  if (lane == 0) idx_out[k] = node;
}

__global__ __launch_bounds__(256) void k_per_weights(const float* __restrict__ tree, const float* __restrict__ top, int64_t capacity,
                                                     const int64_t* __restrict__ idx, int64_t b, float n_valid, float beta,
                                                     float* __restrict__ w_out, float* __restrict__ wmax_out) {
  const int lane = threadIdx.x & 63;
  const float total = per_total(top, lane);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float w = 0.f;
  if (i < b) {
    const int64_t r = idx[i];
    if (r >= 0 && r < capacity) w = per_weight(n_valid, tree[r], total, beta);
    w_out[i] = w;
  }
  w = wave_max(w);
  if (lane == 0) atomicMax(reinterpret_cast<unsigned int*>(wmax_out), __float_as_uint(w));
}

extern "C" int pqlk_per_sample(const float* tree, int64_t capacity, const float* u, int64_t b, int64_t* idx_out,
                               pqlk_stream_t stream) {
  PQLK_REQUIRE(tree && u && idx_out, PQLK_E_NULL);
  PQLK_REQUIRE(capacity > 0 && b > 0, PQLK_E_SHAPE);
  hipLaunchKernelGGL(k_per_sample, dim3(per_wave_blocks(b)), dim3(256), 0, pqlk_s(stream), tree, per_geom(capacity), u, b, idx_out);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

extern "C" int pqlk_per_weights(const float* tree, int64_t capacity, const int64_t* idx, int64_t b, int64_t n_valid, float beta,
                                float* w_out, float* wmax_out, pqlk_stream_t stream) {
  PQLK_REQUIRE(tree && idx && w_out && wmax_out, PQLK_E_NULL);
  PQLK_REQUIRE(capacity > 0 && b > 0 && n_valid > 0, PQLK_E_SHAPE);
  PQLK_REQUIRE(n_valid <= capacity, PQLK_E_RANGE);
  const PerGeom g = per_geom(capacity);
  hipError_t e = hipMemsetAsync(wmax_out, 0, sizeof(float), pqlk_s(stream));
  if (e != hipSuccess) return -(int)e;
  hipLaunchKernelGGL(k_per_weights, dim3((unsigned)((b + 255) / 256)), dim3(256), 0, pqlk_s(stream), tree, tree + g.off[g.levels - 1],
                     capacity, idx, b, (float)n_valid, beta, w_out, wmax_out);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

// ------------------------------------------------------------------------------------------------ a run of steps in one launch
// The samples and weights of `steps` batches drawn from the tree as it stands: sample k of step s is
// per_walk for stratum k of b with u = r[s b + k] 2^-24, and its weight per_weight on the leaf the walk ended at.  One wave per
// sample, a row of blocks (blockIdx.y) per step.  The maximum of a step's weights is an integer atomic max like k_per_weights'; a wave
// whose weight does not exceed what it reads there first leaves the atomic out (the word only grows, so whatever it reads is at
// most the final maximum and the result is the same bits).
__global__ __launch_bounds__(256) void k_per_sample_steps(const float* __restrict__ tree, PerGeom g, const int64_t* __restrict__ r,
                                                          int64_t b, float n_valid, float beta,
                                                          int64_t* __restrict__ idx_out, float* __restrict__ w_out,
                                                          float* __restrict__ wmax_out) {
  const int lane = threadIdx.x & 63;
  const int64_t s = blockIdx.y, k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= b) return;   // (whole waves leave)
  const int64_t i = s * b + k;
  const float total = per_total(tree + g.off[g.levels - 1], lane);
  const float seg = total / (float)b;
  const float u = (float)r[i] * 0x1p-24f;   // exact: r < 2^24
  float leaf;
  const int64_t node = per_walk(tree, g, ((float)k + u) * seg, lane, &leaf);
  if (lane == 0) {
    const float w = per_weight(n_valid, leaf, total, beta);
    idx_out[i] = node;
    w_out[i] = w;
    unsigned int* m = reinterpret_cast<unsigned int*>(wmax_out + s);
    const unsigned int bits = __float_as_uint(w);
    if (bits > *reinterpret_cast<volatile unsigned int*>(m)) atomicMax(m, bits);
  }
}

extern "C" int pqlk_per_sample_steps(const float* tree, int64_t capacity, const int64_t* r, int64_t b, int64_t steps, int64_t n_valid,
                                     float beta, int64_t* idx_out, float* w_out, float* wmax_out, pqlk_stream_t stream) {
  PQLK_REQUIRE(tree && r && idx_out && w_out && wmax_out, PQLK_E_NULL);
  PQLK_REQUIRE(capacity > 0 && b > 0 && steps > 0 && n_valid > 0, PQLK_E_SHAPE);
  PQLK_REQUIRE(steps <= 65535 && b <= 4 * (int64_t)INT32_MAX, PQLK_E_SHAPE);   // (the grid: blocks of 4 samples x steps)
  PQLK_REQUIRE(n_valid <= capacity, PQLK_E_RANGE);
  hipError_t e = hipMemsetAsync(wmax_out, 0, (size_t)steps * sizeof(float), pqlk_s(stream));
  if (e != hipSuccess) return -(int)e;
  hipLaunchKernelGGL(k_per_sample_steps, dim3(per_wave_blocks(b), (unsigned)steps), dim3(256), 0, pqlk_s(stream), tree, per_geom(capacity), r, b,
                     (float)n_valid, beta, idx_out, w_out, wmax_out);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}
