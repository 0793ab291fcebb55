// Forward-only bf16-MFMA sibling of the whole-stack forward of the residual LayerNorm critic (fwd_bro.hip), for the forward nothing
// goes back through: the target critic of DDPG / SAC with algo.cri_class=DoubleQBroNet, algo.bronet_fused_forward=True and
// algo.critic_target_dtype=bfloat16.  One launch computes, for both nets (blockIdx.y), the stem, K residual blocks and the output layer:
//   z0 = a~ W~0' + b0, h0 = ELU(LN(z0));  k = 1..K: za = bf16(h_{k-1}) W~a' + ba, t = ELU(LN(za)), zb = bf16(t) W~b' + bb,
//   h_k = h_{k-1} + LN(zb);  Q = bf16(h_K) W~o' + bo.
// The law is written op by op in include/pqlk.h ("bf16 residual law"); fwd_bro.hip, fwd_ln.hip, fwd_ln_bf16.hip, ln.hip, gemm.hip and
// fused.h are untouched, and nothing here writes a stash.
//
// Work split: a block of 8 waves owns 32 R batch rows of one net through all 2 K + 2 layers, their current Linear input in ONE bf16 LDS
// image [row][max(roundup16(in_dim), W) + 8] that every layer overwrites in place, and two [wave][row] fp32 row-sum tables.  R = 2
// where W <= 512 (and the 64-row image fits), else R = 1: (512, R = 2) is 66 560 B + 4 096 B.  Every hidden layer has the width W, so
// the tiles a wave holds (NTW = ceil((W / 32) / 8), 1 .. 4) are a template argument of the whole stack: the kernel branches once, on W,
// and walks ONE packed pointer and ONE arena pointer from layer to layer -- no per-layer offset arrays, so K reaches 16.
//
// Linear: v_mfma_f32_32x32x16_bf16, the WEIGHT fragment from the packed copy (pqlk_bro_pack_bf16) as A -- one k step of one tile is one
// contiguous 1 KB run per wave -- and the activation fragment (one ds_read_b128 per row tile and k step) as B, so a lane holds one
// batch row (lane = 32 h + r: row r) and four consecutive features sit in four consecutive accumulator registers.  Wave w takes the
// tiles w, w + 8, ..; the fragments of k step s + 1 are issued before the MFMAs of step s.
//
// LayerNorm from registers: z = acc + b stays in the accumulators; lane partial, lane-pair fold, [wave][row] table, barrier, partials
// added in wave order; the same again for the squared deviations.  Three barriers per hidden layer.
//
// The skip, in the accumulator layout, in fp32 registers: the (row, feature) -> (wave, lane, register) map is the same in every hidden
// layer, so the lane that finishes u = LN(zb) for a feature held that feature of h_{k-1}.  h lives in NTW x R x 16 fp32 registers per
// lane (64 at (512, R = 2) and at (1024, R = 1)): the stem's epilogue writes them, an opening epilogue leaves them alone, a closing
// one adds u, keeps the sum and writes bf16(h_k) into the image, four features per ds_write_b64.  The residual stream is never rounded
// and never touches LDS or HBM; only the copy that feeds the next Linear is bf16.
//
// The output layer (width 1) rides on the last epilogue (the stem's at K = 0, else a closing one) through the first table, so nothing
// but Q leaves the block.  Plain vector stores, no atomics, no scratch; 64 accumulators + 64 skip registers + fragments put the kernel
// at 2 waves per SIMD, one block per CU.  A row's bits depend on neither m, its position in the batch, nor the launch.
#include "lnrow.h"

constexpr int BB_NW = 8;                 // waves per block
constexpr int BB_LDS_MAX = 160 * 1024;
constexpr int BB_PAD = 8;                // bf16 elements of row padding in LDS (16 B: consecutive rows start 4 banks apart)
constexpr int BB_MAX_R2_WIDTH = 512;     // widest stack at R = 2: 2 tiles x 2 row tiles x 16 = 64 accumulator (and 64 skip) registers

typedef __bf16 bb_bf16x8 __attribute__((ext_vector_type(8)));
typedef float bb_f32x16 __attribute__((ext_vector_type(16)));

// fp32 -> bf16, round to nearest even, ties included; NaN stays a (quiet) NaN, overflow goes to +-inf
__device__ __forceinline__ unsigned bb_rne(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
__device__ __forceinline__ unsigned bb_pack2(float lo, float hi) { return bb_rne(lo) | (bb_rne(hi) << 16); }
__device__ __forceinline__ float bb_round(float f) { return __uint_as_float(bb_rne(f) << 16); }   // the fp32 value of bf16(f)

struct BroBf16P {
  const float* X; const float* arena; const uint16_t* packed; float* q;
  int64_t net_stride, packed_net_stride;   // floats / bf16 elements
  int in_dim, ldin, W, K, m, ldx, ld;
  float eps;
};

struct BroPackBf16P {
  const float* arena; uint16_t* packed;
  int64_t net_stride, units_per_net, stem_units, blk_units;   // units = 16 B = 8 bf16
  int64_t stem, blk;                                           // floats of layer 0 / of a block layer in the arena
  int in_dim, ldin, W, K, n_nets;
};

extern __shared__ __attribute__((aligned(16))) unsigned char bb_sm[];

// the sum of a row's partials, one per wave that holds features, in wave order
__device__ __forceinline__ float bb_row_total(const float* tab, int rows, int row, int nw) {
  float t = tab[row];
  for (int w = 1; w < nw; ++w) t += tab[w * rows + row];
  return t;
}

enum { BB_STEM = 0, BB_OPEN = 1, BB_CLOSE = 2 };

// what is the same in every hidden layer of a stack: hoisted out of the layer loop
struct BbGeom {
  int W, ld, cnt, nw, r, h;   // cnt: this wave's tiles (wave, wave + 8, ..; <= NTW); nw: the waves that hold features
  float n;
};

// One hidden layer for the block's 32 R rows: img holds a~ (16 KS columns, zeros past the stem's input width) and is overwritten with
// a~ of the next Linear -- or, with wout (the last hidden layer), the rows' Q partials are left in tab1.  lay: [b | gamma | beta] of the
// layer in the arena.  KIND: BB_STEM / BB_OPEN: y = elu(xhat gamma + beta), BB_STEM keeps it in hs; BB_CLOSE: hs += xhat gamma + beta,
// y = hs.  Every wave of the block runs through the same barriers; ends behind the one after which the image (or tab1) is complete.
template <int R, int NTW, int KIND>
__device__ __forceinline__ void bb_layer(const BbGeom& g, const uint4* __restrict__ w, int KS, const float* __restrict__ lay, float eps,
                                         const uint16_t* __restrict__ wout, uint16_t* img, float* tab1, float* tab2,
                                         bb_f32x16 (&hs)[NTW][R], int wave, int lane) {
  constexpr int ROWS = 32 * R;
  const int r = g.r, h = g.h, cnt = g.cnt, nw = g.nw, ld = g.ld;
  const float *bias = lay, *gamma = lay + g.W, *beta = lay + 2 * g.W;
  bb_f32x16 acc[NTW][R];
#pragma unroll
  for (int j = 0; j < NTW; ++j)
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][i][e] = 0.f;
  if (cnt > 0) {
    const uint4* wp = w + (long long)wave * KS * 64 + lane;   // tile t, k step ks: 64 fragments at (t KS + ks) 64
    const long long tstep = (long long)BB_NW * KS * 64;
    const uint16_t* ap = img + r * ld + 8 * h;
    uint4 wf[NTW] = {};
#pragma unroll
    for (int j = 0; j < NTW; ++j)
      if (j < cnt) wf[j] = wp[j * tstep];
    for (int ks = 0; ks < KS; ++ks) {
      const int kn = ks + 1 < KS ? ks + 1 : ks;   // the next k step's fragments (the last step fetches itself again)
      uint4 wn[NTW] = {}, af[R];
#pragma unroll
      for (int j = 0; j < NTW; ++j)
        if (j < cnt) wn[j] = wp[j * tstep + kn * 64];
#pragma unroll
      for (int i = 0; i < R; ++i) af[i] = *reinterpret_cast<const uint4*>(ap + 32 * i * ld + 16 * ks);
#pragma unroll
      for (int j = 0; j < NTW; ++j)
        if (j < cnt) {
#pragma unroll
          for (int i = 0; i < R; ++i)
            acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bb_bf16x8, wf[j]), __builtin_bit_cast(bb_bf16x8, af[i]),
                                                                acc[j][i], 0, 0, 0);
        }
#pragma unroll
      for (int j = 0; j < NTW; ++j) wf[j] = wn[j];
    }
  }
  // ---- z = acc + b stays in acc; the row sum: this lane's features in (tile, register) order, the lane pair, the waves in order
  float s[R];
#pragma unroll
  for (int i = 0; i < R; ++i) s[i] = 0.f;
#pragma unroll
  for (int j = 0; j < NTW; ++j)
    if (j < cnt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n0 = 32 * (wave + BB_NW * j) + 8 * q + 4 * h;   // accumulator registers 4q .. 4q+3 = features n0 .. n0+3 of row r
        const float4 b4 = *reinterpret_cast<const float4*>(bias + n0);
#pragma unroll
        for (int i = 0; i < R; ++i) {
          acc[j][i][4 * q] += b4.x; acc[j][i][4 * q + 1] += b4.y; acc[j][i][4 * q + 2] += b4.z; acc[j][i][4 * q + 3] += b4.w;
#pragma unroll
          for (int e = 0; e < 4; ++e) s[i] += acc[j][i][4 * q + e];
        }
      }
    }
#pragma unroll
  for (int i = 0; i < R; ++i) {
    s[i] += __shfl_xor(s[i], 32, 64);
    if (cnt > 0 && h == 0) tab1[wave * ROWS + 32 * i + r] = s[i];
  }
  __syncthreads();   // the partials are there, and nobody reads the layer's input any more
  // ---- d = z - mean stays in acc; the sum of d * d the same way
#pragma unroll
  for (int i = 0; i < R; ++i) s[i] = 0.f;
  if (cnt > 0) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const float mu = bb_row_total(tab1, ROWS, 32 * i + r, nw) / g.n;
#pragma unroll
      for (int j = 0; j < NTW; ++j)
        if (j < cnt) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const float d = acc[j][i][e] - mu;
            acc[j][i][e] = d;
            s[i] += d * d;
          }
        }
    }
  }
#pragma unroll
  for (int i = 0; i < R; ++i) {
    s[i] += __shfl_xor(s[i], 32, 64);
    if (cnt > 0 && h == 0) tab2[wave * ROWS + 32 * i + r] = s[i];
  }
  __syncthreads();   // (tab1 has been read by everybody: the output layer may write over it)
  // ---- y (ELU, or the skip), a~ = bf16(y): into the image, or multiplied out with the output layer's weights
  float rs[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    rs[i] = 0.f;
    s[i] = 0.f;
  }
  if (cnt > 0) {
#pragma unroll
    for (int i = 0; i < R; ++i) rs[i] = 1.0f / sqrtf(bb_row_total(tab2, ROWS, 32 * i + r, nw) / g.n + eps);
#pragma unroll
    for (int j = 0; j < NTW; ++j)
      if (j < cnt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n0 = 32 * (wave + BB_NW * j) + 8 * q + 4 * h;
          const float4 g4 = *reinterpret_cast<const float4*>(gamma + n0);
          const float4 e4 = *reinterpret_cast<const float4*>(beta + n0);
          const float ga[4] = {g4.x, g4.y, g4.z, g4.w}, be[4] = {e4.x, e4.y, e4.z, e4.w};
          uint2 wo = make_uint2(0u, 0u);
          if (wout) wo = *reinterpret_cast<const uint2*>(wout + n0);
#pragma unroll
          for (int i = 0; i < R; ++i) {
            float y[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if constexpr (KIND != BB_CLOSE) {
                y[e] = ln_elu(acc[j][i][4 * q + e] * rs[i] * ga[e] + be[e]);
              } else {   // u = xhat gamma; u = u + beta; h_k = h_{k-1} + u, all fp32, the sum kept as it is
                float u = acc[j][i][4 * q + e] * rs[i] * ga[e];
                u = u + be[e];
                y[e] = hs[j][i][4 * q + e] + u;
              }
              if constexpr (KIND != BB_OPEN) hs[j][i][4 * q + e] = y[e];
            }
            if (!wout) {
              *reinterpret_cast<uint2*>(img + (32 * i + r) * ld + n0) = make_uint2(bb_pack2(y[0], y[1]), bb_pack2(y[2], y[3]));
            } else {   // a product of two bf16 values is exact in fp32: only the additions round
              s[i] += bb_round(y[0]) * __uint_as_float(wo.x << 16);
              s[i] += bb_round(y[1]) * __uint_as_float(wo.x & 0xffff0000u);
              s[i] += bb_round(y[2]) * __uint_as_float(wo.y << 16);
              s[i] += bb_round(y[3]) * __uint_as_float(wo.y & 0xffff0000u);
            }
          }
        }
      }
  }
  if (wout) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      s[i] += __shfl_xor(s[i], 32, 64);
      if (cnt > 0 && h == 0) tab1[wave * ROWS + 32 * i + r] = s[i];
    }
  }
  __syncthreads();   // the image (the Q partials) is complete
}

// every layer of one net for the block's rows, at one geometry (<= NTW tiles per wave); leaves the rows' Q partials in tab1
template <int R, int NTW>
__device__ __forceinline__ void bb_stack(const BroBf16P& p, const float* __restrict__ prm, const uint16_t* __restrict__ pk, uint16_t* img,
                                         float* tab1, float* tab2, int wave, int lane) {
  const int W = p.W, K = p.K, NT = W >> 5;
  BbGeom g;
  g.W = W; g.ld = p.ld; g.r = lane & 31; g.h = lane >> 5; g.n = (float)W;
  g.cnt = wave < NT ? (NT - 1 - wave) / BB_NW + 1 : 0;
  g.nw = NT < BB_NW ? NT : BB_NW;
  const int KS0 = (p.in_dim + 15) >> 4, KS = W >> 4;
  const long long pstem = (long long)W * KS0 * 16, pblk = (long long)W * W;   // packed elements of the stem / of a block layer
  const long long wstem = (long long)W * p.ldin, wblk = (long long)W * W;     // floats in front of [b | gamma | beta] in the arena
  const uint16_t* wout = pk + pstem + 2 * K * pblk;                            // the output layer's row of W weights
  bb_f32x16 hs[NTW][R];
#pragma unroll
  for (int j = 0; j < NTW; ++j)
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) hs[j][i][e] = 0.f;
  const float* lay = prm;   // the current layer's start in the arena
  bb_layer<R, NTW, BB_STEM>(g, reinterpret_cast<const uint4*>(pk), KS0, lay + wstem, p.eps, K == 0 ? wout : nullptr, img, tab1, tab2, hs,
                            wave, lane);
  lay += wstem + 3 * W;
  pk += pstem;
  for (int k = 1; k <= K; ++k) {
    bb_layer<R, NTW, BB_OPEN>(g, reinterpret_cast<const uint4*>(pk), KS, lay + wblk, p.eps, nullptr, img, tab1, tab2, hs, wave, lane);
    lay += wblk + 3 * W;
    pk += pblk;
    bb_layer<R, NTW, BB_CLOSE>(g, reinterpret_cast<const uint4*>(pk), KS, lay + wblk, p.eps, k == K ? wout : nullptr, img, tab1, tab2, hs,
                               wave, lane);
    lay += wblk + 3 * W;
    pk += pblk;
  }
}

template <int R>
__global__ __launch_bounds__(64 * BB_NW) void k_bro_fwd_bf16(BroBf16P p) {
  constexpr int ROWS = 32 * R;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int net = blockIdx.y, ld = p.ld;
  const long long row0 = (long long)blockIdx.x * ROWS;
  uint16_t* img = reinterpret_cast<uint16_t*>(bb_sm);
  float* tab1 = reinterpret_cast<float*>(bb_sm + (size_t)ROWS * ld * sizeof(uint16_t));
  float* tab2 = tab1 + BB_NW * ROWS;
  // stage the fp32 input tile as bf16; rows past m and columns past in_dim (up to the next multiple of 16) become zero
  {
    const int K0 = p.in_dim, qpr = ((K0 + 15) & ~15) >> 2;
    for (int i = tid; i < ROWS * qpr; i += 64 * BB_NW) {
      const int row = i / qpr, c = (i - row * qpr) << 2;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row0 + row < p.m && c < K0) {   // c + 3 < ldx: ldx >= roundup(K0, 32)
        v = *reinterpret_cast<const float4*>(p.X + (row0 + row) * p.ldx + c);
        if (c + 1 >= K0) v.y = 0.f;
        if (c + 2 >= K0) v.z = 0.f;
        if (c + 3 >= K0) v.w = 0.f;
      }
      *reinterpret_cast<uint2*>(img + row * ld + c) = make_uint2(bb_pack2(v.x, v.y), bb_pack2(v.z, v.w));
    }
  }
  __syncthreads();
  const float* prm = p.arena + (long long)net * p.net_stride;
  const uint16_t* pk = p.packed + (long long)net * p.packed_net_stride;
  const int W = p.W;   // (block-uniform: the barriers inside are reached by every wave)
  if (W <= 256) bb_stack<R, 1>(p, prm, pk, img, tab1, tab2, wave, lane);
  else if (W <= 512) bb_stack<R, 2>(p, prm, pk, img, tab1, tab2, wave, lane);
  else if constexpr (R == 1) {
    if (W <= 768) bb_stack<1, 3>(p, prm, pk, img, tab1, tab2, wave, lane);
    else bb_stack<1, 4>(p, prm, pk, img, tab1, tab2, wave, lane);
  }
  // Q = (the row's partials in wave order) + b: column 0 of the row's 32 floats, the rest zero; 8 threads write a row
  {
    const int row = tid >> 3, quad = tid & 7, NT = W >> 5;
    if (row < ROWS && row0 + row < p.m) {
      const float qv = bb_row_total(tab1, ROWS, row, NT < BB_NW ? NT : BB_NW) + prm[p.net_stride - 32];   // [Wo (W) | bo (32)] ends a net
      float* q = p.q + ((long long)net * p.m + row0 + row) * 32;
      *reinterpret_cast<float4*>(q + 4 * quad) = make_float4(quad == 0 ? qv : 0.f, 0.f, 0.f, 0.f);
    }
  }
}

// fp32 arena -> the packed bf16 copy, one 16-byte unit (8 elements) per thread and step.  A hidden layer (K padded to 16 with zeros):
//   packed[net][layer][tile n/32][k/16][lane = 32 h + r][j] = bf16(W[32 tile + r][16 (k/16) + 8 h + j])
// the output layer (one row of W weights): packed[net][2 K + 1][k] = bf16(Wo[0][k]).  A unit's layer comes from arithmetic: the stem's
// units, then the uniform block layers by division, then the output row.
__global__ __launch_bounds__(256) void k_bro_pack_bf16(BroPackBf16P p) {
  const long long total = p.units_per_net * p.n_nets;
  for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < total; u += (long long)gridDim.x * 256) {
    const long long net = u / p.units_per_net, v = u - net * p.units_per_net;
    const float* src = p.arena + net * p.net_stride;
    int K = p.W, ldw = p.W, k0;
    long long wq = v;
    bool out = false;
    if (v < p.stem_units) {
      K = p.in_dim; ldw = p.ldin;
    } else {
      wq = v - p.stem_units;
      const long long l = wq / p.blk_units;   // 0 .. 2 K - 1: a block layer; 2 K: the output row
      out = l >= 2 * p.K;
      wq -= (out ? 2 * p.K : l) * p.blk_units;
      src += p.stem + (out ? 2 * p.K : l) * p.blk;
    }
    if (out) {
      k0 = (int)(8 * wq);
    } else {
      const int lane = (int)(wq & 63), KS = (K + 15) >> 4;
      const long long kt = wq >> 6;
      const int t = (int)(kt / KS), ks = (int)(kt - (long long)t * KS);
      k0 = 16 * ks + 8 * (lane >> 5);
      src += (long long)(32 * t + (lane & 31)) * ldw;
    }
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (k0 + 8 <= K) {
      const float4 a = *reinterpret_cast<const float4*>(src + k0), b = *reinterpret_cast<const float4*>(src + k0 + 4);
      f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (k0 + j < K) f[j] = src[k0 + j];
    }
    reinterpret_cast<uint4*>(p.packed)[u] = make_uint4(bb_pack2(f[0], f[1]), bb_pack2(f[2], f[3]), bb_pack2(f[4], f[5]), bb_pack2(f[6], f[7]));
  }
}

// ---- host side
struct BroBf16Layout {
  int in_dim, ldin, W, K, n_nets, r, ld;          // r: row tiles per block; ld: the image's row length in bf16 elements
  int64_t stem, blk, net_stride;                   // the arena law, floats: layer 0, a block layer, a net
  int64_t p_stem, p_blk, packed_net_elems;         // the packed copy, bf16 elements
};

static size_t bb_lds_bytes(int ld, int r) { return (size_t)32 * r * ld * sizeof(uint16_t) + (size_t)2 * BB_NW * 32 * r * sizeof(float); }

// the layout of an eligible stack -> *out; false: not eligible.  The arena's size is pqlk_bro_param_floats', asked of the library itself.
static bool bb_layout(int32_t in_dim, int32_t width, int32_t blocks, int32_t n_nets, BroBf16Layout* out) {
  if (!pqlk_bro_ok(in_dim, width, blocks, n_nets)) return false;
  BroBf16Layout d = {};
  d.in_dim = in_dim; d.ldin = (int)pqlk_ld(in_dim); d.W = width; d.K = blocks; d.n_nets = n_nets;
  d.stem = (int64_t)width * d.ldin + 3 * width;
  d.blk = (int64_t)width * width + 3 * width;
  d.net_stride = pqlk_bro_param_floats(in_dim, width, blocks, n_nets) / n_nets;
  if (d.net_stride != d.stem + 2 * blocks * d.blk + width + 32) return false;
  const int kin = (in_dim + 15) & ~15;
  d.p_stem = (int64_t)width * kin;
  d.p_blk = (int64_t)width * width;
  d.packed_net_elems = d.p_stem + 2 * blocks * d.p_blk + width;
  d.ld = (kin > width ? kin : width) + BB_PAD;
  d.r = width <= BB_MAX_R2_WIDTH && bb_lds_bytes(d.ld, 2) <= (size_t)BB_LDS_MAX ? 2 : 1;
  if (bb_lds_bytes(d.ld, d.r) > (size_t)BB_LDS_MAX) return false;   // (never: in_dim <= 1248 is an 82 KB image with its tables)
  *out = d;
  return true;
}

extern "C" int pqlk_bro_bf16_ok(int32_t in_dim, int32_t width, int32_t blocks, int32_t n_nets) {
  BroBf16Layout d;
  return bb_layout(in_dim, width, blocks, n_nets, &d) ? 1 : 0;
}

extern "C" int64_t pqlk_bro_packed_bf16_elems(int32_t in_dim, int32_t width, int32_t blocks, int32_t n_nets) {
  BroBf16Layout d;
  return bb_layout(in_dim, width, blocks, n_nets, &d) ? d.packed_net_elems * d.n_nets : 0;
}

extern "C" int pqlk_bro_pack_bf16(int32_t in_dim, int32_t width, int32_t blocks, int32_t n_nets, const float* arena, uint16_t* packed,
                                  pqlk_stream_t stream) {
  PQLK_REQUIRE(arena && packed, PQLK_E_NULL);
  BroBf16Layout d;
  PQLK_REQUIRE(bb_layout(in_dim, width, blocks, n_nets, &d), PQLK_E_SHAPE);
  PQLK_REQUIRE(pqlk_aligned16(arena) && pqlk_aligned16(packed), PQLK_E_ALIGN);
  BroPackBf16P p = {};
  p.arena = arena; p.packed = packed; p.net_stride = d.net_stride;
  p.units_per_net = d.packed_net_elems / 8; p.stem_units = d.p_stem / 8; p.blk_units = d.p_blk / 8;
  p.stem = d.stem; p.blk = d.blk;
  p.in_dim = d.in_dim; p.ldin = d.ldin; p.W = d.W; p.K = d.K; p.n_nets = d.n_nets;
  const int64_t total = p.units_per_net * d.n_nets;
  const unsigned grid = (unsigned)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(k_bro_pack_bf16, dim3(grid), dim3(256), 0, pqlk_s(stream), p);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

extern "C" int pqlk_bro_forward_bf16(int32_t in_dim, int32_t width, int32_t blocks, int32_t n_nets, const float* arena,
                                     const uint16_t* packed, const float* x, int64_t ldx, int64_t m, float eps, float* q_out,
                                     pqlk_stream_t stream) {
  PQLK_REQUIRE(arena && packed && x && q_out, PQLK_E_NULL);
  BroBf16Layout d;
  PQLK_REQUIRE(bb_layout(in_dim, width, blocks, n_nets, &d), PQLK_E_SHAPE);
  PQLK_REQUIRE(m > 0 && m < (1LL << 30), PQLK_E_SHAPE);
  PQLK_REQUIRE(ldx % 32 == 0 && ldx >= d.ldin, PQLK_E_ALIGN);
  PQLK_REQUIRE(pqlk_aligned16(arena) && pqlk_aligned16(packed) && pqlk_aligned16(x) && pqlk_aligned16(q_out), PQLK_E_ALIGN);
  BroBf16P p = {};
  p.X = x; p.arena = arena; p.packed = packed; p.q = q_out;
  p.net_stride = d.net_stride; p.packed_net_stride = d.packed_net_elems;
  p.in_dim = d.in_dim; p.ldin = d.ldin; p.W = d.W; p.K = d.K; p.m = (int)m; p.ldx = (int)ldx; p.ld = d.ld; p.eps = eps;
  static PqlkPerDeviceOnce attr_once;
  if (int arc = attr_once.run([&] {
        const void* ks[2] = {reinterpret_cast<const void*>(&k_bro_fwd_bf16<1>), reinterpret_cast<const void*>(&k_bro_fwd_bf16<2>)};
        for (const void* k : ks) {
          hipError_t err = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, BB_LDS_MAX);
          if (err != hipSuccess) return -(int)err;
        }
        return 0;
      }))
    return arc;
  dim3 grid((unsigned)((m + 32 * d.r - 1) / (32 * d.r)), (unsigned)d.n_nets), block(64 * BB_NW);
  if (d.r == 2) hipLaunchKernelGGL(k_bro_fwd_bf16<2>, grid, block, bb_lds_bytes(d.ld, 2), pqlk_s(stream), p);
  else hipLaunchKernelGGL(k_bro_fwd_bf16<1>, grid, block, bb_lds_bytes(d.ld, 1), pqlk_s(stream), p);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}
