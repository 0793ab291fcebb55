// Forward-only bf16-MFMA sibling of the whole-stack LayerNorm critic forward (fwd_ln.hip), for the forwards nothing goes back through:
// the target critic of DDPG / SAC with algo.critic_target_dtype=bfloat16.  One launch computes, for both nets (blockIdx.y),
// x -> [Linear -> LayerNorm(eps, affine) -> ELU] x H -> Linear -> Q.  The law is written op by op in include/pqlk.h ("bf16 LayerNorm
// law"); fwd_ln.hip, ln.hip, fwd_bf16.hip, gemm.hip and fused.h are untouched, and nothing here writes a stash.
//
// Work split: a block of 8 waves owns 32 R batch rows through every layer, their current activations in ONE bf16 LDS image
// [row][feature] (row length = widest layer + 8 elements = 16 B of padding) that every layer overwrites in place.  R = 2 where no
// hidden layer is wider than 512 (the default [512, 512, 256]: 66.5 KB + a 4 KB table, two blocks per CU), R = 1 otherwise (a
// 1024-wide layer: 66 KB + 2 KB); either way a wave holds at most 64 accumulator registers.
//
// Linear: v_mfma_f32_32x32x16_bf16 with the WEIGHT tile as the A operand and the activation tile from LDS as B, so a lane holds one
// batch row (lane = 32 h + r: row r) and four consecutive output features sit in four consecutive accumulator registers.  Wave w takes
// the 32-feature tiles w, w + 8, ... (at most 2 at R = 2, 4 at R = 1).  Weights come from the packed, fragment-ordered bf16 copy
// (pqlk_lnmlp_pack_bf16): a wave's 64 16-byte loads of one k step are one contiguous 1 KB run, fetched one k step ahead of the MFMAs
// that use them; activations come with one ds_read_b128 per row tile and k step.
//
// LayerNorm from registers: z = acc + b never leaves the accumulator registers.  Every lane sums its features of its row in register
// order, the lane pair (r, r + 32) folds its two halves, and the wave writes one partial per row into a [wave][row] LDS table; behind
// a barrier (which is also the one after which nobody reads the layer's input any more) every lane adds the partials of its row in
// wave order.  The same again for the squared deviations, through a second table.  Then xhat * gamma + beta, ELU, RNE, and four
// features go as one ds_write_b64 into the image.  The output layer (width 1) rides on the last epilogue: the rounded activations are
// multiplied with the bf16 output weights in the registers and summed through the first table, so nothing but Q leaves the block.
// Three barriers per hidden layer, no atomics, no scratch; a row's bits depend on neither m, its position in the batch, nor the launch.
//
// Dropout (DoubleQDropoutLayerNorm's target with algo.critic_target_dtype=bfloat16; pqlk_lnmlp_drop_forward_bf16): lb_layer and the
// kernel end in a parameter pack that is either empty (the plain kernel: the instructions and the bits of pqlk_lnmlp_forward_bf16 are
// what they were) or one LnDrop.  Accumulator registers 4g .. 4g+3 of a lane are four consecutive, 4-aligned features of one row:
// exactly one Philox4x32-10 block of the mask law.  So behind z = acc + b the lane generates that block in registers and leaves
// u = keep ? z * s : 0 in the accumulators, in front of the first row-sum table; everything behind it runs on u as it ran on z.  The
// mask's row index is the row's index in the whole batch (row0 + its row of the block), the tag tag_base | (net << 4) | layer.
#include "lnrow.h"
#include "lndrop.h"

constexpr int LB_NW = 8;                 // waves per block
constexpr int LB_LDS_MAX = 160 * 1024;
constexpr int LB_PAD = 8;                // bf16 elements of row padding in LDS (16 B: consecutive rows start 4 banks apart)
constexpr int LB_MAX_R2_WIDTH = 512;     // widest hidden layer at R = 2: 2 tiles x 2 row tiles x 16 = 64 accumulator registers

typedef __bf16 lb_bf16x8 __attribute__((ext_vector_type(8)));
typedef float lb_f32x16 __attribute__((ext_vector_type(16)));

// fp32 -> bf16, round to nearest even, ties included; NaN stays a (quiet) NaN, overflow goes to +-inf
__device__ __forceinline__ unsigned lb_rne(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
__device__ __forceinline__ unsigned lb_pack2(float lo, float hi) { return lb_rne(lo) | (lb_rne(hi) << 16); }
__device__ __forceinline__ float lb_round(float f) { return __uint_as_float(lb_rne(f) << 16); }   // the fp32 value of bf16(f)

struct LnBf16P {
  const float* X; const float* arena; const uint16_t* packed; float* q;
  int64_t net_stride, packed_net_stride;                                                    // floats / bf16 elements
  int64_t b_off[PQLK_MAX_LAYERS], g_off[PQLK_MAX_LAYERS], be_off[PQLK_MAX_LAYERS];          // floats inside a net of the arena
  int64_t p_off[PQLK_MAX_LAYERS];                                                           // bf16 elements inside a net of the packed copy
  int dims[PQLK_MAX_LAYERS + 1];
  int n_layers, m, ldx, ld;
  float eps;
};

struct LnPackBf16P {
  const float* arena; uint16_t* packed;
  int64_t net_stride, units_per_net;                          // units = 16 B = 8 bf16
  int64_t w_off[PQLK_MAX_LAYERS], u_off[PQLK_MAX_LAYERS];     // weight offset (floats) / first unit of the layer, inside a net
  int dims[PQLK_MAX_LAYERS + 1];
  int n_layers, n_nets;
};

extern __shared__ __attribute__((aligned(16))) unsigned char lb_sm[];

// what lb_layer's dropout form gets: the mask constants with the tag of its (net, layer), and the block's first batch row
struct LbDrop {
  LnDrop d;
  uint32_t row0;
};
__device__ __forceinline__ LbDrop lb_drop_of() { return LbDrop{}; }
__device__ __forceinline__ LbDrop lb_drop_of(const LbDrop& d) { return d; }
__device__ __forceinline__ LbDrop lb_drop_at(const LnDrop& d, int net, int layer, long long row0) {
  return LbDrop{ln_drop_at(d, net, layer), (uint32_t)row0};
}

// the sum of a row's partials, one per wave that holds features, in wave order
__device__ __forceinline__ float lb_row_total(const float* tab, int rows, int row, int nw) {
  float t = tab[row];
  for (int w = 1; w < nw; ++w) t += tab[w * rows + row];
  return t;
}

// One hidden layer for the block's 32 R rows: img holds a~ (K columns, zeros past the input's width up to a multiple of 16) and is
// overwritten with a~ of the next layer (N columns) -- or, with wout (the last hidden layer), the rows' Q partials are left in tab1.
// Every wave of the block runs through the same barriers; ends behind the one after which the image (or tab1) is complete.
template <int R, int NTW, typename... D>
__device__ __forceinline__ void lb_layer(const uint4* __restrict__ w, int KS, int N, const float* __restrict__ bias,
                                         const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                         const uint16_t* __restrict__ wout, uint16_t* img, int ld, float* tab1, float* tab2, int wave,
                                         int lane, D... dr) {
  constexpr int ROWS = 32 * R;
  const int r = lane & 31, h = lane >> 5, NT = N >> 5;
  const int cnt = wave < NT ? (NT - 1 - wave) / LB_NW + 1 : 0;   // this wave's tiles: wave, wave + 8, ... (<= NTW)
  const int nw = NT < LB_NW ? NT : LB_NW;                         // the waves that hold features
  const float n = (float)N;
  lb_f32x16 acc[NTW][R];
#pragma unroll
  for (int j = 0; j < NTW; ++j)
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][i][e] = 0.f;
  if (cnt > 0) {
    const uint4* wp = w + (long long)wave * KS * 64 + lane;   // tile t, k step ks: 64 fragments at (t KS + ks) 64
    const long long tstep = (long long)LB_NW * KS * 64;
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
            acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(lb_bf16x8, wf[j]), __builtin_bit_cast(lb_bf16x8, af[i]),
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
      for (int g = 0; g < 4; ++g) {
        const int n0 = 32 * (wave + LB_NW * j) + 8 * g + 4 * h;   // accumulator registers 4g .. 4g+3 = features n0 .. n0+3 of row r
        const float4 b4 = *reinterpret_cast<const float4*>(bias + n0);
#pragma unroll
        for (int i = 0; i < R; ++i) {
          acc[j][i][4 * g] += b4.x; acc[j][i][4 * g + 1] += b4.y; acc[j][i][4 * g + 2] += b4.z; acc[j][i][4 * g + 3] += b4.w;
          if constexpr (ln_has<LbDrop, D...>) {   // u = keep ? z * s : 0: the four registers are one Philox block of row row0 + 32 i + r
            const LbDrop d = lb_drop_of(dr...);
            const float4 u = ln_drop4(d.d, d.row0 + (uint32_t)(32 * i + r), n0,
                                      make_float4(acc[j][i][4 * g], acc[j][i][4 * g + 1], acc[j][i][4 * g + 2], acc[j][i][4 * g + 3]));
            acc[j][i][4 * g] = u.x; acc[j][i][4 * g + 1] = u.y; acc[j][i][4 * g + 2] = u.z; acc[j][i][4 * g + 3] = u.w;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) s[i] += acc[j][i][4 * g + e];
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
      const float mu = lb_row_total(tab1, ROWS, 32 * i + r, nw) / n;
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
  // ---- y = elu(d rstd gamma + beta), a~ = bf16(y): into the image, or multiplied out with the output layer's weights
  float rs[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    rs[i] = 0.f;
    s[i] = 0.f;
  }
  if (cnt > 0) {
#pragma unroll
    for (int i = 0; i < R; ++i) rs[i] = 1.0f / sqrtf(lb_row_total(tab2, ROWS, 32 * i + r, nw) / n + eps);
#pragma unroll
    for (int j = 0; j < NTW; ++j)
      if (j < cnt) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n0 = 32 * (wave + LB_NW * j) + 8 * g + 4 * h;
          const float4 g4 = *reinterpret_cast<const float4*>(gamma + n0);
          const float4 e4 = *reinterpret_cast<const float4*>(beta + n0);
          uint2 wo = make_uint2(0u, 0u);
          if (wout) wo = *reinterpret_cast<const uint2*>(wout + n0);
#pragma unroll
          for (int i = 0; i < R; ++i) {
            const float y0 = ln_elu(acc[j][i][4 * g] * rs[i] * g4.x + e4.x), y1 = ln_elu(acc[j][i][4 * g + 1] * rs[i] * g4.y + e4.y);
            const float y2 = ln_elu(acc[j][i][4 * g + 2] * rs[i] * g4.z + e4.z), y3 = ln_elu(acc[j][i][4 * g + 3] * rs[i] * g4.w + e4.w);
            if (!wout) {
              *reinterpret_cast<uint2*>(img + (32 * i + r) * ld + n0) = make_uint2(lb_pack2(y0, y1), lb_pack2(y2, y3));
            } else {   // a product of two bf16 values is exact in fp32: only the additions round
              s[i] += lb_round(y0) * __uint_as_float(wo.x << 16);
              s[i] += lb_round(y1) * __uint_as_float(wo.x & 0xffff0000u);
              s[i] += lb_round(y2) * __uint_as_float(wo.y << 16);
              s[i] += lb_round(y3) * __uint_as_float(wo.y & 0xffff0000u);
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

template <int R, typename... D>
__global__ __launch_bounds__(64 * LB_NW) void k_lnmlp_fwd_bf16(LnBf16P p, D... dr) {
  constexpr int ROWS = 32 * R;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int net = blockIdx.y, H = p.n_layers - 1, ld = p.ld;
  const long long row0 = (long long)blockIdx.x * ROWS;
  uint16_t* img = reinterpret_cast<uint16_t*>(lb_sm);
  float* tab1 = reinterpret_cast<float*>(lb_sm + (size_t)ROWS * ld * sizeof(uint16_t));
  float* tab2 = tab1 + LB_NW * ROWS;
  // stage the fp32 input tile as bf16; rows past m and columns past dims[0] (up to the next multiple of 16) become zero
  {
    const int K0 = p.dims[0], qpr = ((K0 + 15) & ~15) >> 2;
    for (int i = tid; i < ROWS * qpr; i += 64 * LB_NW) {
      const int row = i / qpr, c = (i - row * qpr) << 2;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row0 + row < p.m && c < K0) {   // c + 3 < ldx: ldx >= roundup(K0, 32)
        v = *reinterpret_cast<const float4*>(p.X + (row0 + row) * p.ldx + c);
        if (c + 1 >= K0) v.y = 0.f;
        if (c + 2 >= K0) v.z = 0.f;
        if (c + 3 >= K0) v.w = 0.f;
      }
      *reinterpret_cast<uint2*>(img + row * ld + c) = make_uint2(lb_pack2(v.x, v.y), lb_pack2(v.z, v.w));
    }
  }
  __syncthreads();
  const float* prm = p.arena + (long long)net * p.net_stride;
  const uint16_t* pk = p.packed + (long long)net * p.packed_net_stride;
  for (int l = 0; l < H; ++l) {
    const int KS = (p.dims[l] + 15) >> 4, N = p.dims[l + 1];
    const uint4* w = reinterpret_cast<const uint4*>(pk + p.p_off[l]);
    const float *bias = prm + p.b_off[l], *ga = prm + p.g_off[l], *be = prm + p.be_off[l];
    const uint16_t* wout = l == H - 1 ? pk + p.p_off[H] : nullptr;
    const int ntw = ((N >> 5) + LB_NW - 1) / LB_NW;   // (block-uniform: the barriers inside are reached by every wave)
    // (dr: empty, or the launch's LnDrop, which gets the tag of this (net, layer) and the block's first row)
#define LB_LAYER(R_, NTW) lb_layer<R_, NTW>(w, KS, N, bias, ga, be, p.eps, wout, img, ld, tab1, tab2, wave, lane, lb_drop_at(dr, net, l, row0)...)
    if (ntw == 1) LB_LAYER(R, 1);
    else if (ntw == 2) LB_LAYER(R, 2);
    else if constexpr (R == 1) {
      if (ntw == 3) LB_LAYER(1, 3);
      else LB_LAYER(1, 4);
    }
#undef LB_LAYER
  }
  // Q = (the row's partials in wave order) + b: column 0 of the row's 32 floats, the rest zero; 8 threads write a row
  {
    const int row = tid >> 3, quad = tid & 7, NT = p.dims[H] >> 5;
    if (row < ROWS && row0 + row < p.m) {
      const float qv = lb_row_total(tab1, ROWS, row, NT < LB_NW ? NT : LB_NW) + prm[p.b_off[H]];
      float* q = p.q + ((long long)net * p.m + row0 + row) * 32;
      *reinterpret_cast<float4*>(q + 4 * quad) = make_float4(quad == 0 ? qv : 0.f, 0.f, 0.f, 0.f);
    }
  }
}

// fp32 arena -> the packed bf16 copy, one 16-byte unit (8 elements) per thread and step.  A hidden layer (K padded to 16 with zeros):
//   packed[net][layer][tile n/32][k/16][lane = 32 h + r][j] = bf16(W[32 tile + r][16 (k/16) + 8 h + j])
// the output layer (one row of dims[H] weights): packed[net][H][k] = bf16(W[0][k])
__global__ __launch_bounds__(256) void k_lnmlp_pack_bf16(LnPackBf16P p) {
  const long long total = p.units_per_net * p.n_nets;
  for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < total; u += (long long)gridDim.x * 256) {
    const long long net = u / p.units_per_net, v = u - net * p.units_per_net;
    int l = 0;
    for (int k = 1; k < p.n_layers; ++k)
      if (v >= p.u_off[k]) l = k;
    const long long wq = v - p.u_off[l];
    const int K = p.dims[l];
    const float* src;
    int k0;
    if (l == p.n_layers - 1) {
      k0 = (int)(8 * wq);
      src = p.arena + net * p.net_stride + p.w_off[l];
    } else {
      const int lane = (int)(wq & 63), KS = (K + 15) >> 4;
      const long long kt = wq >> 6;
      const int t = (int)(kt / KS), ks = (int)(kt - (long long)t * KS);
      k0 = 16 * ks + 8 * (lane >> 5);
      src = p.arena + net * p.net_stride + p.w_off[l] + (long long)(32 * t + (lane & 31)) * ((K + 31) & ~31);
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
    reinterpret_cast<uint4*>(p.packed)[u] = make_uint4(lb_pack2(f[0], f[1]), lb_pack2(f[2], f[3]), lb_pack2(f[4], f[5]), lb_pack2(f[6], f[7]));
  }
}

// ---- host side
struct LnBf16Layout {
  int n_layers, n_nets, r, ld;                                  // r: row tiles per block; ld: the image's row length in bf16 elements
  int dims[PQLK_MAX_LAYERS + 1];
  int64_t lin_off[PQLK_MAX_LAYERS], gamma_off[PQLK_MAX_LAYERS], beta_off[PQLK_MAX_LAYERS], net_stride;   // the arena law, floats
  int64_t p_off[PQLK_MAX_LAYERS], packed_net_elems;             // the packed copy, bf16 elements
};

static size_t lb_lds_bytes(int ld, int r) { return (size_t)32 * r * ld * sizeof(uint16_t) + (size_t)2 * LB_NW * 32 * r * sizeof(float); }

// the layout of an eligible descriptor -> *out; false: not eligible.  The arena law is pqlk_lnmlp_offsets', asked of the library itself.
static bool lb_layout(const PqlMlpDesc* m, LnBf16Layout* out) {
  if (!m || !pqlk_lnmlp_ok(m)) return false;
  LnBf16Layout d = {};
  d.n_layers = m->n_layers; d.n_nets = m->n_nets;
  d.net_stride = pqlk_lnmlp_param_floats(m) / m->n_nets;
  int cols = (m->dims[0] + 15) & ~15, widest = 0;
  int64_t e = 0;
  for (int l = 0; l < d.n_layers; ++l) {
    d.dims[l] = m->dims[l]; d.dims[l + 1] = m->dims[l + 1];
    if (pqlk_lnmlp_offsets(m, l, &d.lin_off[l], &d.gamma_off[l], &d.beta_off[l]) != PQLK_OK) return false;
    d.p_off[l] = e;
    if (l < d.n_layers - 1) {
      e += (int64_t)m->dims[l + 1] * ((m->dims[l] + 15) & ~15);
      widest = widest > m->dims[l + 1] ? widest : m->dims[l + 1];
    } else {
      e += m->dims[l];
    }
  }
  d.packed_net_elems = e;
  cols = cols > widest ? cols : widest;
  d.ld = cols + LB_PAD;
  d.r = widest <= LB_MAX_R2_WIDTH && lb_lds_bytes(d.ld, 2) <= (size_t)LB_LDS_MAX ? 2 : 1;
  if (lb_lds_bytes(d.ld, d.r) > (size_t)LB_LDS_MAX) return false;   // (bounds the input width: a 32-row bf16 image and its tables)
  *out = d;
  return true;
}

extern "C" int pqlk_lnmlp_bf16_ok(const PqlMlpDesc* desc) {
  LnBf16Layout d;
  return lb_layout(desc, &d) ? 1 : 0;
}

extern "C" int64_t pqlk_lnmlp_packed_bf16_elems(const PqlMlpDesc* desc) {
  LnBf16Layout d;
  return lb_layout(desc, &d) ? d.packed_net_elems * d.n_nets : 0;
}

extern "C" int pqlk_lnmlp_pack_bf16(const PqlMlpDesc* desc, const float* arena, uint16_t* packed, pqlk_stream_t stream) {
  PQLK_REQUIRE(desc && arena && packed, PQLK_E_NULL);
  LnBf16Layout d;
  PQLK_REQUIRE(lb_layout(desc, &d), PQLK_E_SHAPE);
  PQLK_REQUIRE(pqlk_aligned16(arena) && pqlk_aligned16(packed), PQLK_E_ALIGN);
  LnPackBf16P p = {};
  p.arena = arena; p.packed = packed; p.net_stride = d.net_stride; p.units_per_net = d.packed_net_elems / 8;
  p.n_layers = d.n_layers; p.n_nets = d.n_nets;
  for (int l = 0; l <= d.n_layers; ++l) p.dims[l] = d.dims[l];
  for (int l = 0; l < d.n_layers; ++l) {
    p.w_off[l] = d.lin_off[l]; p.u_off[l] = d.p_off[l] / 8;
  }
  const int64_t total = p.units_per_net * d.n_nets;
  const unsigned blocks = (unsigned)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(k_lnmlp_pack_bf16, dim3(blocks), dim3(256), 0, pqlk_s(stream), p);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

// the one dispatch of the plain entry (an empty pack) and the dropout entry (one LnDrop, its tag the launch's tag_base)
template <typename... D>
static int lb_forward(const LnBf16Layout& d, const float* arena, const uint16_t* packed, const float* x, int64_t ldx, int64_t m, float eps,
                      float* q_out, pqlk_stream_t stream, D... dr) {
  PQLK_REQUIRE(ldx % 32 == 0 && ldx >= pqlk_ld(d.dims[0]), PQLK_E_ALIGN);
  PQLK_REQUIRE(pqlk_aligned16(arena) && pqlk_aligned16(packed) && pqlk_aligned16(x) && pqlk_aligned16(q_out), PQLK_E_ALIGN);
  const int L = d.n_layers;
  LnBf16P p = {};
  p.X = x; p.arena = arena; p.packed = packed; p.q = q_out;
  p.net_stride = d.net_stride; p.packed_net_stride = d.packed_net_elems;
  p.n_layers = L; p.m = (int)m; p.ldx = (int)ldx; p.ld = d.ld; p.eps = eps;
  for (int l = 0; l <= L; ++l) p.dims[l] = d.dims[l];
  for (int l = 0; l < L; ++l) {
    p.b_off[l] = d.lin_off[l] + (int64_t)d.dims[l + 1] * pqlk_ld(d.dims[l]);
    p.p_off[l] = d.p_off[l];
    if (l < L - 1) { p.g_off[l] = d.gamma_off[l]; p.be_off[l] = d.beta_off[l]; }
  }
  static PqlkPerDeviceOnce attr_once;   // (one per instantiation: each entry raises the limit of its own two kernels)
  if (int arc = attr_once.run([&] {
        const void* ks[2] = {reinterpret_cast<const void*>(&k_lnmlp_fwd_bf16<1, D...>), reinterpret_cast<const void*>(&k_lnmlp_fwd_bf16<2, D...>)};
        for (const void* k : ks) {
          hipError_t err = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, LB_LDS_MAX);
          if (err != hipSuccess) return -(int)err;
        }
        return 0;
      }))
    return arc;
  dim3 grid((unsigned)((m + 32 * d.r - 1) / (32 * d.r)), (unsigned)d.n_nets), block(64 * LB_NW);
  if (d.r == 2) hipLaunchKernelGGL((k_lnmlp_fwd_bf16<2, D...>), grid, block, lb_lds_bytes(d.ld, 2), pqlk_s(stream), p, dr...);
  else hipLaunchKernelGGL((k_lnmlp_fwd_bf16<1, D...>), grid, block, lb_lds_bytes(d.ld, 1), pqlk_s(stream), p, dr...);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

extern "C" int pqlk_lnmlp_forward_bf16(const PqlMlpDesc* desc, const float* arena, const uint16_t* packed, const float* x, int64_t ldx,
                                       int64_t m, float eps, float* q_out, pqlk_stream_t stream) {
  PQLK_REQUIRE(desc && arena && packed && x && q_out, PQLK_E_NULL);
  LnBf16Layout d;
  PQLK_REQUIRE(lb_layout(desc, &d) && m > 0 && m < (1LL << 30), PQLK_E_SHAPE);
  return lb_forward(d, arena, packed, x, ldx, m, eps, q_out, stream);
}

extern "C" int pqlk_lnmlp_drop_forward_bf16(const PqlMlpDesc* desc, const float* arena, const uint16_t* packed, const float* x, int64_t ldx,
                                            int64_t m, float eps, float p, uint64_t seed, uint64_t tag_base, float* q_out,
                                            pqlk_stream_t stream) {
  PQLK_REQUIRE(desc && arena && packed && x && q_out, PQLK_E_NULL);
  LnBf16Layout d;
  PQLK_REQUIRE(lb_layout(desc, &d) && m > 0 && m < (1LL << 30), PQLK_E_SHAPE);
  LnDrop dr;
  PQLK_REQUIRE(ln_drop_make_stack(p, seed, tag_base, m, d.n_nets, d.n_layers - 1, &dr), PQLK_E_SHAPE);
  return lb_forward(d, arena, packed, x, ldx, m, eps, q_out, stream, dr);
}
