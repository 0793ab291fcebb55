// Forward-only MLP stack on bf16 MFMA (gfx950): the V-learner's two no-gradient forwards (target policy, target twin critic)
// with `algo.target_dtype=bfloat16`.  The fp32 kernels of gemm.hip / fused.h are untouched; nothing here carries a gradient.
//
// The numerical law ("bf16 law"), for every net of the descriptor:
//   1. x~ = bf16(x[:, :dims[0]]), round to nearest even; columns [dims[0], ldx) are ignored
//   2. W~_l = bf16(W_l) for every layer, the output layer included (RNE); biases stay fp32
//   3. z_l = sum_k a~_{l-1,k} W~_l[j,k] + b_l[j], accumulated in fp32 (the MFMA's own k order, then the bias)
//   4. hidden layers: a_l = bf16(elu(z_l)), ELU in fp32 exactly like fused_elu (x > 0 ? x : __expf(x) - 1), RNE with ties
//   5. output layer: z_L stays fp32, out_act in fp32 exactly like pqlk_mlp_forward, written as fp32 with zero pad columns
//   6. NaN / Inf propagate; a row's bits depend on neither B, its position in the batch, nor the launch
//
// Orientation: D[n][m] = sum_k W[n][k] X[m][k] with the WEIGHT as the MFMA's A operand and the activation tile as B, so the
// batch row sits on the lane and four consecutive output features in four consecutive accumulator registers: the epilogue
// packs them to 8 bytes of bf16 and writes them with one ds_write_b64 into the [row][feature] image the next layer reads
// back with ds_read_b128 -- both operands use the same "row r, k = 8 h + j" lane map (lane = 32 h + r).
#include "pqlk_common.h"

constexpr int BF_NW = 8;           // waves per block
constexpr int BF_LDS_MAX = 160 * 1024;
constexpr int BF_PAD = 8;          // bf16 elements of row padding in LDS (16 B: rows land on different 4-bank slots)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16b __attribute__((ext_vector_type(16)));

// fp32 -> bf16, round to nearest even, ties included; NaN stays a (quiet) NaN, overflow goes to +-inf
__device__ __forceinline__ unsigned bf16_rne(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
__device__ __forceinline__ unsigned bf16_pack2(float lo, float hi) { return bf16_rne(lo) | (bf16_rne(hi) << 16); }
__device__ __forceinline__ float bf16_elu(float x) { return x > 0.f ? x : __expf(x) - 1.f; }

struct Bf16P {
  const float* X; const float* params; const uint16_t* packed; const float* draw;
  float* out; float* out2;
  long long net_stride, packed_net_stride;
  long long b_off[PQLK_MAX_LAYERS], p_off[PQLK_MAX_LAYERS];   // bias offset (floats) / packed offset (elements) inside a net
  int dims[PQLK_MAX_LAYERS + 1];
  int n_layers, B, ldx, ld_out, ld_out2, lds_ld, out_act;
  float noise_std, noise_clip;
};

struct PackBf16P {
  const float* params; uint16_t* packed;
  long long net_stride, units_per_net;                        // units = 16-B fragments (8 bf16)
  long long w_off[PQLK_MAX_LAYERS], u_off[PQLK_MAX_LAYERS];   // weight offset (floats) / first unit of the layer inside a net
  int dims[PQLK_MAX_LAYERS + 1];
  int n_layers, n_nets;
};

extern __shared__ __attribute__((aligned(16))) unsigned char bf_sm[];

__device__ __forceinline__ f32x16b bf_mfma(const uint4& a, const uint4& b, f32x16b c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// NTW tiles of 32 output features x MT tiles of 32 rows: z = W~ a~ + b, a = bf16(elu(z)) -> the next layer's LDS image
template <int MT, int NTW>
__device__ __forceinline__ void bf_hidden_tiles(const uint4* __restrict__ w, int KS, const uint16_t* in, uint16_t* outb, int ld,
                                                const float* __restrict__ bias, int t, int lane) {
  const int r = lane & 31, h = lane >> 5;
  f32x16b acc[NTW][MT];
#pragma unroll
  for (int j = 0; j < NTW; ++j)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][i][e] = 0.f;
  const uint4* wp = w + (long long)t * KS * 64 + lane;
  const uint16_t* ap = in + r * ld + 8 * h;
  for (int ks = 0; ks < KS; ++ks) {
    uint4 wf[NTW], af[MT];
#pragma unroll
    for (int j = 0; j < NTW; ++j) wf[j] = wp[((long long)j * KS + ks) * 64];
#pragma unroll
    for (int i = 0; i < MT; ++i) af[i] = *reinterpret_cast<const uint4*>(ap + 32 * i * ld + 16 * ks);
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[j][i] = bf_mfma(wf[j], af[i], acc[j][i]);
  }
#pragma unroll
  for (int j = 0; j < NTW; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n0 = 32 * (t + j) + 8 * g + 4 * h;   // accumulator registers 4g .. 4g+3 = features n0 .. n0+3 of row r
      const float4 b4 = *reinterpret_cast<const float4*>(bias + n0);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        uint2 o;
        o.x = bf16_pack2(bf16_elu(acc[j][i][4 * g] + b4.x), bf16_elu(acc[j][i][4 * g + 1] + b4.y));
        o.y = bf16_pack2(bf16_elu(acc[j][i][4 * g + 2] + b4.z), bf16_elu(acc[j][i][4 * g + 3] + b4.w));
        *reinterpret_cast<uint2*>(outb + (32 * i + r) * ld + n0) = o;
      }
    }
}

template <int MT>
__global__ __launch_bounds__(64 * BF_NW) void k_mlp_fwd_bf16(Bf16P p) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int net = blockIdx.y, L = p.n_layers, ld = p.lds_ld;
  const long long row0 = (long long)blockIdx.x * (32 * MT);
  uint16_t* buf0 = reinterpret_cast<uint16_t*>(bf_sm);
  uint16_t* buf1 = buf0 + 32 * MT * ld;
  // stage the fp32 input tile as bf16; rows past B and columns past dims[0] become zero (never a product with what is there)
  {
    const int K0 = p.dims[0], qpr = ((K0 + 15) & ~15) >> 2;
    for (int i = tid; i < 32 * MT * qpr; i += 64 * BF_NW) {
      const int row = i / qpr, c = (i - row * qpr) << 2;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row0 + row < p.B && c < K0) {   // c + 3 < ldx: ldx >= roundup(K0, 32)
        v = *reinterpret_cast<const float4*>(p.X + (row0 + row) * p.ldx + c);
        if (c + 1 >= K0) v.y = 0.f;
        if (c + 2 >= K0) v.z = 0.f;
        if (c + 3 >= K0) v.w = 0.f;
      }
      uint2 o;
      o.x = bf16_pack2(v.x, v.y); o.y = bf16_pack2(v.z, v.w);
      *reinterpret_cast<uint2*>(buf0 + row * ld + c) = o;
    }
  }
  __syncthreads();
  const uint16_t* pk = p.packed + (long long)net * p.packed_net_stride;
  const float* prm = p.params + (long long)net * p.net_stride;
  for (int l = 0; l + 1 < L; ++l) {
    const uint16_t* in = (l & 1) ? buf1 : buf0;
    uint16_t* outb = (l & 1) ? buf0 : buf1;
    const int KS = (p.dims[l] + 15) >> 4, NT = p.dims[l + 1] >> 5;
    const uint4* w = reinterpret_cast<const uint4*>(pk + p.p_off[l]);
    const float* bias = prm + p.b_off[l];
    if (NT >= 2 * BF_NW) {   // wide layer: two feature tiles share every activation fragment read
      for (int t = 2 * wave; t < NT; t += 2 * BF_NW) {
        if (t + 1 < NT) bf_hidden_tiles<MT, 2>(w, KS, in, outb, ld, bias, t, lane);
        else bf_hidden_tiles<MT, 1>(w, KS, in, outb, ld, bias, t, lane);
      }
    } else {
      for (int t = wave; t < NT; t += BF_NW) bf_hidden_tiles<MT, 1>(w, KS, in, outb, ld, bias, t, lane);
    }
    __syncthreads();   // the image is complete, and nobody reads `in` any more: the next layer writes over it
  }
  // output layer: one more MFMA layer (<= 64 features = one or two tiles), fp32 epilogue
  {
    const uint16_t* in = ((L - 1) & 1) ? buf1 : buf0;
    const int KS = p.dims[L - 1] >> 4, N = p.dims[L], NT = (N + 31) >> 5;
    const uint4* w = reinterpret_cast<const uint4*>(pk + p.p_off[L - 1]);
    const float* bias = prm + p.b_off[L - 1];
    float* out = p.out + (long long)net * p.B * p.ld_out;
    for (int t = wave; t < NT; t += BF_NW) {
      f32x16b acc[MT];
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
      const uint4* wp = w + (long long)t * KS * 64 + lane;
      const uint16_t* ap = in + r * ld + 8 * h;
      for (int ks = 0; ks < KS; ++ks) {
        const uint4 wf = wp[ks * 64];
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i] = bf_mfma(wf, *reinterpret_cast<const uint4*>(ap + 32 * i * ld + 16 * ks), acc[i]);
      }
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const long long m = row0 + 32 * i + r;
        if (m >= p.B) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n0 = 32 * t + 8 * g + 4 * h;
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int n = n0 + e;
            float x = 0.f;   // pad column
            if (n < N) {
              x = acc[i][4 * g + e] + bias[n];
              if (p.out_act == PQLK_ACT_TANH) x = tanhf(x);
              else if (p.out_act == PQLK_ACT_TANH_NOISE) {
                x = tanhf(x);
                float nz = p.noise_std * p.draw[m * N + n];
                nz = fminf(fmaxf(nz, -p.noise_clip), p.noise_clip);
                x = fminf(fmaxf(x + nz, -1.f), 1.f);
              }
              if (p.out2) p.out2[m * p.ld_out2 + n] = x;   // (n_nets == 1)
            }
            v[e] = x;
          }
          *reinterpret_cast<float4*>(out + m * p.ld_out + n0) = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    }
  }
}

// fp32 arena -> fragment-ordered bf16 copy of every layer's weights, K padded to 16 and N to 32 with zeros:
//   packed[net][layer][tile n/32][k/16][lane = 32 h + r][j] = bf16(W[32 tile + r][16 (k/16) + 8 h + j])
__global__ __launch_bounds__(256) void k_pack_bf16(PackBf16P p) {
  const long long total = p.units_per_net * p.n_nets;
  for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < total; u += (long long)gridDim.x * 256) {
    const long long net = u / p.units_per_net, v = u - net * p.units_per_net;
    int l = 0;
    for (int k = 1; k < p.n_layers; ++k)
      if (v >= p.u_off[k]) l = k;
    const long long wq = v - p.u_off[l];
    const int lane = (int)(wq & 63), K = p.dims[l], N = p.dims[l + 1], KS = (K + 15) >> 4;
    const long long kt = wq >> 6;
    const int t = (int)(kt / KS), ks = (int)(kt - (long long)t * KS);
    const int n = 32 * t + (lane & 31), k0 = 16 * ks + 8 * (lane >> 5);
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (n < N) {
      const float* row = p.params + net * p.net_stride + p.w_off[l] + (long long)n * ((K + 31) & ~31);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (k0 + j < K) f[j] = row[k0 + j];
    }
    uint4 o;
    o.x = bf16_pack2(f[0], f[1]); o.y = bf16_pack2(f[2], f[3]); o.z = bf16_pack2(f[4], f[5]); o.w = bf16_pack2(f[6], f[7]);
    reinterpret_cast<uint4*>(p.packed)[u] = o;
  }
}

// LDS row length in bf16 elements: the widest layer input (K padded to 16) plus the padding
static int bf_lds_ld(const PqlMlpDesc* d) {
  int w = 0;
  for (int l = 0; l < d->n_layers; ++l) w = w > ((d->dims[l] + 15) & ~15) ? w : ((d->dims[l] + 15) & ~15);
  return w + BF_PAD;
}
static size_t bf_lds_bytes(const PqlMlpDesc* d, int mt) { return (size_t)2 * 32 * mt * bf_lds_ld(d) * sizeof(uint16_t); }

static bool bf_ok(const PqlMlpDesc* d) {
  if (desc_ok(d) != PQLK_OK || d->n_layers < 2) return false;
  for (int l = 1; l < d->n_layers; ++l)
    if (d->dims[l] % 32 != 0 || d->dims[l] > 1024) return false;
  if (d->dims[d->n_layers] > 64) return false;
  return bf_lds_bytes(d, 1) <= (size_t)BF_LDS_MAX;   // (bounds the input width: two 32-row images must fit)
}

static int64_t bf_layer_elems(const PqlMlpDesc* d, int l) {
  return (int64_t)((d->dims[l + 1] + 31) & ~31) * ((d->dims[l] + 15) & ~15);
}
static int64_t bf_net_elems(const PqlMlpDesc* d) {
  int64_t n = 0;
  for (int l = 0; l < d->n_layers; ++l) n += bf_layer_elems(d, l);
  return n;
}

extern "C" int pqlk_mlp_bf16_ok(const PqlMlpDesc* d) { return bf_ok(d) ? 1 : 0; }

extern "C" int64_t pqlk_mlp_packed_bf16_elems(const PqlMlpDesc* d) { return bf_ok(d) ? bf_net_elems(d) * d->n_nets : 0; }

extern "C" int pqlk_mlp_pack_bf16(const PqlMlpDesc* d, const float* params, uint16_t* packed, pqlk_stream_t stream) {
  int rc = desc_ok(d);
  if (rc) return rc;
  PQLK_REQUIRE(params && packed, PQLK_E_NULL);
  PQLK_REQUIRE(pqlk_aligned16(params) && pqlk_aligned16(packed), PQLK_E_ALIGN);
  PQLK_REQUIRE(bf_ok(d), PQLK_E_UNSUPPORTED);
  PackBf16P p = {};
  p.params = params; p.packed = packed; p.net_stride = pqlk_mlp_net_stride(d); p.units_per_net = bf_net_elems(d) / 8;
  p.n_layers = d->n_layers; p.n_nets = d->n_nets;
  int64_t u = 0;
  for (int l = 0; l <= d->n_layers; ++l) p.dims[l] = d->dims[l];
  for (int l = 0; l < d->n_layers; ++l) {
    int64_t w_off, b_off;
    pqlk_mlp_layer_offsets(d, l, &w_off, &b_off);
    p.w_off[l] = w_off; p.u_off[l] = u;
    u += bf_layer_elems(d, l) / 8;
  }
  const int64_t total = p.units_per_net * d->n_nets;
  const unsigned blocks = (unsigned)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(k_pack_bf16, dim3(blocks), dim3(256), 0, pqlk_s(stream), p);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

extern "C" int pqlk_mlp_forward_bf16(const PqlMlpDesc* d, const float* params, const uint16_t* packed, const float* x, int64_t ldx,
                                     int64_t b, int32_t out_act, const float* draw, float noise_std, float noise_clip, float* out,
                                     float* out2, int64_t ld_out2, pqlk_stream_t stream) {
  int rc = desc_ok(d);
  if (rc) return rc;
  PQLK_REQUIRE(params && packed && x && out, PQLK_E_NULL);
  PQLK_REQUIRE(b > 0 && b < (1LL << 30), PQLK_E_SHAPE);
  PQLK_REQUIRE(ldx % 32 == 0 && ldx >= pqlk_ld(d->dims[0]), PQLK_E_ALIGN);
  PQLK_REQUIRE(pqlk_aligned16(params) && pqlk_aligned16(packed) && pqlk_aligned16(x) && pqlk_aligned16(out), PQLK_E_ALIGN);
  PQLK_REQUIRE(out_act == PQLK_ACT_NONE || out_act == PQLK_ACT_TANH || out_act == PQLK_ACT_TANH_NOISE, PQLK_E_UNSUPPORTED);
  if (out_act == PQLK_ACT_TANH_NOISE) PQLK_REQUIRE(draw, PQLK_E_NULL);
  if (out2) PQLK_REQUIRE(d->n_nets == 1 && ld_out2 >= d->dims[d->n_layers], PQLK_E_SHAPE);
  PQLK_REQUIRE(bf_ok(d), PQLK_E_UNSUPPORTED);
  const int L = d->n_layers;
  Bf16P p = {};
  p.X = x; p.params = params; p.packed = packed; p.draw = draw; p.out = out; p.out2 = out2;
  p.net_stride = pqlk_mlp_net_stride(d); p.packed_net_stride = bf_net_elems(d);
  p.n_layers = L; p.B = (int)b; p.ldx = (int)ldx; p.ld_out = (int)pqlk_ld(d->dims[L]); p.ld_out2 = (int)ld_out2;
  p.lds_ld = bf_lds_ld(d); p.out_act = out_act; p.noise_std = noise_std; p.noise_clip = noise_clip;
  int64_t e = 0;
  for (int l = 0; l <= L; ++l) p.dims[l] = d->dims[l];
  for (int l = 0; l < L; ++l) {
    int64_t w_off, b_off;
    pqlk_mlp_layer_offsets(d, l, &w_off, &b_off);
    p.b_off[l] = b_off; p.p_off[l] = e;
    e += bf_layer_elems(d, l);
  }
  static PqlkPerDeviceOnce attr_once;
  if (int arc = attr_once.run([&] {
        const void* ks[2] = {reinterpret_cast<const void*>(&k_mlp_fwd_bf16<1>), reinterpret_cast<const void*>(&k_mlp_fwd_bf16<2>)};
        for (const void* k : ks) {
          hipError_t err = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, BF_LDS_MAX);
          if (err != hipSuccess) return -(int)err;
        }
        return 0;
      }))
    return arc;
  const int mt = bf_lds_bytes(d, 2) <= (size_t)BF_LDS_MAX ? 2 : 1;   // 64 rows per block where two images of them fit
  dim3 grid((unsigned)((b + 32 * mt - 1) / (32 * mt)), (unsigned)d->n_nets), block(64 * BF_NW);
  if (mt == 2) hipLaunchKernelGGL(k_mlp_fwd_bf16<2>, grid, block, bf_lds_bytes(d, 2), pqlk_s(stream), p);
  else hipLaunchKernelGGL(k_mlp_fwd_bf16<1>, grid, block, bf_lds_bytes(d, 1), pqlk_s(stream), p);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}
