// Whole-stack forward of the residual LayerNorm twin critic (DoubleQBroNet with algo.bronet_fused_forward): one launch computes, for
// both nets (blockIdx.y), the stem, K residual blocks and the output layer (the law op by op in include/pqlk.h):
//   z0 = x W0' + b0, h0 = ELU(LN(z0));  k = 1..K: za = h_{k-1} Wa' + ba, t = ELU(LN(za)), zb = t Wb' + bb, h_k = h_{k-1} + LN(zb);
//   Q = h_K Wo' + bo.
// The per-layer form (a one-layer GEMM launch and a row launch of ln.hip per net and layer) stays what it was.
//
// Work split: a block of 8 waves owns 32 * R batch rows through all 2 K + 2 layers, their current activations in ONE fp32 LDS image
// [row][max(ld(in), W) + 4].  R = 2 where W <= 512 and the 64-row image fits 160 KB, R = 1 otherwise.  Every hidden layer has the
// width W, so the vector width of the row routine (VPL) and the tiles a wave holds (NTW) are template arguments of the whole stack:
// the kernel branches once, on W, and what follows is straight code for one geometry.
//
// Linear: v_mfma_f32_32x32x2_f32, the WEIGHT tile as A and the activation tile from LDS as B (lane = 32 h + r: batch row r, four
// consecutive features in four consecutive accumulator registers).  Wave w takes the feature tiles w, w + 8, ..; at most 64
// accumulators.  Fragments and the k order inside an 8-wide group (0, 4, 1, 5, 2, 6, 3, 7) are pqlk_lnmlp_forward's, so z's bits are
// defined by the header.  The k loop is software-pipelined: the 16-byte weight (HBM / L2) and activation (LDS) fragments of step s + 1
// are fetched ahead of the MFMAs of step s; no sum changes its order by that.
//
// Skip in registers: in the epilogue row rr of the block belongs to wave rr mod 8 in EVERY layer, so the wave that normalises a row
// also normalised it two layers earlier.  The epilogue runs its 4 R rows as a fully unrolled loop (a row >= m is predicated off) and
// keeps h_{k-1} of those rows in VPL x 4 R registers: the stem's and every closing epilogue write them, an opening epilogue leaves
// them alone, a closing one reads them as the skip.  The residual stream never touches LDS or HBM; the image only ever holds the
// current layer's input or output.
//
// Output layer: rides on the last epilogue (the stem's for K = 0, else a closing one): y in registers x Wo in register order, the row
// sum's butterfly, + bo.  Without STASH nothing but Q leaves the block; with it z, y (16-byte runs), mean, rstd of every hidden layer
// go where backward_raw reads them.  Plain vector stores, no atomics, no scratch; a row's bits depend on neither m, its position in
// the batch, nor STASH.
#include "lnrow.h"

constexpr int BR_NW = 8;                 // waves per block
constexpr int BR_LDS_MAX = 160 * 1024;
constexpr int BR_PAD = 4;                // floats of row padding in LDS (16 B: consecutive rows start 4 banks apart)
constexpr int BR_MAX_R2_WIDTH = 512;     // widest stack at R = 2: 2 tiles x 2 row tiles x 16 = 64 accumulator registers
constexpr int BR_MAX_WIDTH = 1024;
constexpr int BR_MAX_BLOCKS = 16;

typedef float f32x16b __attribute__((ext_vector_type(16)));

struct BroP {
  const float* X; const float* arena; float* stash; float* q;
  int64_t net_stride, stash_net_stride, m4;   // m4: m rounded up to 4, the length of a mean / rstd vector in the stash
  int in_dim, ldin, W, K, m, ldx, ld;
  float eps;
};

extern __shared__ __attribute__((aligned(16))) unsigned char br_sm[];

// the fragments of k step s: the weights of this wave's tiles (HBM / L2) and the activations of the block's row tiles (LDS)
template <int R, int NTW>
__device__ __forceinline__ void br_fetch(const float* __restrict__ wp, int ldw, const float* ap, int ld, int s, int cnt,
                                         float4 (&wf)[NTW], float4 (&af)[R]) {
#pragma unroll
  for (int j = 0; j < NTW; ++j)
    if (j < cnt) wf[j] = *reinterpret_cast<const float4*>(wp + (long long)j * (32 * BR_NW) * ldw + 8 * s);
#pragma unroll
  for (int i = 0; i < R; ++i) af[i] = *reinterpret_cast<const float4*>(ap + 32 * i * ld + 8 * s);
}

// the four MFMAs of one k step per (tile, row tile): MFMA e takes columns 8 s + e (h = 0) and 8 s + 4 + e (h = 1)
template <int R, int NTW>
__device__ __forceinline__ void br_mfma(f32x16b (&acc)[NTW][R], int cnt, const float4 (&wf)[NTW], const float4 (&af)[R]) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int j = 0; j < NTW; ++j)
      if (j < cnt) {
        const float wv = e == 0 ? wf[j].x : e == 1 ? wf[j].y : e == 2 ? wf[j].z : wf[j].w;
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const float av = e == 0 ? af[i].x : e == 1 ? af[i].y : e == 2 ? af[i].z : af[i].w;
          acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, av, acc[j][i], 0, 0, 0);
        }
      }
}

// z = W a + b of one hidden layer for the block's 32 R rows: img holds a (8 KS columns, zeros past the layer's input width) and is
// overwritten with z.  cnt: this wave's tiles (wave, wave + 8, ..; <= NTW).  Ends behind the barrier after which z is complete.
template <int R, int NTW>
__device__ __forceinline__ void br_linear(const float* __restrict__ W, int ldw, int KS, const float* __restrict__ bias, float* img, int ld,
                                          int cnt, int wave, int lane) {
  const int r = lane & 31, h = lane >> 5;
  f32x16b acc[NTW][R];
#pragma unroll
  for (int j = 0; j < NTW; ++j)
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][i][e] = 0.f;
  if (cnt > 0) {
    const float* wp = W + (long long)(32 * wave + r) * ldw + 4 * h;
    const float* ap = img + r * ld + 4 * h;
    float4 wf[NTW], af[R], wn[NTW], an[R];
    br_fetch<R, NTW>(wp, ldw, ap, ld, 0, cnt, wf, af);
    for (int s = 1; s < KS; ++s) {   // step s is in flight while step s - 1 multiplies
      br_fetch<R, NTW>(wp, ldw, ap, ld, s, cnt, wn, an);
      br_mfma<R, NTW>(acc, cnt, wf, af);
#pragma unroll
      for (int j = 0; j < NTW; ++j)
        if (j < cnt) wf[j] = wn[j];
#pragma unroll
      for (int i = 0; i < R; ++i) af[i] = an[i];
    }
    br_mfma<R, NTW>(acc, cnt, wf, af);
  }
  __syncthreads();   // nobody reads the layer's input any more
#pragma unroll
  for (int j = 0; j < NTW; ++j)
    if (j < cnt) {
      const int t = wave + BR_NW * j;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n0 = 32 * t + 8 * g + 4 * h;   // accumulator registers 4g .. 4g+3 = features n0 .. n0+3 of row r
        const float4 b4 = *reinterpret_cast<const float4*>(bias + n0);
#pragma unroll
        for (int i = 0; i < R; ++i)
          *reinterpret_cast<float4*>(img + (32 * i + r) * ld + n0) =
              make_float4(acc[j][i][4 * g] + b4.x, acc[j][i][4 * g + 1] + b4.y, acc[j][i][4 * g + 2] + b4.z, acc[j][i][4 * g + 3] + b4.w);
      }
    }
  __syncthreads();   // z is complete
}

enum { BR_STEM = 0, BR_OPEN = 1, BR_CLOSE = 2 };

// The norm step of hidden layer `l` over the block's rows, wave w its rows w, w + 8, ..: z -> y in the image.  KIND: BR_STEM / BR_OPEN:
// y = ELU(LN(z)); BR_CLOSE: y = skip + LN(z).  BR_STEM and BR_CLOSE leave y in `skip`.  wout (the last hidden layer only): the output
// layer's weights; y is then not written back but multiplied out to Q, column 0 of the row's 32 floats of qout (pad columns zero).
template <int VPL, int R, bool STASH, int KIND>
__device__ __forceinline__ void br_norm(float* img, int ld, int cols, long long row0, int m, const float* __restrict__ prm_gamma, float eps,
                                        float* __restrict__ sb, long long m4, int l, int nh, const float* __restrict__ wout,
                                        float* __restrict__ qout, float (&skip)[4 * R][VPL], int wave, int lane) {
  using M = LnMap<VPL, true>;
  float ga[VPL], be[VPL], wo[VPL];
  ln_load<VPL, true>(prm_gamma, cols, lane, ga);
  ln_load<VPL, true>(prm_gamma + cols, cols, lane, be);   // beta lies behind gamma (ld(W) = W)
  float bout = 0.f;
  if (wout) {   // [Wo (ld(W) = W) | bo]
    ln_load<VPL, true>(wout, cols, lane, wo);
    bout = wout[cols];
  }
  const float n = (float)cols;
  [[maybe_unused]] float *sz = nullptr, *sy = nullptr, *smean = nullptr, *srstd = nullptr;
  if constexpr (STASH) {
    sz = sb + 2ll * l * m * cols; sy = sz + (long long)m * cols;
    smean = sb + 2ll * nh * m * cols + 2ll * l * m4; srstd = smean + m4;
  }
#pragma unroll
  for (int i = 0; i < 4 * R; ++i) {
    const int rr = wave + BR_NW * i;
    const long long row = row0 + rr;
    if (row < m) {
      float v[VPL];
      ln_load<VPL, true>(img + rr * ld, cols, lane, v);
      if constexpr (STASH) ln_store<VPL, true>(sz + row * cols, cols, lane, v);
      LN_ROW_CENTER(v)
      if constexpr (KIND != BR_CLOSE) {
#pragma unroll
        for (int j = 0; j < VPL; ++j) v[j] = ln_elu(v[j] * rs * ga[j] + be[j]);
      } else {
#pragma unroll
        for (int j = 0; j < VPL; ++j) v[j] = skip[i][j] + (v[j] * rs * ga[j] + be[j]);
      }
      if constexpr (KIND != BR_OPEN) {
#pragma unroll
        for (int j = 0; j < VPL; ++j) skip[i][j] = v[j];
      }
      if constexpr (STASH) {
        ln_store<VPL, true>(sy + row * cols, cols, lane, v);
        if (lane == 0) { smean[row] = mu; srstd[row] = rs; }
      }
      if (!wout) {
        ln_store<VPL, true>(img + rr * ld, cols, lane, v);
      } else {   // Q = sum_j y_j w_j + b: per-lane partials in register order (slots past cols hold 0), the butterfly, then the bias
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j) dot += v[j] * wo[j];
        const float qv = wave_sum(dot) + bout;
        if (lane < 8) *reinterpret_cast<float4*>(qout + row * 32 + 4 * lane) = make_float4(lane == 0 ? qv : 0.f, 0.f, 0.f, 0.f);
      }
    }
  }
}

// every layer of one net for the block's rows, at one geometry (VPL values per lane in a row, <= NTW tiles per wave)
template <int R, bool STASH, int VPL, int NTW>
__device__ __forceinline__ void br_stack(const BroP& p, float* img, const float* __restrict__ prm, float* __restrict__ sb,
                                         float* __restrict__ q, long long row0, int wave, int lane) {
  const int W = p.W, K = p.K, ld = p.ld, NT = W >> 5, nh = 2 * K + 1;
  const int cnt = wave < NT ? (NT - 1 - wave) / BR_NW + 1 : 0;
  const long long blk = (long long)W * W + 3 * W;                // a block layer: [W | b | gamma | beta]
  const float* lay = prm;                                         // the current layer's start
  float skip[4 * R][VPL];
#pragma unroll
  for (int i = 0; i < 4 * R; ++i)
#pragma unroll
    for (int j = 0; j < VPL; ++j) skip[i][j] = 0.f;
  // stem
  {
    const long long wsz = (long long)W * p.ldin;
    br_linear<R, NTW>(lay, p.ldin, (p.in_dim + 7) >> 3, lay + wsz, img, ld, cnt, wave, lane);
    const float* next = lay + wsz + 3 * W;   // (behind the last hidden layer: the output layer)
    br_norm<VPL, R, STASH, BR_STEM>(img, ld, W, row0, p.m, lay + wsz + W, p.eps, sb, p.m4, 0, nh, K == 0 ? next : nullptr, q, skip, wave, lane);
    lay = next;
  }
  const int KS = W >> 3;
  const long long wsz = (long long)W * W;
  for (int k = 1; k <= K; ++k) {
    __syncthreads();   // h_{k-1} is complete in the image
    br_linear<R, NTW>(lay, W, KS, lay + wsz, img, ld, cnt, wave, lane);
    br_norm<VPL, R, STASH, BR_OPEN>(img, ld, W, row0, p.m, lay + wsz + W, p.eps, sb, p.m4, 2 * k - 1, nh, nullptr, q, skip, wave, lane);
    lay += blk;
    __syncthreads();   // t is complete
    br_linear<R, NTW>(lay, W, KS, lay + wsz, img, ld, cnt, wave, lane);
    br_norm<VPL, R, STASH, BR_CLOSE>(img, ld, W, row0, p.m, lay + wsz + W, p.eps, sb, p.m4, 2 * k, nh, k == K ? lay + blk : nullptr, q, skip,
                                     wave, lane);
    lay += blk;
  }
}

template <int R, bool STASH>
__global__ __launch_bounds__(64 * BR_NW) void k_bro_fwd(BroP p) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int net = blockIdx.y, ld = p.ld;
  const long long row0 = (long long)blockIdx.x * (32 * R);
  float* img = reinterpret_cast<float*>(br_sm);
  // stage the input tile; rows past m and columns past in_dim (up to the next multiple of 8) become zero
  {
    const int K0 = p.in_dim, qpr = ((K0 + 7) & ~7) >> 2;
    for (int i = tid; i < 32 * R * qpr; i += 64 * BR_NW) {
      const int row = i / qpr, c = (i - row * qpr) << 2;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row0 + row < p.m && c < K0) {   // c + 3 < ldx: ldx >= roundup(K0, 32)
        v = *reinterpret_cast<const float4*>(p.X + (row0 + row) * p.ldx + c);
        if (c + 1 >= K0) v.y = 0.f;
        if (c + 2 >= K0) v.z = 0.f;
        if (c + 3 >= K0) v.w = 0.f;
      }
      *reinterpret_cast<float4*>(img + row * ld + c) = v;
    }
  }
  __syncthreads();
  const float* prm = p.arena + (long long)net * p.net_stride;
  float* sb = STASH ? p.stash + (long long)net * p.stash_net_stride : nullptr;
  float* q = p.q + (long long)net * p.m * 32;
  const int W = p.W;   // (block-uniform: the barriers inside are reached by every wave)
  if (W <= 128) br_stack<R, STASH, 2, 1>(p, img, prm, sb, q, row0, wave, lane);
  else if (W <= 256) br_stack<R, STASH, 4, 1>(p, img, prm, sb, q, row0, wave, lane);
  else if (R == 2 || W <= 512) br_stack<R, STASH, 8, 2>(p, img, prm, sb, q, row0, wave, lane);
  else if constexpr (R == 1) br_stack<1, STASH, 16, 4>(p, img, prm, sb, q, row0, wave, lane);
}

// ---- host side
// the arena law of the normalised twin critics (include/pqlk.h) for the stack (in, W x (2 K + 1), 1): all offsets from three numbers
struct BroLayout {
  int in_dim, ldin, W, K, n_nets;
  int64_t stem, blk, net_stride;   // floats of layer 0, of a block layer, of a net
};

static int br_image_cols(const BroLayout* d) { return d->ldin > d->W ? d->ldin : d->W; }
static size_t br_lds_bytes(const BroLayout* d, int r) { return (size_t)32 * r * (br_image_cols(d) + BR_PAD) * sizeof(float); }

static bool br_shape_ok(int32_t width, int32_t blocks, int32_t n_nets) {
  return width > 0 && width % 32 == 0 && width <= BR_MAX_WIDTH && blocks >= 0 && blocks <= BR_MAX_BLOCKS && (n_nets == 1 || n_nets == 2);
}

// the layout of an eligible stack -> *out; false: not eligible
static bool br_layout(int32_t in_dim, int32_t width, int32_t blocks, int32_t n_nets, BroLayout* out) {
  if (!br_shape_ok(width, blocks, n_nets) || in_dim < 1 || in_dim > 1248) return false;   // (pqlk_ld(in_dim) <= 1248)
  BroLayout d = {};
  d.in_dim = in_dim; d.ldin = (int)pqlk_ld(in_dim); d.W = width; d.K = blocks; d.n_nets = n_nets;
  d.stem = (int64_t)width * d.ldin + 3 * width;
  d.blk = (int64_t)width * width + 3 * width;
  d.net_stride = d.stem + 2 * blocks * d.blk + width + pqlk_ld(1);
  if (br_lds_bytes(&d, 1) > (size_t)BR_LDS_MAX) return false;
  *out = d;
  return true;
}

static int64_t br_round4(int64_t x) { return (x + 3) & ~(int64_t)3; }

// a net's stash: z, y of every hidden layer, (m, W) each, then mean, rstd of every hidden layer, m floats rounded up to 4
static int64_t br_stash_net_floats(int32_t width, int32_t blocks, int64_t m) {
  return (int64_t)(2 * blocks + 1) * (2 * m * width + 2 * br_round4(m));
}

extern "C" int pqlk_bro_ok(int32_t in_dim, int32_t width, int32_t blocks, int32_t n_nets) {
  BroLayout d;
  return br_layout(in_dim, width, blocks, n_nets, &d) ? 1 : 0;
}

extern "C" int64_t pqlk_bro_param_floats(int32_t in_dim, int32_t width, int32_t blocks, int32_t n_nets) {
  BroLayout d;
  return br_layout(in_dim, width, blocks, n_nets, &d) ? d.net_stride * d.n_nets : 0;
}

extern "C" int pqlk_bro_offsets(int32_t in_dim, int32_t width, int32_t blocks, int32_t layer, int64_t* lin_off, int64_t* gamma_off,
                                int64_t* beta_off) {
  PQLK_REQUIRE(lin_off && gamma_off && beta_off, PQLK_E_NULL);
  BroLayout d;
  PQLK_REQUIRE(br_layout(in_dim, width, blocks, 1, &d), PQLK_E_SHAPE);
  PQLK_REQUIRE(layer >= 0 && layer <= 2 * blocks + 1, PQLK_E_RANGE);
  const int64_t lin = layer == 0 ? 0 : d.stem + (layer - 1) * d.blk;
  const bool hidden = layer <= 2 * blocks;
  *lin_off = lin;
  *gamma_off = hidden ? lin + (layer == 0 ? d.stem : d.blk) - 2 * width : -1;
  *beta_off = hidden ? *gamma_off + width : -1;
  return PQLK_OK;
}

extern "C" int64_t pqlk_bro_stash_floats(int32_t width, int32_t blocks, int32_t n_nets, int64_t m) {
  return br_shape_ok(width, blocks, n_nets) && m > 0 ? br_stash_net_floats(width, blocks, m) * n_nets : 0;
}

extern "C" int pqlk_bro_stash_offset(int32_t width, int32_t blocks, int32_t n_nets, int64_t m, int32_t net, int32_t layer, int32_t which,
                                     int64_t* off, int64_t* ld) {
  PQLK_REQUIRE(off && ld, PQLK_E_NULL);
  PQLK_REQUIRE(br_shape_ok(width, blocks, n_nets) && m > 0, PQLK_E_SHAPE);
  const int nh = 2 * blocks + 1;
  PQLK_REQUIRE(net >= 0 && net < n_nets && layer >= 0 && layer < nh && which >= PQLK_LNMLP_Z && which <= PQLK_LNMLP_RSTD, PQLK_E_RANGE);
  const int64_t base = (int64_t)net * br_stash_net_floats(width, blocks, m);
  if (which <= PQLK_LNMLP_Y) {   // (the kernel's br_norm forms the same sums)
    *off = base + (2 * (int64_t)layer + (which == PQLK_LNMLP_Y ? 1 : 0)) * m * width;
    *ld = width;
  } else {
    *off = base + 2 * (int64_t)nh * m * width + (2 * (int64_t)layer + (which == PQLK_LNMLP_RSTD ? 1 : 0)) * br_round4(m);
    *ld = 1;
  }
  return PQLK_OK;
}

extern "C" int pqlk_bro_forward(int32_t in_dim, int32_t width, int32_t blocks, int32_t n_nets, const float* arena, const float* x,
                                int64_t ldx, int64_t m, float eps, float* stash, float* q_out, pqlk_stream_t stream) {
  PQLK_REQUIRE(arena && x && q_out, PQLK_E_NULL);
  BroLayout lay;
  PQLK_REQUIRE(br_layout(in_dim, width, blocks, n_nets, &lay), PQLK_E_SHAPE);
  const BroLayout* d = &lay;
  PQLK_REQUIRE(m > 0 && m < (1LL << 30), PQLK_E_SHAPE);
  PQLK_REQUIRE(ldx % 32 == 0 && ldx >= d->ldin, PQLK_E_ALIGN);
  PQLK_REQUIRE(pqlk_aligned16(arena) && pqlk_aligned16(x) && pqlk_aligned16(stash) && pqlk_aligned16(q_out), PQLK_E_ALIGN);
  BroP p = {};
  p.X = x; p.arena = arena; p.stash = stash; p.q = q_out;
  p.net_stride = d->net_stride; p.stash_net_stride = br_stash_net_floats(width, blocks, m); p.m4 = br_round4(m);
  p.in_dim = in_dim; p.ldin = d->ldin; p.W = width; p.K = blocks; p.m = (int)m; p.ldx = (int)ldx; p.ld = br_image_cols(d) + BR_PAD;
  p.eps = eps;
  static PqlkPerDeviceOnce attr_once;
  if (int arc = attr_once.run([&] {
        const void* ks[4] = {reinterpret_cast<const void*>(&k_bro_fwd<1, false>), reinterpret_cast<const void*>(&k_bro_fwd<1, true>),
                             reinterpret_cast<const void*>(&k_bro_fwd<2, false>), reinterpret_cast<const void*>(&k_bro_fwd<2, true>)};
        for (const void* k : ks) {
          hipError_t err = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, BR_LDS_MAX);
          if (err != hipSuccess) return -(int)err;
        }
        return 0;
      }))
    return arc;
  const int r = br_lds_bytes(d, 2) <= (size_t)BR_LDS_MAX && width <= BR_MAX_R2_WIDTH ? 2 : 1;
  dim3 grid((unsigned)((m + 32 * r - 1) / (32 * r)), (unsigned)n_nets), block(64 * BR_NW);
  hipStream_t s = pqlk_s(stream);
  if (r == 2 && stash) hipLaunchKernelGGL((k_bro_fwd<2, true>), grid, block, br_lds_bytes(d, 2), s, p);
  else if (r == 2) hipLaunchKernelGGL((k_bro_fwd<2, false>), grid, block, br_lds_bytes(d, 2), s, p);
  else if (stash) hipLaunchKernelGGL((k_bro_fwd<1, true>), grid, block, br_lds_bytes(d, 1), s, p);
  else hipLaunchKernelGGL((k_bro_fwd<1, false>), grid, block, br_lds_bytes(d, 1), s, p);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}
