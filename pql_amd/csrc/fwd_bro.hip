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
// Linear: the fp32 steps of lnstack.h -- the geometry, the fragments and the k order inside an 8-wide group are pqlk_lnmlp_forward's,
// one text for both, so z's bits are defined by the header.  The k loop here is software-pipelined: the 16-byte weight (HBM / L2) and
// activation (LDS) fragments of step s + 1 are fetched ahead of the MFMAs of step s; no sum changes its order by that.
//
// Skip in registers: in the epilogue row rr of the block belongs to wave rr mod 8 in EVERY layer, so the wave that normalises a row
// also normalised it two layers earlier.  The epilogue runs its 4 R rows as a fully unrolled loop (a row >= m is predicated off) and
// keeps h_{k-1} of those rows in VPL x 4 R registers: the stem's and every closing epilogue write them, an opening epilogue leaves
// them alone, a closing one reads them as the skip.  The residual stream never touches LDS or HBM; the image only ever holds the
// current layer's input or output.
//
// Output layer: rides on the last epilogue (the stem's for K = 0, else a closing one) through lnstack.h's ls_q_row.  Without STASH nothing but Q leaves the block; with it z, y (16-byte runs), mean, rstd of every hidden layer
// go where backward_raw reads them.  Plain vector stores, no atomics, no scratch; a row's bits depend on neither m, its position in
// the batch, nor STASH.
#include "lnstack.h"

constexpr int BR_MAX_WIDTH = 1024;
constexpr int BR_MAX_BLOCKS = 16;

struct BroP {
  const float* X; const float* arena; float* stash; float* q;
  int64_t net_stride, stash_net_stride, m4;   // m4: m rounded up to 4, the length of a mean / rstd vector in the stash
  int in_dim, ldin, W, K, m, ldx, ld;
  float eps;
};

// z = W a + b of one hidden layer for the block's 32 R rows: img holds a (8 KS columns, zeros past the layer's input width) and is
// overwritten with z.  cnt: this wave's tiles (wave, wave + 8, ..; <= NTW).  Ends behind the barrier after which z is complete.
// The k loop is software-pipelined: step s is in flight while step s - 1 multiplies.
template <int R, int NTW>
__device__ __forceinline__ void br_linear(const float* __restrict__ W, int ldw, int KS, const float* __restrict__ bias, float* img, int ld,
                                          int cnt, int wave, int lane) {
  const int r = lane & 31, h = lane >> 5;
  ls_f32x16 acc[NTW][R];
  ls_zero<R, NTW>(acc);
  if (cnt > 0) {
    const float* wp = W + (long long)(32 * wave + r) * ldw + 4 * h;
    const float* ap = img + r * ld + 4 * h;
    float4 wf[NTW], af[R], wn[NTW], an[R];
    ls_fetch<R, NTW>(wp, ldw, ap, ld, 0, cnt, wf, af);
    for (int s = 1; s < KS; ++s) {
      ls_fetch<R, NTW>(wp, ldw, ap, ld, s, cnt, wn, an);
      ls_mfma<R, NTW>(acc, cnt, wf, af);
#pragma unroll
      for (int j = 0; j < NTW; ++j)
        if (j < cnt) wf[j] = wn[j];
#pragma unroll
      for (int i = 0; i < R; ++i) af[i] = an[i];
    }
    ls_mfma<R, NTW>(acc, cnt, wf, af);
  }
  ls_write_z<R, NTW>(acc, cnt, bias, img, ld, wave, lane);
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
    const int rr = wave + LS_NW * i;
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
      } else {
        ls_q_row<VPL>(v, wo, bout, qout + row * 32, lane);
      }
    }
  }
}

// every layer of one net for the block's rows, at one geometry (VPL values per lane in a row, <= NTW tiles per wave)
template <int R, bool STASH, int VPL, int NTW>
__device__ __forceinline__ void br_stack(const BroP& p, float* img, const float* __restrict__ prm, float* __restrict__ sb,
                                         float* __restrict__ q, long long row0, int wave, int lane) {
  const int W = p.W, K = p.K, ld = p.ld, NT = W >> 5, nh = 2 * K + 1;
  const int cnt = ls_tiles(NT, wave);
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
__global__ __launch_bounds__(64 * LS_NW) void k_bro_fwd(BroP p) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int net = blockIdx.y, ld = p.ld;
  const long long row0 = (long long)blockIdx.x * (32 * R);
  float* img = reinterpret_cast<float*>(ls_sm);
  ls_stage<32 * R>(p, p.in_dim, img, ld, row0, tid);
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
static size_t br_lds_bytes(const BroLayout* d, int r) { return ls_lds_bytes(br_image_cols(d), r); }

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
  if (br_lds_bytes(&d, 1) > (size_t)LS_LDS_MAX) return false;
  *out = d;
  return true;
}

// a net's stash: z, y of every hidden layer, (m, W) each, then mean, rstd of every hidden layer, m floats rounded up to 4
static int64_t br_stash_net_floats(int32_t width, int32_t blocks, int64_t m) {
  return (int64_t)(2 * blocks + 1) * (2 * m * width + 2 * ls_round4(m));
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
    *off = base + 2 * (int64_t)nh * m * width + (2 * (int64_t)layer + (which == PQLK_LNMLP_RSTD ? 1 : 0)) * ls_round4(m);
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
  if (int rc = ls_forward_args(ldx, in_dim, arena, x, stash, q_out)) return rc;
  BroP p = {};
  p.X = x; p.arena = arena; p.stash = stash; p.q = q_out;
  p.net_stride = d->net_stride; p.stash_net_stride = br_stash_net_floats(width, blocks, m); p.m4 = ls_round4(m);
  p.in_dim = in_dim; p.ldin = d->ldin; p.W = width; p.K = blocks; p.m = (int)m; p.ldx = (int)ldx; p.ld = br_image_cols(d) + LS_PAD;
  p.eps = eps;
  const int r = ls_r2_ok(br_lds_bytes(d, 2), width) ? 2 : 1;
  if (stash) return ls_launch<&k_bro_fwd<1, true>, &k_bro_fwd<2, true>>(r, m, n_nets, br_lds_bytes(d, r), stream, p);
  return ls_launch<&k_bro_fwd<1, false>, &k_bro_fwd<2, false>>(r, m, n_nets, br_lds_bytes(d, r), stream, p);
}
