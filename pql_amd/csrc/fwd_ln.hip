// Whole-stack forward of the LayerNorm twin critic (DoubleQLayerNorm with algo.critic_fused_forward): one launch computes, for both
// nets (blockIdx.y), x -> [Linear -> LayerNorm(eps, affine) -> ELU] x H -> Linear -> Q.  The per-layer form (a one-layer GEMM launch,
// a row launch of ln.hip, per net and layer) stays what it was; gemm.hip, fused.h and ln.hip's kernels are untouched.  The law is
// written op by op in include/pqlk.h.
//
// Work split: a block of 8 waves owns 32 * R batch rows through every layer, their current activations in ONE fp32 LDS image
// [row][feature] (row length = widest layer + 4 floats of padding).  R = 2 where the 64-row image fits 160 KB and no hidden layer is
// wider than 512 (the default [512, 512, 256]: 132 KB), R = 1 otherwise (a 1024-wide layer: 131.6 KB).
//
// Linear: v_mfma_f32_32x32x2_f32 with the WEIGHT tile as the A operand and the activation tile from LDS as B, so a lane holds one
// batch row (lane = 32 h + r: row r) and four consecutive output features sit in four consecutive accumulator registers.  Wave w
// takes the 32-feature tiles w, w + 8, ... (at most 4); the accumulators (tiles x R x 16 <= 64 registers) stay in registers over the
// whole k loop.  Weights come straight from the arena, row-major W (out, ld(in)), as 16-byte loads -- lane (r, h) takes
// W[n0 + r][8 s + 4 h .. 8 s + 4 h + 3] -- and the activations with the matching ds_read_b128; component e of both feeds MFMA e of
// the group, whose two k slots are then columns 8 s + e (h = 0) and 8 s + 4 + e (h = 1): an 8-wide k group is consumed in the order
// 0, 4, 1, 5, 2, 6, 3, 7.  There is no packed copy of the weights.
//
// LayerNorm + ELU: an epilogue over the image.  Barrier (every wave has read the layer's input), z = acc + b is written over the
// image, barrier, then wave w takes rows w, w + 8, ... with the row routine of lnrow.h (LnMap<VPL, true>, ln.hip's own) and writes y
// back in place; with STASH it also writes z, y, mean, rstd of the row to HBM where backward_raw reads them.  The output layer
// (width 1) rides on the last epilogue: the wave that normalised a row still holds its y in registers, multiplies it with the output
// weights in register order and sums with the same butterfly, so nothing but Q leaves the block when STASH is off.
// No atomics, no scratch; a row's bits depend on neither m, its position in the batch, nor STASH.
//
// Dropout (DoubleQDropoutLayerNorm with algo.droq_fused_forward; pqlk_lnmlp_drop_forward): lm_norm and the kernel end in a parameter
// pack `D... dr` that is either empty (the plain kernel: the instructions and the bits of pqlk_lnmlp_forward are what they were) or
// one LnDrop.  With it the wave that holds a row under LnMap<VPL, true> regenerates the row's keep bits -- one Philox4x32-10 block per
// chunk of four columns, ln.hip's own ln_keep_bits -- and normalises u = keep ? z * s : 0; the row index of the mask is the row's
// index in the whole batch, the tag tag_base | (net << 4) | layer.  The stashed z stays the pre-dropout z, so the per-layer dropout
// backward, which regenerates the masks itself, reads the stash as it reads the per-layer forward's.
#include "lnrow.h"
#include "lndrop.h"
#include "lnmlp.h"

typedef float f32x16l __attribute__((ext_vector_type(16)));

struct LnMlpP {
  const float* X; const float* arena; float* stash; float* q;
  int64_t net_stride, stash_net_stride;
  int64_t w_off[PQLK_MAX_LAYERS], b_off[PQLK_MAX_LAYERS], g_off[PQLK_MAX_LAYERS], be_off[PQLK_MAX_LAYERS];   // inside a net
  int64_t z_off[PQLK_MAX_LAYERS], y_off[PQLK_MAX_LAYERS], mean_off[PQLK_MAX_LAYERS], rstd_off[PQLK_MAX_LAYERS];   // inside a net's stash
  int dims[PQLK_MAX_LAYERS + 1];
  int n_layers, m, ldx, ld;
  float eps;
};

extern __shared__ __attribute__((aligned(16))) unsigned char lm_sm[];

// z = W a + b of one hidden layer for the block's 32 R rows: img holds a (K columns, K a multiple of 8 with zeros past the layer's
// width) and is overwritten with z (32 NT columns).  Ends behind the barrier after which the image is complete.
template <int R, int NTW>
__device__ __forceinline__ void lm_linear(const float* __restrict__ W, int ldw, int KS, const float* __restrict__ bias, float* img, int ld,
                                          int NT, int wave, int lane) {
  const int r = lane & 31, h = lane >> 5;
  const int cnt = wave < NT ? (NT - 1 - wave) / LM_NW + 1 : 0;   // this wave's tiles: wave, wave + 8, ... (< NTW + 1)
  f32x16l acc[NTW][R];
#pragma unroll
  for (int j = 0; j < NTW; ++j)
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][i][e] = 0.f;
  if (cnt > 0) {
    const float* wp = W + (long long)(32 * wave + r) * ldw + 4 * h;
    const float* ap = img + r * ld + 4 * h;
    for (int s = 0; s < KS; ++s) {
      float4 wf[NTW], af[R];
#pragma unroll
      for (int j = 0; j < NTW; ++j)
        if (j < cnt) wf[j] = *reinterpret_cast<const float4*>(wp + (long long)j * (32 * LM_NW) * ldw + 8 * s);
#pragma unroll
      for (int i = 0; i < R; ++i) af[i] = *reinterpret_cast<const float4*>(ap + 32 * i * ld + 8 * s);
#pragma unroll
      for (int e = 0; e < 4; ++e)   // MFMA e: k slots = columns 8 s + e (h = 0) and 8 s + 4 + e (h = 1)
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
  }
  __syncthreads();   // nobody reads the layer's input any more
#pragma unroll
  for (int j = 0; j < NTW; ++j)
    if (j < cnt) {
      const int t = wave + LM_NW * j;
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

// the stash of one (net, hidden layer): where backward_raw reads z, y (m, cols), mean, rstd (m)
struct LmStash {
  float *z, *y, *mean, *rstd;
};

// LayerNorm + ELU over the block's rows of the image, a wave per row: z -> y in place.  wout (the last hidden layer only): the output
// layer's weights; y is then not written back but multiplied out to Q, column 0 of the row's 32 floats of qout (pad columns zero).
template <int VPL, bool STASH, typename... D>
__device__ __forceinline__ void lm_norm(float* img, int ld, int cols, int rows, long long row0, int m, const float* __restrict__ gamma,
                                        const float* __restrict__ beta, float eps, const LmStash& st, const float* __restrict__ wout,
                                        float bout, float* __restrict__ qout, int wave, int lane, D... dr) {
  using M = LnMap<VPL, true>;
  float ga[VPL], be[VPL], wo[VPL];
  ln_load<VPL, true>(gamma, cols, lane, ga);
  ln_load<VPL, true>(beta, cols, lane, be);
  if (wout) ln_load<VPL, true>(wout, cols, lane, wo);
  const float n = (float)cols;
  for (int rr = wave; rr < rows; rr += LM_NW) {
    const long long row = row0 + rr;
    if (row >= m) break;
    float v[VPL];
    ln_load<VPL, true>(img + rr * ld, cols, lane, v);
    if constexpr (STASH) ln_store<VPL, true>(st.z + row * cols, cols, lane, v);
    if constexpr (ln_has<LnDrop, D...>) {   // u = keep ? z * s : 0, the mask of the row's place in the whole batch
      const LnDrop d = ln_drop_of(dr...);
      const unsigned km = ln_keep_bits<VPL, true>(d, (uint32_t)row, cols, lane);
#pragma unroll
      for (int i = 0; i < VPL; ++i) v[i] = (km >> i) & 1u ? v[i] * d.s : 0.f;
    }
    LN_ROW_CENTER(v)
#pragma unroll
    for (int i = 0; i < VPL; ++i) v[i] = ln_elu(v[i] * rs * ga[i] + be[i]);
    if constexpr (STASH) {
      ln_store<VPL, true>(st.y + row * cols, cols, lane, v);
      if (lane == 0) { st.mean[row] = mu; st.rstd[row] = rs; }
    }
    if (!wout) {
      ln_store<VPL, true>(img + rr * ld, cols, lane, v);
    } else {   // Q = sum_j y_j w_j + b: per-lane partials in register order (slots past cols hold 0), the butterfly, then the bias
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) dot += v[i] * wo[i];
      const float qv = wave_sum(dot) + bout;
      if (lane < 8) *reinterpret_cast<float4*>(qout + row * 32 + 4 * lane) = make_float4(lane == 0 ? qv : 0.f, 0.f, 0.f, 0.f);
    }
  }
}

template <int R, bool STASH, typename... D>
__global__ __launch_bounds__(64 * LM_NW) void k_lnmlp_fwd(LnMlpP p, D... dr) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int net = blockIdx.y, H = p.n_layers - 1, ld = p.ld;
  const long long row0 = (long long)blockIdx.x * (32 * R);
  float* img = reinterpret_cast<float*>(lm_sm);
  // stage the input tile; rows past m and columns past dims[0] (up to the next multiple of 8) become zero
  {
    const int K0 = p.dims[0], qpr = ((K0 + 7) & ~7) >> 2;
    for (int i = tid; i < 32 * R * qpr; i += 64 * LM_NW) {
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
  for (int l = 0; l < H; ++l) {
    const int K = p.dims[l], N = p.dims[l + 1], KS = (K + 7) >> 3, NT = N >> 5, ldw = (K + 31) & ~31;
    const float* W = prm + p.w_off[l];
    const float* bias = prm + p.b_off[l];
    const int ntw = (NT + LM_NW - 1) / LM_NW;   // (block-uniform: the barriers inside are reached by every wave)
    if (ntw == 1) lm_linear<R, 1>(W, ldw, KS, bias, img, ld, NT, wave, lane);
    else if (ntw == 2) lm_linear<R, 2>(W, ldw, KS, bias, img, ld, NT, wave, lane);
    else if constexpr (R == 1) {
      if (ntw == 3) lm_linear<1, 3>(W, ldw, KS, bias, img, ld, NT, wave, lane);
      else lm_linear<1, 4>(W, ldw, KS, bias, img, ld, NT, wave, lane);
    }
    const bool last = l == H - 1;
    const float* wout = last ? prm + p.w_off[H] : nullptr;
    const float bout = last ? prm[p.b_off[H]] : 0.f;
    const float *ga = prm + p.g_off[l], *be = prm + p.be_off[l];
    LmStash st = {};
    if constexpr (STASH) st = LmStash{sb + p.z_off[l], sb + p.y_off[l], sb + p.mean_off[l], sb + p.rstd_off[l]};
    // (dr: empty, or the launch's LnDrop, which gets the tag of this (net, layer))
#define LM_NORM(VPL) lm_norm<VPL, STASH>(img, ld, N, 32 * R, row0, p.m, ga, be, p.eps, st, wout, bout, q, wave, lane, ln_drop_at(dr, net, l)...)
    if (N <= 128) LM_NORM(2);
    else if (N <= 256) LM_NORM(4);
    else if (R == 2 || N <= 512) LM_NORM(8);
    else if constexpr (R == 1) LM_NORM(16);
#undef LM_NORM
    if (!last) __syncthreads();   // y is complete: the next layer reads it
  }
}

// ---- host side
// (the arena, stash and image layout: lnmlp.h, shared with bwd_ln.hip)
extern "C" int pqlk_lnmlp_ok(const PqlMlpDesc* desc) {
  LmLayout d;
  return lm_layout(desc, &d) ? 1 : 0;
}

extern "C" int64_t pqlk_lnmlp_param_floats(const PqlMlpDesc* desc) {
  LmLayout d;
  return lm_layout(desc, &d) ? d.net_stride * d.n_nets : 0;
}

extern "C" int pqlk_lnmlp_offsets(const PqlMlpDesc* desc, int32_t layer, int64_t* lin_off, int64_t* gamma_off, int64_t* beta_off) {
  PQLK_REQUIRE(desc && lin_off && gamma_off && beta_off, PQLK_E_NULL);
  LmLayout d;
  PQLK_REQUIRE(lm_layout(desc, &d), PQLK_E_SHAPE);
  PQLK_REQUIRE(layer >= 0 && layer < d.n_layers, PQLK_E_RANGE);
  *lin_off = d.lin_off[layer];
  *gamma_off = layer < d.n_layers - 1 ? d.gamma_off[layer] : -1;
  *beta_off = layer < d.n_layers - 1 ? d.beta_off[layer] : -1;
  return PQLK_OK;
}

extern "C" int64_t pqlk_lnmlp_stash_floats(const PqlMlpDesc* desc, int64_t m) {
  LmLayout d;
  return lm_layout(desc, &d) && m > 0 ? lm_stash_net_floats(&d, m) * d.n_nets : 0;
}

extern "C" int pqlk_lnmlp_stash_offset(const PqlMlpDesc* desc, int64_t m, int32_t net, int32_t layer, int32_t which, int64_t* off,
                                       int64_t* ld) {
  PQLK_REQUIRE(desc && off && ld, PQLK_E_NULL);
  LmLayout d;
  PQLK_REQUIRE(lm_layout(desc, &d) && m > 0, PQLK_E_SHAPE);
  PQLK_REQUIRE(net >= 0 && net < d.n_nets && layer >= 0 && layer < d.n_layers - 1 && which >= PQLK_LNMLP_Z && which <= PQLK_LNMLP_RSTD,
               PQLK_E_RANGE);
  lm_stash_at(&d, m, layer, which, off, ld);
  *off += (int64_t)net * lm_stash_net_floats(&d, m);
  return PQLK_OK;
}

// the one dispatch of the plain entry (an empty pack) and the dropout entry (one LnDrop, its tag the launch's tag_base)
template <typename... D>
static int lm_forward(const PqlMlpDesc* desc, const float* arena, const float* x, int64_t ldx, int64_t m, float eps, float* stash,
                      float* q_out, pqlk_stream_t stream, D... dr) {
  LmLayout lay;
  PQLK_REQUIRE(lm_layout(desc, &lay), PQLK_E_SHAPE);
  const LmLayout* d = &lay;
  PQLK_REQUIRE(ldx % 32 == 0 && ldx >= pqlk_ld(d->dims[0]), PQLK_E_ALIGN);
  PQLK_REQUIRE(pqlk_aligned16(arena) && pqlk_aligned16(x) && pqlk_aligned16(stash) && pqlk_aligned16(q_out), PQLK_E_ALIGN);
  const int L = d->n_layers;
  LnMlpP p = {};
  p.X = x; p.arena = arena; p.stash = stash; p.q = q_out;
  p.net_stride = d->net_stride; p.stash_net_stride = lm_stash_net_floats(d, m);
  p.n_layers = L; p.m = (int)m; p.ldx = (int)ldx; p.ld = lm_image_cols(d) + LM_PAD; p.eps = eps;
  int widest = 0;
  for (int l = 0; l <= L; ++l) p.dims[l] = d->dims[l];
  for (int l = 0; l < L; ++l) {
    p.w_off[l] = d->lin_off[l];
    p.b_off[l] = d->lin_off[l] + (int64_t)d->dims[l + 1] * pqlk_ld(d->dims[l]);
    if (l == L - 1) break;
    p.g_off[l] = d->gamma_off[l]; p.be_off[l] = d->beta_off[l];
    int64_t unused;
    lm_stash_at(d, m, l, PQLK_LNMLP_Z, &p.z_off[l], &unused);
    lm_stash_at(d, m, l, PQLK_LNMLP_Y, &p.y_off[l], &unused);
    lm_stash_at(d, m, l, PQLK_LNMLP_MEAN, &p.mean_off[l], &unused);
    lm_stash_at(d, m, l, PQLK_LNMLP_RSTD, &p.rstd_off[l], &unused);
    widest = widest > d->dims[l + 1] ? widest : d->dims[l + 1];
  }
  static PqlkPerDeviceOnce attr_once;   // (one per instantiation: each entry raises the limit of its own four kernels)
  if (int arc = attr_once.run([&] {
        const void* ks[4] = {reinterpret_cast<const void*>(&k_lnmlp_fwd<1, false, D...>), reinterpret_cast<const void*>(&k_lnmlp_fwd<1, true, D...>),
                             reinterpret_cast<const void*>(&k_lnmlp_fwd<2, false, D...>), reinterpret_cast<const void*>(&k_lnmlp_fwd<2, true, D...>)};
        for (const void* k : ks) {
          hipError_t err = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, LM_LDS_MAX);
          if (err != hipSuccess) return -(int)err;
        }
        return 0;
      }))
    return arc;
  const int r = lm_lds_bytes(d, 2) <= (size_t)LM_LDS_MAX && widest <= LM_MAX_R2_WIDTH ? 2 : 1;
  dim3 grid((unsigned)((m + 32 * r - 1) / (32 * r)), (unsigned)d->n_nets), block(64 * LM_NW);
  hipStream_t s = pqlk_s(stream);
  if (r == 2 && stash) hipLaunchKernelGGL((k_lnmlp_fwd<2, true, D...>), grid, block, lm_lds_bytes(d, 2), s, p, dr...);
  else if (r == 2) hipLaunchKernelGGL((k_lnmlp_fwd<2, false, D...>), grid, block, lm_lds_bytes(d, 2), s, p, dr...);
  else if (stash) hipLaunchKernelGGL((k_lnmlp_fwd<1, true, D...>), grid, block, lm_lds_bytes(d, 1), s, p, dr...);
  else hipLaunchKernelGGL((k_lnmlp_fwd<1, false, D...>), grid, block, lm_lds_bytes(d, 1), s, p, dr...);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

extern "C" int pqlk_lnmlp_forward(const PqlMlpDesc* desc, const float* arena, const float* x, int64_t ldx, int64_t m, float eps,
                                  float* stash, float* q_out, pqlk_stream_t stream) {
  PQLK_REQUIRE(desc && arena && x && q_out, PQLK_E_NULL);
  PQLK_REQUIRE(pqlk_lnmlp_ok(desc) && m > 0 && m < (1LL << 30), PQLK_E_SHAPE);
  return lm_forward(desc, arena, x, ldx, m, eps, stash, q_out, stream);
}

extern "C" int pqlk_lnmlp_drop_forward(const PqlMlpDesc* desc, const float* arena, const float* x, int64_t ldx, int64_t m, float eps,
                                       float p, uint64_t seed, uint64_t tag_base, float* stash, float* q_out, pqlk_stream_t stream) {
  PQLK_REQUIRE(desc && arena && x && q_out, PQLK_E_NULL);
  PQLK_REQUIRE(pqlk_lnmlp_ok(desc) && m > 0 && m < (1LL << 30), PQLK_E_SHAPE);
  LnDrop dr;
  PQLK_REQUIRE(ln_drop_make_stack(p, seed, tag_base, m, desc->n_nets, desc->n_layers - 1, &dr), PQLK_E_SHAPE);
  return lm_forward(desc, arena, x, ldx, m, eps, stash, q_out, stream, dr);
}
