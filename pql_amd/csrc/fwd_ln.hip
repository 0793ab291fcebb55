// Whole-stack forward of the LayerNorm twin critic (DoubleQLayerNorm with algo.critic_fused_forward): one launch computes, for both
// nets (blockIdx.y), x -> [Linear -> LayerNorm(eps, affine) -> ELU] x H -> Linear -> Q.  The per-layer form (a one-layer GEMM launch,
// a row launch of ln.hip, per net and layer) stays what it was; gemm.hip, fused.h and ln.hip's kernels are untouched.  The law is
// written op by op in include/pqlk.h.
//
// Work split: a block of 8 waves owns 32 * R batch rows through every layer, their current activations in ONE fp32 LDS image
// [row][feature] (row length = widest layer + 4 floats of padding).  R = 2 where the 64-row image fits 160 KB and no hidden layer is
// wider than 512 (the default [512, 512, 256]: 132 KB), R = 1 otherwise (a 1024-wide layer: 131.6 KB).
//
// Linear: the fp32 steps of lnstack.h (the block geometry, the fragments, the k order inside an 8-wide group, z = acc + b over the
// image between two barriers) in a straight k loop: weights come from the arena as it lies, row-major W (out, ld(in)) -- lane (r, h)
// takes W[n0 + r][8 s + 4 h .. 8 s + 4 h + 3] --; there is no packed copy.  The tiles a wave holds (at most 4) are chosen per layer.
//
// LayerNorm + ELU: an epilogue over the image.  Barrier (every wave has read the layer's input), z = acc + b is written over the
// image, barrier, then wave w takes rows w, w + 8, ... with the row routine of lnrow.h (LnMap<VPL, true>, ln.hip's own) and writes y
// back in place; with STASH it also writes z, y, mean, rstd of the row to HBM where backward_raw reads them.  The output layer
// (width 1) rides on the last epilogue: the wave that normalised a row still holds its y in registers and multiplies it out
// (lnstack.h's ls_q_row), so nothing but Q leaves the block when STASH is off.
// No atomics, no scratch; a row's bits depend on neither m, its position in the batch, nor STASH.
//
// Dropout (DoubleQDropoutLayerNorm with algo.droq_fused_forward; pqlk_lnmlp_drop_forward): lm_norm and the kernel end in a parameter
// pack `D... dr` that is either empty (the plain kernel: the instructions and the bits of pqlk_lnmlp_forward are what they were) or
// one LnDrop.  With it the wave that holds a row under LnMap<VPL, true> regenerates the row's keep bits -- one Philox4x32-10 block per
// chunk of four columns, ln.hip's own ln_keep_bits -- and normalises u = keep ? z * s : 0; the row index of the mask is the row's
// index in the whole batch, the tag tag_base | (net << 4) | layer.  The stashed z stays the pre-dropout z, so the per-layer dropout
// backward, which regenerates the masks itself, reads the stash as it reads the per-layer forward's.
#include "lndrop.h"
#include "lnmlp.h"

struct LnMlpP {
  const float* X; const float* arena; float* stash; float* q;
  int64_t net_stride, stash_net_stride;
  int64_t w_off[PQLK_MAX_LAYERS], b_off[PQLK_MAX_LAYERS], g_off[PQLK_MAX_LAYERS], be_off[PQLK_MAX_LAYERS];   // inside a net
  int64_t z_off[PQLK_MAX_LAYERS], y_off[PQLK_MAX_LAYERS], mean_off[PQLK_MAX_LAYERS], rstd_off[PQLK_MAX_LAYERS];   // inside a net's stash
  int dims[PQLK_MAX_LAYERS + 1];
  int n_layers, m, ldx, ld;
  float eps;
};

// z = W a + b of one hidden layer for the block's 32 R rows: img holds a (K columns, K a multiple of 8 with zeros past the layer's
// width) and is overwritten with z (32 NT columns).  Ends behind the barrier after which the image is complete.  The k loop is
// straight: a step's fragments are fetched, then multiplied.
template <int R, int NTW>
__device__ __forceinline__ void lm_linear(const float* __restrict__ W, int ldw, int KS, const float* __restrict__ bias, float* img, int ld,
                                          int NT, int wave, int lane) {
  const int r = lane & 31, h = lane >> 5;
  const int cnt = ls_tiles(NT, wave);   // (< NTW + 1)
  ls_f32x16 acc[NTW][R];
  ls_zero<R, NTW>(acc);
  if (cnt > 0) {
    const float* wp = W + (long long)(32 * wave + r) * ldw + 4 * h;
    const float* ap = img + r * ld + 4 * h;
    for (int s = 0; s < KS; ++s) {
      float4 wf[NTW], af[R];
      ls_fetch<R, NTW>(wp, ldw, ap, ld, s, cnt, wf, af);
      ls_mfma<R, NTW>(acc, cnt, wf, af);
    }
  }
  ls_write_z<R, NTW>(acc, cnt, bias, img, ld, wave, lane);
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
  for (int rr = wave; rr < rows; rr += LS_NW) {
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
    } else {
      ls_q_row<VPL>(v, wo, bout, qout + row * 32, lane);
    }
  }
}

template <int R, bool STASH, typename... D>
__global__ __launch_bounds__(64 * LS_NW) void k_lnmlp_fwd(LnMlpP p, D... dr) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int net = blockIdx.y, H = p.n_layers - 1, ld = p.ld;
  const long long row0 = (long long)blockIdx.x * (32 * R);
  float* img = reinterpret_cast<float*>(ls_sm);
  ls_stage<32 * R>(p, p.dims[0], img, ld, row0, tid);
  __syncthreads();
  const float* prm = p.arena + (long long)net * p.net_stride;
  float* sb = STASH ? p.stash + (long long)net * p.stash_net_stride : nullptr;
  float* q = p.q + (long long)net * p.m * 32;
  for (int l = 0; l < H; ++l) {
    const int K = p.dims[l], N = p.dims[l + 1], KS = (K + 7) >> 3, NT = N >> 5, ldw = (K + 31) & ~31;
    const float* W = prm + p.w_off[l];
    const float* bias = prm + p.b_off[l];
    const int ntw = (NT + LS_NW - 1) / LS_NW;   // (block-uniform: the barriers inside are reached by every wave)
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
  if (int rc = ls_forward_args(ldx, d->dims[0], arena, x, stash, q_out)) return rc;
  const int L = d->n_layers;
  LnMlpP p = {};
  p.X = x; p.arena = arena; p.stash = stash; p.q = q_out;
  p.net_stride = d->net_stride; p.stash_net_stride = lm_stash_net_floats(d, m);
  p.n_layers = L; p.m = (int)m; p.ldx = (int)ldx; p.ld = lm_image_cols(d) + LS_PAD; p.eps = eps;
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
  const int r = ls_r2_ok(lm_lds_bytes(d, 2), widest) ? 2 : 1;
  if (stash) return ls_launch<&k_lnmlp_fwd<1, true, D...>, &k_lnmlp_fwd<2, true, D...>>(r, m, d->n_nets, lm_lds_bytes(d, r), stream, p, dr...);
  return ls_launch<&k_lnmlp_fwd<1, false, D...>, &k_lnmlp_fwd<2, false, D...>>(r, m, d->n_nets, lm_lds_bytes(d, r), stream, p, dr...);
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
