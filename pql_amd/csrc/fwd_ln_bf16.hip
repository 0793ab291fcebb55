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
// Linear and LayerNorm: lnstack.h's bf16 layer (weights from the packed, fragment-ordered copy of pqlk_lnmlp_pack_bf16, z = acc + b and
// the row sums in the accumulator registers, three barriers per hidden layer), with y = elu(xhat gamma + beta) as this critic's
// expression; the tiles a wave holds (at most 2 at R = 2, 4 at R = 1) are chosen per layer.  The output layer (width 1) rides on the
// last epilogue through the first row-sum table, so nothing but Q leaves the block.  No atomics, no scratch; a row's bits depend on
// neither m, its position in the batch, nor the launch.
//
// Dropout (DoubleQDropoutLayerNorm's target with algo.critic_target_dtype=bfloat16; pqlk_lnmlp_drop_forward_bf16): lb_layer and the
// kernel end in a parameter pack that is either empty (the plain kernel: the instructions and the bits of pqlk_lnmlp_forward_bf16 are
// what they were) or one LnDrop.  Accumulator registers 4g .. 4g+3 of a lane are four consecutive, 4-aligned features of one row:
// exactly one Philox4x32-10 block of the mask law.  So behind z = acc + b the lane generates that block in registers and leaves
// u = keep ? z * s : 0 in the accumulators, in front of the first row-sum table; everything behind it runs on u as it ran on z.  The
// mask's row index is the row's index in the whole batch (row0 + its row of the block), the tag tag_base | (net << 4) | layer.
#include "lndrop.h"
#include "lnstack.h"

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

// One hidden layer for the block's 32 R rows, ls_bf16_layer with this critic's two expressions: with a dropout pack z = acc + b becomes
// u = keep ? z * s : 0 -- the four registers of a group are one Philox block of row row0 + 32 i + r --, and y = elu(xhat gamma + beta).
template <int R, int NTW, typename... D>
__device__ __forceinline__ void lb_layer(const uint4* __restrict__ w, int KS, int N, const float* __restrict__ bias,
                                         const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                         const uint16_t* __restrict__ wout, uint16_t* img, int ld, float* tab1, float* tab2, int wave,
                                         int lane, D... dr) {
  const LsGeom g = ls_geom(N, ld, wave, lane);
  ls_bf16_layer<R, NTW>(
      g, w, KS, bias, gamma, beta, eps, wout, img, tab1, tab2, wave, lane,
      [&](int i, int n0, float4 z) {
        if constexpr (ln_has<LbDrop, D...>) {
          const LbDrop d = lb_drop_of(dr...);
          z = ln_drop4(d.d, d.row0 + (uint32_t)(32 * i + g.r), n0, z);
        }
        return z;
      },
      [](int, int, int, float t) { return ln_elu(t); });
}

template <int R, typename... D>
__global__ __launch_bounds__(64 * LS_NW) void k_lnmlp_fwd_bf16(LnBf16P p, D... dr) {
  constexpr int ROWS = 32 * R;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int net = blockIdx.y, H = p.n_layers - 1, ld = p.ld;
  const long long row0 = (long long)blockIdx.x * ROWS;
  uint16_t* img = reinterpret_cast<uint16_t*>(ls_sm);
  float* tab1 = reinterpret_cast<float*>(ls_sm + (size_t)ROWS * ld * sizeof(uint16_t));
  float* tab2 = tab1 + LS_NW * ROWS;
  ls_stage<ROWS>(p, p.dims[0], img, ld, row0, tid);
  __syncthreads();
  const float* prm = p.arena + (long long)net * p.net_stride;
  const uint16_t* pk = p.packed + (long long)net * p.packed_net_stride;
  for (int l = 0; l < H; ++l) {
    const int KS = (p.dims[l] + 15) >> 4, N = p.dims[l + 1];
    const uint4* w = reinterpret_cast<const uint4*>(pk + p.p_off[l]);
    const float *bias = prm + p.b_off[l], *ga = prm + p.g_off[l], *be = prm + p.be_off[l];
    const uint16_t* wout = l == H - 1 ? pk + p.p_off[H] : nullptr;
    const int ntw = ((N >> 5) + LS_NW - 1) / LS_NW;   // (block-uniform: the barriers inside are reached by every wave)
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
  ls_q_write<R>(tab1, p.dims[H], prm + p.b_off[H], p.q + (long long)net * p.m * 32, row0, p.m, tid);
}

// fp32 arena -> the packed bf16 copy, one unit per thread and step: packed[net][layer] is a hidden layer in lnstack.h's fragment order,
// the output layer (one row of dims[H] weights) as it lies: packed[net][H][k] = bf16(W[0][k]).  A unit's layer comes from the table
// of first units.
__global__ __launch_bounds__(256) void k_lnmlp_pack_bf16(LnPackBf16P p) {
  const long long total = p.units_per_net * p.n_nets;
  for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < total; u += (long long)gridDim.x * 256) {
    const long long net = u / p.units_per_net, v = u - net * p.units_per_net;
    int l = 0;
    for (int k = 1; k < p.n_layers; ++k)
      if (v >= p.u_off[k]) l = k;
    const long long wq = v - p.u_off[l];
    const int K = p.dims[l];
    const float* src = p.arena + net * p.net_stride + p.w_off[l];
    int k0 = (int)(8 * wq);
    if (l < p.n_layers - 1) {
      int row;
      ls_pack_unit(wq, K, &row, &k0);
      src += (long long)row * ((K + 31) & ~31);
    }
    reinterpret_cast<uint4*>(p.packed)[u] = ls_pack8(src, k0, K);
  }
}

// ---- host side
struct LnBf16Layout {
  int n_layers, n_nets, r, ld;                                  // r: row tiles per block; ld: the image's row length in bf16 elements
  int dims[PQLK_MAX_LAYERS + 1];
  int64_t lin_off[PQLK_MAX_LAYERS], gamma_off[PQLK_MAX_LAYERS], beta_off[PQLK_MAX_LAYERS], net_stride;   // the arena law, floats
  int64_t p_off[PQLK_MAX_LAYERS], packed_net_elems;             // the packed copy, bf16 elements
};

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
  d.ld = cols + LS_PAD_BF16;
  d.r = ls_r2_ok(ls_lds_bytes_bf16(d.ld, 2), widest) ? 2 : 1;
  if (ls_lds_bytes_bf16(d.ld, d.r) > (size_t)LS_LDS_MAX) return false;   // (bounds the input width: a 32-row bf16 image and its tables)
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
  if (int rc = ls_forward_args(ldx, d.dims[0], arena, packed, x, q_out)) return rc;
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
  return ls_launch<&k_lnmlp_fwd_bf16<1, D...>, &k_lnmlp_fwd_bf16<2, D...>>(d.r, m, d.n_nets, ls_lds_bytes_bf16(d.ld, d.r), stream, p, dr...);
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
