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
// Linear and LayerNorm: lnstack.h's bf16 layer (weights from the packed copy of pqlk_bro_pack_bf16, z = acc + b and the row sums in the
// accumulator registers, three barriers per hidden layer); this file adds the epilogue expression of a stem, opening or closing layer.
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
#include "lnstack.h"

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

enum { BB_STEM = 0, BB_OPEN = 1, BB_CLOSE = 2 };

// One hidden layer for the block's 32 R rows, ls_bf16_layer with this critic's epilogue.  lay: [b | gamma | beta] of the layer in the
// arena.  KIND: BB_STEM / BB_OPEN: y = elu(xhat gamma + beta), BB_STEM keeps it in hs; BB_CLOSE: hs += xhat gamma + beta, y = hs --
// u = xhat gamma; u = u + beta; h_k = h_{k-1} + u, all fp32, the sum kept as it is.
template <int R, int NTW, int KIND>
__device__ __forceinline__ void bb_layer(const LsGeom& g, const uint4* __restrict__ w, int KS, const float* __restrict__ lay, float eps,
                                         const uint16_t* __restrict__ wout, uint16_t* img, float* tab1, float* tab2,
                                         ls_f32x16 (&hs)[NTW][R], int wave, int lane) {
  ls_bf16_layer<R, NTW>(
      g, w, KS, lay, lay + g.N, lay + 2 * g.N, eps, wout, img, tab1, tab2, wave, lane, [](int, int, float4 z) { return z; },
      [&](int j, int i, int e, float t) {
        const float y = KIND != BB_CLOSE ? ln_elu(t) : hs[j][i][e] + t;
        if constexpr (KIND != BB_OPEN) hs[j][i][e] = y;
        return y;
      });
}

// every layer of one net for the block's rows, at one geometry (<= NTW tiles per wave); leaves the rows' Q partials in tab1
template <int R, int NTW>
__device__ __forceinline__ void bb_stack(const BroBf16P& p, const float* __restrict__ prm, const uint16_t* __restrict__ pk, uint16_t* img,
                                         float* tab1, float* tab2, int wave, int lane) {
  const int W = p.W, K = p.K;
  const LsGeom g = ls_geom(W, p.ld, wave, lane);   // the same in every hidden layer: hoisted out of the layer loop
  const int KS0 = (p.in_dim + 15) >> 4, KS = W >> 4;
  const long long pstem = (long long)W * KS0 * 16, pblk = (long long)W * W;   // packed elements of the stem / of a block layer
  const long long wstem = (long long)W * p.ldin, wblk = (long long)W * W;     // floats in front of [b | gamma | beta] in the arena
  const uint16_t* wout = pk + pstem + 2 * K * pblk;                            // the output layer's row of W weights
  ls_f32x16 hs[NTW][R];
  ls_zero<R, NTW>(hs);
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
__global__ __launch_bounds__(64 * LS_NW) void k_bro_fwd_bf16(BroBf16P p) {
  constexpr int ROWS = 32 * R;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int net = blockIdx.y, ld = p.ld;
  const long long row0 = (long long)blockIdx.x * ROWS;
  uint16_t* img = reinterpret_cast<uint16_t*>(ls_sm);
  float* tab1 = reinterpret_cast<float*>(ls_sm + (size_t)ROWS * ld * sizeof(uint16_t));
  float* tab2 = tab1 + LS_NW * ROWS;
  ls_stage<ROWS>(p, p.in_dim, img, ld, row0, tid);
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
  ls_q_write<R>(tab1, W, prm + p.net_stride - 32, p.q + (long long)net * p.m * 32, row0, p.m, tid);   // [Wo (W) | bo (32)] ends a net
}

// fp32 arena -> the packed bf16 copy, one unit per thread and step: packed[net][layer] is a hidden layer in lnstack.h's fragment order,
// the output layer (one row of W weights) as it lies: packed[net][2 K + 1][k] = bf16(Wo[0][k]).  A unit's layer comes from arithmetic:
// the stem's units, then the uniform block layers by division, then the output row.
__global__ __launch_bounds__(256) void k_bro_pack_bf16(BroPackBf16P p) {
  const long long total = p.units_per_net * p.n_nets;
  for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < total; u += (long long)gridDim.x * 256) {
    const long long net = u / p.units_per_net, v = u - net * p.units_per_net;
    const float* src = p.arena + net * p.net_stride;
    int K = p.W, ldw = p.W;
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
    int k0 = (int)(8 * wq);
    if (!out) {
      int row;
      ls_pack_unit(wq, K, &row, &k0);
      src += (long long)row * ldw;
    }
    reinterpret_cast<uint4*>(p.packed)[u] = ls_pack8(src, k0, K);
  }
}

// ---- host side
struct BroBf16Layout {
  int in_dim, ldin, W, K, n_nets, r, ld;          // r: row tiles per block; ld: the image's row length in bf16 elements
  int64_t stem, blk, net_stride;                   // the arena law, floats: layer 0, a block layer, a net
  int64_t p_stem, p_blk, packed_net_elems;         // the packed copy, bf16 elements
};

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
  d.ld = (kin > width ? kin : width) + LS_PAD_BF16;
  d.r = ls_r2_ok(ls_lds_bytes_bf16(d.ld, 2), width) ? 2 : 1;
  if (ls_lds_bytes_bf16(d.ld, d.r) > (size_t)LS_LDS_MAX) return false;   // (never: in_dim <= 1248 is an 82 KB image with its tables)
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
  if (int rc = ls_forward_args(ldx, in_dim, arena, packed, x, q_out)) return rc;
  BroBf16P p = {};
  p.X = x; p.arena = arena; p.packed = packed; p.q = q_out;
  p.net_stride = d.net_stride; p.packed_net_stride = d.packed_net_elems;
  p.in_dim = d.in_dim; p.ldin = d.ldin; p.W = d.W; p.K = d.K; p.m = (int)m; p.ldx = (int)ldx; p.ld = d.ld; p.eps = eps;
  return ls_launch<&k_bro_fwd_bf16<1>, &k_bro_fwd_bf16<2>>(d.r, m, d.n_nets, ls_lds_bytes_bf16(d.ld, d.r), stream, p);
}
