// Input gradient of the LayerNorm twin critic with its parameters frozen (DoubleQLayerNorm with algo.critic_fused_dx: the actor step
// of DDPG and SAC): ONE launch walks back through both nets and every layer, dq -> d sum_n(dq_n Q_n) / dx, from the stash slab that
// pqlk_lnmlp_forward wrote and the arena as it lies.  No weight gradient, no column sum: nothing crosses batch rows.  The per-layer
// form (a row launch of ln.hip and a one-layer backward GEMM per net and layer, a torch add of the nets, a torch slice and tanh
// factor) stays what it was; no existing kernel is touched.  The law is written op by op in include/pqlk.h.  (The gradient form of the
// chain, for the critic's own update -- dz to HBM, column sums, no layer-0 product -- is the second half of this file.)
//
// Work split: a block of 8 waves owns 32 * R batch rows through the whole chain and through BOTH nets, one after the other; the
// current gradient sits in ONE fp32 LDS image [row][feature], the forward's (lnmlp.h: row length = widest layer + 4 floats).
//
// Output layer (width 1): rank 1, d[j] = dq * w_out[j], written into the image by the whole block.
//
// Norm step: wave w takes rows w, w + 8, ... of the image with the register map of lnrow.h (LnMap<VPL, true>), y / z of the row from
// the stash in the map's vector loads, and runs the operations of ln.hip's k_ln_elu_bwd in its order: dz, written back in place, is
// bit for bit what pqlk_ln_elu_backward without parameter gradients gives on the same d.
//
// Product d_in[k] = sum_n dz[n] W[n][k]: v_mfma_f32_32x32x2_f32 with the WEIGHT tile as the A operand and the image as B, the
// reduction index being the layer's OUTPUT feature n.  Lane (r, h) of MFMA e of group s supplies W[8 s + 4 h + e][k0 + r] -- a dword
// load from row-major W (out, ld(in)), one contiguous 128-byte segment per half-wave -- and dz[row r][8 s + 4 h + e], component e of
// one ds_read_b128; an 8-wide n group is consumed in the forward's order 0, 4, 1, 5, 2, 6, 3, 7.  There is no packed or transposed
// copy of the weights.  The accumulator tile is 32 input features x 32 rows: registers 4 g .. 4 g + 3 of lane (r, h) are features
// k0 + 8 g + 4 h .. + 3 of row r, so the epilogue writes 16 bytes at a time.  Wave w takes the tiles w, w + 8, ... (at most 4 at
// R = 1, 2 at R = 2: 64 accumulator registers); a hidden layer's tiles all fit one pass, so the image is overwritten behind one
// barrier.  Layer 0 writes to dx, not to the image, and takes as many passes as its tiles need (an input of 1248 padded columns has
// 39); in the tanh form only the tiles that intersect [col0, col0 + cols) are formed at all.
//
// Summing the nets: net 0's layer-0 epilogue stores its partial to dx, net 1's re-reads the same elements -- the same lanes, the same
// addresses, so program order suffices --, adds (net 0 + net 1) and, in the tanh form, applies 1 - a^2 before it stores.  No atomics,
// no second launch.  A row's bits depend on neither m nor its position in the batch; rows at or past m are neither read nor written.
#include "lnmlp.h"

struct LnDxP {
  const float* arena; const float* stash; const float* dq; const float* tanh_of; float* dx;
  int64_t net_stride, stash_net_stride;
  int64_t w_off[PQLK_MAX_LAYERS], g_off[PQLK_MAX_LAYERS];                                                            // inside a net
  int64_t z_off[PQLK_MAX_LAYERS], y_off[PQLK_MAX_LAYERS], mean_off[PQLK_MAX_LAYERS], rstd_off[PQLK_MAX_LAYERS];   // inside a net's stash
  int dims[PQLK_MAX_LAYERS + 1];
  int n_layers, n_nets, m, ld, ld_dx, ld_a, col0, cols;
};

// LayerNorm + ELU backward over the block's rows of the image, a wave per row: d (grad of y) -> dz in place.  The body of ln.hip's
// k_ln_elu_bwd<VPL, true, false>, operation for operation.
template <int VPL>
__device__ __forceinline__ void ld_norm(float* img, int ld, int cols, int rows, long long row0, int m, const float* __restrict__ gamma,
                                        const float* __restrict__ y, const float* __restrict__ z, const float* __restrict__ mean,
                                        const float* __restrict__ rstd, int wave, int lane) {
  using M = LnMap<VPL, true>;
  float ga[VPL];
  ln_load<VPL, true>(gamma, cols, lane, ga);
  const float n = (float)cols;
  for (int rr = wave; rr < rows; rr += LS_NW) {
    const long long row = row0 + rr;
    if (row >= m) break;
    const float mu = mean[row], rs = rstd[row];
    float h[VPL], xh[VPL], yv[VPL];
    ln_load<VPL, true>(img + rr * ld, cols, lane, h);
    ln_load<VPL, true>(y + row * cols, cols, lane, yv);
    ln_load<VPL, true>(z + row * cols, cols, lane, xh);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const bool in = M::col(i, lane) < cols;
      const float g = in ? h[i] * (yv[i] > 0.f ? 1.f : yv[i] + 1.f) : 0.f;
      const float x = in ? (xh[i] - mu) * rs : 0.f;
      const float hh = g * ga[i];
      s1 += hh;
      s2 += hh * x;
      h[i] = hh; xh[i] = x;
    }
    const float c1 = wave_sum(s1) / n, c2 = wave_sum(s2) / n;
#pragma unroll
    for (int i = 0; i < VPL; ++i) h[i] = rs * (h[i] - c1 - xh[i] * c2);
    ln_store<VPL, true>(img + rr * ld, cols, lane, h);
  }
}

// d_in = dz W of one layer for the block's 32 R rows: img holds dz (N = 8 NS columns).  Tiles [t_lo, t_lo + T) of 32 input features.
// L0 false (a hidden layer: T <= 8 NTW, one pass): img is overwritten with d_in and the call ends behind the barrier after which it is
// complete.  L0 true (layer 0): the tiles go to p.dx in passes of 8 NTW, summed over the nets and, with TANH, through the tanh
// factor; the image is only read.
template <int R, int NTW, bool L0, bool TANH>
__device__ __forceinline__ void ld_product(const float* __restrict__ W, int ldw, int NS, float* img, int ld, int t_lo, int T, int wave,
                                           int lane, const LnDxP& p, long long row0, bool first, bool last) {
  const int r = lane & 31, h = lane >> 5;
  for (int u0 = 0; u0 < T; u0 += LS_NW * NTW) {   // (block-uniform; a hidden layer runs it once)
    const int left = T - u0;
    const int cnt = wave < left ? min((left - 1 - wave) / LS_NW + 1, NTW) : 0;   // this wave's tiles: u0 + wave, u0 + wave + 8, ...
    ls_f32x16 acc[NTW][R];
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
      for (int i = 0; i < R; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][i][e] = 0.f;
    if (cnt > 0) {
      const float* wp = W + (size_t)(4 * h) * ldw + 32 * (t_lo + u0 + wave) + r;
      const float* ap = img + r * ld + 4 * h;
      float wf[NTW][4];
#pragma unroll
      for (int j = 0; j < NTW; ++j)
        if (j < cnt)
#pragma unroll
          for (int e = 0; e < 4; ++e) wf[j][e] = wp[(size_t)e * ldw + 32 * LS_NW * j];
      for (int s = 0; s < NS; ++s) {
        float wn[NTW][4];
        if (s + 1 < NS) {   // the next group's weights, under this group's MFMAs
          const float* wq = wp + (size_t)(8 * (s + 1)) * ldw;
#pragma unroll
          for (int j = 0; j < NTW; ++j)
            if (j < cnt)
#pragma unroll
              for (int e = 0; e < 4; ++e) wn[j][e] = wq[(size_t)e * ldw + 32 * LS_NW * j];
        }
        float4 af[R];
#pragma unroll
        for (int i = 0; i < R; ++i) af[i] = *reinterpret_cast<const float4*>(ap + 32 * i * ld + 8 * s);
#pragma unroll
        for (int e = 0; e < 4; ++e)   // MFMA e: reduction slots n = 8 s + e (h = 0) and 8 s + 4 + e (h = 1)
#pragma unroll
          for (int j = 0; j < NTW; ++j)
            if (j < cnt) {
#pragma unroll
              for (int i = 0; i < R; ++i) {
                const float av = e == 0 ? af[i].x : e == 1 ? af[i].y : e == 2 ? af[i].z : af[i].w;
                acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[j][e], av, acc[j][i], 0, 0, 0);
              }
            }
        if (s + 1 < NS) {
#pragma unroll
          for (int j = 0; j < NTW; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) wf[j][e] = wn[j][e];
        }
      }
    }
    if constexpr (!L0) __syncthreads();   // nobody reads dz any more
#pragma unroll
    for (int j = 0; j < NTW; ++j)
      if (j < cnt) {
        const int t = t_lo + u0 + wave + LS_NW * j;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c0 = 32 * t + 8 * g + 4 * h;   // accumulator registers 4g .. 4g+3 = input features c0 .. c0+3 of row r
#pragma unroll
          for (int i = 0; i < R; ++i) {
            float v[4] = {acc[j][i][4 * g], acc[j][i][4 * g + 1], acc[j][i][4 * g + 2], acc[j][i][4 * g + 3]};
            if constexpr (!L0) {
              *reinterpret_cast<float4*>(img + (32 * i + r) * ld + c0) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
              const long long row = row0 + 32 * i + r;
              if (row >= p.m) continue;
              if constexpr (!TANH) {   // c0 + 3 < pqlk_ld(dims[0]) <= ld_dx; the pad columns are written as zeros
                float4* o = reinterpret_cast<float4*>(p.dx + row * p.ld_dx + c0);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  if (c0 + e >= p.dims[0]) v[e] = 0.f;
                if (!first) {
                  const float4 s0 = *o;
                  v[0] = s0.x + v[0]; v[1] = s0.y + v[1]; v[2] = s0.z + v[2]; v[3] = s0.w + v[3];
                }
                *o = make_float4(v[0], v[1], v[2], v[3]);
              } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const int jc = c0 + e - p.col0;
                  if (jc < 0 || jc >= p.cols) continue;
                  float* o = p.dx + row * p.ld_dx + jc;
                  float gsum = first ? v[e] : *o + v[e];
                  if (last) {
                    const float a = p.tanh_of[row * p.ld_a + jc];
                    gsum = gsum * (1.0f - a * a);
                  }
                  *o = gsum;
                }
              }
            }
          }
        }
      }
    if constexpr (!L0) __syncthreads();   // d_in is complete
  }
}

template <int R, bool TANH>
__global__ __launch_bounds__(64 * LS_NW) void k_lnmlp_dx(LnDxP p) {
  constexpr int NTW_MAX = R == 2 ? 2 : 4;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int H = p.n_layers - 1, ld = p.ld;
  const long long row0 = (long long)blockIdx.x * (32 * R);
  float* img = reinterpret_cast<float*>(ls_sm);
  for (int net = 0; net < p.n_nets; ++net) {
    const float* prm = p.arena + (long long)net * p.net_stride;
    const float* sb = p.stash + (long long)net * p.stash_net_stride;
    const float* dq = p.dq + (long long)net * p.m * 32;
    if (net > 0) __syncthreads();   // the previous net's layer 0 has read the image
    // the output layer: d[j] = dq * w_out[j]; rows past m become zero
    {
      const int N = p.dims[H], qpr = N >> 2;
      const float* wout = prm + p.w_off[H];
      for (int i = tid; i < 32 * R * qpr; i += 64 * LS_NW) {
        const int row = i / qpr, c = (i - row * qpr) << 2;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + row < p.m) {
          const float q = dq[(row0 + row) * 32];
          const float4 w4 = *reinterpret_cast<const float4*>(wout + c);
          v = make_float4(q * w4.x, q * w4.y, q * w4.z, q * w4.w);
        }
        *reinterpret_cast<float4*>(img + row * ld + c) = v;
      }
    }
    __syncthreads();
    for (int l = H - 1; l >= 0; --l) {
      const int K = p.dims[l], N = p.dims[l + 1], ldw = (K + 31) & ~31;
      const float* ga = prm + p.g_off[l];
#define LD_NORM(VPL) ld_norm<VPL>(img, ld, N, 32 * R, row0, p.m, ga, sb + p.y_off[l], sb + p.z_off[l], sb + p.mean_off[l], sb + p.rstd_off[l], wave, lane)
      if (N <= 128) LD_NORM(2);
      else if (N <= 256) LD_NORM(4);
      else if (R == 2 || N <= 512) LD_NORM(8);
      else if constexpr (R == 1) LD_NORM(16);
#undef LD_NORM
      __syncthreads();   // dz is complete
      const float* W = prm + p.w_off[l];
      const bool first = net == 0, last = net == p.n_nets - 1;
      int t_lo = 0, T = ldw >> 5;
      if (TANH && l == 0) { t_lo = p.col0 >> 5; T = ((p.col0 + p.cols - 1) >> 5) - t_lo + 1; }
      const int ntw = min((T + LS_NW - 1) / LS_NW, NTW_MAX);   // (block-uniform: the barriers inside are reached by every wave)
#define LD_PRODUCT(NTW)                                                                                          \
  do {                                                                                                           \
    if (l > 0) ld_product<R, NTW, false, TANH>(W, ldw, N >> 3, img, ld, t_lo, T, wave, lane, p, row0, first, last); \
    else ld_product<R, NTW, true, TANH>(W, ldw, N >> 3, img, ld, t_lo, T, wave, lane, p, row0, first, last);     \
  } while (0)
      if (ntw == 1) LD_PRODUCT(1);
      else if (ntw == 2) LD_PRODUCT(2);
      else if constexpr (R == 1) {
        if (ntw == 3) LD_PRODUCT(3);
        else LD_PRODUCT(4);
      }
#undef LD_PRODUCT
    }
  }
}

// ---- host side
// rows per block = 32 R when the caller leaves the choice (r = 0).  A block takes both nets and the kernel's registers leave one block per
// CU, so what counts is the number of rounds of blocks over the MI355X's 256 CUs: tools/bench_lnmlp.py --dx has a 64-row block at 1.63x
// the time of a 32-row one, so R = 2 pays as soon as R = 1 needs a second round, m > 32 * 256 (measured at m = 8192 and 32768)
constexpr int64_t LD_CUS = 256;
static int ld_choose_r(bool r2_ok, int64_t m) { return r2_ok && (m + 31) / 32 > LD_CUS ? 2 : 1; }

extern "C" int pqlk_lnmlp_dx(const PqlMlpDesc* desc, const float* arena, const float* stash, const float* dq, int64_t m, float* dx,
                             int64_t ld_dx, int32_t col0, int32_t cols, const float* tanh_of, int64_t ld_a, int32_t r,
                             pqlk_stream_t stream) {
  PQLK_REQUIRE(desc && arena && stash && dq && dx, PQLK_E_NULL);
  LmLayout lay;
  PQLK_REQUIRE(lm_layout(desc, &lay) && m > 0 && m < (1LL << 30), PQLK_E_SHAPE);
  const LmLayout* d = &lay;
  const int L = d->n_layers;
  int widest = 0;
  for (int l = 1; l < L; ++l) widest = widest > d->dims[l] ? widest : d->dims[l];
  const bool r2_ok = ls_r2_ok(lm_lds_bytes(d, 2), widest);
  PQLK_REQUIRE(r == 0 || r == 1 || (r == 2 && r2_ok), PQLK_E_SHAPE);
  if (tanh_of) {
    PQLK_REQUIRE(col0 >= 0 && cols >= 1 && (int64_t)col0 + cols <= d->dims[0], PQLK_E_RANGE);
    PQLK_REQUIRE(ld_dx >= cols && ld_a >= cols && ld_a < (1LL << 30), PQLK_E_SHAPE);
  } else {
    PQLK_REQUIRE(ld_dx >= pqlk_ld(d->dims[0]), PQLK_E_SHAPE);
  }
  PQLK_REQUIRE(ld_dx < (1LL << 30), PQLK_E_SHAPE);
  PQLK_REQUIRE(ld_dx % 4 == 0, PQLK_E_ALIGN);
  PQLK_REQUIRE(pqlk_aligned16(arena) && pqlk_aligned16(stash) && pqlk_aligned16(dq) && pqlk_aligned16(dx) && pqlk_aligned16(tanh_of),
               PQLK_E_ALIGN);
  LnDxP p = {};
  p.arena = arena; p.stash = stash; p.dq = dq; p.tanh_of = tanh_of; p.dx = dx;
  p.net_stride = d->net_stride; p.stash_net_stride = lm_stash_net_floats(d, m);
  p.n_layers = L; p.n_nets = d->n_nets; p.m = (int)m; p.ld = lm_image_cols(d) + LS_PAD;
  p.ld_dx = (int)ld_dx; p.ld_a = (int)ld_a; p.col0 = tanh_of ? col0 : 0; p.cols = tanh_of ? cols : d->dims[0];
  for (int l = 0; l <= L; ++l) p.dims[l] = d->dims[l];
  for (int l = 0; l < L; ++l) {
    p.w_off[l] = d->lin_off[l];
    if (l == L - 1) break;
    p.g_off[l] = d->gamma_off[l];
    int64_t unused;
    lm_stash_at(d, m, l, PQLK_LNMLP_Z, &p.z_off[l], &unused);
    lm_stash_at(d, m, l, PQLK_LNMLP_Y, &p.y_off[l], &unused);
    lm_stash_at(d, m, l, PQLK_LNMLP_MEAN, &p.mean_off[l], &unused);
    lm_stash_at(d, m, l, PQLK_LNMLP_RSTD, &p.rstd_off[l], &unused);
  }
  const int rr = r ? r : ld_choose_r(r2_ok, m);
  if (tanh_of) return ls_launch<&k_lnmlp_dx<1, true>, &k_lnmlp_dx<2, true>>(rr, m, 1, lm_lds_bytes(d, rr), stream, p);
  return ls_launch<&k_lnmlp_dx<1, false>, &k_lnmlp_dx<2, false>>(rr, m, 1, lm_lds_bytes(d, rr), stream, p);
}

// ---- the gradient form: the chain of the critic's own update (pqlk_lnmlp_grad_chain; DoubleQLayerNorm with algo.critic_fused_backward)
// The same block, the same image, the same norm step and hidden-layer products -- dz of every (net, hidden layer) has k_lnmlp_dx's
// bits -- with three differences.  No layer-0 product: the update needs no dx, the chain ends behind layer 0's norm step, so the image
// row is the widest HIDDEN layer + LS_PAD.  dz goes to HBM too, a matrix (m, dims[l + 1]) per net and layer in the workspace: the dy
// operand of the weight-gradient GEMMs, which stay what they are.  And the norm step forms the column sums dbeta_j = sum_r g_rj,
// dgamma_j = sum_r g_rj xhat_rj from the g and xhat it holds anyway.  Their unit is a 32-row tile, whatever R: wave w adds rows w, w + 8,
// w + 16, w + 24 of the tile in row order in 2 VPL registers per lane; the 8 waves are then added in wave order through ONE table of
// 2 N floats behind the image (wave 0 stores, wave 1 .. 6 add to it, wave 7 adds and stores the tile's partial row to the workspace,
// part[net][layer][tile][{0: dbeta, 1: dgamma}][N], in the map's vector stores).  k_lnmlp_grad_fold, a second launch for every net and
// layer at once, adds the ceil(m / 32) tile rows as k_ln_fold of ln.hip does.  No float atomics, no ticket, no cross-block wait.
struct LnGradP {
  LnDxP c;   // the chain's arguments (dx, tanh_of, ld_dx, ld_a, col0, cols unused; ld = widest hidden layer + LS_PAD)
  float* ws;
  float* grads;
  int64_t dz_off[2][PQLK_MAX_LAYERS], part_off[2][PQLK_MAX_LAYERS];   // in ws, per net and hidden layer
  int64_t b_off[PQLK_MAX_LAYERS];                                     // beta inside a net (gamma: c.g_off)
  int tab, tiles;                                                     // floats from the image's start to the table; ceil(m / 32)
};

// ld_norm over the block's `tiles` 32-row tiles, with dz also stored to its matrix and the tile's column sums to its partial row.
// Every wave reaches every barrier: the tile loop's bounds are block-uniform.
template <int VPL>
__device__ __forceinline__ void ld_norm_sums(float* img, int ld, int cols, int tiles, long long row0, int m, const float* __restrict__ gamma,
                                             const float* __restrict__ y, const float* __restrict__ z, const float* __restrict__ mean,
                                             const float* __restrict__ rstd, float* __restrict__ dz, float* tab, float* __restrict__ part,
                                             int wave, int lane) {
  using M = LnMap<VPL, true>;
  float ga[VPL];
  ln_load<VPL, true>(gamma, cols, lane, ga);
  const float n = (float)cols;
  for (int t = 0; t < tiles; ++t) {
    const long long trow = row0 + 32 * t;
    if (trow >= m) break;   // (block-uniform) a tile past m: no rows, no partial row
    float accb[VPL], accg[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) accb[i] = accg[i] = 0.f;
    for (int rr = wave; rr < 32; rr += LS_NW) {
      const long long row = trow + rr;
      if (row >= m) break;
      float* ir = img + (32 * t + rr) * ld;
      const float mu = mean[row], rs = rstd[row];
      float h[VPL], xh[VPL], yv[VPL];
      ln_load<VPL, true>(ir, cols, lane, h);
      ln_load<VPL, true>(y + row * cols, cols, lane, yv);
      ln_load<VPL, true>(z + row * cols, cols, lane, xh);
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const bool in = M::col(i, lane) < cols;
        const float g = in ? h[i] * (yv[i] > 0.f ? 1.f : yv[i] + 1.f) : 0.f;
        const float x = in ? (xh[i] - mu) * rs : 0.f;
        const float hh = g * ga[i];
        accb[i] += g; accg[i] += g * x;
        s1 += hh;
        s2 += hh * x;
        h[i] = hh; xh[i] = x;
      }
      const float c1 = wave_sum(s1) / n, c2 = wave_sum(s2) / n;
#pragma unroll
      for (int i = 0; i < VPL; ++i) h[i] = rs * (h[i] - c1 - xh[i] * c2);
      ln_store<VPL, true>(ir, cols, lane, h);
      ln_store<VPL, true>(dz + row * cols, cols, lane, h);
    }
    float* pr = part + (trow >> 5) * (2 * cols);
#pragma unroll
    for (int w = 0; w < LS_NW; ++w) {
      if (wave == w) {
        if (w > 0) {
          float tb[VPL], tg[VPL];
          ln_load<VPL, true>(tab, cols, lane, tb);
          ln_load<VPL, true>(tab + cols, cols, lane, tg);
#pragma unroll
          for (int i = 0; i < VPL; ++i) { accb[i] = tb[i] + accb[i]; accg[i] = tg[i] + accg[i]; }
        }
        float* o = w < LS_NW - 1 ? tab : pr;
        ln_store<VPL, true>(o, cols, lane, accb);
        ln_store<VPL, true>(o + cols, cols, lane, accg);
      }
      __syncthreads();   // the table is wave w + 1's; behind the last one it is free again and the tile's dz is complete
    }
  }
}

template <int R>
__global__ __launch_bounds__(64 * LS_NW) void k_lnmlp_grad(LnGradP q) {
  constexpr int NTW_MAX = R == 2 ? 2 : 4;
  const LnDxP& p = q.c;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int H = p.n_layers - 1, ld = p.ld;
  const long long row0 = (long long)blockIdx.x * (32 * R);
  float* img = reinterpret_cast<float*>(ls_sm);
  float* tab = img + q.tab;
  for (int net = 0; net < p.n_nets; ++net) {
    const float* prm = p.arena + (long long)net * p.net_stride;
    const float* sb = p.stash + (long long)net * p.stash_net_stride;
    const float* dq = p.dq + (long long)net * p.m * 32;
    // the output layer: d[j] = dq * w_out[j]; rows past m become zero (the previous net's last norm step ended behind a barrier)
    {
      const int N = p.dims[H], qpr = N >> 2;
      const float* wout = prm + p.w_off[H];
      for (int i = tid; i < 32 * R * qpr; i += 64 * LS_NW) {
        const int row = i / qpr, c = (i - row * qpr) << 2;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + row < p.m) {
          const float d = dq[(row0 + row) * 32];
          const float4 w4 = *reinterpret_cast<const float4*>(wout + c);
          v = make_float4(d * w4.x, d * w4.y, d * w4.z, d * w4.w);
        }
        *reinterpret_cast<float4*>(img + row * ld + c) = v;
      }
    }
    __syncthreads();
    for (int l = H - 1; l >= 0; --l) {
      const int K = p.dims[l], N = p.dims[l + 1];
      const float* ga = prm + p.g_off[l];
#define LD_NORM_SUMS(VPL)                                                                                                            \
  ld_norm_sums<VPL>(img, ld, N, R, row0, p.m, ga, sb + p.y_off[l], sb + p.z_off[l], sb + p.mean_off[l], sb + p.rstd_off[l],           \
                    q.ws + q.dz_off[net][l], tab, q.ws + q.part_off[net][l], wave, lane)
      if (N <= 128) LD_NORM_SUMS(2);
      else if (N <= 256) LD_NORM_SUMS(4);
      else if (R == 2 || N <= 512) LD_NORM_SUMS(8);
      else if constexpr (R == 1) LD_NORM_SUMS(16);
#undef LD_NORM_SUMS
      if (l == 0) break;   // no layer-0 product: the update needs no dx
      const int T = K >> 5;   // (a hidden layer's width is a multiple of 32)
      const int ntw = min((T + LS_NW - 1) / LS_NW, NTW_MAX);   // (block-uniform)
      const float* W = prm + p.w_off[l];
#define LD_PRODUCT(NTW) ld_product<R, NTW, false, false>(W, K, N >> 3, img, ld, 0, T, wave, lane, p, row0, false, false)
      if (ntw == 1) LD_PRODUCT(1);
      else if (ntw == 2) LD_PRODUCT(2);
      else if constexpr (R == 1) {
        if (ntw == 3) LD_PRODUCT(3);
        else LD_PRODUCT(4);
      }
#undef LD_PRODUCT
    }
  }
}

// dgamma, dbeta of every net and hidden layer <- the tile rows, in k_ln_fold's order: 16 columns x 16 groups of consecutive tiles per
// block, each group in tile order, then the groups in group order.  blockIdx.y: 0 -> dbeta, 1 -> dgamma; blockIdx.z: net * H + layer.
constexpr int LN_GRAD_FOLD_GROUPS = 16;
__global__ __launch_bounds__(256) void k_lnmlp_grad_fold(LnGradP q) {
  __shared__ float sh[LN_GRAD_FOLD_GROUPS][16];
  const int H = q.c.n_layers - 1, net = blockIdx.z / H, l = blockIdx.z - net * H;
  const int cols = q.c.dims[l + 1];
  if ((int)blockIdx.x * 16 >= cols) return;   // (uniform over the block) a narrower layer than the widest
  const int cl = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl, which = blockIdx.y;   // (c < cols: a multiple of 32)
  const float* part = q.ws + q.part_off[net][l];
  const int per = (q.tiles + LN_GRAD_FOLD_GROUPS - 1) / LN_GRAD_FOLD_GROUPS;
  const int k0 = g * per, k1 = min(q.tiles, k0 + per);
  float s = 0.f;
  for (int k = k0; k < k1; ++k) s += part[((int64_t)k * 2 + which) * cols + c];
  sh[g][cl] = s;
  __syncthreads();
  if (g == 0) {
    float t = sh[0][cl];
#pragma unroll
    for (int j = 1; j < LN_GRAD_FOLD_GROUPS; ++j) t += sh[j][cl];
    q.grads[(int64_t)net * q.c.net_stride + (which ? q.c.g_off[l] : q.b_off[l]) + c] = t;
  }
}

// ---- host side of the gradient form
static int lg_widest(const LmLayout* d) {
  int w = 0;
  for (int l = 1; l < d->n_layers; ++l) w = w > d->dims[l] ? w : d->dims[l];
  return w;
}
static size_t lg_lds_bytes(const LmLayout* d, int r) { return ((size_t)32 * r * (lg_widest(d) + LS_PAD) + 2 * lg_widest(d)) * sizeof(float); }
static bool lg_r2_ok(const LmLayout* d) { return ls_r2_ok(lg_lds_bytes(d, 2), lg_widest(d)); }
static int64_t lg_tiles(int64_t m) { return (m + 31) / 32; }

// the workspace: dz (m, dims[l + 1]) of every net and hidden layer, net after net, then the partial rows (tiles, 2, dims[l + 1]) in
// the same order.  Every width is a multiple of 32, so every offset is a multiple of 4.
static int64_t lg_ws_floats(const LmLayout* d, int64_t m) {
  int64_t o = 0;
  for (int l = 1; l < d->n_layers; ++l) o += (m + 2 * lg_tiles(m)) * d->dims[l];
  return o * d->n_nets;
}
static void lg_at(const LmLayout* d, int64_t m, int net, int layer, int64_t* dz_off, int64_t* part_off) {
  int64_t per_net = 0, before = 0;
  for (int l = 1; l < d->n_layers; ++l) {
    if (l - 1 < layer) before += d->dims[l];
    per_net += d->dims[l];
  }
  *dz_off = m * (net * per_net + before);
  *part_off = m * d->n_nets * per_net + 2 * lg_tiles(m) * (net * per_net + before);
}

extern "C" int64_t pqlk_lnmlp_grad_ws_floats(const PqlMlpDesc* desc, int64_t m) {
  LmLayout d;
  return desc && lm_layout(desc, &d) && m > 0 && m < (1LL << 30) ? lg_ws_floats(&d, m) : 0;
}

extern "C" int pqlk_lnmlp_grad_offset(const PqlMlpDesc* desc, int64_t m, int32_t net, int32_t layer, int64_t* off, int64_t* ld) {
  PQLK_REQUIRE(desc && off && ld, PQLK_E_NULL);
  LmLayout d;
  PQLK_REQUIRE(lm_layout(desc, &d) && m > 0 && m < (1LL << 30), PQLK_E_SHAPE);
  PQLK_REQUIRE(net >= 0 && net < d.n_nets && layer >= 0 && layer < d.n_layers - 1, PQLK_E_RANGE);
  int64_t unused;
  lg_at(&d, m, net, layer, off, &unused);
  *ld = d.dims[layer + 1];
  return PQLK_OK;
}

extern "C" int pqlk_lnmlp_grad_chain(const PqlMlpDesc* desc, const float* arena, const float* stash, const float* dq, int64_t m, float* ws,
                                     int64_t ws_floats, float* grads, int32_t r, pqlk_stream_t stream) {
  PQLK_REQUIRE(desc && arena && stash && dq && ws && grads, PQLK_E_NULL);
  LmLayout lay;
  PQLK_REQUIRE(lm_layout(desc, &lay) && lay.n_nets <= 2 && m > 0 && m < (1LL << 30), PQLK_E_SHAPE);
  const LmLayout* d = &lay;
  const int L = d->n_layers;
  const bool r2_ok = lg_r2_ok(d);
  PQLK_REQUIRE(r == 0 || r == 1 || (r == 2 && r2_ok), PQLK_E_SHAPE);
  PQLK_REQUIRE(ws_floats >= lg_ws_floats(d, m), PQLK_E_SHAPE);
  PQLK_REQUIRE(pqlk_aligned16(arena) && pqlk_aligned16(stash) && pqlk_aligned16(dq) && pqlk_aligned16(ws) && pqlk_aligned16(grads),
               PQLK_E_ALIGN);
  LnGradP q = {};
  LnDxP& p = q.c;
  p.arena = arena; p.stash = stash; p.dq = dq;
  p.net_stride = d->net_stride; p.stash_net_stride = lm_stash_net_floats(d, m);
  p.n_layers = L; p.n_nets = d->n_nets; p.m = (int)m; p.ld = lg_widest(d) + LS_PAD;
  q.ws = ws; q.grads = grads; q.tiles = (int)lg_tiles(m);
  for (int l = 0; l <= L; ++l) p.dims[l] = d->dims[l];
  for (int l = 0; l < L; ++l) {
    p.w_off[l] = d->lin_off[l];
    if (l == L - 1) break;
    p.g_off[l] = d->gamma_off[l]; q.b_off[l] = d->beta_off[l];
    int64_t unused;
    lm_stash_at(d, m, l, PQLK_LNMLP_Z, &p.z_off[l], &unused);
    lm_stash_at(d, m, l, PQLK_LNMLP_Y, &p.y_off[l], &unused);
    lm_stash_at(d, m, l, PQLK_LNMLP_MEAN, &p.mean_off[l], &unused);
    lm_stash_at(d, m, l, PQLK_LNMLP_RSTD, &p.rstd_off[l], &unused);
    for (int n = 0; n < d->n_nets; ++n) lg_at(d, m, n, l, &q.dz_off[n][l], &q.part_off[n][l]);
  }
  const int rr = r ? r : ld_choose_r(r2_ok, m);
  q.tab = 32 * rr * p.ld;
  if (int rc = ls_launch<&k_lnmlp_grad<1>, &k_lnmlp_grad<2>>(rr, m, 1, lg_lds_bytes(d, rr), stream, q)) return rc;
  hipLaunchKernelGGL(k_lnmlp_grad_fold, dim3((unsigned)((lg_widest(d) + 15) / 16), 2, (unsigned)(d->n_nets * (L - 1))), dim3(256), 0, pqlk_s(stream), q);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}
