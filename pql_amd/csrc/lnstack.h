// What the whole-stack launches of the LayerNorm critic family share (fwd_ln.hip, fwd_ln_bf16.hip, fwd_bro.hip, fwd_bro_bf16.hip,
// bwd_ln.hip): the block geometry, the staging of the input tile, the fp32 linear's steps and Q tail, the bf16 layer with its row sums
// in registers, the packed bf16 weight unit, and the host code that checks a forward's arguments and launches at R = 1 or 2.  Each file
// keeps what is its own: its parameter struct and arena walk, its loop schedule, its norm step or epilogue expression.
//
// The geometry: a block of LS_NW waves owns 32 R batch rows through every layer, their activations in ONE LDS image [row][feature].
// A linear has the WEIGHT tile as the MFMA's A operand and the image as B, so a lane holds one batch row (lane = 32 h + r: row r) and
// accumulator registers 4 g .. 4 g + 3 are the four consecutive features n0 = 32 t + 8 g + 4 h .. n0 + 3 of tile t.  Wave w takes the
// 32-feature tiles w, w + 8, ..: at most NTW, and NTW x R x 16 <= 64 accumulator registers, which is what LS_MAX_R2_WIDTH says.
#pragma once
#include "bf16.h"
#include "lnrow.h"

constexpr int LS_NW = 8;                 // waves per block
constexpr int LS_LDS_MAX = 160 * 1024;
constexpr int LS_PAD = 4;                // floats of row padding in an fp32 image (16 B: consecutive rows start 4 banks apart)
constexpr int LS_PAD_BF16 = 8;           // bf16 elements of row padding in a bf16 image (the same 16 B)
constexpr int LS_MAX_R2_WIDTH = 512;     // widest hidden layer at R = 2: 2 tiles x 2 row tiles x 16 = 64 accumulator registers

typedef __bf16 ls_bf16x8 __attribute__((ext_vector_type(8)));
typedef float ls_f32x16 __attribute__((ext_vector_type(16)));

extern __shared__ __attribute__((aligned(16))) unsigned char ls_sm[];

// this wave's tiles of a layer of NT tiles: wave, wave + 8, ...
__device__ __forceinline__ int ls_tiles(int NT, int wave) { return wave < NT ? (NT - 1 - wave) / LS_NW + 1 : 0; }

template <int R, int NTW>
__device__ __forceinline__ void ls_zero(ls_f32x16 (&acc)[NTW][R]) {
#pragma unroll
  for (int j = 0; j < NTW; ++j)
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][i][e] = 0.f;
}

// Stages the block's ROWS rows of the fp32 input p.X (K0 columns, row stride p.ldx) into the image: as they are (T = float) or rounded
// to bf16 (T = uint16_t).  Rows past p.m and columns from K0 up to the next multiple of the k step (8 fp32, 16 bf16) become zero.
// P: the kernel's parameter struct, taken as it lies (X, m, ldx).
template <int ROWS, typename T, typename P>
__device__ __forceinline__ void ls_stage(const P& p, int K0, T* img, int ld, long long row0, int tid) {
  constexpr int KSTEP = sizeof(T) == sizeof(float) ? 8 : 16;
  const int qpr = ((K0 + KSTEP - 1) & ~(KSTEP - 1)) >> 2;
  for (int i = tid; i < ROWS * qpr; i += 64 * LS_NW) {
    const int row = i / qpr, c = (i - row * qpr) << 2;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + row < p.m && c < K0) {   // c + 3 < ldx: ldx >= roundup(K0, 32), which ls_forward_args holds the caller to
      v = *reinterpret_cast<const float4*>(p.X + (row0 + row) * p.ldx + c);
      if (c + 1 >= K0) v.y = 0.f;
      if (c + 2 >= K0) v.z = 0.f;
      if (c + 3 >= K0) v.w = 0.f;
    }
    if constexpr (sizeof(T) == sizeof(float)) *reinterpret_cast<float4*>(img + row * ld + c) = v;
    else *reinterpret_cast<uint2*>(img + row * ld + c) = make_uint2(bf16_pack2(v.x, v.y), bf16_pack2(v.z, v.w));
  }
}

// ---- the fp32 linear z = W a + b (v_mfma_f32_32x32x2_f32), in steps: a file's loop over them is its schedule
// the fragments of k step s: the weights of this wave's tiles (row-major W from the arena: HBM / L2) and the activations of the
// block's row tiles (LDS), 16 bytes each.  wp = W + (32 wave + r) ldw + 4 h, ap = img + r ld + 4 h
template <int R, int NTW>
__device__ __forceinline__ void ls_fetch(const float* __restrict__ wp, int ldw, const float* ap, int ld, int s, int cnt,
                                         float4 (&wf)[NTW], float4 (&af)[R]) {
#pragma unroll
  for (int j = 0; j < NTW; ++j)
    if (j < cnt) wf[j] = *reinterpret_cast<const float4*>(wp + (long long)j * (32 * LS_NW) * ldw + 8 * s);
#pragma unroll
  for (int i = 0; i < R; ++i) af[i] = *reinterpret_cast<const float4*>(ap + 32 * i * ld + 8 * s);
}

// the four MFMAs of one k step per (tile, row tile): MFMA e takes columns 8 s + e (h = 0) and 8 s + 4 + e (h = 1), so an 8-wide k
// group is consumed in the order 0, 4, 1, 5, 2, 6, 3, 7
template <int R, int NTW>
__device__ __forceinline__ void ls_mfma(ls_f32x16 (&acc)[NTW][R], int cnt, const float4 (&wf)[NTW], const float4 (&af)[R]) {
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

// z = acc + b over the image, between the barrier behind which nobody reads the layer's input any more and the one behind which z is
// complete
template <int R, int NTW>
__device__ __forceinline__ void ls_write_z(const ls_f32x16 (&acc)[NTW][R], int cnt, const float* __restrict__ bias, float* img, int ld,
                                           int wave, int lane) {
  const int r = lane & 31, h = lane >> 5;
  __syncthreads();   // nobody reads the layer's input any more
#pragma unroll
  for (int j = 0; j < NTW; ++j)
    if (j < cnt) {
      const int t = wave + LS_NW * j;
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

// the output layer (width 1) on the row a wave holds under LnMap<VPL, true>: Q = sum_j y_j w_j + b as per-lane partials in register
// order (slots past the row's width hold 0), the butterfly, then the bias; Q goes to column 0 of the row's 32 floats, the rest zero
template <int VPL>
__device__ __forceinline__ void ls_q_row(const float (&y)[VPL], const float (&wo)[VPL], float bout, float* __restrict__ qrow, int lane) {
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) dot += y[i] * wo[i];
  const float qv = wave_sum(dot) + bout;
  if (lane < 8) *reinterpret_cast<float4*>(qrow + 4 * lane) = make_float4(lane == 0 ? qv : 0.f, 0.f, 0.f, 0.f);
}

// ---- the bf16 layer (v_mfma_f32_32x32x16_bf16): Linear from the packed copy, LayerNorm from the accumulator registers
// what a wave and a lane are to a hidden layer of N features; the same in every layer of a stack of one width
struct LsGeom {
  int N, ld, cnt, nw, r, h;   // ld: the image's row length; cnt: this wave's tiles; nw: the waves that hold features
  float n;
};
__device__ __forceinline__ LsGeom ls_geom(int N, int ld, int wave, int lane) {
  const int NT = N >> 5;
  return LsGeom{N, ld, ls_tiles(NT, wave), NT < LS_NW ? NT : LS_NW, lane & 31, lane >> 5, (float)N};
}

// the sum of a row's partials, one per wave that holds features, in wave order
__device__ __forceinline__ float ls_row_total(const float* tab, int rows, int row, int nw) {
  float t = tab[row];
  for (int w = 1; w < nw; ++w) t += tab[w * rows + row];
  return t;
}

// a lane's partials of its rows -> the lane pair (r, r + 32) folds its two halves -> one partial per row in the [wave][row] table
template <int R>
__device__ __forceinline__ void ls_row_partials(const LsGeom& g, float (&s)[R], float* tab, int wave) {
#pragma unroll
  for (int i = 0; i < R; ++i) {
    s[i] += __shfl_xor(s[i], 32, 64);
    if (g.cnt > 0 && g.h == 0) tab[wave * (32 * R) + 32 * i + g.r] = s[i];
  }
}

// One hidden layer for the block's 32 R rows: img holds a~ (16 KS columns, zeros past the input's width) and is overwritten with a~ of
// the next Linear -- or, with wout (the last hidden layer), the rows' Q partials are left in tab1 for ls_q_write.  w: the layer's
// packed weights, tile t, k step ks: 64 fragments at (t KS + ks) 64, so a wave's 64 16-byte loads of one k step are one contiguous
// 1 KB run, fetched one k step ahead of the MFMAs that use them; the activations come with one ds_read_b128 per row tile and k step.
// z = acc + b never leaves the accumulator registers: lane partial in (tile, register) order, ls_row_partials, a barrier, the partials
// added in wave order; the same again for the squared deviations through tab2.  Three barriers, reached by every wave of the block;
// ends behind the one after which the image (or tab1) is complete.
// What a critic's layer adds is two expressions, inlined: fz(i, n0, z4) -> what is normalised in place of z = acc + b of row tile i,
// features n0 .. n0 + 3 (the dropout mask; else z4 itself); fy(j, i, e, t) -> y of accumulator register e of (tile j, row tile i)
// from t = xhat gamma + beta (ELU; the skip).
template <int R, int NTW, typename FZ, typename FY>
__device__ __forceinline__ void ls_bf16_layer(const LsGeom& g, const uint4* __restrict__ w, int KS, const float* __restrict__ bias,
                                              const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                              const uint16_t* __restrict__ wout, uint16_t* img, float* tab1, float* tab2, int wave, int lane,
                                              FZ&& fz, FY&& fy) {
  constexpr int ROWS = 32 * R;
  const int r = g.r, h = g.h, cnt = g.cnt, nw = g.nw, ld = g.ld;
  ls_f32x16 acc[NTW][R];
  ls_zero<R, NTW>(acc);
  if (cnt > 0) {
    const uint4* wp = w + (long long)wave * KS * 64 + lane;
    const long long tstep = (long long)LS_NW * KS * 64;
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
            acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(ls_bf16x8, wf[j]), __builtin_bit_cast(ls_bf16x8, af[i]),
                                                                acc[j][i], 0, 0, 0);
        }
#pragma unroll
      for (int j = 0; j < NTW; ++j) wf[j] = wn[j];
    }
  }
  // ---- z = acc + b (through fz) stays in acc; the row sum: this lane's features in (tile, register) order, the lane pair, the waves
  float s[R];
#pragma unroll
  for (int i = 0; i < R; ++i) s[i] = 0.f;
#pragma unroll
  for (int j = 0; j < NTW; ++j)
    if (j < cnt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n0 = 32 * (wave + LS_NW * j) + 8 * q + 4 * h;   // accumulator registers 4q .. 4q+3 = features n0 .. n0+3 of row r
        const float4 b4 = *reinterpret_cast<const float4*>(bias + n0);
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const float4 z = fz(i, n0, make_float4(acc[j][i][4 * q] + b4.x, acc[j][i][4 * q + 1] + b4.y, acc[j][i][4 * q + 2] + b4.z,
                                                 acc[j][i][4 * q + 3] + b4.w));
          acc[j][i][4 * q] = z.x; acc[j][i][4 * q + 1] = z.y; acc[j][i][4 * q + 2] = z.z; acc[j][i][4 * q + 3] = z.w;
#pragma unroll
          for (int e = 0; e < 4; ++e) s[i] += acc[j][i][4 * q + e];
        }
      }
    }
  ls_row_partials<R>(g, s, tab1, wave);
  __syncthreads();   // the partials are there, and nobody reads the layer's input any more
  // ---- d = z - mean stays in acc; the sum of d * d the same way
#pragma unroll
  for (int i = 0; i < R; ++i) s[i] = 0.f;
  if (cnt > 0) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const float mu = ls_row_total(tab1, ROWS, 32 * i + r, nw) / g.n;
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
  ls_row_partials<R>(g, s, tab2, wave);
  __syncthreads();   // (tab1 has been read by everybody: the output layer may write over it)
  // ---- y = fy(xhat gamma + beta), a~ = bf16(y): into the image, or multiplied out with the output layer's weights
  float rs[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    rs[i] = 0.f;
    s[i] = 0.f;
  }
  if (cnt > 0) {
#pragma unroll
    for (int i = 0; i < R; ++i) rs[i] = 1.0f / sqrtf(ls_row_total(tab2, ROWS, 32 * i + r, nw) / g.n + eps);
#pragma unroll
    for (int j = 0; j < NTW; ++j)
      if (j < cnt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n0 = 32 * (wave + LS_NW * j) + 8 * q + 4 * h;
          const float4 g4 = *reinterpret_cast<const float4*>(gamma + n0);
          const float4 e4 = *reinterpret_cast<const float4*>(beta + n0);
          const float ga[4] = {g4.x, g4.y, g4.z, g4.w}, be[4] = {e4.x, e4.y, e4.z, e4.w};
          uint2 wo = make_uint2(0u, 0u);
          if (wout) wo = *reinterpret_cast<const uint2*>(wout + n0);
#pragma unroll
          for (int i = 0; i < R; ++i) {
            float y[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = fy(j, i, 4 * q + e, acc[j][i][4 * q + e] * rs[i] * ga[e] + be[e]);
            if (!wout) {   // four features as one ds_write_b64
              *reinterpret_cast<uint2*>(img + (32 * i + r) * ld + n0) = make_uint2(bf16_pack2(y[0], y[1]), bf16_pack2(y[2], y[3]));
            } else {   // a product of two bf16 values is exact in fp32: only the additions round
              s[i] += bf16_round(y[0]) * __uint_as_float(wo.x << 16);
              s[i] += bf16_round(y[1]) * __uint_as_float(wo.x & 0xffff0000u);
              s[i] += bf16_round(y[2]) * __uint_as_float(wo.y << 16);
              s[i] += bf16_round(y[3]) * __uint_as_float(wo.y & 0xffff0000u);
            }
          }
        }
      }
  }
  if (wout) ls_row_partials<R>(g, s, tab1, wave);
  __syncthreads();   // the image (the Q partials) is complete
}

// Q = (the row's partials in tab1, in wave order) + *bout: column 0 of the row's 32 floats of the net's q, the rest zero; 8 threads
// write a row.  N: the last hidden layer's width
template <int R>
__device__ __forceinline__ void ls_q_write(const float* tab1, int N, const float* __restrict__ bout, float* __restrict__ q, long long row0,
                                           int m, int tid) {
  const int row = tid >> 3, quad = tid & 7, NT = N >> 5;
  if (row < 32 * R && row0 + row < m) {
    const float qv = ls_row_total(tab1, 32 * R, row, NT < LS_NW ? NT : LS_NW) + *bout;
    *reinterpret_cast<float4*>(q + (row0 + row) * 32 + 4 * quad) = make_float4(quad == 0 ? qv : 0.f, 0.f, 0.f, 0.f);
  }
}

// ---- the packed bf16 copy of a stack's weights, one 16-byte unit (8 elements) per thread and step.  A hidden layer, K padded to 16:
//   packed[tile n/32][k/16][lane = 32 h + r][j] = bf16(W[32 tile + r][16 (k/16) + 8 h + j])
// unit wq of such a layer -> its weight row and its first column
__device__ __forceinline__ void ls_pack_unit(long long wq, int K, int* row, int* k0) {
  const int lane = (int)(wq & 63), KS = (K + 15) >> 4;
  const long long kt = wq >> 6;
  const int t = (int)(kt / KS), ks = (int)(kt - (long long)t * KS);
  *row = 32 * t + (lane & 31);
  *k0 = 16 * ks + 8 * (lane >> 5);
}

// src[k0 .. k0 + 8) of a weight row of K columns, zeros from K on, as one unit
__device__ __forceinline__ uint4 ls_pack8(const float* __restrict__ src, int k0, int K) {
  float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (k0 + 8 <= K) {
    const float4 a = *reinterpret_cast<const float4*>(src + k0), b = *reinterpret_cast<const float4*>(src + k0 + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (k0 + j < K) f[j] = src[k0 + j];
  }
  return make_uint4(bf16_pack2(f[0], f[1]), bf16_pack2(f[2], f[3]), bf16_pack2(f[4], f[5]), bf16_pack2(f[6], f[7]));
}

// ---- host side
static int64_t ls_round4(int64_t x) { return (x + 3) & ~(int64_t)3; }

// LDS of a block of 32 r rows: an fp32 image of `cols` columns; a bf16 image of row length ld and its two [wave][row] tables
static size_t ls_lds_bytes(int cols, int r) { return (size_t)32 * r * (cols + LS_PAD) * sizeof(float); }
static size_t ls_lds_bytes_bf16(int ld, int r) { return (size_t)32 * r * ld * sizeof(uint16_t) + (size_t)2 * LS_NW * 32 * r * sizeof(float); }

// whether a block may take 64 rows: their LDS fits and no hidden layer is wider than the accumulators allow
static bool ls_r2_ok(size_t lds_bytes_r2, int widest) { return lds_bytes_r2 <= (size_t)LS_LDS_MAX && widest <= LS_MAX_R2_WIDTH; }

// what every forward asks of its input matrix (in_dim columns, row stride ldx) and of the pointers its kernels read in 16-byte runs
template <typename... Ptr>
static int ls_forward_args(int64_t ldx, int in_dim, Ptr... ptrs) {
  PQLK_REQUIRE(ldx % 32 == 0 && ldx >= pqlk_ld(in_dim), PQLK_E_ALIGN);
  PQLK_REQUIRE((pqlk_aligned16(ptrs) && ...), PQLK_E_ALIGN);
  return PQLK_OK;
}

// Launches K1 (r = 1) or K2 (r = 2), the two row-tile counts of one kernel, over m rows: ceil(m / 32 r) x grid_y blocks of LS_NW waves
// with lds_bytes of dynamic LDS.  The first launch of a pair on a device raises the pair's dynamic-LDS limit there.
template <auto K1, auto K2, typename... Args>
static int ls_launch(int r, int64_t m, int grid_y, size_t lds_bytes, pqlk_stream_t stream, Args... args) {
  static PqlkPerDeviceOnce attr_once;   // (one per pair of kernels)
  if (int arc = attr_once.run([] {
        for (const void* k : {reinterpret_cast<const void*>(K1), reinterpret_cast<const void*>(K2)}) {
          hipError_t err = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, LS_LDS_MAX);
          if (err != hipSuccess) return -(int)err;
        }
        return 0;
      }))
    return arc;
  dim3 grid((unsigned)((m + 32 * r - 1) / (32 * r)), (unsigned)grid_y), block(64 * LS_NW);
  if (r == 2) hipLaunchKernelGGL(K2, grid, block, lds_bytes, pqlk_s(stream), args...);
  else hipLaunchKernelGGL(K1, grid, block, lds_bytes, pqlk_s(stream), args...);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}
