// fp32 MFMA GEMMs for the MLP family and the per-MLP forward/backward drivers.
//
// Reference arithmetic: nn.Linear / ELU / tanh chains of pql/models/mlp.py:15-40,177-203,244-267 and
// their autograd.  All three products run on v_mfma_f32_32x32x2_f32 (exact fp32, k-ordered fma chain,
// 256 FLOP/clk/CU = the 157 TFLOP/s fp32 roof of gfx950):
//   FWD  Y[m,n]  = act( sum_k X[m,k] W[n,k] + b[n] )                 (X, W both k-contiguous)
//   DX   dX[m,k] = ( sum_g sum_n dY_g[m,n] W_g[n,k] ) * act'(H[m,k])  (dY k-contiguous, W reduction-row)
//   DW   dW[n,k] = sum_{m in split} dY[m,n] X[m,k] ; db[n] = sum_m dY[m,n]   (both reduction-row)
// Block = 256 threads = 2x2 waves, each wave a (BM/2)x(BN/2) patch of 32x32 MFMA tiles; reduction is
// walked in 32-wide steps through double-buffered LDS with register prefetch (one barrier per step).
//
// MFMA operand maps (cdna_hip_programming.md section 3): lane l = (r = l&31, h = l>>5):
//   A operand = A[i=r][k=h], B operand = B[k=h][j=r]; D: col = r, row = (reg&3) + 8*(reg>>2) + 4*h.
// The kernels feed the WEIGHT-side fragment as the MFMA's A operand and the batch-side fragment as B, i.e. they
// compute the transposed tile, so that a lane owns one output row and four consecutive columns per register quad.
// A 32-wide reduction step is consumed as 4 groups (k8) x 4 MFMAs (t); lane half h supplies reduction
// index kk = 8*k8 + 4*h + t.  A and B use the same map, so any such bijection is a valid dot product;
// this one lets k-contiguous operands be fetched with one ds_read_b128 per four MFMAs.
#include <cstdlib>
#include <type_traits>
#include "pqlk_common.h"
#include "skinny.h"
#include "fused.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { MODE_FWD = 0, MODE_DX = 1, MODE_DW = 2 };
enum { EPI_NONE = 0, EPI_ELU = 1, EPI_TANH = 2, EPI_TANH_NOISE = 3, EPI_DELU = 4, EPI_DTANH_SLICE = 5 };

struct GemmP {
  const float* A;
  const float* B;
  float* C;
  const float* bias;  // FWD: bias (per group); DW: unused
  const float* aux;   // FWD/TANH_NOISE: draw (M, N) contiguous; DX/DELU: H (M, ldaux); DX/DTANH: a (M, ldaux)
  float* C2;          // FWD: optional second destination of the final output (group 0 only)
  float* dbias;       // DW: bias-gradient slab (per group/split)
  int M, N, K;        // C is M x N; reduction length K (FWD: padded in-features; DX: out-features; DW: batch)
  int lda, ldb, ldc, ldaux, ldc2;
  int ncols_store;    // FWD/DX: columns [N, ncols_store) are written as zero (pad); DW: = N
  long long sA, sB, sC, sBias, sAux;  // per-group strides (floats)
  int groups;         // DX with zsum: groups summed inside the block; otherwise grid.z = groups
  int zsum;
  int splits;         // DW: grid.z = groups*splits, split s covers rows [s*rows_per_split, ...)
  int rows_per_split;
  long long sSplit;   // DW: floats between split slabs (C and dbias)
  int epi;
  int col0, ncol;     // DX/DTANH_SLICE: only columns [col0, col0+ncol) are written, compacted to column 0
  int n_base;         // first output column covered by the grid (multiple of 4)
  float noise_std, noise_clip;
  // "min-net" compaction of the DPG backward (minnet.h): rows of A / C are COMPACT rows -- the samples whose min(Q1, Q2) came
  // from net 0, then (from row mn[2] on, a multiple of 128) those of net 1 -- perm[i] = batch row of compact row i (-1: pad),
  // mn = {c0, c1, first row of net 1, rows in use (multiple of 128)}.  A row tile belongs to ONE net: the block picks that
  // net's weights (B) and activations (aux, row perm[i]); tiles past mn[3] exit at once.
  const int* perm;
  const int* mn;
  int xcd_remap;      // set by launch_gemm when the grid divides into whole groups per XCD
};

#include "narrow.h"
#include "minnet.h"

#define KT_MAX 32   // reduction elements per LDS stage (template parameter KT: 32 or 16)
#ifndef PQLK_KT
#define PQLK_KT 16   // 16: half the LDS per block -> a third block per CU; +3 % on the streamed learner step vs 32
#endif
// row stride of a k-contiguous tile = KT + 4 floats (36 or 20: odd multiple of 4 -> conflict-free b128 reads)

// Native 4-float vector for the register tiles: HIP's float4 is a struct whose copies lower to llvm.memcpy, and a memcpy
// from global into a private object that a later iteration stores to LDS is not promoted to registers (the tiles of the
// two-deep prefetch ended up in scratch memory).
typedef float f4v __attribute__((ext_vector_type(4)));

// ---- tile loaders: global -> registers -> LDS -------------------------------------------------
// k-contiguous tile: ROWS rows x 32 floats.  Chunk c (16 B): row = c>>3, kc = c&7.
template <int ROWS, int KT>
struct KcTile {
  static constexpr int CPR = KT / 4;            // 16-B chunks per row
  static constexpr int LD = KT + 4;
  static constexpr int CH = ROWS * CPR / 256;   // float4 chunks per thread
  f4v v[CH];
  __device__ __forceinline__ void load(const float* __restrict__ base, int ld, int row0, int row_lim, int k0, int k_lim,
                                       int tid) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = tid + 256 * i;
      const int row = row0 + c / CPR;
      const int k = k0 + ((c % CPR) << 2);
      if (row < row_lim && k < k_lim)
        v[i] = *reinterpret_cast<const f4v*>(base + (long long)row * ld + k);
      else
        v[i] = f4v{0.f, 0.f, 0.f, 0.f};
    }
  }
  // interior tile: no bounds tests, so the loads are straight-line code and the compiler can keep a later tile's loads
  // in flight behind a counted s_waitcnt vmcnt(N)
  __device__ __forceinline__ void load_inner(const float* __restrict__ base, int ld, int row0, int k0, int tid) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = tid + 256 * i;
      v[i] = *reinterpret_cast<const f4v*>(base + (long long)(row0 + c / CPR) * ld + k0 + ((c % CPR) << 2));
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ lds, int tid) const {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = tid + 256 * i;
      *reinterpret_cast<f4v*>(lds + (c / CPR) * LD + ((c % CPR) << 2)) = v[i];
    }
  }
};

// reduction-row tile: KT rows x COLS floats, row stride COLS+4.  Chunk c: row = c / (COLS/4), cc = c % (COLS/4).
template <int COLS, int KT>
struct RrTile {
  static constexpr int CPR = COLS / 4;
  static constexpr int CH = KT * CPR / 256;
  static constexpr int LD = COLS + 4;
  f4v v[CH];
  __device__ __forceinline__ void load(const float* __restrict__ base, int ld, int row0, int row_lim, int col0, int col_lim,
                                       int tid) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = tid + 256 * i;
      const int row = row0 + c / CPR;
      const int col = col0 + ((c % CPR) << 2);
      if (row < row_lim && col < col_lim)
        v[i] = *reinterpret_cast<const f4v*>(base + (long long)row * ld + col);
      else
        v[i] = f4v{0.f, 0.f, 0.f, 0.f};
    }
  }
  __device__ __forceinline__ void load_inner(const float* __restrict__ base, int ld, int row0, int col0, int tid) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = tid + 256 * i;
      v[i] = *reinterpret_cast<const f4v*>(base + (long long)(row0 + c / CPR) * ld + col0 + ((c % CPR) << 2));
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ lds, int tid) const {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = tid + 256 * i;
      *reinterpret_cast<f4v*>(lds + (c / CPR) * LD + ((c % CPR) << 2)) = v[i];
    }
  }
};

template <int MODE, int BM, int BN, int KT>
struct Smem {
  static constexpr int A_FLOATS = (MODE == MODE_DW) ? KT * (BM + 4) : BM * (KT + 4);
  static constexpr int B_FLOATS = (MODE == MODE_FWD) ? BN * (KT + 4) : KT * (BN + 4);
  static constexpr int STAGE = A_FLOATS + B_FLOATS;
};

// ELU(alpha=1).  exp through the hardware 2^x unit (__expf): absolute error <= ~1.2e-7 on (-inf, 0], two orders of
// magnitude inside the 1e-5 parity bar, and ~6 us cheaper per 8192x512x2 epilogue than libm's expm1f.
__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : __expf(x) - 1.f; }

// One output tile of one product; (bx, by, bz) = the block's place in a (gx, gy, .) grid of tiles.  (A device function so that one
// launch can host tiles of two products: dW_l and dX_l of a layer read the same dZ_l and nothing of each other, and a launch
// holding both -- round 3, `k_gemm_pair`, blocks of two different lengths per CU so that one's epilogue runs under the other's
// MFMA stream -- measured 2 % SLOWER than the two launches: 268.1 vs 262.7 us on the twin critic's backward, interleaved rounds
// on one box; the same verdict as round 2's fork onto a second stream.  Removed.)
template <int MODE, int BM, int BN, int EPI, int KT, bool DMA>
__device__ __forceinline__ void gemm_body(const GemmP& p, int bx, int by, int bz, const int gx, const int gy) {
  constexpr int WM = BM / 2, WN = BN / 2;  // per-wave patch
  constexpr int MI = WM / 32, NJ = WN / 32;
  constexpr int KC_LD = KT + 4;
  using S = Smem<MODE, BM, BN, KT>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // DMA = the LDS stages are filled by global_load_lds_dwordx4 (no VGPR round trip, no ds_write, four stages): unpadded tiles
  // whose 16-B slots are XOR-swizzled instead (a DMA instruction deposits one contiguous KiB, lane i at +16 i)
  static_assert(!DMA || MODE != MODE_FWD, "the LDS-DMA main loop serves the backward products");
  constexpr int SA_F = DMA ? BM * KT : S::A_FLOATS;              // floats of the A part of a stage
  constexpr int STG_F = DMA ? (BM + BN) * KT : S::STAGE;         // floats per stage
  constexpr int A_RLD = DMA ? BM : BM + 4, B_RLD = DMA ? BN : BN + 4;   // row stride of a reduction-row tile

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wm = (wave >> 1) * WM, wn = (wave & 1) * WN;
  // XCD-aware tile order.  Workgroups go to the 8 XCDs round robin in dispatch order (x fastest), so the tiles that share an
  // operand -- the column tiles of one row tile (dX / forward: the same rows of A), all tiles of one (net, batch split) of a dW
  // product (the same rows of dY and X) -- would sit under 8 different L2s and each fetch the operand across the fabric.
  // Re-label: dispatch slot w lands on XCD w % 8; give that XCD whole groups of G sharing tiles, G consecutive slots each.
  if (p.xcd_remap == 1) {
    const int G = (MODE == MODE_DW) ? gx * gy : gx;
    const int w = bx + gx * (by + gy * bz), sl = w >> 3;
    const int L = ((sl / G) * 8 + (w & 7)) * G + sl % G;
    bx = L % gx; by = (L / gx) % gy; bz = L / (gx * gy);
  } else if (p.xcd_remap > 1) {
    // any grid (p.xcd_remap = number of tiles): the slots of XCD class x = w % 8 take one CONTIGUOUS run of tile numbers, runs of
    // q or q + 1 tiles (q = tiles / 8) -- bijective for every tile count (cdna_hip_programming.md, 256^2 template).  The compact
    // dX products (66 x 8 tiles: not a whole number of 8-tile groups per XCD) ran without any re-labelling before: each of
    // their row tiles of dZ was fetched by eight L2s.
    const int nt = p.xcd_remap, q = nt >> 3, rr = nt & 7;
    const int w = bx + gx * (by + gy * bz), x = w & 7;
    const int L = (x < rr ? x * (q + 1) : rr * (q + 1) + (x - rr) * q) + (w >> 3);
    bx = L % gx; by = (L / gx) % gy; bz = L / (gx * gy);
  }
  const int m0 = by * BM, n0 = p.n_base + bx * BN;

  int g0 = 0, g1 = 1, split = 0;
  if (MODE == MODE_DX && p.perm) {   // compact rows: one net per row tile (sA = sC = 0, grid.z = 1 on the host side)
    if (m0 >= p.mn[3]) return;       // block-uniform, before any barrier
    g0 = m0 >= p.mn[2] ? 1 : 0;
    g1 = g0 + 1;
  } else if (MODE == MODE_DW) {
    g0 = bz / p.splits;
    split = bz % p.splits;
    g1 = g0 + 1;
  } else if (MODE == MODE_DX && p.zsum) {
    g0 = 0;
    g1 = p.groups;
  } else {
    g0 = bz;
    g1 = g0 + 1;
  }

  f32x16 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // Compact rows: the last tile of each net's run is mostly padding (a run is padded to a multiple of 128 rows).  A wave whose
  // WM-row patch holds no sample issues no MFMAs (its rows of C come out zero, as before): the block still takes part in every
  // DMA request and barrier, but its share of the CU's matrix pipe goes to the co-resident blocks.  The compact grid is 2.03-2.06
  // tiles per CU, so a few CUs host three blocks and set the launch's length; with this their third block is only as
  // expensive as its real rows (to WM-row granularity).  ONE wave-uniform branch per stage: per-sub-tile predicates cost registers.
  bool live = true;
  if (MODE == MODE_DX && p.perm) {
    const int c0 = p.mn[0], c1 = p.mn[1], base1 = p.mn[2], r0 = m0 + wm;
    live = __builtin_amdgcn_readfirstlane((r0 < c0 || (r0 >= base1 && r0 < base1 + c1)) ? 1 : 0) != 0;   // (a scalar branch)
  }

  float dbacc = 0.f;  // DW: partial column sum of dY for row tid % BM of this block's dW tile (bx == 0 only)

  // two register tile sets of the interior main loop (function scope: declared inside the group loop they are kept in
  // scratch memory instead of registers)
  KcTile<BM, KT> a_kc0, a_kc1;
  RrTile<BM, KT> a_rr0, a_rr1;
  KcTile<BN, KT> b_kc0, b_kc1;
  RrTile<BN, KT> b_rr0, b_rr1;

  for (int g = g0; g < g1; ++g) {
    const float* A = p.A + (long long)g * p.sA;
    const float* B = p.B + (long long)g * p.sB;
    // reduction range
    int kbeg = 0, kend = p.K;
    if (MODE == MODE_DW) {
      kbeg = split * p.rows_per_split;
      kend = min(p.K, kbeg + p.rows_per_split);
    }
    const int nk = (kend - kbeg + KT - 1) / KT;
    if (nk <= 0) continue;

    // one LDS stage -> MFMAs
    auto compute = [&](int kt, int stage) {
      const float* sa = smem + stage * STG_F;
      const float* sb = sa + SA_F;

      if (MODE == MODE_DW && bx == 0) {   // db: thread (column tid % BM, row group tid / BM) sums its rows of the dY stage
        constexpr int DBR = KT / (256 / BM);      // (all four waves share the work: on wave 0 alone the 16 dependent LDS
#pragma unroll                                    //  reads per stage held the whole block at the barrier, +5 us on a 26-us GEMM)
        for (int rr = 0; rr < DBR; ++rr) {
          const int row = (tid / BM) * DBR + rr;
          dbacc += sa[row * A_RLD + ((tid % BM) ^ (DMA ? ((row >> 2) & 1) * 32 : 0))];
        }
      }

      if (!live) return;   // (compact rows: a patch of padding only)
#pragma unroll
      for (int k8 = 0; k8 < KT / 8; ++k8) {
        float af[MI][4], bf[NJ][4];
        (void)kt;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          if (MODE == MODE_DW) {
#pragma unroll
            for (int t = 0; t < 4; ++t) af[i][t] = sa[(8 * k8 + 4 * h + t) * A_RLD + ((wm + 32 * i + r) ^ (DMA ? 32 * h : 0))];
          } else {
            const float4 v = DMA ? *reinterpret_cast<const float4*>(sa + (wm + 32 * i + r) * KT + 4 * ((2 * k8 + h) ^ ((r >> 2) & 3)))
                                 : *reinterpret_cast<const float4*>(sa + (wm + 32 * i + r) * KC_LD + 8 * k8 + 4 * h);
            af[i][0] = v.x; af[i][1] = v.y; af[i][2] = v.z; af[i][3] = v.w;
          }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if (MODE == MODE_FWD) {
            const float4 v = *reinterpret_cast<const float4*>(sb + (wn + 32 * j + r) * KC_LD + 8 * k8 + 4 * h);
            bf[j][0] = v.x; bf[j][1] = v.y; bf[j][2] = v.z; bf[j][3] = v.w;
          } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) bf[j][t] = sb[(8 * k8 + 4 * h + t) * B_RLD + ((wn + 32 * j + r) ^ (DMA ? 32 * h : 0))];
          }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[j][t], af[i][t], acc[i][j], 0, 0, 0);
      }
    };

    if constexpr (DMA) {
      // ---- LDS-DMA main loop (launch_gemm picks it when every tile of the grid is interior and nk % 4 == 0).  What the
      // probes of the register-staged loop below said: its cost is neither the barrier nor the ds_write
      // but the wave stalling on `vmcnt` before the ds_write -- in order, so it cannot issue MFMAs either -- although the
      // request ran two tiles ahead.  Here a tile is requested THREE iterations before it is read, straight into the stage
      // the previous iteration vacated, and costs no VGPRs; a wave only ever waits at the top of an iteration.
      // Slot maps (16-B slots; lane i of DMA instruction q fills slot 64 q + i of its tile):
      //   k-contiguous tile (dY of the dX product), rows of KT floats = 4 slots:  slot(row, s) = 4 row + (s ^ ((row >> 2) & 3))
      //   reduction-row tile, rows of COLS floats:  slot(row, c4) = (COLS / 4) row + (c4 ^ 8 ((row >> 2) & 1))
      // -> the ds_read_b128 of 16 consecutive rows and the ds_read_b32 of rows k, k + 4 by the two lane halves hit distinct banks.
      constexpr int AI = BM * KT / 1024, BI = BN * KT / 1024, NI = AI + BI;   // DMA instructions per wave and tile
      static_assert(BM * KT % 1024 == 0 && BN * KT % 1024 == 0 && KT == 16, "tile does not split into whole-KiB DMA instructions");
      const int wv = __builtin_amdgcn_readfirstlane(wave);
      const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float*)smem;
      const float* ga[AI];
      const float* gb[BI];
#pragma unroll
      for (int u = 0; u < AI; ++u) {
        const int L = 64 * (wv * AI + u) + lane;
        if (MODE == MODE_DX) {
          const int row = L >> 2, sl = (L & 3) ^ ((row >> 2) & 3);
          ga[u] = A + (long long)(m0 + row) * p.lda + kbeg + 4 * sl;
        } else {
          const int row = L / (BM / 4), c4 = (L % (BM / 4)) ^ (((row >> 2) & 1) * 8);
          ga[u] = A + (long long)(kbeg + row) * p.lda + m0 + 4 * c4;
        }
      }
#pragma unroll
      for (int u = 0; u < BI; ++u) {
        const int L = 64 * (wv * BI + u) + lane;
        const int row = L / (BN / 4), c4 = (L % (BN / 4)) ^ (((row >> 2) & 1) * 8);
        gb[u] = B + (long long)(kbeg + row) * p.ldb + n0 + 4 * c4;
      }
      const long long a_step = (MODE == MODE_DX) ? (long long)KT : (long long)KT * p.lda, b_step = (long long)KT * p.ldb;
      // (M0 -- the DMA's LDS base -- is written inside the asm.  It is a register reserved to the compiler, which therefore never
      //  keeps a value of its own in it across foreign code; this kernel has no other M0 user: no LDS-DMA builtin, no
      //  readlane / movrel / sendmsg.  Naming it as a clobber only draws -Winline-asm's "reserved register" warning.)
      int issued = 0;   // tiles requested so far; past the last one the tail re-requests it into a stage nobody reads again
#define PQLK_DMA(STG)                                                                                                          \
  do {                                                                                                                         \
    _Pragma("unroll") for (int u = 0; u < AI; ++u)                                                                             \
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"                                           \
                   ::"s"(lds0 + 4u * ((STG) * STG_F) + 1024u * (wv * AI + u)), "v"(ga[u]) : "memory");                         \
    _Pragma("unroll") for (int u = 0; u < BI; ++u)                                                                             \
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"                                           \
                   ::"s"(lds0 + 4u * ((STG) * STG_F + SA_F) + 1024u * (wv * BI + u)), "v"(gb[u]) : "memory");                   \
    ++issued;                                                                                                                  \
    const long long as_ = issued < nk ? a_step : 0, bs_ = issued < nk ? b_step : 0;                                            \
    _Pragma("unroll") for (int u = 0; u < AI; ++u) ga[u] += as_;                                                               \
    _Pragma("unroll") for (int u = 0; u < BI; ++u) gb[u] += bs_;                                                               \
  } while (0)
      // wait until at most two tiles' worth of this wave's requests are outstanding (vmcnt only; expcnt / lgkmcnt untouched)
#define PQLK_DMA_WAIT(N) __builtin_amdgcn_s_waitcnt(((N) & 0xF) | 0x70 | 0xF00 | ((((N) >> 4) & 3) << 14))
      __syncthreads();  // previous group's stages may still be in use
      PQLK_DMA(0);
      PQLK_DMA(1);
      PQLK_DMA(2);
      if constexpr (MODE == MODE_DX) {
        // ---- fragments one STAGE ahead.  In the loop below a wave reads a stage's operand fragments right behind the barrier that
        // publishes the stage and its first MFMA waits out the LDS latency; the co-resident block is often at the same point.  Here
        // the counted wait is one tile tighter (tile kt + 1 has landed at the top of iteration kt: two tiles of lead instead of
        // three), so the 32 registers of tile kt + 1's fragments are filled WHILE tile kt's 32 MFMAs issue, into a second register
        // set (the kernel used 166 of its 256 VGPRs); behind each barrier the MFMAs start at once.  Same k order: same bits.
        // dX products only (k-contiguous dY fragments: four ds_read_b128 + sixteen ds_read_b32 per stage): backward of the twin
        // critic 270.3 -> 262.9 us; the dW products (both operands reduction-row: 32 ds_read2st64_b32 per stage) ran 2 % SLOWER
        // with it and keep the loop below (tools/kbench.py, interleaved rounds on one box, round 3).
        float fa0[KT / 8][MI][4], fb0[KT / 8][NJ][4], fa1[KT / 8][MI][4], fb1[KT / 8][NJ][4];
#define PQLK_LDF(STG, FA, FB)                                                                                                  \
  do {                                                                                                                         \
    const float* sa_ = smem + (STG) * STG_F;                                                                                   \
    const float* sb_ = sa_ + SA_F;                                                                                             \
    _Pragma("unroll") for (int k8 = 0; k8 < KT / 8; ++k8) {                                                                    \
      _Pragma("unroll") for (int i = 0; i < MI; ++i) {                                                                         \
        if (MODE == MODE_DW) {                                                                                                 \
          _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                                        \
            FA[k8][i][t] = sa_[(8 * k8 + 4 * h + t) * A_RLD + ((wm + 32 * i + r) ^ (32 * h))];                                 \
        } else {                                                                                                               \
          const float4 v_ = *reinterpret_cast<const float4*>(sa_ + (wm + 32 * i + r) * KT + 4 * ((2 * k8 + h) ^ ((r >> 2) & 3))); \
          FA[k8][i][0] = v_.x; FA[k8][i][1] = v_.y; FA[k8][i][2] = v_.z; FA[k8][i][3] = v_.w;                                  \
        }                                                                                                                      \
      }                                                                                                                        \
      _Pragma("unroll") for (int j = 0; j < NJ; ++j)                                                                           \
        _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                                          \
          FB[k8][j][t] = sb_[(8 * k8 + 4 * h + t) * B_RLD + ((wn + 32 * j + r) ^ (32 * h))];                                   \
    }                                                                                                                          \
  } while (0)
#define PQLK_MMF(STG, FA, FB)                                                                                                  \
  do {                                                                                                                         \
    if (MODE == MODE_DW && bx == 0) {                                                                                          \
      const float* sa_ = smem + (STG) * STG_F;                                                                                 \
      constexpr int DBR = KT / (256 / BM);                                                                                     \
      _Pragma("unroll") for (int rr = 0; rr < DBR; ++rr) {                                                                     \
        const int row = (tid / BM) * DBR + rr;                                                                                 \
        dbacc += sa_[row * A_RLD + ((tid % BM) ^ (((row >> 2) & 1) * 32))];                                                    \
      }                                                                                                                        \
    }                                                                                                                          \
    if (live)                                                                                                                  \
    _Pragma("unroll") for (int k8 = 0; k8 < KT / 8; ++k8)                                                                      \
      _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                                            \
        _Pragma("unroll") for (int i = 0; i < MI; ++i)                                                                         \
          _Pragma("unroll") for (int j = 0; j < NJ; ++j)                                                                       \
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(FB[k8][j][t], FA[k8][i][t], acc[i][j], 0, 0, 0);                  \
    __builtin_amdgcn_sched_barrier(0);   /* hipcc otherwise moves all but one MFMA behind the NEXT barrier, next to its reads */ \
  } while (0)
        PQLK_DMA_WAIT(2 * NI); __syncthreads();   // tile 0 has landed
        PQLK_LDF(0, fa0, fb0);
        for (int kt = 0; kt < nk; kt += 4) {
          PQLK_DMA_WAIT(NI); __syncthreads(); PQLK_DMA(3); PQLK_LDF(1, fa1, fb1); PQLK_MMF(0, fa0, fb0);
          PQLK_DMA_WAIT(NI); __syncthreads(); PQLK_DMA(0); PQLK_LDF(2, fa0, fb0); PQLK_MMF(1, fa1, fb1);
          PQLK_DMA_WAIT(NI); __syncthreads(); PQLK_DMA(1); PQLK_LDF(3, fa1, fb1); PQLK_MMF(2, fa0, fb0);
          PQLK_DMA_WAIT(NI); __syncthreads(); PQLK_DMA(2); PQLK_LDF(0, fa0, fb0); PQLK_MMF(3, fa1, fb1);
        }
#undef PQLK_LDF
#undef PQLK_MMF
      } else {
        for (int kt = 0; kt < nk; kt += 4) {
          PQLK_DMA_WAIT(2 * NI); __syncthreads(); PQLK_DMA(3); compute(kt, 0);
          PQLK_DMA_WAIT(2 * NI); __syncthreads(); PQLK_DMA(0); compute(kt + 1, 1);
          PQLK_DMA_WAIT(2 * NI); __syncthreads(); PQLK_DMA(1); compute(kt + 2, 2);
          PQLK_DMA_WAIT(2 * NI); __syncthreads(); PQLK_DMA(2); compute(kt + 3, 3);
        }
      }
      PQLK_DMA_WAIT(0);
      __syncthreads();   // the tail's re-requests have landed and every wave is done reading: LDS is free for the epilogue
#undef PQLK_DMA
#undef PQLK_DMA_WAIT
      continue;
    }
    // ---- interior blocks: every tile is full, so the loads need no bounds tests, are straight-line code, and can run TWO
    // tiles ahead: tile kt+2 is requested at the top of iteration kt into the register set that tile kt vacated, tile kt+1
    // (requested one iteration earlier) is moved to LDS at the bottom behind a counted wait.  With one tile of lead
    // (32 MFMAs per wave, ~1 us) the wait before the LDS store regularly outlasts the MFMAs; two tiles cover an L2 / HBM
    // round trip.  The tail re-requests the last tile instead of branching (a branch would void the counted waits).
    bool inner = (m0 + BM <= p.M) && ((kend - kbeg) % KT == 0) && (nk % 2 == 0);
    if (MODE == MODE_FWD) inner = inner && (n0 + BN <= p.N);
    if (MODE == MODE_DX) inner = inner && (n0 + BN <= p.ldb) && (kend <= p.lda);
    if (MODE == MODE_DW) inner = inner && (m0 + BM <= p.lda) && (n0 + BN <= p.ldb);
    if (inner) {
      // (plain macros, not lambdas taking the tiles by reference: those keep the tiles in scratch memory)
#define PQLK_GL(KTILE, Q)                                                                                                      \
  do {                                                                                                                         \
    const int k0_ = kbeg + (KTILE) * KT;                                                                                       \
    if (MODE == MODE_FWD) { a_kc##Q.load_inner(A, p.lda, m0, k0_, tid); b_kc##Q.load_inner(B, p.ldb, n0, k0_, tid); }          \
    else if (MODE == MODE_DX) { a_kc##Q.load_inner(A, p.lda, m0, k0_, tid); b_rr##Q.load_inner(B, p.ldb, k0_, n0, tid); }      \
    else { a_rr##Q.load_inner(A, p.lda, k0_, m0, tid); b_rr##Q.load_inner(B, p.ldb, k0_, n0, tid); }                           \
  } while (0)
#define PQLK_SS(STG, Q)                                                                                                        \
  do {                                                                                                                         \
    float* sa_ = smem + (STG) * S::STAGE;                                                                                      \
    float* sb_ = sa_ + S::A_FLOATS;                                                                                            \
    if (MODE == MODE_FWD) { a_kc##Q.store(sa_, tid); b_kc##Q.store(sb_, tid); }                                                \
    else if (MODE == MODE_DX) { a_kc##Q.store(sa_, tid); b_rr##Q.store(sb_, tid); }                                            \
    else { a_rr##Q.store(sa_, tid); b_rr##Q.store(sb_, tid); }                                                                 \
  } while (0)
      PQLK_GL(0, 0);
      __syncthreads();  // previous group's last stage may still be in use
      PQLK_SS(0, 0);
      PQLK_GL(1, 1);
      __syncthreads();
      for (int kt = 0; kt < nk; kt += 2) {
        PQLK_GL(min(kt + 2, nk - 1), 0);
        __builtin_amdgcn_sched_barrier(0);   // keep the requests at the top of the iteration
        compute(kt, 0);
        PQLK_SS(1, 1);
        __syncthreads();
        PQLK_GL(min(kt + 3, nk - 1), 1);
        __builtin_amdgcn_sched_barrier(0);
        compute(kt + 1, 1);
        PQLK_SS(0, 0);
        __syncthreads();
      }
#undef PQLK_GL
#undef PQLK_SS
      continue;
    }

    // ---- generic path (edge tiles): bounds-tested loads, one tile of lead
    KcTile<BM, KT> a_kc;
    RrTile<BM, KT> a_rr;
    KcTile<BN, KT> b_kc;
    RrTile<BN, KT> b_rr;

    auto gload = [&](int kt) {
      const int k0 = kbeg + kt * KT;
      if (MODE == MODE_FWD) {
        a_kc.load(A, p.lda, m0, p.M, k0, kend, tid);
        b_kc.load(B, p.ldb, n0, p.N, k0, kend, tid);
      } else if (MODE == MODE_DX) {
        a_kc.load(A, p.lda, m0, p.M, k0, p.lda, tid);   // dY pad columns are zero
        b_rr.load(B, p.ldb, k0, kend, n0, p.ldb, tid);  // W rows n (reduction), cols = in-features (padded ld)
      } else {
        a_rr.load(A, p.lda, k0, kend, m0, p.lda, tid);  // dY rows m (reduction), cols = dW rows
        b_rr.load(B, p.ldb, k0, kend, n0, p.ldb, tid);  // X rows m, cols = dW cols
      }
    };
    auto sstore = [&](int stage) {
      float* sa = smem + stage * S::STAGE;
      float* sb = sa + S::A_FLOATS;
      if (MODE == MODE_FWD) {
        a_kc.store(sa, tid);
        b_kc.store(sb, tid);
      } else if (MODE == MODE_DX) {
        a_kc.store(sa, tid);
        b_rr.store(sb, tid);
      } else {
        a_rr.store(sa, tid);
        b_rr.store(sb, tid);
      }
    };

    gload(0);
    __syncthreads();  // previous group's last stage may still be in use
    sstore(0);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
      const int stage = kt & 1;
      if (kt + 1 < nk) gload(kt + 1);
      compute(kt, stage);
      if (kt + 1 < nk) sstore(stage ^ 1);
      __syncthreads();
    }
  }

  if (MODE == MODE_DW && bx == 0) {   // block-uniform: fold the row groups' partial column sums in group order
    smem[tid] = dbacc;                        // (the last pipeline stage is no longer read: the k loop ends on a barrier)
    __syncthreads();
    if (tid < BM) {
      dbacc = smem[tid];
#pragma unroll
      for (int g = 1; g < 256 / BM; ++g) dbacc += smem[g * BM + tid];
    }
    __syncthreads();
  }
  // ------------------------------------------------------------------------------ epilogue
  // Accumulator layout after the operand swap (the MFMA computes the TRANSPOSED 32x32 tile): lane (r, h) owns output
  // row `.. + r` and, in register quad q = e>>2, the four consecutive columns `.. + 8q + 4h + (e&3)`: every quad is one
  // 16-B store / load instead of four scalar ones (the epilogue is store-issue bound: 64 -> 16 instructions per tile).
  //
  // Full tiles of the backward products (dX with or without ELU', dW slabs) go out through LDS instead: straight from the
  // accumulators one store instruction touches 32 rows x 32 B (and the ELU' operand comes in the same way), i.e. quarter
  // lines; staged through the (now idle) pipeline stages, each wave re-reads its 32 x WN patch row by row and one
  // instruction moves 64 / (WN / 4) whole row segments of WN x 4 B (256 B at WN = 64): full 128-B lines both ways.
  // The patch is private to the wave (rows wm.., columns wn..): no block barrier inside the passes.
  if (MODE != MODE_FWD && EPI != EPI_DTANH_SLICE) {
    const bool whole = (m0 + BM <= p.M) && (n0 + BN <= p.N) && (MODE == MODE_DW || !p.C2);
    if (whole) {   // block-uniform
      constexpr int PLD = WN + 4;            // patch row stride: conflict-free b128 writes (lane rows 4 banks apart) and reads
      constexpr int LPR = WN / 4;            // lanes per patch row
      constexpr int RPI = 64 / LPR;          // rows per wave instruction
      // (launch_gemm sizes the dynamic LDS as max(two pipeline stages, four patches))
      float* patch = smem + wave * (32 * PLD);
      const int gq = (MODE == MODE_DX && p.zsum) ? 0 : g0;
      float* Cw = (MODE == MODE_DW) ? p.C + (long long)g0 * p.sC + (long long)split * p.sSplit : p.C + (long long)gq * p.sC;
      const float* auxw = (EPI == EPI_DELU && p.aux) ? p.aux + (long long)gq * p.sAux : nullptr;
      const int prow = lane / LPR, pc4 = lane % LPR;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        // ELU' operand of this pass: ALL of its requests go out before the patch is staged, into registers the k loop has
        // vacated.  Written as load -> use -> store per row group (rounds 1-2 and the start of round 3) the stores to C and the
        // next load of H may alias as far as the compiler can tell, so it put `s_waitcnt vmcnt(0)` between them: sixteen
        // dependent load + store round trips per block, which is what made the dX products slower than the dW products of the
        // same size (round 2 hid it behind a prefetch in front of the k loop; the stage-ahead fragments took those registers).
        f4v h4s[(EPI == EPI_DELU) ? 32 / RPI : 1];
        if (EPI == EPI_DELU) {
          long long arow[32 / RPI];
          const long long grow0 = m0 + wm + 32 * i + prow;
          if (MODE == MODE_DX && p.perm) {   // one branch around all the index loads, so that they too are in flight together
            int pr[32 / RPI];
#pragma unroll
            for (int it = 0; it < 32 / RPI; ++it) pr[it] = p.perm[grow0 + it * RPI];
#pragma unroll
            for (int it = 0; it < 32 / RPI; ++it) arow[it] = pr[it] < 0 ? 0 : pr[it];   // pad rows: dZ is zero anyway
          } else {
#pragma unroll
            for (int it = 0; it < 32 / RPI; ++it) arow[it] = grow0 + it * RPI;
          }
#pragma unroll
          for (int it = 0; it < 32 / RPI; ++it)
            h4s[it] = *reinterpret_cast<const f4v*>(auxw + arow[it] * p.ldaux + n0 + wn + 4 * pc4);
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            *reinterpret_cast<float4*>(patch + r * PLD + 32 * j + 8 * q + 4 * h) =
                make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
        // no block barrier: the patch is this wave's own and a wave's LDS instructions execute in order (the k loop ended on a
        // barrier, so nobody still reads the stages underneath); the four waves drain their passes independently
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int it = 0; it < 32 / RPI; ++it) {
          const int rr = it * RPI + prow;
          float4 v = *reinterpret_cast<const float4*>(patch + rr * PLD + 4 * pc4);
          const long long grow = m0 + wm + 32 * i + rr;
          const int gcol = n0 + wn + 4 * pc4;
          if (EPI == EPI_DELU) {
            const f4v h4 = h4s[it];
            v.x = h4.x > 0.f ? v.x : v.x * (h4.x + 1.f);  // ELU'(x) = exp(x) = elu(x) + 1 for x <= 0
            v.y = h4.y > 0.f ? v.y : v.y * (h4.y + 1.f);
            v.z = h4.z > 0.f ? v.z : v.z * (h4.z + 1.f);
            v.w = h4.w > 0.f ? v.w : v.w * (h4.w + 1.f);
          }
          *reinterpret_cast<float4*>(Cw + grow * p.ldc + gcol) = v;
        }
        if (i + 1 < MI) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
      }
      if (MODE == MODE_DW && bx == 0 && tid < BM && p.dbias) {
        float* db = p.dbias + (long long)g0 * p.sBias + (long long)split * p.sSplit;
        const int row = m0 + tid;
        if (row < p.ncols_store) db[row] = row < p.M ? dbacc : 0.f;
      }
      return;
    }
  }
  if (MODE == MODE_DW) {
    float* C = p.C + (long long)g0 * p.sC + (long long)split * p.sSplit;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int row = m0 + wm + 32 * i + r;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int col = n0 + wn + 32 * j + 8 * q + 4 * h;
          if (row < p.M && col < p.N)  // N (= padded in-features) is a multiple of 32: a quad is never split
            *reinterpret_cast<float4*>(C + (long long)row * p.ldc + col) =
                make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
        }
      }
    if (bx == 0 && tid < BM && p.dbias) {
      float* db = p.dbias + (long long)g0 * p.sBias + (long long)split * p.sSplit;
      const int row = m0 + tid;
      if (row < p.ncols_store) db[row] = row < p.M ? dbacc : 0.f;  // ncols_store = pqlk_ld(out): zero bias pad
    }
    return;
  }

  // EPI is a compile-time parameter: one straight-line epilogue per instantiation (a runtime switch inside the
  // 64-element unrolled store loop inlined tanhf/expf four times over and cost ~10 us per launch).
  const int g = (MODE == MODE_DX && p.zsum) ? 0 : g0;
  float* C = p.C + (long long)g * p.sC;
  const float* bias = (MODE == MODE_FWD && p.bias) ? p.bias + (long long)g * p.sBias : nullptr;
  const float* aux = p.aux ? p.aux + (long long)g * p.sAux : nullptr;
  // full = the whole tile lies inside the logical matrix: vector path with no per-element bounds tests
  const bool full = (m0 + BM <= p.M) && (n0 + BN <= p.N) && EPI != EPI_DTANH_SLICE && EPI != EPI_TANH_NOISE && !p.C2;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int row = m0 + wm + 32 * i + r;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = n0 + wn + 32 * j + 8 * q + 4 * h;
        float v[4] = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
        if (full) {
          if (MODE == MODE_FWD) {
            const float4 b4 = bias ? *reinterpret_cast<const float4*>(bias + col) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[0] += b4.x; v[1] += b4.y; v[2] += b4.z; v[3] += b4.w;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              if (EPI == EPI_ELU) v[u] = elu1(v[u]);
              else if (EPI == EPI_TANH) v[u] = tanhf(v[u]);
            }
          } else if (EPI == EPI_DELU) {
            const float4 h4 = *reinterpret_cast<const float4*>(aux + (long long)row * p.ldaux + col);
            v[0] = h4.x > 0.f ? v[0] : v[0] * (h4.x + 1.f);  // ELU'(x) = exp(x) = elu(x) + 1 for x <= 0
            v[1] = h4.y > 0.f ? v[1] : v[1] * (h4.y + 1.f);
            v[2] = h4.z > 0.f ? v[2] : v[2] * (h4.z + 1.f);
            v[3] = h4.w > 0.f ? v[3] : v[3] * (h4.w + 1.f);
          }
          *reinterpret_cast<float4*>(C + (long long)row * p.ldc + col) = make_float4(v[0], v[1], v[2], v[3]);
          continue;
        }
        if (row >= p.M) continue;
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // edge tiles, pad columns, slices, second destination: per element
          const int c = col + u;
          float x = v[u];
          if (EPI == EPI_DTANH_SLICE) {
            const int cc = c - p.col0;
            if (cc >= 0 && cc < p.ncol) {
              const float a = aux[(long long)row * p.ldaux + cc];
              C[(long long)row * p.ldc + cc] = x * (1.f - a * a);
            }
            continue;
          }
          if (c >= p.ncols_store) continue;
          if (c < p.N) {
            if (MODE == MODE_FWD) {
              x += bias ? bias[c] : 0.f;
              if (EPI == EPI_ELU) x = elu1(x);
              else if (EPI == EPI_TANH) x = tanhf(x);
              else if (EPI == EPI_TANH_NOISE) {
                x = tanhf(x);
                float nz = p.noise_std * aux[(long long)row * p.N + c];
                nz = fminf(fmaxf(nz, -p.noise_clip), p.noise_clip);
                x = fminf(fmaxf(x + nz, -1.f), 1.f);
              }
              if (p.C2 && g == 0) p.C2[(long long)row * p.ldc2 + c] = x;
            } else if (EPI == EPI_DELU) {
              const float hval = aux[(long long)row * p.ldaux + c];
              x = hval > 0.f ? x : x * (hval + 1.f);
            }
          } else {
            x = 0.f;  // pad column
          }
          C[(long long)row * p.ldc + c] = x;
        }
      }
    }
}

template <int MODE, int BM, int BN, int EPI, int KT, bool DMA = false>
// exactly 2 waves per SIMD (3 for the 128 x 64 tile): the register allocator otherwise aims for 4 and spills the second tile set
#define PQLK_GEMM_WPE (BM == 128 && BN == 64 ? 3 : 2)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PQLK_GEMM_WPE, PQLK_GEMM_WPE))) void k_gemm(GemmP p) {
  gemm_body<MODE, BM, BN, EPI, KT, DMA>(p, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y);
}

// PQLK_GEMM_DMA=0 keeps every GEMM on the register-staged main loop (A/B switch of the LDS-DMA loop; read once)
static bool gemm_dma_enabled() {
  static const bool on = [] { const char* e = getenv("PQLK_GEMM_DMA"); return !(e && e[0] == '0'); }();
  return on;
}

static bool gemm_xcd_enabled() {   // PQLK_GEMM_XCD=0: dispatch-order tiles (A/B switch of the XCD-aware order; read once)
  static const bool on = [] { const char* e = getenv("PQLK_GEMM_XCD"); return !(e && e[0] == '0'); }();
  return on;
}

// grid, XCD re-labelling and main-loop choice of one product; returns true when the LDS-DMA loop applies (every tile of the
// grid interior, whole 16-deep stages in multiples of four, 16-B aligned operands)
template <int MODE, int BM, int BN, int EPI>
static bool gemm_plan(GemmP& p, int gz, dim3& grid) {
  constexpr int KT = PQLK_KT;
  int ncols = (MODE == MODE_DW) ? p.N : p.ncols_store;
  p.n_base = 0;
  if (MODE == MODE_DX && EPI == EPI_DTANH_SLICE) {  // only the action columns are wanted
    p.n_base = p.col0 & ~3;
    ncols = p.col0 + p.ncol - p.n_base;
  }
  grid = dim3((unsigned)((ncols + BN - 1) / BN), (unsigned)((p.M + BM - 1) / BM), (unsigned)gz);
  {
    const long long tiles = (long long)grid.x * grid.y * grid.z, group = (MODE == MODE_DW) ? (long long)grid.x * grid.y : grid.x;
    p.xcd_remap = 0;
    if (gemm_xcd_enabled() && tiles < (1LL << 30)) {
      if (tiles % (8 * group) == 0) p.xcd_remap = 1;                       // whole groups of operand-sharing tiles per XCD
      else if (tiles >= 64) p.xcd_remap = (int)tiles;                      // contiguous runs (see gemm_body)
    }
  }
  if constexpr (KT == 16 && (MODE == MODE_DX || MODE == MODE_DW) && (EPI == EPI_DELU || EPI == EPI_NONE)) {
    bool dma = gemm_dma_enabled() && p.M % BM == 0 && !p.C2 && pqlk_aligned16(p.A) &&
               pqlk_aligned16(p.B) && p.lda % 4 == 0 && p.ldb % 4 == 0 && (EPI != EPI_DELU || (p.aux && pqlk_aligned16(p.aux) && p.ldaux % 4 == 0));
    if (MODE == MODE_DX) dma = dma && ncols % BN == 0 && p.N % BN == 0 && p.K % (4 * KT) == 0 && p.K <= p.lda && ncols <= p.ldb && p.sA % 4 == 0 &&
                               p.sB % 4 == 0;
    // dW: the column tiles of X need not divide N as long as the LAST tile's loads stay inside X's rows (round_up(N, BN) <= ldb:
    // e.g. the actor's 88 -> 96 inputs read from a 128-float-wide tile); whatever those extra columns hold only reaches accumulator
    // columns >= N, which the (masked) epilogue of a partial tile never stores.  Round 4: the actor's layer-1 dW product had been the
    // one backward GEMM left on the register-staged loop.
    else dma = dma && pqlk_round_up(p.N, BN) <= p.ldb && p.rows_per_split % (4 * KT) == 0 && p.K % p.rows_per_split == 0 &&
               p.K / p.rows_per_split == p.splits && p.M <= p.lda && p.N <= p.ldb && p.sA % 4 == 0 && p.sB % 4 == 0;
    return dma;
  }
  return false;
}

template <int BM, int BN, int KT>
static constexpr size_t gemm_dma_lds() {
  constexpr size_t dma_floats = (size_t)4 * (BM + BN) * KT, patch_floats = (size_t)4 * 32 * (BN / 2 + 4);
  return (dma_floats > patch_floats ? dma_floats : patch_floats) * sizeof(float);
}

template <int MODE, int BM, int BN, int EPI>
static int launch_gemm(GemmP p, int gz, hipStream_t st) {
  constexpr int KT = PQLK_KT;
  using S = Smem<MODE, BM, BN, KT>;
  constexpr size_t stage_floats = (size_t)2 * S::STAGE;
  constexpr size_t patch_floats = (size_t)4 * 32 * (BN / 2 + 4);   // the epilogue's per-wave staging patches
  const size_t shmem = (stage_floats > patch_floats ? stage_floats : patch_floats) * sizeof(float);
  static PqlkPerDeviceOnce attr_once;
  if (int rc = attr_once.run([&] {
        return -(int)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm<MODE, BM, BN, EPI, KT>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
      }))
    return rc;
  dim3 grid;
  const bool dma = gemm_plan<MODE, BM, BN, EPI>(p, gz, grid);
  if constexpr (KT == 16 && (MODE == MODE_DX || MODE == MODE_DW) && (EPI == EPI_DELU || EPI == EPI_NONE)) {
    if (dma) {
      constexpr size_t dshmem = gemm_dma_lds<BM, BN, KT>();
      static PqlkPerDeviceOnce dma_once;
      if (int rc = dma_once.run([&] {
            return -(int)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm<MODE, BM, BN, EPI, KT, true>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)dshmem);
          }))
        return rc;
      hipLaunchKernelGGL((k_gemm<MODE, BM, BN, EPI, KT, true>), grid, dim3(256), dshmem, st, p);
      PQLK_LAUNCH_CHECK();
      return PQLK_OK;
    }
  }
  hipLaunchKernelGGL((k_gemm<MODE, BM, BN, EPI, KT>), grid, dim3(256), shmem, st, p);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

// Pick the tile: 128x128 when that already gives every CU a block, else 64x64.
template <int MODE, int EPI>
static int launch_tile(const GemmP& p, int gz, hipStream_t st) {
  const int ncols = (MODE == MODE_DW) ? p.N : p.ncols_store;
  const long long big = (long long)((p.M + 127) / 128) * ((ncols + 127) / 128) * gz;
  // (128 x 64 tiles at three blocks per CU for the dense products: dX the same, dW 1-2 % slower -- measured, not used)
  // (the same tiles for launches of exactly one 128 x 128 tile per CU, so that no block sits alone on its CU: neutral to -1 % with
  //  the LDS-DMA loop -- a lone block there already keeps three tiles in flight)
  if (big >= 256 && ncols >= 128 && EPI != EPI_DTANH_SLICE) return launch_gemm<MODE, 128, 128, EPI>(p, gz, st);
  // (128 x 64 dW tiles for the products that 128 x 128 tiles leave at under one block per CU -- layer 1 of the critic, the actor's
  //  256-row layer: V step 617.5 -> 618.9 us, P step 542.8 -> 543.7: not used; round 3)
  return launch_gemm<MODE, 64, 64, EPI>(p, gz, st);
}

template <int MODE>
static int launch_auto(const GemmP& p, int gz, hipStream_t st) {
  if (MODE == MODE_FWD) {
    switch (p.epi) {
      case EPI_ELU: return launch_tile<MODE_FWD, EPI_ELU>(p, gz, st);
      case EPI_TANH: return launch_tile<MODE_FWD, EPI_TANH>(p, gz, st);
      case EPI_TANH_NOISE: return launch_tile<MODE_FWD, EPI_TANH_NOISE>(p, gz, st);
      default: return launch_tile<MODE_FWD, EPI_NONE>(p, gz, st);
    }
  } else if (MODE == MODE_DX) {
    switch (p.epi) {
      case EPI_DELU: return launch_tile<MODE_DX, EPI_DELU>(p, gz, st);
      case EPI_DTANH_SLICE: return launch_tile<MODE_DX, EPI_DTANH_SLICE>(p, gz, st);
      default: return launch_tile<MODE_DX, EPI_NONE>(p, gz, st);
    }
  }
  return launch_tile<MODE_DW, EPI_NONE>(p, gz, st);
}

// ================================================================================================
// geometry: the one definition of the parameter arena and the activation stash of (d, b), built once per call
//   arena: n_nets blocks of net_stride floats; layer l of a net is W (dims[l + 1], ld[l]) at w_off[l], then b (ld[l + 1]) at b_off[l]
//   stash: layer l's output is (n_nets, b, ld[l + 1]) at a_off[l]
struct MlpGeom {
  const PqlMlpDesc* d; int64_t b;
  int L, n_nets;
  int64_t ld[PQLK_MAX_LAYERS + 1];   // pqlk_ld(dims[l]): layer l reads rows of ld[l] floats (ld_in) and writes rows of ld[l + 1] (ld_out)
  int64_t w_off[PQLK_MAX_LAYERS], b_off[PQLK_MAX_LAYERS], a_off[PQLK_MAX_LAYERS];
  int64_t net_stride, arena, acts_floats, max_hidden_ld;
  int64_t head_floats;               // the last layer's W and b of one net: what a head partial holds
};

static MlpGeom mlp_geom(const PqlMlpDesc* d, int64_t b) {   // d has passed desc_ok
  MlpGeom g = {};
  g.d = d; g.b = b; g.L = d->n_layers; g.n_nets = d->n_nets;
  for (int l = 0; l <= g.L; ++l) g.ld[l] = pqlk_ld(d->dims[l]);
  for (int l = 0; l < g.L; ++l) {
    g.w_off[l] = g.net_stride; g.b_off[l] = g.w_off[l] + (int64_t)d->dims[l + 1] * g.ld[l];
    g.net_stride = g.b_off[l] + g.ld[l + 1];
    g.a_off[l] = g.acts_floats; g.acts_floats += (int64_t)g.n_nets * b * g.ld[l + 1];
    g.max_hidden_ld = g.ld[l + 1] > g.max_hidden_ld ? g.ld[l + 1] : g.max_hidden_ld;
  }
  g.arena = g.net_stride * g.n_nets; g.head_floats = g.net_stride - g.w_off[g.L - 1];
  return g;
}

extern "C" int64_t pqlk_mlp_net_stride(const PqlMlpDesc* d) { return desc_ok(d) ? 0 : mlp_geom(d, 0).net_stride; }
extern "C" int64_t pqlk_mlp_param_floats(const PqlMlpDesc* d) { return desc_ok(d) ? 0 : mlp_geom(d, 0).arena; }

extern "C" int pqlk_mlp_layer_offsets(const PqlMlpDesc* d, int32_t layer, int64_t* w_off, int64_t* b_off) {
  int rc = desc_ok(d);
  if (rc) return rc;
  PQLK_REQUIRE(layer >= 0 && layer < d->n_layers, PQLK_E_RANGE);
  const MlpGeom g = mlp_geom(d, 0);
  if (w_off) *w_off = g.w_off[layer];
  if (b_off) *b_off = g.b_off[layer];
  return PQLK_OK;
}

extern "C" int64_t pqlk_mlp_acts_floats(const PqlMlpDesc* d, int64_t b) { return desc_ok(d) || b <= 0 ? 0 : mlp_geom(d, b).acts_floats; }

extern "C" int pqlk_mlp_act_offset(const PqlMlpDesc* d, int64_t b, int32_t net, int32_t layer, int64_t* off, int64_t* ld) {
  int rc = desc_ok(d);
  if (rc) return rc;
  PQLK_REQUIRE(layer >= 0 && layer < d->n_layers && net >= 0 && net < d->n_nets && b > 0, PQLK_E_RANGE);
  const MlpGeom g = mlp_geom(d, b);
  if (off) *off = g.a_off[layer] + (int64_t)net * b * g.ld[layer + 1];
  if (ld) *ld = g.ld[layer + 1];
  return PQLK_OK;
}

// ---- the two workspace formats: every pointer into a workspace and every size check comes from these -----------------------------
// compact DPG workspace (minnet.h), in floats: [dz0 | dz1 | perm (rows_cap ints) | mn (64 ints) | tie0 (rows_cap ints)]
struct CompactWs { int64_t rows_cap, dz[2], perm, mn, tie0, total; };
static CompactWs compact_ws(int64_t max_hidden_ld, int64_t b) {
  CompactWs w = {};
  w.rows_cap = 2 * pqlk_round_up(b, MN_TILE);   // every sample a tie: both runs full
  w.dz[1] = w.rows_cap * max_hidden_ld; w.perm = 2 * w.dz[1]; w.mn = w.perm + w.rows_cap; w.tie0 = w.mn + 64;
  w.total = w.tie0 + w.rows_cap;
  return w;
}

// backward workspace, in floats: [dZ0 | dZ1 | splits x arena slabs | head partials].  splits = 0 is a call without `grads`: it needs
// neither slabs nor head partials
struct BwdWs { int64_t dz[2], slabs, head_part, head_part_floats, total; };
static BwdWs bwd_ws(const MlpGeom& g, int splits) {
  BwdWs w = {};
  w.dz[1] = (int64_t)g.n_nets * g.b * g.max_hidden_ld; w.slabs = 2 * w.dz[1]; w.head_part = w.slabs + (int64_t)splits * g.arena;
  // room for k_skinny_bwd's per-block partials: k_skinny_bwd's blocks; the fused forward's TD head leaves one per row tile of 32 or
  // 64; the DPG slice kernel (k_dx_slice<D, QPW>) one per 32-row tile of the compact layout (2 x b rounded up to 128 rows)
  const int64_t skinny = skinny_bwd_blocks(g.b, g.n_nets), tiles = compact_ws(0, g.b).rows_cap / 32;
  w.head_part_floats = (skinny > tiles ? skinny : tiles) * g.n_nets * g.head_floats;
  w.total = w.head_part + (splits ? w.head_part_floats : 0);
  return w;
}

extern "C" int64_t pqlk_mlp_bwd_ws_floats(const PqlMlpDesc* d, int64_t b, int32_t splits) {
  if (desc_ok(d) || b <= 0 || splits < 1) return 0;
  return bwd_ws(mlp_geom(d, b), splits).total;
}

// ================================================================================================
// fused hidden-layer path (fused.h)
// fusable: at least one hidden layer, hidden widths multiples of 32 and <= 1024 (4 output tiles per wave), and one
// 32-row activation tile + the bias table within the 160 KB of LDS
static size_t fused_lds_bytes(const PqlMlpDesc* d, int buf_ld, int R) {
  const size_t acts = ((size_t)32 * R * buf_ld + (size_t)(d->n_layers - 1) * (buf_ld - 4)) * sizeof(float);
  const size_t head = (size_t)8 * R * 16 * 64 * sizeof(float);   // partial tiles of the fused output layer (narrow nets: larger)
  return acts > head ? acts : head;
}

static bool fusable(const PqlMlpDesc* d, int* buf_ld_out) {
  if (d->n_layers < 2) return false;
  int64_t w = pqlk_ld(d->dims[0]);
  for (int l = 1; l < d->n_layers; ++l) {
    if (d->dims[l] % 32 != 0 || d->dims[l] > 1024) return false;
    w = d->dims[l] > w ? d->dims[l] : w;
  }
  const int64_t buf_ld = w + 4;
  if (fused_lds_bytes(d, (int)buf_ld, 1) > 160 * 1024) return false;
  if (buf_ld_out) *buf_ld_out = (int)buf_ld;
  return true;
}

static int64_t packed_net_stride(const PqlMlpDesc* d) {
  int64_t n = 0;
  for (int l = 0; l + 1 < d->n_layers; ++l) n += (int64_t)d->dims[l + 1] * pqlk_ld(d->dims[l]);
  return n;
}

extern "C" int64_t pqlk_mlp_packed_floats(const PqlMlpDesc* d) {
  if (desc_ok(d) || !fusable(d, nullptr)) return 0;
  return packed_net_stride(d) * d->n_nets;
}

extern "C" int pqlk_mlp_pack(const PqlMlpDesc* d, const float* params, float* packed, pqlk_stream_t stream) {
  int rc = desc_ok(d);
  if (rc) return rc;
  PQLK_REQUIRE(params && packed, PQLK_E_NULL);
  PQLK_REQUIRE(fusable(d, nullptr), PQLK_E_UNSUPPORTED);
  const MlpGeom g = mlp_geom(d, 0);
  PackP pp = {};
  int64_t p_off = 0, most = 0;
  for (int l = 0; l + 1 < d->n_layers; ++l) {
    pp.w_off[l] = g.w_off[l]; pp.p_off[l] = p_off;
    pp.N[l] = d->dims[l + 1]; pp.K[l] = (int)g.ld[l];
    const int64_t elems = (int64_t)pp.N[l] * pp.K[l];
    if (elems > most) most = elems;
    p_off += elems;
  }
  pp.n_layers = d->n_layers - 1;
  int blocks = (int)((most + 255) / 256);   // sized for the largest layer; the kernel's loop is grid-strided
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(k_mlp_pack, dim3(blocks, d->n_nets, pp.n_layers), dim3(256), 0, pqlk_s(stream), params, packed, pp,
                     (long long)g.net_stride, (long long)packed_net_stride(d));
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

struct FusedHead {   // output layer to run inside the fused launch (n = 0: none)
  int n, epi;
  const float* draw;
  float noise_std, noise_clip;
  float* out2;
  int64_t ld_out2;
  float* qc;   // compact copy of a scalar head's output (pqlk_mlp_forward_qc)
  const float* x2; int64_t ldx2; int x2_col0;   // second input source (pqlk_mlp_forward_qc)
  // TD head (pqlk_mlp_forward_td): see FusedP
  const float* td_qt; const float* td_rew; const float* td_done; float td_gamma_n;
  float* td_dz; float* td_head_part; float* td_loss_part;
};

// the output layer can ride along when it is at most one 32-column tile wide and the last hidden width is a multiple of 32
static bool head_fusable(const PqlMlpDesc* d) {
  return d->n_layers >= 2 && d->dims[d->n_layers] <= 32 && d->dims[d->n_layers - 1] % 32 == 0;
}
static bool fused_head_enabled() {   // PQLK_NO_FUSED_HEAD: tuning / A-B switch, read once per process
  static const bool off = getenv("PQLK_NO_FUSED_HEAD") != nullptr;
  return !off;
}
// the hidden stack AND the output layer in one launch
static bool fused_with_head(const PqlMlpDesc* d, int* buf_ld_out = nullptr) {
  return fusable(d, buf_ld_out) && head_fusable(d) && fused_head_enabled();
}

// rows per block of the fused forward, in tiles of 32: 2 (64 rows) when no hidden layer is wider than 512 (two output tiles per
// wave, 132 KB of LDS) and the halved grid still fills the 256 CUs about as well -- cost model: rounds x rows per block, 32-row
// blocks ~15 % less efficient per row.  PQLK_FUSED_ROWS = 32 / 64 overrides (tuning).
static int fused_rows(const PqlMlpDesc* d, int buf_ld, int64_t b) {
  bool wide = false;
  for (int l = 1; l < d->n_layers; ++l) wide = wide || d->dims[l] > 512;
  int R = 1;
  if (!wide && fused_lds_bytes(d, buf_ld, 2) <= 160 * 1024) {
    const int64_t b1 = ((b + 31) / 32) * d->n_nets, b2 = ((b + 63) / 64) * d->n_nets;
    const double c1 = 1.15 * (double)((b1 + 255) / 256), c2 = 2.0 * (double)((b2 + 255) / 256);
    if (c2 <= c1) R = 2;
    static const int forced = [] { const char* e = getenv("PQLK_FUSED_ROWS"); return e ? atoi(e) : 0; }();
    if (forced == 32) R = 1;
    if (forced == 64) R = 2;
  }
  return R;
}

static int launch_fused_hidden(const MlpGeom& g, const float* params, const float* packed, const float* x, int64_t ldx, float* acts,
                               int stash_all, hipStream_t st, const FusedHead* head = nullptr, bool out_only = false) {
  const PqlMlpDesc* d = g.d;
  const int64_t b = g.b;
  FusedP p = {};
  int buf_ld = 0;
  if (!fusable(d, &buf_ld)) return PQLK_E_UNSUPPORTED;
  p.X = x; p.params = params; p.packed = packed; p.acts = acts;
  p.B = (int)b; p.ldx = (int)ldx; p.n_hidden = d->n_layers - 1; p.stash_all = stash_all; p.buf_ld = buf_ld; p.n_nets = d->n_nets;
  p.net_stride = g.net_stride; p.packed_net_stride = packed_net_stride(d);
  int64_t p_off = 0;
  for (int l = 0; l <= d->n_layers; ++l) p.dims[l] = d->dims[l];
  for (int l = 0; l + 1 < d->n_layers; ++l) {
    p.b_off[l] = g.b_off[l]; p.p_off[l] = p_off; p.a_off[l] = g.a_off[l];
    p_off += (int64_t)d->dims[l + 1] * g.ld[l];
  }
  if (head && head->n > 0) {
    const int L = d->n_layers;
    p.head_n = head->n; p.head_epi = head->epi; p.head_ld = (int)g.ld[L]; p.ld_out2 = (int)head->ld_out2;
    p.head_w_off = g.w_off[L - 1]; p.head_b_off = g.b_off[L - 1];
    p.head_a_off = out_only ? 0 : g.a_off[L - 1];   // out_only: `acts` IS the output block
    p.draw = head->draw; p.out2 = head->out2; p.noise_std = head->noise_std; p.noise_clip = head->noise_clip;
    p.qc = head->n == 1 ? head->qc : nullptr;
    p.X2 = head->x2; p.ldx2 = (int)head->ldx2; p.x2_col0 = head->x2_col0;
    if (head->td_dz) {
      p.td_qt = head->td_qt; p.td_rew = head->td_rew; p.td_done = head->td_done; p.td_gamma_n = head->td_gamma_n;
      p.td_two_over_b = 2.0f / (float)b;
      p.td_dz = head->td_dz; p.td_head_part = head->td_head_part; p.td_loss_part = head->td_loss_part;
      p.td_part_floats = g.head_floats;
    }
  }
  bool wide = false;
  for (int l = 1; l < d->n_layers; ++l) wide = wide || d->dims[l] > 512;
  const int R = fused_rows(d, buf_ld, b);
  static PqlkPerDeviceOnce attr_once;
  if (int rc = attr_once.run([&] {
        const void* ks[6] = {reinterpret_cast<const void*>(&k_mlp_fwd_fused<1, 2>), reinterpret_cast<const void*>(&k_mlp_fwd_fused<2, 2>),
                             reinterpret_cast<const void*>(&k_mlp_fwd_fused<1, 4>), reinterpret_cast<const void*>(&k_mlp_fwd_fused<1, 2, true>),
                             reinterpret_cast<const void*>(&k_mlp_fwd_fused<2, 2, true>), reinterpret_cast<const void*>(&k_mlp_fwd_fused<1, 4, true>)};
        for (const void* k : ks) {
          hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
          if (e != hipSuccess) return -(int)e;
        }
        return 0;
      }))
    return rc;
  const size_t shmem = fused_lds_bytes(d, buf_ld, R);
  dim3 grid((unsigned)(((b + 32 * R - 1) / (32 * R)) * d->n_nets)), block(64 * FUSED_NW);
  if (out_only) {
    if (wide) hipLaunchKernelGGL((k_mlp_fwd_fused<1, 4, true>), grid, block, shmem, st, p);
    else if (R == 2) hipLaunchKernelGGL((k_mlp_fwd_fused<2, 2, true>), grid, block, shmem, st, p);
    else hipLaunchKernelGGL((k_mlp_fwd_fused<1, 2, true>), grid, block, shmem, st, p);
  } else if (wide) hipLaunchKernelGGL((k_mlp_fwd_fused<1, 4>), grid, block, shmem, st, p);
  else if (R == 2) hipLaunchKernelGGL((k_mlp_fwd_fused<2, 2>), grid, block, shmem, st, p);
  else hipLaunchKernelGGL((k_mlp_fwd_fused<1, 2>), grid, block, shmem, st, p);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

extern "C" int pqlk_mlp_forward(const PqlMlpDesc* d, const float* params, const float* packed, int32_t stash_all,
                                const float* x, int64_t ldx, int64_t b, int32_t out_act, const float* draw, float noise_std,
                                float noise_clip, float* acts, float* out2, int64_t ld_out2, pqlk_stream_t stream) {
  int rc = desc_ok(d);
  if (rc) return rc;
  PQLK_REQUIRE(params && x && acts, PQLK_E_NULL);
  PQLK_REQUIRE(b > 0 && b < (1LL << 30), PQLK_E_SHAPE);
  PQLK_REQUIRE(ldx % 32 == 0 && ldx >= pqlk_ld(d->dims[0]), PQLK_E_ALIGN);
  PQLK_REQUIRE(pqlk_aligned16(params) && pqlk_aligned16(x) && pqlk_aligned16(acts), PQLK_E_ALIGN);
  PQLK_REQUIRE(out_act == PQLK_ACT_NONE || out_act == PQLK_ACT_TANH || out_act == PQLK_ACT_TANH_NOISE, PQLK_E_UNSUPPORTED);
  if (out_act == PQLK_ACT_TANH_NOISE) PQLK_REQUIRE(draw, PQLK_E_NULL);
  if (out2) PQLK_REQUIRE(d->n_nets == 1 && ld_out2 >= d->dims[d->n_layers], PQLK_E_SHAPE);
  PQLK_REQUIRE(stash_all >= 0 && stash_all <= PQLK_STASH_OUTPUT_ONLY, PQLK_E_RANGE);
  const MlpGeom g = mlp_geom(d, b);
  const int L = d->n_layers;
  int l_first = 0;
  const bool out_only = stash_all == PQLK_STASH_OUTPUT_ONLY;   // `acts` = the output block alone: fused stack + fused head only
  if (out_only) PQLK_REQUIRE(packed && fused_with_head(d), PQLK_E_UNSUPPORTED);
  if (packed && fusable(d, nullptr)) {  // all hidden layers in one launch, activations resident in LDS
    PQLK_REQUIRE(pqlk_aligned16(packed), PQLK_E_ALIGN);
    FusedHead head = {};
    if (head_fusable(d) && fused_head_enabled()) {   // ... and the output layer too
      head.n = d->dims[L]; head.epi = out_act; head.draw = draw; head.noise_std = noise_std; head.noise_clip = noise_clip;
      head.out2 = out2; head.ld_out2 = ld_out2;
    }
    rc = launch_fused_hidden(g, params, packed, x, ldx, acts, stash_all == 1 ? 1 : 0, pqlk_s(stream), &head, out_only);
    if (rc) return rc;
    l_first = head.n > 0 ? L : L - 1;
  }
  for (int l = l_first; l < L; ++l) {
    const int64_t ld_in = g.ld[l], ld_out = g.ld[l + 1];
    GemmP p = {};
    if (l == 0) {
      p.A = x; p.lda = (int)ldx; p.sA = 0;
    } else {
      p.A = acts + g.a_off[l - 1]; p.lda = (int)ld_in; p.sA = b * ld_in;
    }
    p.B = params + g.w_off[l]; p.ldb = (int)ld_in; p.sB = g.net_stride;
    p.bias = params + g.b_off[l]; p.sBias = g.net_stride;
    p.C = acts + g.a_off[l]; p.ldc = (int)ld_out; p.sC = b * ld_out;
    p.M = (int)b; p.N = d->dims[l + 1]; p.K = (int)ld_in;
    p.ncols_store = (int)ld_out;
    p.groups = d->n_nets;
    p.epi = EPI_ELU;
    if (l == L - 1) {
      p.epi = out_act == PQLK_ACT_TANH ? EPI_TANH : (out_act == PQLK_ACT_TANH_NOISE ? EPI_TANH_NOISE : EPI_NONE);
      p.aux = draw; p.sAux = 0;
      p.noise_std = noise_std; p.noise_clip = noise_clip;
      p.C2 = out2; p.ldc2 = (int)ld_out2;
    }
    if (l == L - 1 && skinny_fwd_ok(d->dims[l + 1], p.K)) {  // out features <= 16: streaming VALU kernel, no MFMA tile waste
      SkinnyP q = {};
      q.X = p.A; q.ldx = p.lda; q.sX = p.sA;
      q.W = p.B; q.ldk = p.ldb; q.sW = p.sB;
      q.bias = p.bias; q.sBias = p.sBias;
      q.C = p.C; q.ldc = p.ldc; q.sC = p.sC;
      q.M = p.M; q.N = p.N; q.K = p.K;
      q.epi = p.epi == EPI_TANH ? SK_EPI_TANH : (p.epi == EPI_TANH_NOISE ? SK_EPI_TANH_NOISE : SK_EPI_NONE);
      q.draw = p.aux; q.noise_std = noise_std; q.noise_clip = noise_clip;
      q.C2 = p.C2; q.ldc2 = p.ldc2;
      rc = launch_skinny_fwd(q, d->n_nets, pqlk_s(stream));
    } else if (l == L - 1 && narrow_fwd_ok(p)) {   // 5..64 outputs (action heads, C51 logits): one wave per 32-row tile
      rc = launch_fwd_narrow(p, d->n_nets, pqlk_s(stream));
    } else {
      rc = launch_auto<MODE_FWD>(p, d->n_nets, pqlk_s(stream));
    }
    if (rc) return rc;
  }
  return PQLK_OK;
}

// ------------------------------------------------------------------------------------------------
// sum the split slabs in fixed order -> gradient arena (deterministic).  Two optional extras ride in the same launch:
//  * head partials: when the last layer's dW / db came out of k_skinny_bwd (one partial per 64-row block instead of one per
//    split) the main blocks skip arena offsets inside [head_off, net_stride) of each net and `head_blocks` extra blocks fold
//    them: one WAVE per 16-B quad, lane l sums partials l, l + 64, ... in that order, then a fixed xor-shuffle tree -- all
//    partials of a quad are in flight at once (one thread walking 128 partials serially cost 30 us);
//  * the squared-norm partials of clip_grad_norm_: with `sq_part` every block also leaves sum(g^2) over what it reduced, and
//    block 0 bumps the optimiser's step counter: k_adamw folds those partials exactly as it folds k_sumsq's.
struct ReduceP {
  const float* slabs; int splits; long long n;
  float* out;
  const float* head_part; int head_parts; int n_nets; long long net_stride, head_off, head_floats;
  long long seg_off, seg_len;   // the arena range [seg_off, seg_off + seg_len) of every net is reduced (whole arena: 0, net_stride)
  int main_blocks;
  float* sq_part; int32_t* step_dev;
  const int* parts_dev;   // optional: only the first (parts_dev[3] + 31) / 32 head partials exist (compact tiles in use, minnet.h)
};

__global__ __launch_bounds__(256) void k_reduce_slabs(ReduceP p) {
  __shared__ float shw[4];
  float acc = 0.f;
  if ((int)blockIdx.x < p.main_blocks) {
    const long long sq = p.seg_len >> 2, n4 = sq * p.n_nets;  // layer blocks start and end on multiples of 32 floats
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)p.main_blocks * 256) {
      long long q = i, base = p.seg_off;
      while (q >= sq) { q -= sq; base += p.net_stride; }
      if (p.head_parts > 0 && p.seg_off + (q << 2) >= p.head_off) continue;   // a quad never straddles the head's start
      const long long off = base + (q << 2);
      float4 s = *reinterpret_cast<const float4*>(p.slabs + off);
      for (int k = 1; k < p.splits; ++k) {
        const float4 t = *reinterpret_cast<const float4*>(p.slabs + (long long)k * p.n + off);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
      }
      *reinterpret_cast<float4*>(p.out + off) = s;
      acc += (s.x * s.x + s.y * s.y) + (s.z * s.z + s.w * s.w);
    }
    if (!p.sq_part) return;
    acc = wave_sum(acc);
  } else {
    const int lane = threadIdx.x & 63;
    const long long hq = p.head_floats >> 2;                                      // quads per net
    const long long e = ((long long)blockIdx.x - p.main_blocks) * 4 + (threadIdx.x >> 6);   // this wave's quad
    if (e < hq * p.n_nets) {
      const long long net = e / hq, q = e - net * hq;
      const float* hp = p.head_part + net * p.head_floats + 4 * q;
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      const int parts = p.parts_dev ? min(p.head_parts, (p.parts_dev[3] + 31) / 32) : p.head_parts;
      for (int k = lane; k < parts; k += 64) {
        const float4 t = *reinterpret_cast<const float4*>(hp + (long long)k * p.n_nets * p.head_floats);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
      }
      s.x = wave_sum(s.x); s.y = wave_sum(s.y); s.z = wave_sum(s.z); s.w = wave_sum(s.w);
      if (lane == 0) *reinterpret_cast<float4*>(p.out + net * p.net_stride + p.head_off + 4 * q) = s;
      acc = (s.x * s.x + s.y * s.y) + (s.z * s.z + s.w * s.w);   // same value in every lane
    }
    if (!p.sq_part) return;
  }
  if ((threadIdx.x & 63) == 0) shw[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    p.sq_part[blockIdx.x] = (shw[0] + shw[1]) + (shw[2] + shw[3]);
    if (blockIdx.x == 0 && p.step_dev) p.step_dev[0] += 1;
  }
}

// The output layer's backward takes one of three kernels; decided HERE and nowhere else (pqlk_mlp_norm_parts, the TD entry points
// and the DPG predicates read it through head_is_fused)
enum HeadBwd { HEAD_GEMM, HEAD_SKINNY, HEAD_FUSED };   // k_gemm dW + dX | k_skinny_dw + k_skinny_dx | k_skinny_bwd (with grads only)
static HeadBwd head_bwd_kind(const PqlMlpDesc* d) {
  const int L = d->n_layers, N = d->dims[L], K = (int)pqlk_ld(d->dims[L - 1]);
  if (!skinny_bwd_ok(N, K)) return HEAD_GEMM;
  return L >= 2 && skinny_bwd_fused_ok(N, K) ? HEAD_FUSED : HEAD_SKINNY;
}
static bool head_is_fused(const PqlMlpDesc* d) { return head_bwd_kind(d) == HEAD_FUSED; }
static int head_fold_blocks(const MlpGeom& g) { return (int)((g.head_floats / 4 * g.n_nets + 3) / 4); }   // one wave per quad
static int reduce_main_blocks(int64_t arena, bool for_norm) {
  int64_t blocks = (arena / 4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  const int64_t cap = for_norm ? 1024 : 2048;
  return (int)(blocks > cap ? cap : blocks);
}

// number of squared-norm partials pqlk_mlp_backward_norm leaves for pqlk_adamw_polyak_fused(prenorm = this)
extern "C" int32_t pqlk_mlp_norm_parts(const PqlMlpDesc* d) {
  if (desc_ok(d)) return 0;
  const MlpGeom g = mlp_geom(d, 0);
  return reduce_main_blocks(g.arena, true) + (head_is_fused(d) ? head_fold_blocks(g) : 0);
}

struct TdHead {   // the scalar twin-Q head forms dL/dQ itself (pqlk_mlp_backward_td)
  const float* qt; const float* rew; const float* done; float gamma_n; float* loss_part;
};

// One backward call.  Filled field by field; a mode that is not in use stays zero.
struct BwdCall {
  const PqlMlpDesc* d; const float* params; const float* x; int64_t ldx, b; const float* acts;
  const float* dy;             // dL/dZ of the last layer; not read with td, head_done or a layer range below the last layer
  float* grads; int splits;    // parameter gradient through `splits` slabs of the workspace
  float* dx; int64_t ld_dx;    // input gradient, summed over nets ...
  int dx_col0, dx_cols; const float* dx_tanh_of; int64_t ld_tanh;   // ... or columns [dx_col0, dx_col0 + dx_cols) of it through tanh'
  float* ws; int64_t ws_floats;
  float* sq_part; int32_t* step_dev;   // squared-norm partials and the step increment out of the reduction (pqlk_mlp_backward_norm)
  pqlk_stream_t stream;
  const TdHead* td;            // TD head: the fused head kernel forms dL/dQ itself
  // layer range: only layers l_hi >= l >= l_lo of the chain (dW_l, dX_l) and the slab reduction of exactly those layers (the
  // data-parallel buckets of pqlk_mlp_backward_layers); calls must walk the layers downwards over the same workspace
  bool ranged; int l_hi, l_lo;
  // head_done > 0: the last layer's backward already ran elsewhere (pqlk_mlp_forward_td, pqlk_dpg_backward_fused): dL/dZ of the last
  // hidden layer sits in the first dZ buffer and `head_done` row-tile partials of the head's dW / db in the partial area, of which
  // only the first (head_parts_dev[3] + 31) / 32 exist when head_parts_dev is given
  int head_done; const int* head_parts_dev;
};

static BwdCall bwd_call(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b, const float* acts,
                        float* grads, int32_t splits, float* ws, int64_t ws_floats, pqlk_stream_t stream) {
  BwdCall c = {};
  c.d = d; c.params = params; c.x = x; c.ldx = ldx; c.b = b; c.acts = acts;
  c.grads = grads; c.splits = splits; c.ws = ws; c.ws_floats = ws_floats; c.stream = stream;
  return c;
}

struct BwdRun {   // what the steps of one call share
  const BwdCall& c; MlpGeom g; int splits;
  float* dact[2]; float* slabs; float* head_part;
  hipStream_t st;
};
struct LayerIO {   // layer l reads dL/dZ_l from where layer l + 1 left it and writes dL/dZ_{l-1} into the other buffer
  const float* dy;                                     // (n_nets, b, ld_out)
  const float* in; int64_t in_ld, in_stride;           // the layer's input: x or the stash
  float* dz;
};
static LayerIO bwd_layer_io(const BwdRun& r, int l) {
  const int L = r.g.L;
  LayerIO io = {};
  io.dy = l == L - 1 ? r.c.dy : r.dact[(L - 2 - l) & 1];
  io.dz = r.dact[(L - 1 - l) & 1];
  if (l == 0) {
    io.in = r.c.x; io.in_ld = r.c.ldx; io.in_stride = 0;
  } else {
    io.in = r.c.acts + r.g.a_off[l - 1]; io.in_ld = r.g.ld[l]; io.in_stride = r.c.b * r.g.ld[l];
  }
  return io;
}

static int bwd_layer_dw(const BwdRun& r, int l, const LayerIO& io) {   // dW_l, db_l into the slabs
  const MlpGeom& g = r.g;
  GemmP p = {};
  p.A = io.dy; p.lda = (int)g.ld[l + 1]; p.sA = g.b * g.ld[l + 1];
  p.B = io.in; p.ldb = (int)io.in_ld; p.sB = io.in_stride;
  p.C = r.slabs + g.w_off[l]; p.ldc = (int)g.ld[l]; p.sC = g.net_stride;
  p.dbias = r.slabs + g.b_off[l]; p.sBias = g.net_stride;
  p.M = g.d->dims[l + 1]; p.N = (int)g.ld[l]; p.K = (int)g.b;
  p.ncols_store = (int)g.ld[l + 1];
  p.groups = g.n_nets; p.splits = r.splits;
  p.rows_per_split = (int)pqlk_round_up((g.b + r.splits - 1) / r.splits, KT_MAX);
  p.sSplit = g.arena;
  // B operand limit: X has ldx >= ld_in columns; only the first ld_in are wanted.  The loader bounds
  // columns by p.ldb, so clamp through N: tiles never start beyond N and pads inside ldb are zero.
  return launch_auto<MODE_DW>(p, g.n_nets * r.splits, r.st);
}

static int bwd_layer_dx(const BwdRun& r, int l, const LayerIO& io) {
  const MlpGeom& g = r.g;
  const BwdCall& c = r.c;
  if (l == 0 && !c.dx) return PQLK_OK;
  GemmP p = {};
  p.A = io.dy; p.lda = (int)g.ld[l + 1]; p.sA = g.b * g.ld[l + 1];
  p.B = c.params + g.w_off[l]; p.ldb = (int)g.ld[l]; p.sB = g.net_stride;
  p.M = (int)g.b; p.N = g.d->dims[l]; p.K = g.d->dims[l + 1];
  p.ncols_store = (int)g.ld[l];
  p.groups = g.n_nets;
  if (l > 0) {  // dH_{l-1} = (dY_l W_l) * ELU'(H_{l-1})
    p.C = io.dz; p.ldc = (int)g.ld[l]; p.sC = g.b * g.ld[l];
    p.aux = io.in; p.ldaux = (int)io.in_ld; p.sAux = io.in_stride;
    p.zsum = 0; p.epi = EPI_DELU;
    return launch_auto<MODE_DX>(p, g.n_nets, r.st);
  }
  // input gradient, summed over nets
  p.C = c.dx; p.ldc = (int)c.ld_dx; p.sC = 0;
  p.zsum = 1; p.epi = EPI_NONE;
  if (c.dx_tanh_of) {
    p.epi = EPI_DTANH_SLICE; p.aux = c.dx_tanh_of; p.ldaux = (int)c.ld_tanh; p.col0 = c.dx_col0; p.ncol = c.dx_cols;
  }
  if (dx_slice_ok(p)) return launch_dx_slice(p, r.st);   // narrow slice: split-reduction MFMA kernel (narrow.h)
  return launch_auto<MODE_DX>(p, 1, r.st);
}

// the last layer; *head_blocks = number of per-block partials of its dW / db left in head_part (0: they went into the slabs)
static int bwd_head(const BwdRun& r, const LayerIO& io, int* head_blocks) {
  const MlpGeom& g = r.g;
  const BwdCall& c = r.c;
  const int l = g.L - 1;
  const HeadBwd kind = head_bwd_kind(g.d);
  int rc = PQLK_OK;
  if (kind == HEAD_GEMM || io.in_ld < g.ld[l]) {
    if (c.grads) rc = bwd_layer_dw(r, l, io);
    return rc ? rc : bwd_layer_dx(r, l, io);
  }
  SkinnyP q = {};
  q.X = io.in; q.ldx = (int)io.in_ld; q.sX = io.in_stride;
  q.dY = io.dy; q.ldy = (int)g.ld[l + 1]; q.sY = g.b * g.ld[l + 1];
  q.M = (int)g.b; q.N = g.d->dims[l + 1]; q.K = (int)g.ld[l]; q.ldk = (int)g.ld[l]; q.ldc = (int)g.ld[l + 1];
  if (c.grads && kind == HEAD_FUSED) {   // dX + dW + db in one pass over the activations
    q.W = c.params + g.w_off[l]; q.sW = g.net_stride;
    q.C = io.dz; q.sC = g.b * g.ld[l];
    q.epi = SK_EPI_DELU;
    *head_blocks = skinny_bwd_blocks(g.b, g.n_nets);
    if (c.td) {
      q.td_q = c.acts + g.a_off[l]; q.td_qt = c.td->qt; q.td_rew = c.td->rew; q.td_done = c.td->done;
      q.td_gamma_n = c.td->gamma_n; q.td_two_over_b = 2.0f / (float)g.b; q.td_part = c.td->loss_part;
    }
    return launch_skinny_bwd(q, g.n_nets, r.head_part, (long long)g.head_floats, r.st);
  }
  if (c.grads) {
    q.dW = r.slabs + g.w_off[l]; q.dB = r.slabs + g.b_off[l]; q.sW = g.net_stride; q.sBias = g.net_stride; q.sSplit = g.arena;
    q.splits = r.splits; q.rows_per_split = (int)pqlk_round_up((g.b + r.splits - 1) / r.splits, KT_MAX);
    rc = launch_skinny_dw(q, g.n_nets, r.st);
    if (rc) return rc;
  }
  if (l == 0) return bwd_layer_dx(r, l, io);   // a one-layer net: the input gradient is a GEMM
  q.W = c.params + g.w_off[l]; q.sW = g.net_stride;
  q.C = io.dz; q.sC = g.b * g.ld[l];
  q.epi = SK_EPI_DELU;
  return launch_skinny_dx(q, g.n_nets, r.st);
}

static int mlp_backward_impl(const BwdCall& c) {
  const PqlMlpDesc* d = c.d;
  int rc = desc_ok(d);
  if (rc) return rc;
  const int L = d->n_layers, l_hi = c.ranged ? c.l_hi : L - 1, l_lo = c.l_lo;
  PQLK_REQUIRE(l_lo >= 0 && l_lo <= l_hi && l_hi < L, PQLK_E_RANGE);
  PQLK_REQUIRE(!c.ranged || (c.grads && !c.dx && !c.sq_part), PQLK_E_UNSUPPORTED);
  PQLK_REQUIRE(c.params && c.x && c.acts && (c.dy || c.td || c.head_done || l_hi < L - 1) && c.ws, PQLK_E_NULL);
  PQLK_REQUIRE(!c.head_done || (!c.ranged && c.grads && !c.dx && !c.td && L >= 2), PQLK_E_UNSUPPORTED);
  if (c.td) PQLK_REQUIRE(c.grads && d->n_nets == 2 && d->dims[L] == 1 && head_is_fused(d), PQLK_E_UNSUPPORTED);
  PQLK_REQUIRE(c.b > 0 && c.b < (1LL << 30), PQLK_E_SHAPE);
  PQLK_REQUIRE(c.ldx % 32 == 0 && c.ldx >= pqlk_ld(d->dims[0]), PQLK_E_ALIGN);
  PQLK_REQUIRE(c.grads || c.dx, PQLK_E_NULL);
  if (c.grads) PQLK_REQUIRE(c.splits >= 1 && c.splits <= 64, PQLK_E_SHAPE);
  BwdRun r = {c, mlp_geom(d, c.b), c.grads ? c.splits : 0};
  const MlpGeom& g = r.g;
  const BwdWs w = bwd_ws(g, r.splits);
  PQLK_REQUIRE(c.ws_floats >= w.total, PQLK_E_WORKSPACE);
  PQLK_REQUIRE(!c.sq_part || c.grads, PQLK_E_NULL);
  if (c.dx) {
    PQLK_REQUIRE(c.ld_dx % 32 == 0, PQLK_E_ALIGN);
    if (c.dx_tanh_of) PQLK_REQUIRE(c.dx_col0 >= 0 && c.dx_cols > 0 && c.dx_col0 + c.dx_cols <= d->dims[0] && c.ld_dx >= c.dx_cols,
                                   PQLK_E_RANGE);
    else PQLK_REQUIRE(c.ld_dx >= pqlk_ld(d->dims[0]), PQLK_E_SHAPE);
  }
  r.dact[0] = c.ws + w.dz[0]; r.dact[1] = c.ws + w.dz[1]; r.slabs = c.ws + w.slabs; r.head_part = c.ws + w.head_part;
  r.st = pqlk_s(c.stream);
  int head_blocks = c.head_done;   // > 0: the last layer's dW / db are per-block partials in head_part

  for (int l = c.head_done ? l_hi - 1 : l_hi; l >= l_lo; --l) {
    const LayerIO io = bwd_layer_io(r, l);
    if (l == L - 1) {
      rc = bwd_head(r, io, &head_blocks);
    } else {
      if (c.grads) rc = bwd_layer_dw(r, l, io);
      if (!rc) rc = bwd_layer_dx(r, l, io);
    }
    if (rc) return rc;
  }
  if (c.grads) {
    ReduceP p = {};
    p.slabs = r.slabs; p.splits = r.splits; p.n = g.arena; p.out = c.grads;
    p.head_part = r.head_part; p.head_parts = head_blocks; p.n_nets = g.n_nets; p.net_stride = g.net_stride;
    p.head_off = g.w_off[L - 1]; p.head_floats = g.head_floats;
    p.seg_off = g.w_off[l_lo];   // layers sit in ascending order inside a net's block
    p.seg_len = (l_hi < L - 1 ? g.w_off[l_hi + 1] : g.net_stride) - p.seg_off;
    p.sq_part = c.sq_part; p.step_dev = c.step_dev; p.parts_dev = c.head_parts_dev;
    p.main_blocks = reduce_main_blocks(p.seg_len * g.n_nets, c.sq_part != nullptr);   // with sq_part: at most 1024 + head blocks partials
    const int extra = head_blocks > 0 ? head_fold_blocks(g) : 0;
    hipLaunchKernelGGL(k_reduce_slabs, dim3(p.main_blocks + extra), dim3(256), 0, r.st, p);
    PQLK_LAUNCH_CHECK();
  }
  return PQLK_OK;
}

// ------------------------------------------------------------------------------------------------
// DPG backward through the frozen twin critic (pql_p_learner.py:55-58): input gradient only, action columns only, chained
// through the actor's tanh.  With scalar Q heads the samples are partitioned by the net that attained min(Q1, Q2) and the dX
// chain runs over compact rows (minnet.h): half the MFMA work of the dense chain, same per-sample bits.  Anything else
// (distributional heads, widths that are not multiples of 128, a single net) takes the dense chain of pqlk_mlp_backward.
static bool compact_chain_ok(const PqlMlpDesc* d) {
  const int L = d->n_layers;
  if (d->n_nets != 2 || L < 3 || d->dims[L] != 1) return false;
  if (!skinny_bwd_ok(1, (int)pqlk_ld(d->dims[L - 1]))) return false;
  for (int l = 1; l < L; ++l)
    if (d->dims[l] % 32 != 0) return false;
  for (int l = 1; l < L - 1; ++l)
    if (d->dims[l] % 128 != 0) return false;   // output width of the dX GEMM of layer l + 1: whole 128-column tiles
  return true;
}
static bool minnet_ok(const PqlMlpDesc* d, const float* dx, const float* dx_tanh_of, int dx_cols) {
  return dx && dx_tanh_of && dx_cols <= 32 && compact_chain_ok(d);
}

// Tile shape of the compact dX products (rows = samples partitioned by owning net: b + ties + up to 254 pad rows instead of 2 b).
// 128 x 128 tiles at two per CU leave a handful of CUs with twice the work (82 -> 63 us on the 512-wide layer with 128 x 64 tiles,
// round 2).  Round 4 (`profiles/r04_b_compact_tile_ab.log`, alternating runs): 64 x 64 tiles -- four times the blocks of short
// products (K = 256 / 512) -- run the P-learner alone 2.8 % faster than 128 x 64 (1960-1970 -> 2016-2022 steps/s) and leave the
// three-stream schedule's `value` where it was (medians 1212 vs 1212): the default.  PQLK_COMPACT_TILE = 0 (128 x 64), 1 (128 x
// 128), 2 (64 x 64), 3 / 4 (64 x 64 for the first / the later product only) is the A/B switch.
static int launch_compact_dx(const GemmP& p, bool first, hipStream_t st) {
  static const int ctile = [] { const char* e = getenv("PQLK_COMPACT_TILE"); return e ? atoi(e) : 2; }();
  const bool small = ctile == 2 || (ctile == 3 && first) || (ctile == 4 && !first);
  if (ctile == 1) return launch_gemm<MODE_DX, 128, 128, EPI_DELU>(p, 1, st);
  if (small) return launch_gemm<MODE_DX, 64, 64, EPI_DELU>(p, 1, st);
  return launch_gemm<MODE_DX, 128, 64, EPI_DELU>(p, 1, st);
}

struct CompactRun {   // the critic's side of a compact chain: its geometry, arena, stash and the pieces of its workspace
  const MlpGeom& g; const float* params; const float* acts;
  int64_t rows_cap; float* dz[2]; int* perm; int* mn; int* tie0;
};
static CompactRun compact_run(const MlpGeom& g, const float* params, const float* acts, float* ws) {
  const CompactWs w = compact_ws(g.max_hidden_ld, g.b);
  return {g, params, acts, w.rows_cap, {ws + w.dz[0], ws + w.dz[1]}, reinterpret_cast<int*>(ws + w.perm),
          reinterpret_cast<int*>(ws + w.mn), reinterpret_cast<int*>(ws + w.tie0)};
}

// hidden layers: dH_{l-1} = (dZ_l W_l) * ELU'(H_{l-1}) over compact rows, one net per 128-row tile; dZ_{L-1} is in dz[0] and dZ_1
// ends up in dz[L & 1]
static int compact_dx_chain(const CompactRun& r, hipStream_t st) {
  const MlpGeom& g = r.g;
  int flip = 0;
  for (int l = g.L - 2; l >= 1; --l, flip ^= 1) {
    GemmP p = {};
    p.A = r.dz[flip]; p.lda = (int)g.ld[l + 1]; p.sA = 0;
    p.B = r.params + g.w_off[l]; p.ldb = (int)g.ld[l]; p.sB = g.net_stride;
    p.C = r.dz[flip ^ 1]; p.ldc = (int)g.ld[l]; p.sC = 0;
    p.aux = r.acts + g.a_off[l - 1]; p.ldaux = (int)g.ld[l]; p.sAux = g.b * g.ld[l];
    p.M = (int)r.rows_cap; p.N = g.d->dims[l]; p.K = g.d->dims[l + 1];
    p.ncols_store = p.ldc;
    p.groups = 2; p.zsum = 0; p.epi = EPI_DELU;
    p.perm = r.perm; p.mn = r.mn;
    if (int rc = launch_compact_dx(p, l == g.L - 2, st)) return rc;
  }
  return PQLK_OK;
}

// first layer: columns [col0, col0 + ncol) only, through tanh', scattered back to batch rows of `out`
static GemmP compact_slice(const CompactRun& r, float* out, int64_t ld_out, int col0, int ncol, const float* tanh_of, int64_t ld_tanh) {
  const MlpGeom& g = r.g;
  GemmP p = {};
  p.A = r.dz[g.L & 1]; p.lda = (int)g.ld[1]; p.sA = 0;
  p.B = r.params + g.w_off[0]; p.ldb = (int)g.ld[0]; p.sB = g.net_stride;
  p.C = out; p.ldc = (int)ld_out; p.sC = 0;
  p.M = (int)r.rows_cap; p.N = g.d->dims[0]; p.K = g.d->dims[1];
  p.ncols_store = p.ldb;
  p.groups = 1; p.zsum = 1;
  p.epi = EPI_DTANH_SLICE; p.aux = tanh_of; p.ldaux = (int)ld_tanh; p.col0 = col0; p.ncol = ncol;
  p.perm = r.perm; p.mn = r.mn;
  return p;
}

extern "C" int64_t pqlk_dpg_backward_ws_floats(const PqlMlpDesc* d, int64_t b) {
  if (desc_ok(d) || b <= 0) return 0;
  const MlpGeom g = mlp_geom(d, b);
  const int64_t dense = bwd_ws(g, 1).total, compact = compact_ws(g.max_hidden_ld, b).total;
  return dense > compact ? dense : compact;
}

extern "C" int pqlk_dpg_critic_backward(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b,
                                        const float* acts, const float* dy, float* dx, int64_t ld_dx, int32_t dx_col0,
                                        int32_t dx_cols, const float* dx_tanh_of, int64_t ld_tanh, const uint8_t* owner, float* ws,
                                        int64_t ws_floats, pqlk_stream_t stream) {
  int rc = desc_ok(d);
  if (rc) return rc;
  PQLK_REQUIRE(ws_floats >= pqlk_dpg_backward_ws_floats(d, b), PQLK_E_WORKSPACE);
  if (!minnet_ok(d, dx, dx_tanh_of, dx_cols) || b > 131072) {   // (the one-block partition holds <= 128 samples per thread)
    BwdCall c = bwd_call(d, params, x, ldx, b, acts, nullptr, 1, ws, ws_floats, stream);
    c.dy = dy; c.dx = dx; c.ld_dx = ld_dx; c.dx_col0 = dx_col0; c.dx_cols = dx_cols; c.dx_tanh_of = dx_tanh_of; c.ld_tanh = ld_tanh;
    return mlp_backward_impl(c);
  }
  PQLK_REQUIRE(params && acts && dy && ws, PQLK_E_NULL);
  PQLK_REQUIRE(b > 0 && b < (1LL << 29), PQLK_E_SHAPE);
  PQLK_REQUIRE(ld_dx % 32 == 0 && dx_col0 >= 0 && dx_cols > 0 && dx_col0 + dx_cols <= d->dims[0] && ld_dx >= dx_cols, PQLK_E_RANGE);
  const MlpGeom g = mlp_geom(d, b);
  const CompactRun r = compact_run(g, params, acts, ws);
  const int L = g.L;
  hipStream_t st = pqlk_s(stream);
  // 1. partition by owning net
  hipLaunchKernelGGL(k_minnet_partition, dim3(1), dim3(1024), 0, st, owner, acts + g.a_off[L - 1], g.ld[L], b, r.perm, r.rows_cap, r.mn);
  PQLK_LAUNCH_CHECK();
  // 2. head: dZ_{L-1} in compact rows
  {
    MinnetHeadP h = {};
    h.H = acts + g.a_off[L - 2]; h.sH = b * g.ld[L - 1]; h.ldh = (int)g.ld[L - 1];
    h.W = params + g.w_off[L - 1]; h.sW = g.net_stride; h.ldk = (int)g.ld[L - 1];
    h.dY = dy; h.sY = b * g.ld[L]; h.ldy = (int)g.ld[L];
    h.C = r.dz[0]; h.perm = r.perm; h.mn = r.mn; h.N = 1; h.K = h.ldk; h.rows_cap = r.rows_cap;
    h.zero_out = dx; h.zero_floats = b * ld_dx;
    int64_t blocks = r.rows_cap / 4;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_minnet_head_dx, dim3((unsigned)blocks), dim3(256), (size_t)2 * h.N * h.K * sizeof(float), st, h);
    PQLK_LAUNCH_CHECK();
  }
  // 3. hidden layers, 4. first layer
  rc = compact_dx_chain(r, st);
  if (rc) return rc;
  const GemmP p = compact_slice(r, dx, ld_dx, dx_col0, dx_cols, dx_tanh_of, ld_tanh);
  PQLK_REQUIRE(dx_slice_ok(p), PQLK_E_UNSUPPORTED);
  return launch_dx_slice(p, st);
}

// ---- round 4: the P-learner's backward through the frozen critic in FOUR launches (was seven) -----------------------------------
// k_dpg_minnet_head (DPG loss partials + partition + compact head, off the compact Q the fused forward left), two compact dX GEMMs,
// k_dx_slice<D, QPW> (action slice through tanh' + the ACTOR's head backward).  Needs: twin scalar-head critic that the min-net
// chain takes (compact_chain_ok) with a fused forward + fused head (so that qc exists), first hidden width a multiple of 128 (slice
// ring), an actor whose head is <= 16 wide over 128 or 256 inputs and whose backward takes per-tile head partials (head_is_fused).
static bool dpg_fused_ok(const PqlMlpDesc* c, const PqlMlpDesc* a, int64_t b) {
  if (desc_ok(c) || desc_ok(a) || b <= 0 || b > 131072) return false;
  const int La = a->n_layers, A = a->dims[La];
  if (!compact_chain_ok(c) || a->n_nets != 1 || La < 2 || !fused_with_head(c)) return false;
  return A <= 16 && c->dims[0] >= A && head_is_fused(a) && dx_slice_head_ok(A, (int)pqlk_ld(a->dims[La - 1])) && a->dims[La - 1] % 32 == 0;
}

extern "C" int32_t pqlk_dpg_fused_ok(const PqlMlpDesc* critic, const PqlMlpDesc* actor, int64_t b) {
  return critic && actor && dpg_fused_ok(critic, actor, b) ? 1 : 0;
}

// number of loss partials pqlk_dpg_backward_fused leaves (sums of min(Q1, Q2); fold with scale -1 / b)
extern "C" int32_t pqlk_dpg_fused_loss_parts(void) { return DPG_LOSS_PARTS; }

// number of head partials (one per compact 32-row tile) pqlk_mlp_backward_tail has to be told about
extern "C" int32_t pqlk_dpg_fused_head_parts(int64_t b) { return b > 0 ? (int32_t)(compact_ws(0, b).rows_cap / 32) : 0; }

// The twin scalar-head critic's forward that ALSO leaves the head outputs compact: qc (2, B) = Q1 | Q2 (mlp.py:186-203).
extern "C" int pqlk_mlp_forward_qc(const PqlMlpDesc* d, const float* params, const float* packed, int32_t stash_all, const float* x,
                                   int64_t ldx, const float* x2, int64_t ldx2, int32_t x2_col0, int64_t b, float* acts, float* qc,
                                   pqlk_stream_t stream) {
  int rc = desc_ok(d);
  if (rc) return rc;
  PQLK_REQUIRE(params && packed && x && acts && qc, PQLK_E_NULL);
  PQLK_REQUIRE(b > 0 && b < (1LL << 30), PQLK_E_SHAPE);
  PQLK_REQUIRE(pqlk_aligned16(params) && pqlk_aligned16(packed) && pqlk_aligned16(x) && pqlk_aligned16(acts) && pqlk_aligned16(qc), PQLK_E_ALIGN);
  if (x2) {   // input = [ x[:, :x2_col0] | x2[:, :dims[0] - x2_col0] ]: the two halves of torch.cat((obs, action), dim=1) where they lie
    PQLK_REQUIRE(x2_col0 > 0 && x2_col0 % 4 == 0 && x2_col0 < d->dims[0], PQLK_E_RANGE);
    PQLK_REQUIRE(ldx % 4 == 0 && ldx >= x2_col0 && ldx2 % 4 == 0 && ldx2 >= d->dims[0] - x2_col0 && pqlk_aligned16(x2), PQLK_E_ALIGN);
  } else {
    PQLK_REQUIRE(ldx % 32 == 0 && ldx >= pqlk_ld(d->dims[0]), PQLK_E_ALIGN);
  }
  PQLK_REQUIRE(d->dims[d->n_layers] == 1 && fused_with_head(d), PQLK_E_UNSUPPORTED);
  FusedHead head = {};
  head.n = 1; head.epi = PQLK_ACT_NONE; head.qc = qc;
  head.x2 = x2; head.ldx2 = ldx2; head.x2_col0 = x2_col0;
  return launch_fused_hidden(mlp_geom(d, b), params, packed, x, ldx, acts, stash_all ? 1 : 0, pqlk_s(stream), &head);
}

// DPG loss + the dX chain through the frozen critic + the actor's head backward (pql_p_learner.py:55-58).
//   in : critic params / activation stash (pqlk_mlp_forward_qc, stash_all) / qc; x = the critic's input [obs | pi(obs)];
//        a_out = tanh output of the actor (B, ld_tanh); actor params / activation stash
//   out: loss_part[pqlk_dpg_fused_loss_parts()]; dz_a (B, ld_dz) columns [0, A) = dL/d(pre-tanh action) (pad columns untouched);
//        actor_ws (the workspace of the actor's pqlk_mlp_backward_tail): dL/dZ of the actor's last hidden layer + one head partial
//        per compact 32-row tile.  Follow with pqlk_mlp_backward_tail(actor, ..., pqlk_dpg_fused_head_parts(b), critic_ws).
// critic_ws: pqlk_dpg_backward_ws_floats(critic, b) floats; its perm / mn block stays valid for the tail call.
extern "C" int pqlk_dpg_backward_fused(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b, const float* acts,
                                       const float* qc, float* dz_a, int64_t ld_dz, int32_t dx_col0, const float* a_out, int64_t ld_tanh,
                                       float* loss_part, float* ws, int64_t ws_floats, const PqlMlpDesc* ad, const float* a_params,
                                       const float* a_acts, float* a_ws, int64_t a_ws_floats, int32_t a_splits, pqlk_stream_t stream) {
  PQLK_REQUIRE(d && ad && params && acts && qc && dz_a && a_out && loss_part && ws && a_params && a_acts && a_ws, PQLK_E_NULL);   // (x: not read)
  PQLK_REQUIRE(dpg_fused_ok(d, ad, b), PQLK_E_UNSUPPORTED);
  PQLK_REQUIRE(ws_floats >= pqlk_dpg_backward_ws_floats(d, b), PQLK_E_WORKSPACE);
  const MlpGeom g = mlp_geom(d, b), ga = mlp_geom(ad, b);
  const BwdWs aw = bwd_ws(ga, a_splits);   // the actor's workspace is the one its pqlk_mlp_backward_tail call reads
  PQLK_REQUIRE(a_splits >= 1 && a_splits <= 64 && a_ws_floats >= aw.total, PQLK_E_WORKSPACE);
  const int L = g.L, La = ga.L, A = ad->dims[La];
  PQLK_REQUIRE(ld_dz % 32 == 0 && ld_dz >= A && ld_tanh >= A && dx_col0 >= 0 && dx_col0 + A <= d->dims[0], PQLK_E_RANGE);
  (void)x; (void)ldx;
  PQLK_REQUIRE(pqlk_aligned16(qc) && pqlk_aligned16(ws) && pqlk_aligned16(a_ws) && pqlk_aligned16(acts) && pqlk_aligned16(a_acts), PQLK_E_ALIGN);
  const CompactRun r = compact_run(g, params, acts, ws);
  hipStream_t st = pqlk_s(stream);
  // 1. loss partials + partition + compact head
  {
    DpgHeadP h = {};
    h.qc = qc; h.B = b;
    h.H = acts + g.a_off[L - 2]; h.sH = b * g.ld[L - 1]; h.ldh = (int)g.ld[L - 1];
    h.W = params + g.w_off[L - 1]; h.sW = g.net_stride;
    h.C = r.dz[0]; h.K = (int)g.ld[L - 1];
    h.perm = r.perm; h.tie0 = r.tie0; h.perm_len = r.rows_cap; h.mn = r.mn;
    h.loss_part = loss_part; h.gb = -1.0f / (float)b;
    int64_t blocks = r.rows_cap / 16;
    if (blocks > 256) blocks = 256;
    if (blocks < 1) blocks = 1;
    h.rows_cap_blk = (int)((r.rows_cap + blocks - 1) / blocks);
    const size_t sh = ((size_t)2 * h.rows_cap_blk + (size_t)2 * h.K) * sizeof(float);
    hipLaunchKernelGGL(k_dpg_minnet_head, dim3((unsigned)blocks), dim3(1024), sh, st, h);
    PQLK_LAUNCH_CHECK();
  }
  // 2. hidden layers over compact rows
  if (int rc = compact_dx_chain(r, st)) return rc;
  // 3. action slice through tanh' + the actor head's backward
  const GemmP p = compact_slice(r, dz_a, ld_dz, dx_col0, A, a_out, ld_tanh);
  PQLK_REQUIRE(dx_slice_ok(p), PQLK_E_UNSUPPORTED);
  SliceHeadX hx = {};
  hx.tie0 = r.tie0;
  hx.Hh = a_acts + ga.a_off[La - 2]; hx.ldh = (int)ga.ld[La - 1];
  hx.Wh = a_params + ga.w_off[La - 1]; hx.N = A; hx.Kh = (int)ga.ld[La - 1];
  hx.dXh = a_ws + aw.dz[0]; hx.part = a_ws + aw.head_part; hx.part_floats = ga.head_floats;
  return launch_dx_slice(p, st, &hx);
}

// The rest of a backward whose LAST layer has already been done elsewhere (pqlk_dpg_backward_fused: dL/dZ of the last hidden layer in
// the workspace's first dZ buffer, `head_parts` per-tile partials of the head's dW / db behind the slabs, of which only the first
// (head_parts_dev[3] + 31) / 32 exist when head_parts_dev is given): dW / dX of the layers below, slab reduction incl. the head
// fold, and -- with sumsq_part / step_dev -- the squared-norm partials of pqlk_mlp_backward_norm.
extern "C" int pqlk_mlp_backward_tail(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b, const float* acts,
                                      float* grads, int32_t splits, float* ws, int64_t ws_floats, float* sumsq_part, int32_t* step_dev,
                                      int32_t head_parts, const int32_t* head_parts_dev, pqlk_stream_t stream) {
  int rc = desc_ok(d);
  if (rc) return rc;
  PQLK_REQUIRE(grads, PQLK_E_NULL);
  PQLK_REQUIRE((sumsq_part == nullptr) == (step_dev == nullptr), PQLK_E_NULL);
  PQLK_REQUIRE(head_parts > 0 && head_is_fused(d), PQLK_E_UNSUPPORTED);
  const MlpGeom g = mlp_geom(d, b);
  PQLK_REQUIRE((int64_t)head_parts * g.n_nets * g.head_floats <= bwd_ws(g, splits).head_part_floats, PQLK_E_WORKSPACE);
  BwdCall c = bwd_call(d, params, x, ldx, b, acts, grads, splits, ws, ws_floats, stream);
  c.sq_part = sumsq_part; c.step_dev = step_dev; c.head_done = head_parts; c.head_parts_dev = head_parts_dev;
  return mlp_backward_impl(c);
}

// float offset of mn = {c0, c1, first row of net 1, compact rows in use} inside pqlk_dpg_backward_fused's critic workspace: the
// `head_parts_dev` of the pqlk_mlp_backward_tail call that follows it
extern "C" int64_t pqlk_dpg_fused_mn_offset(const PqlMlpDesc* critic, int64_t b) {
  if (desc_ok(critic) || b <= 0) return -1;
  return compact_ws(mlp_geom(critic, b).max_hidden_ld, b).mn;
}

extern "C" int pqlk_mlp_backward(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b,
                                 const float* acts, const float* dy, float* grads, int32_t splits, float* dx,
                                 int64_t ld_dx, int32_t dx_col0, int32_t dx_cols, const float* dx_tanh_of,
                                 int64_t ld_tanh, float* ws, int64_t ws_floats, pqlk_stream_t stream) {
  BwdCall c = bwd_call(d, params, x, ldx, b, acts, grads, splits, ws, ws_floats, stream);
  c.dy = dy; c.dx = dx; c.ld_dx = ld_dx; c.dx_col0 = dx_col0; c.dx_cols = dx_cols; c.dx_tanh_of = dx_tanh_of; c.ld_tanh = ld_tanh;
  return mlp_backward_impl(c);
}

// The V-learner's scalar-head step: TD target + twin MSE (pql_v_learner.py:104-108) are formed INSIDE the head's backward pass
// (k_skinny_bwd<1, CH, true>), which reads Q and the target Q anyway: pqlk_td_mse_loss's launch disappears and dL/dQ never
// goes through memory.  loss_part receives pqlk_td_head_loss_parts(d, b) partial sums of (Q - y)^2 (both nets), to be folded
// with scale 1 / b.  sumsq_part / step_dev as in pqlk_mlp_backward_norm (both NULL: plain backward).  PQLK_E_UNSUPPORTED
// unless d is a twin net with one output whose head takes the one-pass skinny kernel.
extern "C" int pqlk_mlp_backward_td(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b,
                                    const float* acts, const float* acts_target, const float* rew, const float* done, float gamma_n,
                                    float* loss_part, float* grads, int32_t splits, float* ws, int64_t ws_floats,
                                    float* sumsq_part, int32_t* step_dev, pqlk_stream_t stream) {
  int rc = desc_ok(d);
  if (rc) return rc;
  PQLK_REQUIRE(acts_target && rew && done && loss_part && grads, PQLK_E_NULL);
  PQLK_REQUIRE((sumsq_part == nullptr) == (step_dev == nullptr), PQLK_E_NULL);
  PQLK_REQUIRE(b > 0, PQLK_E_SHAPE);
  const TdHead td = {acts_target + mlp_geom(d, b).a_off[d->n_layers - 1], rew, done, gamma_n, loss_part};
  BwdCall c = bwd_call(d, params, x, ldx, b, acts, grads, splits, ws, ws_floats, stream);
  c.sq_part = sumsq_part; c.step_dev = step_dev; c.td = &td;
  return mlp_backward_impl(c);
}

// Data-parallel buckets: layers layer_hi >= l >= layer_lo of the same backward (dW_l, dX_l) followed by the slab reduction of
// exactly those layers into `grads`, so that their all-reduce can be issued while the launches of the layers below still run.
// Calls walk the layers downwards (layer_hi of the first = n_layers - 1, layer_lo of the last = 0) over the SAME workspace;
// the union of the calls leaves in `grads` the bits one pqlk_mlp_backward / pqlk_mlp_backward_td call leaves (every arena
// element is the same fixed-order sum).  dy is read by the call that holds the last layer only; with acts_target / rew / done /
// loss_part given (all four, else all NULL and dy non-NULL) that call forms the TD error in the head pass like
// pqlk_mlp_backward_td.
extern "C" int pqlk_mlp_backward_layers(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b,
                                        const float* acts, const float* dy, const float* acts_target, const float* rew,
                                        const float* done, float gamma_n, float* loss_part, float* grads, int32_t splits, float* ws,
                                        int64_t ws_floats, int32_t layer_hi, int32_t layer_lo, pqlk_stream_t stream) {
  int rc = desc_ok(d);
  if (rc) return rc;
  PQLK_REQUIRE(grads, PQLK_E_NULL);
  PQLK_REQUIRE(layer_lo >= 0 && layer_lo <= layer_hi && layer_hi < d->n_layers, PQLK_E_RANGE);
  const bool any_td = acts_target || rew || done || loss_part, all_td = acts_target && rew && done && loss_part;
  PQLK_REQUIRE(any_td == all_td, PQLK_E_NULL);
  BwdCall c = bwd_call(d, params, x, ldx, b, acts, grads, splits, ws, ws_floats, stream);
  c.ranged = true; c.l_hi = layer_hi; c.l_lo = layer_lo;
  TdHead td = {};
  if (all_td && layer_hi == d->n_layers - 1) {
    PQLK_REQUIRE(b > 0, PQLK_E_SHAPE);
    td = {acts_target + mlp_geom(d, b).a_off[d->n_layers - 1], rew, done, gamma_n, loss_part};
    c.td = &td;
  } else {
    PQLK_REQUIRE(all_td || dy || layer_hi < d->n_layers - 1, PQLK_E_NULL);
    c.dy = dy;
  }
  return mlp_backward_impl(c);
}

// ---- the same step with the head's backward inside the critic's fused FORWARD launch (fused.h, fused_head's TD part): the
// k_skinny_bwd launch and its second read of the last hidden layer's activations disappear.
// Row tiles of the fused forward when this layout can take it, else 0: twin net, one output, fused hidden stack + fused head, the
// head's partials in k_skinny_bwd's format, 256 free LDS columns beside the last hidden layer for the head's partial tiles.
static int64_t td_forward_tiles(const PqlMlpDesc* d, int64_t b) {
  int buf_ld = 0;
  const int L = d->n_layers;
  if (b <= 0 || !fused_with_head(d, &buf_ld)) return 0;
  if (d->n_nets != 2 || d->dims[L] != 1 || !head_is_fused(d)) return 0;
  if (buf_ld - d->dims[L - 1] < 256 || (int64_t)(L - 1) * (buf_ld - 4) < 128) return 0;
  const int R = fused_rows(d, buf_ld, b);
  return (b + 32 * R - 1) / (32 * R);
}

extern "C" int32_t pqlk_td_forward_loss_parts(const PqlMlpDesc* d, int64_t b) {
  if (desc_ok(d)) return 0;
  return (int32_t)(td_forward_tiles(d, b) * d->n_nets);
}

extern "C" int pqlk_mlp_forward_td(const PqlMlpDesc* d, const float* params, const float* packed, const float* x, int64_t ldx,
                                   int64_t b, float* acts, const float* acts_target, const float* rew, const float* done,
                                   float gamma_n, float* loss_part, float* bwd_ws_p, int64_t bwd_ws_floats, int32_t splits,
                                   pqlk_stream_t stream) {
  int rc = desc_ok(d);
  if (rc) return rc;
  PQLK_REQUIRE(params && packed && x && acts && acts_target && rew && done && loss_part && bwd_ws_p, PQLK_E_NULL);
  PQLK_REQUIRE(b > 0 && b < (1LL << 30), PQLK_E_SHAPE);
  PQLK_REQUIRE(ldx % 32 == 0 && ldx >= pqlk_ld(d->dims[0]), PQLK_E_ALIGN);
  PQLK_REQUIRE(pqlk_aligned16(params) && pqlk_aligned16(packed) && pqlk_aligned16(x) && pqlk_aligned16(acts) && pqlk_aligned16(bwd_ws_p),
               PQLK_E_ALIGN);
  PQLK_REQUIRE(td_forward_tiles(d, b) > 0, PQLK_E_UNSUPPORTED);
  PQLK_REQUIRE(splits >= 1 && splits <= 64, PQLK_E_SHAPE);
  const MlpGeom g = mlp_geom(d, b);
  const BwdWs w = bwd_ws(g, splits);   // of the pqlk_mlp_backward_td_tail call that follows
  PQLK_REQUIRE(bwd_ws_floats >= w.total, PQLK_E_WORKSPACE);
  FusedHead head = {};
  head.n = 1; head.epi = PQLK_ACT_NONE;
  head.td_qt = acts_target + g.a_off[g.L - 1]; head.td_rew = rew; head.td_done = done; head.td_gamma_n = gamma_n;
  head.td_dz = bwd_ws_p + w.dz[0]; head.td_head_part = bwd_ws_p + w.head_part; head.td_loss_part = loss_part;
  return launch_fused_hidden(g, params, packed, x, ldx, acts, 1, pqlk_s(stream), &head);
}

extern "C" int pqlk_mlp_backward_td_tail(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b,
                                         const float* acts, float* grads, int32_t splits, float* ws, int64_t ws_floats,
                                         float* sumsq_part, int32_t* step_dev, pqlk_stream_t stream) {
  int rc = desc_ok(d);
  if (rc) return rc;
  PQLK_REQUIRE(grads, PQLK_E_NULL);
  PQLK_REQUIRE((sumsq_part == nullptr) == (step_dev == nullptr), PQLK_E_NULL);
  const int64_t tiles = td_forward_tiles(d, b);
  PQLK_REQUIRE(tiles > 0, PQLK_E_UNSUPPORTED);
  BwdCall c = bwd_call(d, params, x, ldx, b, acts, grads, splits, ws, ws_floats, stream);
  c.sq_part = sumsq_part; c.step_dev = step_dev; c.head_done = (int)tiles;
  return mlp_backward_impl(c);
}

extern "C" int32_t pqlk_td_head_loss_parts(const PqlMlpDesc* d, int64_t b) {
  if (desc_ok(d) || b <= 0 || d->n_nets != 2 || d->dims[d->n_layers] != 1 || !head_is_fused(d)) return 0;   // 0: unsupported
  return (int32_t)(skinny_bwd_blocks(b, d->n_nets) * d->n_nets);
}

// Same, and the gradient's squared-norm partials + the optimiser's step increment come out of the final reduction pass:
// follow with pqlk_adamw_polyak_fused(prenorm = pqlk_mlp_norm_parts(d)).  Not for data parallel (the all-reduce sits
// between the two).
extern "C" int pqlk_mlp_backward_norm(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b,
                                      const float* acts, const float* dy, float* grads, int32_t splits, float* dx,
                                      int64_t ld_dx, int32_t dx_col0, int32_t dx_cols, const float* dx_tanh_of,
                                      int64_t ld_tanh, float* ws, int64_t ws_floats, float* sumsq_part, int32_t* step_dev,
                                      pqlk_stream_t stream) {
  PQLK_REQUIRE(grads && sumsq_part && step_dev, PQLK_E_NULL);
  BwdCall c = bwd_call(d, params, x, ldx, b, acts, grads, splits, ws, ws_floats, stream);
  c.dy = dy; c.dx = dx; c.ld_dx = ld_dx; c.dx_col0 = dx_col0; c.dx_cols = dx_cols; c.dx_tanh_of = dx_tanh_of; c.ld_tanh = ld_tanh;
  c.sq_part = sumsq_part; c.step_dev = step_dev;
  return mlp_backward_impl(c);
}
