// Replay ring kernels: insert, plain gather, fused gather+normalise+concat.
// Reference behaviour: pql/replay/simple_replay.py:40-104, pql/algo/pql_p_learner.py:49-50,66-85,
// pql/utils/common.py:139-145.  HBM-bound byte movement: one wave per record, 16-B lane accesses,
// records 128-B aligned so a random sample touches the minimum number of HBM lines.
#include "pqlk_common.h"

extern "C" int64_t pqlk_ld(int64_t cols) { return pqlk_round_up(cols < 1 ? 1 : cols, 32); }

extern "C" int64_t pqlk_replay_rec_ld(int32_t obs_dim, int32_t act_dim) {
  if (obs_dim <= 0) return 0;
  return rec_layout(obs_dim, act_dim).ld;
}

extern "C" int64_t pqlk_replay_rec_ld_ex(int32_t obs_dim, int32_t act_dim, int32_t obs_dtype) {
  if (obs_dim <= 0) return 0;
  if (obs_dtype == PQLK_OBS_F32) return rec_layout(obs_dim, act_dim).ld;
  if (obs_dtype == PQLK_OBS_F16) return rec_layout_h(obs_dim, act_dim).ld;
  return 0;
}

// ================================================================================================
// Record formats: fp32 observations (PQLK_OBS_F32, RecLayout) and half-precision ones (PQLK_OBS_F16, RecLayoutH; both layouts in
// pqlk_common.h).  fp16 records are handled as raw 32-bit words: a word that packs two halves is only ever copied or taken apart with integer
// shifts, never treated as a float.  fp32 -> fp16 is the hardware's round-to-nearest-even conversion (v_cvt_f16_f32: overflow
// to +-inf, fp16 subnormals produced, NaN stays NaN), fp16 -> fp32 is exact, so a ring fed x holds q(x) = (float)(half)x.
// Insert, plain gather, the generic fused gather and the whole host side are written ONCE for both formats, over the traits
// RecF32 / RecF16 below.  Only the tuned gathers have kernels of their own per format -- k_replay_gather_fast / _obs (fp32) and
// their _f16 (16-B chunks) and _h8 (8-B chunks) twins: they are latency-bound chains on the one in-order vector-memory counter,
// and a dtype flag or template argument cost k_replay_gather_fast 20 % (round 4: 2 -> 14 full drains of that counter).  An
// optimisation tuned for one workload keeps an implementation of its own; nothing is shared between those six bodies.
__device__ __forceinline__ uint32_t pack_h2(float a, float b) {
  const _Float16 ha = (_Float16)a, hb = (_Float16)b;
  return (uint32_t)__builtin_bit_cast(unsigned short, ha) | ((uint32_t)__builtin_bit_cast(unsigned short, hb) << 16);
}
__device__ __forceinline__ float h_lo(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)); }
__device__ __forceinline__ float h_hi(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
// the 8 columns of one 16-B observation chunk
__device__ __forceinline__ void widen8(const uint4& w, float e[8]) {
  e[0] = h_lo(w.x); e[1] = h_hi(w.x); e[2] = h_lo(w.y); e[3] = h_hi(w.y);
  e[4] = h_lo(w.z); e[5] = h_hi(w.z); e[6] = h_lo(w.w); e[7] = h_hi(w.w);
}

// What the two record formats differ in, for the code that is written once: the layout, the type of a record word, whether
// observations are stored as halves (which tuned kernels the host picks), how many observation columns a 16-B chunk of an
// observation field holds, how such a chunk becomes columns (widen) and how the COLS / 4 columns of one word become that word
// (pack).  (The action, reward and done words are raw fp32 in both formats.)
struct RecF32 {
  typedef RecLayout Layout;
  typedef float word;
  static constexpr bool HALF = false;
  static constexpr int COLS = 4;
  static Layout layout(int O, int A) { return rec_layout(O, A); }
  __device__ __forceinline__ static void widen(const uint4& w, float e[4]) {
    e[0] = __uint_as_float(w.x); e[1] = __uint_as_float(w.y); e[2] = __uint_as_float(w.z); e[3] = __uint_as_float(w.w);
  }
  __device__ __forceinline__ static uint32_t pack(const float e[1]) { return __float_as_uint(e[0]); }
};
struct RecF16 {
  typedef RecLayoutH Layout;
  typedef uint32_t word;
  static constexpr bool HALF = true;
  static constexpr int COLS = 8;
  static Layout layout(int O, int A) { return rec_layout_h(O, A); }
  __device__ __forceinline__ static void widen(const uint4& w, float e[8]) { widen8(w, e); }
  __device__ __forceinline__ static uint32_t pack(const float e[2]) { return pack_h2(e[0], e[1]); }
};

// PQLK_OK, or the error code every replay entry point returns for a malformed ring: null, shape, dtype, rec_ld, in that order
// (pointers: the call's other pointers that must never be null are there; rows: its m or b)
static int ring_ok(const PqlReplayDesc* ring, bool pointers, int64_t rows) {
  PQLK_REQUIRE(ring && ring->records && pointers, PQLK_E_NULL);
  PQLK_REQUIRE(ring->obs_dim > 0 && ring->capacity > 0 && rows >= 0, PQLK_E_SHAPE);
  PQLK_REQUIRE(ring->obs_dtype == PQLK_OBS_F32 || ring->obs_dtype == PQLK_OBS_F16, PQLK_E_SHAPE);
  PQLK_REQUIRE(ring->rec_ld == pqlk_replay_rec_ld_ex(ring->obs_dim, ring->act_dim, ring->obs_dtype), PQLK_E_SHAPE);
  return PQLK_OK;
}

// ------------------------------------------------------------------------------------------------
// insert: row r of the five source arrays -> record (dst_start + r).  One wave per record, a lane per word over the WHOLE
// stride (pad columns, pad halves and pad words written as zero): the source rows are read lane-contiguously.  The branches, and
// the done word as a select of two floats, are those the fp32 insert always had: RecF32 (the default format's hand-off) then
// compiles to the instructions it always had.
template <class F>
__global__ __launch_bounds__(256) void k_replay_insert(typename F::word* __restrict__ records, typename F::Layout L,
                                                       int64_t dst_start, int64_t m, const float* __restrict__ obs,
                                                       int64_t ld_obs, const float* __restrict__ act, int64_t ld_act,
                                                       const float* __restrict__ rew, int64_t ld_rew,
                                                       const float* __restrict__ nobs, int64_t ld_nobs,
                                                       const float* __restrict__ done, int64_t ld_done) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  constexpr int W = F::COLS / 4;      // observation columns per word
  const int ow = (L.O + W - 1) / W;   // words of an observation field that hold a column
  // word k of an observation field, from the source row s
  auto field = [&](const float* __restrict__ s, int k) {
    float e[W];
#pragma unroll
    for (int j = 0; j < W; ++j) e[j] = k * W + j < L.O ? s[k * W + j] : 0.f;
    return F::pack(e);
  };
  for (int64_t r = wave; r < m; r += nwaves) {
    uint32_t* rec = reinterpret_cast<uint32_t*>(records + (dst_start + r) * L.ld);
    for (int c = lane; c < L.ld; c += 64) {
      uint32_t w = 0u;
      if (c < ow) {
        w = field(obs + r * ld_obs, c);
      } else if (L.A >= 0) {
        if (c >= L.off_nobs && c < L.off_nobs + ow) w = field(nobs + r * ld_nobs, c - L.off_nobs);
        else if (c >= L.off_act && c < L.off_act + L.A) w = __float_as_uint(act[r * ld_act + (c - L.off_act)]);
        else if (c == L.off_rd) w = __float_as_uint(rew[r * ld_rew]);
        else if (c == L.off_rd + 1) w = __float_as_uint(done[r * ld_done] != 0.f ? 1.f : 0.f);  // .bool() then .float()
      }
      rec[c] = w;
    }
  }
}

template <class F>
static int replay_insert(const PqlReplayDesc* ring, int64_t dst_start, int64_t m, const float* obs, int64_t ld_obs,
                         const float* act, int64_t ld_act, const float* rew, int64_t ld_rew, const float* next_obs,
                         int64_t ld_nobs, const float* done, int64_t ld_done, pqlk_stream_t stream) {
  int64_t blocks = (m + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_replay_insert<F>, dim3((unsigned)blocks), dim3(256), 0, pqlk_s(stream),
                     reinterpret_cast<typename F::word*>(ring->records), F::layout(ring->obs_dim, ring->act_dim), dst_start, m,
                     obs, ld_obs, act, ld_act, rew, ld_rew, next_obs, ld_nobs, done, ld_done);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

extern "C" int pqlk_replay_insert(const PqlReplayDesc* ring, int64_t dst_start, int64_t m, const float* obs,
                                  int64_t ld_obs, const float* act, int64_t ld_act, const float* rew, int64_t ld_rew,
                                  const float* next_obs, int64_t ld_nobs, const float* done, int64_t ld_done,
                                  pqlk_stream_t stream) {
  if (const int rc = ring_ok(ring, obs != nullptr, m)) return rc;
  PQLK_REQUIRE(dst_start >= 0 && dst_start + m <= ring->capacity, PQLK_E_RANGE);
  if (ring->act_dim >= 0) PQLK_REQUIRE(act && rew && next_obs && done, PQLK_E_NULL);
  PQLK_REQUIRE(ld_obs >= ring->obs_dim, PQLK_E_SHAPE);
  if (m == 0) return PQLK_OK;
  // (RecF32 first: the instantiations are laid out in this order, and k_replay_insert<RecF32> measured 0.1 us (3 %) slower per
  //  hand-off as the code object's second kernel than as its first, where the fp32 insert always stood)
  return ring->obs_dtype == PQLK_OBS_F32
             ? replay_insert<RecF32>(ring, dst_start, m, obs, ld_obs, act, ld_act, rew, ld_rew, next_obs, ld_nobs, done, ld_done, stream)
             : replay_insert<RecF16>(ring, dst_start, m, obs, ld_obs, act, ld_act, rew, ld_rew, next_obs, ld_nobs, done, ld_done, stream);
}

// ------------------------------------------------------------------------------------------------
// plain gather: five contiguous fp32 outputs, byte-exact copies of what the ring holds (fp16 observations widened exactly;
// done already 0.0/1.0).
template <class F>
__global__ __launch_bounds__(256) void k_replay_gather(const typename F::word* __restrict__ records, typename F::Layout L,
                                                       int64_t capacity, const int64_t* __restrict__ idx, int64_t b,
                                                       float* __restrict__ o_obs, float* __restrict__ o_act,
                                                       float* __restrict__ o_rew, float* __restrict__ o_nobs,
                                                       float* __restrict__ o_done) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int nchunk = L.used >> 2;
  for (int64_t r = wave; r < b; r += nwaves) {
    int64_t src = idx[r];
    if (src < 0 || src >= capacity) src = 0;  // never fault on a bad index; host validates in debug paths
    const uint4* rec4 = reinterpret_cast<const uint4*>(records + src * L.ld);
    for (int q = lane; q < nchunk; q += 64) {
      const uint4 w = rec4[q];
      const int c = q << 2;
      if (c < L.off_act) {   // obs / next_obs (an obs-only record ends at off_act)
        const bool nx = c >= L.off_nobs;
        float* o = (nx ? o_nobs : o_obs) + r * L.O;
        const int col = (nx ? c - L.off_nobs : c) * (F::COLS / 4);
        float e[F::COLS];
        F::widen(w, e);
#pragma unroll
        for (int j = 0; j < F::COLS; ++j)
          if (col + j < L.O) o[col + j] = e[j];
      } else if (c < L.off_rd) {
        const int cc = c - L.off_act;
        const uint32_t e[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (cc + j < L.A) o_act[r * L.A + cc + j] = __uint_as_float(e[j]);
      } else {
        o_rew[r] = __uint_as_float(w.x);
        o_done[r] = __uint_as_float(w.y);
      }
    }
  }
}

template <class F>
static int replay_gather(const PqlReplayDesc* ring, const int64_t* idx, int64_t b, float* obs, float* act, float* rew,
                         float* next_obs, float* done, pqlk_stream_t stream) {
  int64_t blocks = (b + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(k_replay_gather<F>, dim3((unsigned)blocks), dim3(256), 0, pqlk_s(stream),
                     reinterpret_cast<const typename F::word*>(ring->records), F::layout(ring->obs_dim, ring->act_dim),
                     ring->capacity, idx, b, obs, act, rew, next_obs, done);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

extern "C" int pqlk_replay_gather(const PqlReplayDesc* ring, const int64_t* idx, int64_t b, float* obs, float* act,
                                  float* rew, float* next_obs, float* done, pqlk_stream_t stream) {
  if (const int rc = ring_ok(ring, idx && obs, b)) return rc;
  if (ring->act_dim >= 0) PQLK_REQUIRE(act && rew && next_obs && done, PQLK_E_NULL);
  if (b == 0) return PQLK_OK;
  return ring->obs_dtype == PQLK_OBS_F16 ? replay_gather<RecF16>(ring, idx, b, obs, act, rew, next_obs, done, stream)
                                         : replay_gather<RecF32>(ring, idx, b, obs, act, rew, next_obs, done, stream);
}

// ------------------------------------------------------------------------------------------------
// fused gather: sample + normalise (+-5 clamp) + concat into the padded GEMM input tiles.
// (A reciprocal per column + two fma corrections (Markstein) also gives the correctly rounded quotient and was tried against the
// fp32 division sequence in round 2: with the range / exceptional-significand guards it needs it is ~15 instructions against the
// hardware sequence's ~11, and measured 0.9 us SLOWER per 32768-row launch.  What replaced that sequence is norm_div.)
// (x - mean) / sd with the division as ONE double-precision product rounded once to fp32 -- bit for bit the IEEE quotient the
// reference's `(x - mean) / sqrt(var + eps)` rounds to (common.py:139-145), in 3 instructions per element instead of the 12 of the
// fp32 division sequence (v_div_scale x2, v_rcp, 6 FMAs / multiplies, v_div_fmas, v_div_fixup): the gather kernels spent ~100 VALU
// instructions per record on four divisions.  rd = 1 / (double)sd is formed once per lane (correctly rounded: relative error
// <= 2^-53), the product adds <= 2^-53, so the double result is within 2^-51.9 (relative) of a / sd.  The exact quotient of two
// fp32 numbers is never that close to a boundary between two fp32 results: a boundary m has <= 25 significant bits, a - m sd != 0
// is a multiple of ulp(m) ulp(sd), which puts |a / sd - m| / |a / sd| above 2^-49 (normal and denormal results alike; the overflow
// threshold is one more such boundary).  Signed zeros, infinities and NaN come out as IEEE division gives them (a * (1 / inf) =
// a * 0).  tests: the gather tests are bit-exact against the oracle's fp32 division; test_gather_division_is_the_ieee_quotient.
__device__ __forceinline__ float norm_div(float a, double rd) { return (float)((double)a * rd); }

#define GATHER_MAX_OBS 1024

// store up to 4 consecutive columns [col, col+4) of a row, clipped to `limit` columns; one 16-B store when the
// destination is 16-B aligned and unclipped, scalar stores otherwise
__device__ __forceinline__ void store4(float* __restrict__ row, int col, int limit, const float e[4], bool aligned) {
  if (aligned && col + 4 <= limit) {
    *reinterpret_cast<float4*>(row + col) = make_float4(e[0], e[1], e[2], e[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (col + j < limit) row[col + j] = e[j];
  }
}

// the F::COLS columns [col, col + COLS) of an observation chunk: one store4 per 4 columns (16-B aligned: col is a multiple of 4)
template <class F>
__device__ __forceinline__ void store_obs(float* __restrict__ row, int col, int limit, const float e[F::COLS]) {
#pragma unroll
  for (int k = 0; k < F::COLS; k += 4) store4(row, col + k, limit, e + k, true);
}

// Generic fused gather (records of more than one 16-B chunk per lane, tiles wider than the lean kernels' pad bound, unaligned
// tiles), for both formats.  R rows per wave per trip with all their record loads in flight at once (memory-level parallelism
// for the random HBM reads); CH = 16-B chunks per lane per record (1 covers records up to 1 KiB, e.g. cfg #2's 784 used bytes).
template <class F, bool HAS_NORM, int R, int CH>
__global__ __launch_bounds__(256) void k_replay_gather_fused(const typename F::word* __restrict__ records, typename F::Layout L,
                                                             int64_t capacity, const int64_t* __restrict__ idx, int64_t b,
                                                             const float* __restrict__ mean, const float* __restrict__ var,
                                                             float eps, int clamp5, float* __restrict__ x_sa, int64_t ld_sa,
                                                             float* __restrict__ xn_sa, float* __restrict__ xn_obs,
                                                             int64_t ld_o, float* __restrict__ o_rew,
                                                             float* __restrict__ o_done, int write_pads) {
  // per-column mean and 1 / sd, sd = sqrt(var + eps) (correctly rounded sqrtf), staged once per block; 1 / sd as a double
  // (norm_div: one double-precision product rounded once)
  __shared__ float s_mean[HAS_NORM ? GATHER_MAX_OBS : 1];
  __shared__ double s_rd[HAS_NORM ? GATHER_MAX_OBS : 1];
  if (HAS_NORM) {
    for (int c = threadIdx.x; c < L.O; c += 256) {
      s_mean[c] = mean[c];
      s_rd[c] = 1.0 / (double)sqrtf(var[c] + eps);
    }
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int nchunk = L.used >> 2;
  const int A = L.A < 0 ? 0 : L.A;
  const int sa_cols = L.O + A;
  const bool act_aligned = (L.O & 3) == 0;
  for (int64_t r0 = wave * R; r0 < b; r0 += nwaves * R) {
    uint4 v[R][CH];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t r = r0 + i;
      int64_t src = r < b ? idx[r] : 0;
      if (src < 0 || src >= capacity) src = 0;  // never fault on a bad index
      const uint4* rec4 = reinterpret_cast<const uint4*>(records + src * L.ld);
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int q = lane + 64 * c;
        v[i][c] = q < nchunk ? rec4[q] : make_uint4(0u, 0u, 0u, 0u);
      }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t r = r0 + i;
      if (r >= b) break;
      float* xs = x_sa ? x_sa + r * ld_sa : nullptr;
      float* xns = xn_sa ? xn_sa + r * ld_sa : nullptr;
      float* xno = xn_obs ? xn_obs + r * ld_o : nullptr;
#pragma unroll
      for (int cch = 0; cch < CH; ++cch) {
        const int q = lane + 64 * cch;
        if (q >= nchunk) continue;
        const uint4 w = v[i][cch];
        const int c = q << 2;
        if (c < L.off_act) {  // obs / next_obs (an obs-only record ends at off_act)
          const bool nx = c >= L.off_nobs;
          const int col = (nx ? c - L.off_nobs : c) * (F::COLS / 4);
          float e[F::COLS];
          F::widen(w, e);
          if (HAS_NORM) {
#pragma unroll
            for (int j = 0; j < F::COLS; ++j)
              if (col + j < L.O) {
                e[j] = norm_div(e[j] - s_mean[col + j], s_rd[col + j]);
                if (clamp5) e[j] = fminf(fmaxf(e[j], -5.f), 5.f);
              }
          }
          if (!nx) {
            if (xs) store_obs<F>(xs, col, L.O, e);
            if (L.A < 0 && xno) store_obs<F>(xno, col, L.O, e);  // obs-only ring: the sample IS the learner's obs batch
          } else {
            if (xns) store_obs<F>(xns, col, L.O, e);
            if (xno) store_obs<F>(xno, col, L.O, e);
          }
        } else if (c < L.off_rd) {  // action -> columns O.. of the critic input
          const int cc = c - L.off_act;
          const float e[4] = {__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w)};
          if (xs) store4(xs + L.O, cc, L.A, e, act_aligned);
        } else {
          if (o_rew) o_rew[r] = __uint_as_float(w.x);
          if (o_done) o_done[r] = __uint_as_float(w.y);
        }
      }
      if (!write_pads) continue;
      // zero the pad columns so the GEMM K-loop can run over the padded width unchecked
      for (int c = sa_cols + lane; c < ld_sa; c += 64) {
        if (xs) xs[c] = 0.f;
        if (xns) xns[c] = 0.f;
      }
      if (xno)
        for (int c = L.O + lane; c < ld_o; c += 64) xno[c] = 0.f;
    }
  }
}

// Fast path for transition rings whose record fits one 16-B chunk per lane (<= 1 KiB used, e.g. cfg #2 and #5): the field
// decode, destination and normalisation constants of a lane depend only on its chunk index, so they are computed ONCE
// per kernel and the per-row work is load -> (sub, IEEE div, clamp) x4 -> one or two 16-B stores.  The generic kernel
// above re-decodes the field per row and is instruction-issue bound (~450 instructions per row).
// (launch-shape overrides for tools/bench_gather.py arrive in the call's flag word: no state between calls)

template <bool HAS_NORM, int R>
__global__ __launch_bounds__(256) void k_replay_gather_fast(const float* __restrict__ records, RecLayout L, int64_t capacity,
                                                            const int64_t* __restrict__ idx, int64_t b,
                                                            const float* __restrict__ mean, const float* __restrict__ var,
                                                            float eps, int clamp5, float* __restrict__ x_sa, int64_t ld_sa,
                                                            float* __restrict__ xn_sa, float* __restrict__ xn_obs, int64_t ld_o,
                                                            float* __restrict__ o_rew, float* __restrict__ o_done, int write_pads,
                                                            int nt_loads, int halves) {
  typedef float f4n __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63;
  // halves == 2: records of 1-2 KiB (cfg #4: 1792 B) -- the odd waves of a block take the second KiB of the rows the even waves
  // take the first of, so a lane still owns ONE 16-B chunk and its plan
  const int half = halves == 2 ? (threadIdx.x >> 6) & 1 : 0;
  const int cl = lane + 64 * half;   // this lane's chunk of the record
  const int c = cl << 2;
  const int nchunk = L.used >> 2;
  // per-lane plan
  float* dstA = nullptr;
  float* dstB = nullptr;
  int64_t ldA = 0, ldB = 0;
  int ncol = -1;    // column of the normalisation constants, -1 = copy
  int nvalid = 4;   // logical elements in this chunk (< 4 only in a field's last chunk when O or A is not a multiple of 4)
  bool vecA = true, is_rd = false;
  if (cl < nchunk) {
    if (c < L.o4) {
      dstA = x_sa ? x_sa + c : nullptr; ldA = ld_sa; ncol = c; nvalid = min(4, L.O - c);
    } else if (c < L.off_act) {
      const int cc = c - L.off_nobs;
      dstA = xn_sa ? xn_sa + cc : nullptr; ldA = ld_sa;
      dstB = xn_obs ? xn_obs + cc : nullptr; ldB = ld_o;
      ncol = cc; nvalid = min(4, L.O - cc);
    } else if (c < L.off_rd) {
      const int cc = c - L.off_act;
      dstA = x_sa ? x_sa + L.O + cc : nullptr; ldA = ld_sa; nvalid = min(4, L.A - cc);
      vecA = (L.O & 3) == 0;   // action columns start at O: 16-B aligned only then
    } else {
      is_rd = true;
    }
  }
  vecA = vecA && nvalid == 4;
  float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f);
  double rd[4] = {1.0, 1.0, 1.0, 1.0};   // 1 / sd (norm_div)
  const bool do_norm = HAS_NORM && ncol >= 0;
  if (do_norm) {   // scalar loads: O need not be a multiple of 4; invalid tail elements keep (0, 1)
    float mm[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nvalid) { mm[j] = mean[ncol + j]; ss[j] = sqrtf(var[ncol + j] + eps); rd[j] = 1.0 / (double)ss[j]; }
    m4 = make_float4(mm[0], mm[1], mm[2], mm[3]);
  }
  // pad columns [O+A, ld_sa) of x_sa / xn_sa and [O, ld_o) of xn_obs: lanes take one 16-B zero store each
  // (scalar, <= 31 per matrix: ld - cols < 32 + 3; pads are a few dozen bytes per row)
  const int sa_cols = L.O + L.A;
  const int npad_sa = (int)(ld_sa - sa_cols), npad_o = xn_obs ? (int)(ld_o - L.O) : 0;
  const bool pad_vec = (sa_cols & 3) == 0 && (L.O & 3) == 0;

  const int hs = halves - 1;   // 0 or 1: a shift, not a 64-bit division (which cost the 8192-row launch 0.3 us)
  // (readfirstlane: the wave's row numbers are provably uniform, so the index loads below are scalar loads -- their own counter,
  //  nothing to do with the in-order vector-memory queue the record loads and the tile stores share)
  const int64_t wave = ((int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) >> hs;
  const int64_t nwaves = ((int64_t)gridDim.x * 4) >> hs;
  // The sample indices run ONE trip ahead of the records they address: idx -> record -> store is a dependent chain per trip, and
  // a wave of the K-batch launch makes five or six trips (65 536 rows over 1536 blocks): the index latency of every trip but the
  // first now passes under the previous trip's record loads and stores.
  int64_t nsrc[R];
#pragma unroll
  for (int i = 0; i < R; ++i) nsrc[i] = wave * R + i < b ? idx[wave * R + i] : 0;
  for (int64_t r0 = wave * R; r0 < b; r0 += nwaves * R) {
    float4 v[R];
    int64_t srcs[R];
#pragma unroll
    for (int i = 0; i < R; ++i) srcs[i] = nsrc[i];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t rn = r0 + nwaves * R + i;
      nsrc[i] = rn < b ? idx[rn] : 0;
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      int64_t src = srcs[i];
      if (src < 0 || src >= capacity) src = 0;
      if (cl < nchunk) {
        if (nt_loads & 1) {   // records are read once per sample: keep them out of the caches the output tiles will be read from
          const f4n t = __builtin_nontemporal_load(reinterpret_cast<const f4n*>(records + src * L.ld) + cl);
          v[i] = make_float4(t[0], t[1], t[2], t[3]);
        } else {
          v[i] = reinterpret_cast<const float4*>(records + src * L.ld)[cl];
        }
      } else {
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t r = r0 + i;
      if (r >= b) break;
      float4 x = v[i];
      if (do_norm) {
        x.x = norm_div(x.x - m4.x, rd[0]); x.y = norm_div(x.y - m4.y, rd[1]);
        x.z = norm_div(x.z - m4.z, rd[2]); x.w = norm_div(x.w - m4.w, rd[3]);
        if (clamp5) {
          x.x = fminf(fmaxf(x.x, -5.f), 5.f); x.y = fminf(fmaxf(x.y, -5.f), 5.f);
          x.z = fminf(fmaxf(x.z, -5.f), 5.f); x.w = fminf(fmaxf(x.w, -5.f), 5.f);
        }
      }
      const float e[4] = {x.x, x.y, x.z, x.w};
      if (dstA) {
        if (vecA) {
          if (nt_loads & 2) __builtin_nontemporal_store(f4n{x.x, x.y, x.z, x.w}, reinterpret_cast<f4n*>(dstA + r * ldA));
          else *reinterpret_cast<float4*>(dstA + r * ldA) = x;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < nvalid) dstA[r * ldA + j] = e[j];
        }
      }
      if (dstB) {
        if (nvalid == 4) *reinterpret_cast<float4*>(dstB + r * ldB) = x;
        else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < nvalid) dstB[r * ldB + j] = e[j];
        }
      }
      if (is_rd) {
        if (o_rew) o_rew[r] = x.x;
        if (o_done) o_done[r] = x.y;
      }
      if (!write_pads || half) continue;
      if (pad_vec) {   // pads start on a 16-B boundary: one 16-B zero store per lane
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < (npad_sa >> 2)) {
          if (x_sa) *reinterpret_cast<float4*>(x_sa + r * ld_sa + sa_cols + 4 * lane) = z4;
          if (xn_sa) *reinterpret_cast<float4*>(xn_sa + r * ld_sa + sa_cols + 4 * lane) = z4;
        }
        if (lane < (npad_o >> 2)) *reinterpret_cast<float4*>(xn_obs + r * ld_o + L.O + 4 * lane) = z4;
      } else {
        if (lane < npad_sa) {
          if (x_sa) x_sa[r * ld_sa + sa_cols + lane] = 0.f;
          if (xn_sa) xn_sa[r * ld_sa + sa_cols + lane] = 0.f;
        }
        if (lane < npad_o) xn_obs[r * ld_o + L.O + lane] = 0.f;
      }
    }
  }
}

// Fast path for OBS-ONLY rings (the P-learner's replay, pql_p_learner.py:32-37,49-50).  A record is O floats -- 384 B at cfg #2,
// 22 of a wave's 64 lanes at one 16-B chunk per lane -- so with one record per wave instruction (the generic kernel above, which
// also re-decodes the field per row: 18 us per 32 768 rows, 0.16 of the HBM roof) two thirds of every load and store instruction
// are idle lanes.  Here a record takes P = 2^lgp lanes (the power of two >= its chunk count) and G = 64 / P records share each
// instruction; a lane's chunk, destinations and normalisation constants are fixed for the whole kernel (as in
// k_replay_gather_fast), a wave keeps R x G records in flight, and the sample indices run one trip ahead of the records.
template <bool HAS_NORM, int R>
__global__ __launch_bounds__(256) void k_replay_gather_obs(const float* __restrict__ records, RecLayout L, int64_t capacity,
                                                           const int64_t* __restrict__ idx, int64_t b,
                                                           const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                           int clamp5, float* __restrict__ x_sa, int64_t ld_sa,
                                                           float* __restrict__ x_obs, int64_t ld_o, int write_pads, int lgp) {
  const int lane = threadIdx.x & 63;
  const int P = 1 << lgp, G = 64 >> lgp;
  const int grp = lane >> lgp, cl = lane & (P - 1);   // record of the instruction, chunk of the record
  const int c = cl << 2;
  const int nchunk = L.used >> 2;
  const bool active = cl < nchunk;
  const int nvalid = active ? min(4, L.O - c) : 0;   // < 4 only in the last chunk when O is not a multiple of 4
  float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f);
  double rd[4] = {1.0, 1.0, 1.0, 1.0};   // 1 / sd (norm_div)
  if (HAS_NORM && active) {
    float mm[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nvalid) { mm[j] = mean[c + j]; ss[j] = sqrtf(var[c + j] + eps); rd[j] = 1.0 / (double)ss[j]; }
    m4 = make_float4(mm[0], mm[1], mm[2], mm[3]);
  }
  const int64_t rows_trip = (int64_t)R * G;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  // Every index and record load below is UNCONDITIONAL straight-line code (rows past b re-read index b - 1, idle lanes re-read
  // chunk 0 of their record: same cache line, nothing stored).  With the loads under `r < b` / `active` branches the compiler put a
  // full `s_waitcnt vmcnt(0)` between the R record loads of a trip -- three dependent memory round trips where one was meant
  // (tools/kernel_resources.py full_drains: 7 -> see the test).
  const int clq = active ? cl : 0;
  int64_t nsrc[R];
#pragma unroll
  for (int i = 0; i < R; ++i) nsrc[i] = idx[min(wave * rows_trip + i * G + grp, b - 1)];
  for (int64_t r0 = wave * rows_trip; r0 < b; r0 += nwaves * rows_trip) {
    float4 v[R];
    int64_t srcs[R];
#pragma unroll
    for (int i = 0; i < R; ++i) srcs[i] = nsrc[i];
#pragma unroll
    for (int i = 0; i < R; ++i) nsrc[i] = idx[min(r0 + nwaves * rows_trip + i * G + grp, b - 1)];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      int64_t src = srcs[i];
      src = (src < 0 || src >= capacity) ? 0 : src;   // never fault on a bad index
      v[i] = reinterpret_cast<const float4*>(records + src * L.ld)[clq];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t r = r0 + i * G + grp;
      if (r >= b) continue;
      float4 x = v[i];
      if (HAS_NORM) {
        x.x = norm_div(x.x - m4.x, rd[0]); x.y = norm_div(x.y - m4.y, rd[1]);
        x.z = norm_div(x.z - m4.z, rd[2]); x.w = norm_div(x.w - m4.w, rd[3]);
        if (clamp5) {
          x.x = fminf(fmaxf(x.x, -5.f), 5.f); x.y = fminf(fmaxf(x.y, -5.f), 5.f);
          x.z = fminf(fmaxf(x.z, -5.f), 5.f); x.w = fminf(fmaxf(x.w, -5.f), 5.f);
        }
      }
      if (nvalid == 4) {
        if (x_sa) *reinterpret_cast<float4*>(x_sa + r * ld_sa + c) = x;
        if (x_obs) *reinterpret_cast<float4*>(x_obs + r * ld_o + c) = x;
      } else {
        const float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < nvalid) {
            if (x_sa) x_sa[r * ld_sa + c + j] = e[j];
            if (x_obs) x_obs[r * ld_o + c + j] = e[j];
          }
      }
      if (!write_pads) continue;   // (the learners keep the pads zero themselves: PQLK_GATHER_PADS_ZERO)
      if (x_sa)
        for (int64_t k = L.O + cl; k < ld_sa; k += P) x_sa[r * ld_sa + k] = 0.f;
      if (x_obs)
        for (int64_t k = L.O + cl; k < ld_o; k += P) x_obs[r * ld_o + k] = 0.f;
    }
  }
}

// k_replay_gather_fast for fp16 transition rings of more than 512 B in use (cfg #4, cfg #5): the same plan-once structure (field decode, destinations and normalisation
// constants per lane once per kernel, R records in flight, scalar index loads one trip ahead).  A lane's 16-B chunk is either
// 8 observation columns (widened, normalised, TWO 16-B stores per destination tile) or 4 raw fp32 words (action / reward, done).
template <bool HAS_NORM, int R>
__global__ __launch_bounds__(256) void k_replay_gather_fast_f16(const uint32_t* __restrict__ records, RecLayoutH L, int64_t capacity,
                                                                const int64_t* __restrict__ idx, int64_t b,
                                                                const float* __restrict__ mean, const float* __restrict__ var,
                                                                float eps, int clamp5, float* __restrict__ x_sa, int64_t ld_sa,
                                                                float* __restrict__ xn_sa, float* __restrict__ xn_obs, int64_t ld_o,
                                                                float* __restrict__ o_rew, float* __restrict__ o_done, int write_pads,
                                                                int nt_loads, int halves) {
  typedef float f4n __attribute__((ext_vector_type(4)));
  typedef uint32_t u4n __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63;
  const int half = halves == 2 ? (threadIdx.x >> 6) & 1 : 0;   // records of 1-2 KiB: two waves per row, one chunk per lane
  const int cl = lane + 64 * half;   // this lane's chunk of the record
  const int c = cl << 2;             // its first word
  const int nchunk = L.used >> 2;
  // per-lane plan
  float* dstA = nullptr;
  float* dstB = nullptr;
  int64_t ldA = 0, ldB = 0;
  int ncol = -1;     // column of the normalisation constants, -1 = raw words
  int nvalid = 4;    // logical columns in this chunk: up to 8 in an observation chunk, up to 4 in an action chunk
  bool is_h = false, alignA = true, is_rd = false;
  if (cl < nchunk) {
    if (c < L.oh) {
      ncol = c << 1; is_h = true;
      dstA = x_sa ? x_sa + ncol : nullptr; ldA = ld_sa; nvalid = min(8, L.O - ncol);
    } else if (c < L.off_act) {
      ncol = (c - L.off_nobs) << 1; is_h = true;
      dstA = xn_sa ? xn_sa + ncol : nullptr; ldA = ld_sa;
      dstB = xn_obs ? xn_obs + ncol : nullptr; ldB = ld_o;
      nvalid = min(8, L.O - ncol);
    } else if (c < L.off_rd) {
      const int cc = c - L.off_act;
      dstA = x_sa ? x_sa + L.O + cc : nullptr; ldA = ld_sa; nvalid = min(4, L.A - cc);
      alignA = (L.O & 3) == 0;   // action columns start at O: 16-B aligned only then
    } else {
      is_rd = true;
    }
  }
  // Stores of a chunk: columns [0, 4) as one 16-B store when the destination is aligned and they are all valid, columns [4, 8) as a
  // second one when all 8 are valid; whatever is left (the tail of a field whose width is no multiple of 4, or an action field that
  // starts on an unaligned column) is ONE group of up to 4 scalar stores at column sbase.
  const bool vec0 = alignA && nvalid >= 4, vec1 = is_h && nvalid == 8;
  const int sbase = vec0 ? 4 : 0;
  const int scnt = !vec0 ? min(nvalid, 4) : (is_h && nvalid < 8 ? nvalid - 4 : 0);
  const int clq = cl < nchunk ? cl : 0;   // idle lanes re-read chunk 0 of the record (same line, nothing stored): unconditional loads
  float mm[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  double rd[8] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0};   // 1 / sd (norm_div)
  const bool do_norm = HAS_NORM && is_h;
  if (do_norm) {   // scalar loads: O need not be a multiple of 8; invalid tail elements keep (0, 1)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nvalid) { mm[j] = mean[ncol + j]; rd[j] = 1.0 / (double)sqrtf(var[ncol + j] + eps); }
  }
  const int sa_cols = L.O + L.A;
  const int npad_sa = (int)(ld_sa - sa_cols), npad_o = xn_obs ? (int)(ld_o - L.O) : 0;
  const bool pad_vec = (sa_cols & 3) == 0 && (L.O & 3) == 0;

  const int hs = halves - 1;
  const int64_t wave = ((int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) >> hs;
  const int64_t nwaves = ((int64_t)gridDim.x * 4) >> hs;
  int64_t nsrc[R];
#pragma unroll
  for (int i = 0; i < R; ++i) nsrc[i] = wave * R + i < b ? idx[wave * R + i] : 0;
  for (int64_t r0 = wave * R; r0 < b; r0 += nwaves * R) {
    u4n v[R];
    int64_t srcs[R];
#pragma unroll
    for (int i = 0; i < R; ++i) srcs[i] = nsrc[i];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t rn = r0 + nwaves * R + i;
      nsrc[i] = rn < b ? idx[rn] : 0;
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      int64_t src = srcs[i];
      if (src < 0 || src >= capacity) src = 0;
      if (nt_loads & 1) v[i] = __builtin_nontemporal_load(reinterpret_cast<const u4n*>(records + src * L.ld) + clq);
      else v[i] = reinterpret_cast<const u4n*>(records + src * L.ld)[clq];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t r = r0 + i;
      if (r >= b) break;
      const u4n w = v[i];
      float e[8];   // the chunk widened as 8 halves (meaningless, and unused, for a chunk of raw fp32 words)
      e[0] = h_lo(w[0]); e[1] = h_hi(w[0]); e[2] = h_lo(w[1]); e[3] = h_hi(w[1]);
      e[4] = h_lo(w[2]); e[5] = h_hi(w[2]); e[6] = h_lo(w[3]); e[7] = h_hi(w[3]);
      if (do_norm) {
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = norm_div(e[j] - mm[j], rd[j]);
        if (clamp5) {
#pragma unroll
          for (int j = 0; j < 8; ++j) e[j] = fminf(fmaxf(e[j], -5.f), 5.f);
        }
      }
      // columns [0, 4): the widened halves of an observation chunk, else the chunk's own four words (selected as integers: copies)
      float lo[4], sc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lo[j] = __uint_as_float(is_h ? __float_as_uint(e[j]) : w[j]);
        sc[j] = sbase ? e[4 + j] : lo[j];
      }
      if (dstA) {
        float* d = dstA + r * ldA;
        if (vec0) {
          if (nt_loads & 2) __builtin_nontemporal_store(f4n{lo[0], lo[1], lo[2], lo[3]}, reinterpret_cast<f4n*>(d));
          else *reinterpret_cast<float4*>(d) = make_float4(lo[0], lo[1], lo[2], lo[3]);
        }
        if (vec1) {
          if (nt_loads & 2) __builtin_nontemporal_store(f4n{e[4], e[5], e[6], e[7]}, reinterpret_cast<f4n*>(d + 4));
          else *reinterpret_cast<float4*>(d + 4) = make_float4(e[4], e[5], e[6], e[7]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < scnt) d[sbase + j] = sc[j];
      }
      if (dstB) {   // only observation chunks have a second destination (always 16-B aligned)
        float* d = dstB + r * ldB;
        if (vec0) *reinterpret_cast<float4*>(d) = make_float4(lo[0], lo[1], lo[2], lo[3]);
        if (vec1) *reinterpret_cast<float4*>(d + 4) = make_float4(e[4], e[5], e[6], e[7]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < scnt) d[sbase + j] = sc[j];
      }
      if (is_rd) {
        if (o_rew) o_rew[r] = lo[0];
        if (o_done) o_done[r] = lo[1];
      }
      if (!write_pads || half) continue;
      if (pad_vec) {   // pads start on a 16-B boundary: one 16-B zero store per lane
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < (npad_sa >> 2)) {
          if (x_sa) *reinterpret_cast<float4*>(x_sa + r * ld_sa + sa_cols + 4 * lane) = z4;
          if (xn_sa) *reinterpret_cast<float4*>(xn_sa + r * ld_sa + sa_cols + 4 * lane) = z4;
        }
        if (lane < (npad_o >> 2)) *reinterpret_cast<float4*>(xn_obs + r * ld_o + L.O + 4 * lane) = z4;
      } else {
        if (lane < npad_sa) {
          if (x_sa) x_sa[r * ld_sa + sa_cols + lane] = 0.f;
          if (xn_sa) xn_sa[r * ld_sa + sa_cols + lane] = 0.f;
        }
        if (lane < npad_o) xn_obs[r * ld_o + L.O + lane] = 0.f;
      }
    }
  }
}

// k_replay_gather_obs for fp16 obs-only rings whose record exceeds the 512 B of the 8-B-chunk kernel below (O = 257..512): P = 2^lgp
// lanes per record, 16-B chunks, every index and record load unconditional, a lane's 8 columns and constants fixed.
template <bool HAS_NORM, int R>
__global__ __launch_bounds__(256) void k_replay_gather_obs_f16(const uint32_t* __restrict__ records, RecLayoutH L, int64_t capacity,
                                                               const int64_t* __restrict__ idx, int64_t b,
                                                               const float* __restrict__ mean, const float* __restrict__ var,
                                                               float eps, int clamp5, float* __restrict__ x_sa, int64_t ld_sa,
                                                               float* __restrict__ x_obs, int64_t ld_o, int write_pads, int lgp) {
  const int lane = threadIdx.x & 63;
  const int P = 1 << lgp, G = 64 >> lgp;
  const int grp = lane >> lgp, cl = lane & (P - 1);   // record of the instruction, chunk of the record
  const int c = cl << 3;                               // first column of the chunk
  const int nchunk = L.used >> 2;
  const bool active = cl < nchunk;
  const int nvalid = active ? min(8, L.O - c) : 0;   // < 8 only in the last chunk when O is not a multiple of 8
  float mm[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  double rd[8] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0};   // 1 / sd (norm_div)
  if (HAS_NORM && active) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nvalid) { mm[j] = mean[c + j]; rd[j] = 1.0 / (double)sqrtf(var[c + j] + eps); }
  }
  const int64_t rows_trip = (int64_t)R * G;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int clq = active ? cl : 0;   // idle lanes re-read chunk 0 of their record: loads stay unconditional
  int64_t nsrc[R];
#pragma unroll
  for (int i = 0; i < R; ++i) nsrc[i] = idx[min(wave * rows_trip + i * G + grp, b - 1)];
  for (int64_t r0 = wave * rows_trip; r0 < b; r0 += nwaves * rows_trip) {
    uint4 v[R];
    int64_t srcs[R];
#pragma unroll
    for (int i = 0; i < R; ++i) srcs[i] = nsrc[i];
#pragma unroll
    for (int i = 0; i < R; ++i) nsrc[i] = idx[min(r0 + nwaves * rows_trip + i * G + grp, b - 1)];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      int64_t src = srcs[i];
      src = (src < 0 || src >= capacity) ? 0 : src;   // never fault on a bad index
      v[i] = reinterpret_cast<const uint4*>(records + src * L.ld)[clq];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t r = r0 + i * G + grp;
      if (r >= b) continue;
      float e[8];
      widen8(v[i], e);
      if (HAS_NORM) {
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = norm_div(e[j] - mm[j], rd[j]);
        if (clamp5) {
#pragma unroll
          for (int j = 0; j < 8; ++j) e[j] = fminf(fmaxf(e[j], -5.f), 5.f);
        }
      }
      if (nvalid == 8) {
        const float4 lo = make_float4(e[0], e[1], e[2], e[3]), hi = make_float4(e[4], e[5], e[6], e[7]);
        if (x_sa) { float* d = x_sa + r * ld_sa + c; *reinterpret_cast<float4*>(d) = lo; *reinterpret_cast<float4*>(d + 4) = hi; }
        if (x_obs) { float* d = x_obs + r * ld_o + c; *reinterpret_cast<float4*>(d) = lo; *reinterpret_cast<float4*>(d + 4) = hi; }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j < nvalid) {
            if (x_sa) x_sa[r * ld_sa + c + j] = e[j];
            if (x_obs) x_obs[r * ld_o + c + j] = e[j];
          }
      }
      if (!write_pads) continue;   // (the learners keep the pads zero themselves: PQLK_GATHER_PADS_ZERO)
      if (x_sa)
        for (int64_t k = L.O + cl; k < ld_sa; k += P) x_sa[r * ld_sa + k] = 0.f;
      if (x_obs)
        for (int64_t k = L.O + cl; k < ld_o; k += P) x_obs[r * ld_o + k] = 0.f;
    }
  }
}

// Narrow variants for fp16 records of at most 512 B in use (cfg #2's 424 B; every obs-only ring up to O = 256): a lane takes an 8-B
// chunk -- 4 observation columns, or 2 raw fp32 words of the action / reward fields -- instead of a 16-B one.  Measured with 16-B
// chunks (tools/bench_gather.py, profiles/replay_fp16_gather.json): a 512-B record keeps only 27 of a wave's 64 lanes busy, each
// with 8 columns to normalise and two half-populated 16-B stores per tile, and the cfg #2 K-batch gather took 31 us against the
// fp32 kernel's 24.  With 8-B chunks the lane -> column map, the arithmetic per lane and the stores (ONE fully populated 16-B store
// per destination tile) are exactly those of k_replay_gather_fast / k_replay_gather_obs; only the loads are half as wide.
__device__ __forceinline__ void widen4(uint32_t w0, uint32_t w1, float e[4]) {
  e[0] = h_lo(w0); e[1] = h_hi(w0); e[2] = h_lo(w1); e[3] = h_hi(w1);
}

template <bool HAS_NORM, int R>
__global__ __launch_bounds__(256) void k_replay_gather_fast_h8(const uint32_t* __restrict__ records, RecLayoutH L, int64_t capacity,
                                                               const int64_t* __restrict__ idx, int64_t b,
                                                               const float* __restrict__ mean, const float* __restrict__ var,
                                                               float eps, int clamp5, float* __restrict__ x_sa, int64_t ld_sa,
                                                               float* __restrict__ xn_sa, float* __restrict__ xn_obs, int64_t ld_o,
                                                               float* __restrict__ o_rew, float* __restrict__ o_done, int write_pads,
                                                               int nt_loads) {
  typedef float f4n __attribute__((ext_vector_type(4)));
  typedef uint32_t u2n __attribute__((ext_vector_type(2)));
  const int lane = threadIdx.x & 63;
  const int c = lane << 1;             // first word of this lane's 8-B chunk
  const int nchunk = L.used >> 1;      // <= 64 (host)
  // per-lane plan
  float* dstA = nullptr;
  float* dstB = nullptr;
  int64_t ldA = 0, ldB = 0;
  int ncol = -1;     // column of the normalisation constants, -1 = raw words
  int nvalid = 0;    // logical columns in this chunk: up to 4 of an observation field, up to 2 of the action field
  bool is_h = false, is_rd = false, act_even = false;
  if (lane < nchunk) {
    if (c < L.oh) {
      ncol = c << 1; is_h = true;
      dstA = x_sa ? x_sa + ncol : nullptr; ldA = ld_sa; nvalid = max(0, min(4, L.O - ncol));
    } else if (c < L.off_act) {
      ncol = (c - L.off_nobs) << 1; is_h = true;
      dstA = xn_sa ? xn_sa + ncol : nullptr; ldA = ld_sa;
      dstB = xn_obs ? xn_obs + ncol : nullptr; ldB = ld_o;
      nvalid = max(0, min(4, L.O - ncol));
    } else if (c < L.off_rd) {
      const int cc = c - L.off_act;
      dstA = x_sa ? x_sa + L.O + cc : nullptr; ldA = ld_sa; nvalid = max(0, min(2, L.A - cc));
      act_even = (L.O & 1) == 0;   // action columns start at O: 8-B aligned only then
    } else if (c == L.off_rd) {
      is_rd = true;
    }
  }
  const bool vec4 = is_h && nvalid == 4, vec2 = act_even && nvalid == 2;
  const int scnt = (vec4 || vec2) ? 0 : nvalid;   // scalar stores: a field's tail, or an action field on an odd column
  float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f);
  double rd[4] = {1.0, 1.0, 1.0, 1.0};   // 1 / sd (norm_div)
  const bool do_norm = HAS_NORM && is_h;
  if (do_norm) {
    float mm[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nvalid) { mm[j] = mean[ncol + j]; rd[j] = 1.0 / (double)sqrtf(var[ncol + j] + eps); }
    m4 = make_float4(mm[0], mm[1], mm[2], mm[3]);
  }
  const int sa_cols = L.O + L.A;
  const int npad_sa = (int)(ld_sa - sa_cols), npad_o = xn_obs ? (int)(ld_o - L.O) : 0;
  const bool pad_vec = (sa_cols & 3) == 0 && (L.O & 3) == 0;
  const int clq = lane < nchunk ? lane : 0;   // idle lanes re-read chunk 0 (same line, nothing stored): unconditional loads

  const int64_t wave = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  int64_t nsrc[R];
#pragma unroll
  for (int i = 0; i < R; ++i) nsrc[i] = wave * R + i < b ? idx[wave * R + i] : 0;
  for (int64_t r0 = wave * R; r0 < b; r0 += nwaves * R) {
    u2n v[R];
    int64_t srcs[R];
#pragma unroll
    for (int i = 0; i < R; ++i) srcs[i] = nsrc[i];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t rn = r0 + nwaves * R + i;
      nsrc[i] = rn < b ? idx[rn] : 0;
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      int64_t src = srcs[i];
      if (src < 0 || src >= capacity) src = 0;
      if (nt_loads & 1) v[i] = __builtin_nontemporal_load(reinterpret_cast<const u2n*>(records + src * L.ld) + clq);
      else v[i] = reinterpret_cast<const u2n*>(records + src * L.ld)[clq];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t r = r0 + i;
      if (r >= b) break;
      const u2n w = v[i];
      float e[4];   // the chunk widened as 4 halves (unused for a chunk of raw fp32 words)
      widen4(w[0], w[1], e);
      if (do_norm) {
        e[0] = norm_div(e[0] - m4.x, rd[0]); e[1] = norm_div(e[1] - m4.y, rd[1]);
        e[2] = norm_div(e[2] - m4.z, rd[2]); e[3] = norm_div(e[3] - m4.w, rd[3]);
        if (clamp5) {
#pragma unroll
          for (int j = 0; j < 4; ++j) e[j] = fminf(fmaxf(e[j], -5.f), 5.f);
        }
      }
      // columns [0, 2): the widened halves of an observation chunk, else the chunk's own two words (selected as integers: copies)
      const float lo0 = __uint_as_float(is_h ? __float_as_uint(e[0]) : w[0]);
      const float lo1 = __uint_as_float(is_h ? __float_as_uint(e[1]) : w[1]);
      const float sc[4] = {lo0, lo1, e[2], e[3]};
      if (dstA) {
        float* d = dstA + r * ldA;
        if (vec4) {
          if (nt_loads & 2) __builtin_nontemporal_store(f4n{e[0], e[1], e[2], e[3]}, reinterpret_cast<f4n*>(d));
          else *reinterpret_cast<float4*>(d) = make_float4(e[0], e[1], e[2], e[3]);
        }
        if (vec2) *reinterpret_cast<float2*>(d) = make_float2(lo0, lo1);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < scnt) d[j] = sc[j];
      }
      if (dstB) {   // only observation chunks have a second destination
        float* d = dstB + r * ldB;
        if (vec4) *reinterpret_cast<float4*>(d) = make_float4(e[0], e[1], e[2], e[3]);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < scnt) d[j] = sc[j];
      }
      if (is_rd) {
        if (o_rew) o_rew[r] = lo0;
        if (o_done) o_done[r] = lo1;
      }
      if (!write_pads) continue;
      if (pad_vec) {   // pads start on a 16-B boundary: one 16-B zero store per lane
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < (npad_sa >> 2)) {
          if (x_sa) *reinterpret_cast<float4*>(x_sa + r * ld_sa + sa_cols + 4 * lane) = z4;
          if (xn_sa) *reinterpret_cast<float4*>(xn_sa + r * ld_sa + sa_cols + 4 * lane) = z4;
        }
        if (lane < (npad_o >> 2)) *reinterpret_cast<float4*>(xn_obs + r * ld_o + L.O + 4 * lane) = z4;
      } else {
        if (lane < npad_sa) {
          if (x_sa) x_sa[r * ld_sa + sa_cols + lane] = 0.f;
          if (xn_sa) xn_sa[r * ld_sa + sa_cols + lane] = 0.f;
        }
        if (lane < npad_o) xn_obs[r * ld_o + L.O + lane] = 0.f;
      }
    }
  }
}

template <bool HAS_NORM, int R>
__global__ __launch_bounds__(256) void k_replay_gather_obs_h8(const uint32_t* __restrict__ records, RecLayoutH L, int64_t capacity,
                                                              const int64_t* __restrict__ idx, int64_t b,
                                                              const float* __restrict__ mean, const float* __restrict__ var,
                                                              float eps, int clamp5, float* __restrict__ x_sa, int64_t ld_sa,
                                                              float* __restrict__ x_obs, int64_t ld_o, int write_pads, int lgp) {
  const int lane = threadIdx.x & 63;
  const int P = 1 << lgp, G = 64 >> lgp;
  const int grp = lane >> lgp, cl = lane & (P - 1);   // record of the instruction, 8-B chunk of the record
  const int c = cl << 2;                               // first column of the chunk
  const int nchunk = L.used >> 1;
  const bool active = cl < nchunk;
  const int nvalid = active ? max(0, min(4, L.O - c)) : 0;   // < 4 only in a field's last chunks (O no multiple of 8)
  float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f);
  double rd[4] = {1.0, 1.0, 1.0, 1.0};   // 1 / sd (norm_div)
  if (HAS_NORM && active) {
    float mm[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nvalid) { mm[j] = mean[c + j]; rd[j] = 1.0 / (double)sqrtf(var[c + j] + eps); }
    m4 = make_float4(mm[0], mm[1], mm[2], mm[3]);
  }
  const int64_t rows_trip = (int64_t)R * G;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int clq = active ? cl : 0;   // idle lanes re-read chunk 0 of their record: loads stay unconditional
  int64_t nsrc[R];
#pragma unroll
  for (int i = 0; i < R; ++i) nsrc[i] = idx[min(wave * rows_trip + i * G + grp, b - 1)];
  for (int64_t r0 = wave * rows_trip; r0 < b; r0 += nwaves * rows_trip) {
    uint2 v[R];
    int64_t srcs[R];
#pragma unroll
    for (int i = 0; i < R; ++i) srcs[i] = nsrc[i];
#pragma unroll
    for (int i = 0; i < R; ++i) nsrc[i] = idx[min(r0 + nwaves * rows_trip + i * G + grp, b - 1)];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      int64_t src = srcs[i];
      src = (src < 0 || src >= capacity) ? 0 : src;   // never fault on a bad index
      v[i] = reinterpret_cast<const uint2*>(records + src * L.ld)[clq];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t r = r0 + i * G + grp;
      if (r >= b) continue;
      float e[4];
      widen4(v[i].x, v[i].y, e);
      if (HAS_NORM) {
        e[0] = norm_div(e[0] - m4.x, rd[0]); e[1] = norm_div(e[1] - m4.y, rd[1]);
        e[2] = norm_div(e[2] - m4.z, rd[2]); e[3] = norm_div(e[3] - m4.w, rd[3]);
        if (clamp5) {
#pragma unroll
          for (int j = 0; j < 4; ++j) e[j] = fminf(fmaxf(e[j], -5.f), 5.f);
        }
      }
      if (nvalid == 4) {
        const float4 x = make_float4(e[0], e[1], e[2], e[3]);
        if (x_sa) *reinterpret_cast<float4*>(x_sa + r * ld_sa + c) = x;
        if (x_obs) *reinterpret_cast<float4*>(x_obs + r * ld_o + c) = x;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < nvalid) {
            if (x_sa) x_sa[r * ld_sa + c + j] = e[j];
            if (x_obs) x_obs[r * ld_o + c + j] = e[j];
          }
      }
      if (!write_pads) continue;   // (the learners keep the pads zero themselves: PQLK_GATHER_PADS_ZERO)
      if (x_sa)
        for (int64_t k = L.O + cl; k < ld_sa; k += P) x_sa[r * ld_sa + k] = 0.f;
      if (x_obs)
        for (int64_t k = L.O + cl; k < ld_o; k += P) x_obs[r * ld_o + k] = 0.f;
    }
  }
}

// ---- host side of the fused gather: one dispatch for both formats (tests/gather_cases.py gather_launch is its mirror) ----
// KERNEL<mean != nullptr, R> of a tuned kernel family on grid g.  R is 1, 2, 4 or, in the fast families, RMAX = 8; the obs families have
// no <., 8> (RMAX = 4: their last rung repeats <., 4> and is never taken).
#define PQLK_GATHER_TUNED_N(KERNEL, NORM, RMAX, ...)                                                                   \
  do {                                                                                                                 \
    if (R == 1) hipLaunchKernelGGL((KERNEL<NORM, 1>), g, dim3(256), 0, st, __VA_ARGS__);                               \
    else if (R == 2) hipLaunchKernelGGL((KERNEL<NORM, 2>), g, dim3(256), 0, st, __VA_ARGS__);                          \
    else if (R == 4) hipLaunchKernelGGL((KERNEL<NORM, 4>), g, dim3(256), 0, st, __VA_ARGS__);                          \
    else hipLaunchKernelGGL((KERNEL<NORM, RMAX>), g, dim3(256), 0, st, __VA_ARGS__);                                   \
  } while (0)
#define PQLK_GATHER_TUNED(KERNEL, RMAX, ...)                                    \
  do {                                                                          \
    if (mean) PQLK_GATHER_TUNED_N(KERNEL, true, RMAX, __VA_ARGS__);             \
    else PQLK_GATHER_TUNED_N(KERNEL, false, RMAX, __VA_ARGS__);                 \
  } while (0)
// k_replay_gather_fused<F, mean != nullptr, R, CH> on `blocks` blocks
#define PQLK_GATHER_GENERIC(R, CH)                                                                                     \
  do {                                                                                                                 \
    if (mean) hipLaunchKernelGGL((k_replay_gather_fused<F, true, R, CH>), dim3((unsigned)blocks), dim3(256), 0, st,    \
                                 records, L, ring->capacity, idx, b, mean, var, eps, clamp5, x_sa, ld_sa, xn_sa, xn_obs, \
                                 ld_o, rew, done, write_pads);                                                         \
    else hipLaunchKernelGGL((k_replay_gather_fused<F, false, R, CH>), dim3((unsigned)blocks), dim3(256), 0, st,        \
                            records, L, ring->capacity, idx, b, mean, var, eps, clamp5, x_sa, ld_sa, xn_sa, xn_obs,    \
                            ld_o, rew, done, write_pads);                                                              \
  } while (0)

template <class F>
static int replay_gather_fused(const PqlReplayDesc* ring, const int64_t* idx, int64_t b, const float* mean, const float* var,
                               float eps, int flags, float* x_sa, int64_t ld_sa, float* xn_sa, float* xn_obs, int64_t ld_o,
                               float* rew, float* done, pqlk_stream_t stream) {
  constexpr bool HALF = F::HALF;
  const int clamp5 = flags & PQLK_GATHER_CLAMP5;
  const int write_pads = (flags & PQLK_GATHER_PADS_ZERO) ? 0 : 1;
  const int tune_R = (flags >> 8) & 15, tune_wpc = (flags >> 12) & 63;
  int nt_loads = ((flags & PQLK_GATHER_NT_LOADS) ? 1 : 0) | ((flags & PQLK_GATHER_NT_STORES) ? 2 : 0);
  const typename F::Layout L = F::layout(ring->obs_dim, ring->act_dim);
  const int nchunk = L.used >> 2;
  PQLK_REQUIRE(nchunk <= 1024, PQLK_E_UNSUPPORTED);
  const typename F::word* records = reinterpret_cast<const typename F::word*>(ring->records);
  const hipStream_t st = pqlk_s(stream);
  // The launch shapes below (rows in flight, waves per CU, the two-waves-per-row split, the 192-MB non-temporal threshold) were
  // measured on fp32 rings and are applied to the fp16 record as they are: nchunk and the bytes read come from the layout, so e.g.
  // cfg #4 (O = 211: 1792 -> 1024 B) moves from the two-waves-per-row shape to one 16-B chunk per lane.  fp16 records with at most
  // 512 B in use (cfg #2, every obs-only ring up to O = 256) go to the 8-B-chunk kernels k_replay_gather_fast_h8 / _obs_h8
  // (`narrow`), the rest to the 16-B-chunk ones: the choice follows from the record alone.
  const bool narrow = HALF && (L.used >> 1) <= 64;
  // aligned transition-ring shape -> lean kernel (pads: at most 64 16-B chunks in total, one lane each)
  // (the pad-column bound only matters when this call has to zero the pads: one lane per pad chunk)
  const bool fast = L.A >= 0 && nchunk <= 128 && (!write_pads || ((ld_sa - L.O - L.A) <= 64 && (!xn_obs || (ld_o - L.O) <= 64))) &&
                    pqlk_aligned16(x_sa) && pqlk_aligned16(xn_sa) && pqlk_aligned16(xn_obs);
  if (fast) {
    // rows in flight per wave: 2 up to 16 Ki rows (more waves, shorter dependent idx -> row chain: 9.3 vs 10.5 us at 8192),
    // 4 beyond (same time at 32 Ki rows, fewer blocks)
    // 2 rows in flight per wave, at most 12 (rounds 1-2: 24) resident waves per CU: beyond that the grid-stride loop takes
    // further trips.  Measured at cfg 5 (32768 rows x 1 KiB, pads not re-zeroed; tools/bench_gather.py): 24 waves/CU x 2 rows
    // 18.5 us, 16 x 2 19.5, 12 x 2 21.4, 32 x 2 22.3, 16 x 4 20.3, 32 x 4 (one trip per wave, the round-1 shape) 23.0, 8 rows
    // in flight 30; at cfg 2 (8192 rows, one trip whatever the cap) 2 rows per wave 7.1 us vs 8.1 (4) and 9.0 (1).
    // Non-temporal record loads: no gain (18.9 vs 18.5).  Requesting trip k+1's records before trip k is normalised and stored
    // (software pipeline): WORSE, 21.5 us -- on gfx9 stores share the in-order vmcnt queue with loads, so the wait for the
    // prefetched records also waits for the previous trip's store acknowledgements.  With the ring small enough to sit in the
    // Infinity Cache (51 MB) the same launch takes 14.9 us: the 5-GB ring's random 1-KiB reads cost ~4 us on top of that, and
    // ring size hardly matters beyond the cache (0.25 GB 18.0 us, 5 GB 19.3, 20 GB 20.1: not a TLB effect).  A loader / consumer
    // split (one wave per workgroup issuing LDS-DMA record loads into a 16-slot LDS ring behind a counted vmcnt, three waves
    // normalising and storing out of the ring, so that no wave ever mixes loads and stores) was built and measured too:
    // 20.2 us at best -- no better than this kernel, i.e. the limit is the memory system's rate for this mix (about 4 TB/s of
    // bytes moved), not the way one wave's loads and stores queue.
    // Round 3 (the K-batch launches: 65 536 rows at cfg 2, five or more trips per wave): with the sample indices loaded one trip
    // ahead, as SCALAR loads (k_replay_gather_fast), the optimum moved to 12 waves per CU -- 25.1 us at cfg 2 x 8 against 26.5
    // at 24 and 31.5 at 8 (before: 35.3 at 12, 27.0 at 24); cfg 4 x 8 54.9-57.0 at 12-32; cfg 5 x 8 flat, 145-148 us at 8-32.
    int R = 2;
    if (tune_R == 1 || tune_R == 2 || tune_R == 4 || tune_R == 8) R = tune_R;
    const int halves = nchunk > 64 ? 2 : 1;   // 1-2 KiB records: two waves per row
    const int rows_blk = 4 / halves * R;
    int64_t fb = (b + rows_blk - 1) / rows_blk;
    const int wpc = tune_wpc ? tune_wpc : 12;
    if (fb > 256 * (int64_t)wpc / 4) fb = 256 * (int64_t)wpc / 4;
    // Launches whose record reads alone exceed what the 256-MB Infinity Cache can hold beside the output tiles (cfg #5 x 8: 262 144
    // rows x 1 KiB) take the records with non-temporal loads: they are read once and would only push the tiles out.  Round 4,
    // tools/bench_gather.py cfg5x8: 150 -> 98 us back to back, 129 -> 123 us one launch at a time; cfg #2 x 8 (59 MB of records):
    // no difference either way, left alone.  (L.ld: the bytes actually read, in either format.)
    if (!tune_R && !tune_wpc && b * (int64_t)L.ld * 4 > ((int64_t)192 << 20)) nt_loads |= 1;
    const dim3 g((unsigned)fb);
#define PQLK_FAST_ARGS records, L, ring->capacity, idx, b, mean, var, eps, clamp5, x_sa, ld_sa, xn_sa, xn_obs, ld_o, rew, done, write_pads, nt_loads
    if constexpr (!HALF) PQLK_GATHER_TUNED(k_replay_gather_fast, 8, PQLK_FAST_ARGS, halves);
    else if (narrow) PQLK_GATHER_TUNED(k_replay_gather_fast_h8, 8, PQLK_FAST_ARGS);   // (<= 64 8-B chunks: never two waves per row)
    else PQLK_GATHER_TUNED(k_replay_gather_fast_f16, 8, PQLK_FAST_ARGS, halves);
#undef PQLK_FAST_ARGS
  } else if (L.A < 0 && nchunk <= 64 && pqlk_aligned16(x_sa) && pqlk_aligned16(xn_obs) && (x_sa || xn_obs)) {
    // obs-only ring whose record fits one 16-B chunk per lane (O <= 256; fp16: O <= 512): several records per wave instruction
    const int nlane = narrow ? (L.used >> 1) : nchunk;   // lanes a record takes: 8-B chunks when they fit a wave, else 16-B chunks
    int lgp = 0;
    while ((1 << lgp) < nlane) ++lgp;
    const int G = 64 >> lgp;
    // rows in flight per wave: R x G, R chosen so that the launch still has ~16 waves per CU to issue from (32 768 rows of
    // cfg #2, G = 2: R = 4, 4096 waves, one trip); waves per CU capped at 16 (grid-stride trips beyond)
    const int64_t groups = (b + G - 1) / G;
    int R = groups >= 4 * 4096 ? 4 : (groups >= 2 * 4096 ? 2 : 1);
    if (tune_R == 1 || tune_R == 2 || tune_R == 4) R = tune_R;
    const int wpc = tune_wpc ? tune_wpc : 16;
    int64_t fb = (groups + 4 * R - 1) / (4 * R);
    if (fb > 256 * (int64_t)wpc / 4) fb = 256 * (int64_t)wpc / 4;
    const dim3 g((unsigned)fb);
#define PQLK_OBS_ARGS records, L, ring->capacity, idx, b, mean, var, eps, clamp5, x_sa, ld_sa, xn_obs, ld_o, write_pads, lgp
    if constexpr (!HALF) PQLK_GATHER_TUNED(k_replay_gather_obs, 4, PQLK_OBS_ARGS);
    else if (narrow) PQLK_GATHER_TUNED(k_replay_gather_obs_h8, 4, PQLK_OBS_ARGS);
    else PQLK_GATHER_TUNED(k_replay_gather_obs_f16, 4, PQLK_OBS_ARGS);
#undef PQLK_OBS_ARGS
  } else {
    const int rows_per_wave = nchunk <= 64 ? 4 : (nchunk <= 128 ? 2 : 1);
    int64_t blocks = (b + 4 * rows_per_wave - 1) / (4 * rows_per_wave);
    if (blocks > 2048) blocks = 2048;
    if (nchunk <= 64) PQLK_GATHER_GENERIC(4, 1);
    else if (nchunk <= 128) PQLK_GATHER_GENERIC(2, 2);
    else if (nchunk <= 256) PQLK_GATHER_GENERIC(1, 4);
    else PQLK_GATHER_GENERIC(1, 16);
  }
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}
#undef PQLK_GATHER_GENERIC
#undef PQLK_GATHER_TUNED
#undef PQLK_GATHER_TUNED_N

extern "C" int pqlk_replay_gather_fused(const PqlReplayDesc* ring, const int64_t* idx, int64_t b, const float* mean,
                                        const float* var, float eps, int flags, float* x_sa, int64_t ld_sa,
                                        float* xn_sa, float* xn_obs, int64_t ld_o, float* rew, float* done,
                                        pqlk_stream_t stream) {
  if (const int rc = ring_ok(ring, idx != nullptr, b)) return rc;
  const int O = ring->obs_dim, A = ring->act_dim;
  PQLK_REQUIRE((mean == nullptr) == (var == nullptr), PQLK_E_NULL);
  if (mean) PQLK_REQUIRE(O <= GATHER_MAX_OBS, PQLK_E_UNSUPPORTED);
  if (x_sa || xn_sa) PQLK_REQUIRE(ld_sa % 32 == 0 && ld_sa >= O + (A < 0 ? 0 : A), PQLK_E_ALIGN);
  if (xn_obs) PQLK_REQUIRE(ld_o % 32 == 0 && ld_o >= O, PQLK_E_ALIGN);
  if (A < 0) PQLK_REQUIRE(xn_sa == nullptr, PQLK_E_UNSUPPORTED);
  if (b == 0) return PQLK_OK;   // (before the cap of 1024 chunks, which replay_gather_fused checks: an empty call is no gather)
  return ring->obs_dtype == PQLK_OBS_F16
             ? replay_gather_fused<RecF16>(ring, idx, b, mean, var, eps, flags, x_sa, ld_sa, xn_sa, xn_obs, ld_o, rew, done, stream)
             : replay_gather_fused<RecF32>(ring, idx, b, mean, var, eps, flags, x_sa, ld_sa, xn_sa, xn_obs, ld_o, rew, done, stream);
}
