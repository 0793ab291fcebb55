// On-policy PPO baseline on the PQL kernels: GAE, the diagonal-Gaussian rollout head, the minibatch gather from the
// trajectory and the clipped policy / value loss heads with their gradients.
//
// Reference arithmetic: AgentPPO.compute_adv / update_net (pql/algo/ppo.py:79-183), DiagGaussianMLPPolicy
// (pql/models/mlp.py:43-75) over torch.distributions.Normal (rsample = loc + eps * scale;
// log_prob = -((v - loc)^2) / (2 var) - log(scale) - log(sqrt(2 pi)); entropy = 0.5 + 0.5 log(2 pi) + log(scale)) summed over
// the action axis by Independent(., 1).  Every reduction runs in a fixed order (no float atomics): two runs give the same bits.
// The MLPs themselves go through pqlk_mlp_forward / pqlk_mlp_backward; clip + AdamW through pqlk_clip_adamw_polyak.
#include "pqlk_common.h"

#define PPO_LOG_SQRT_2PI 0.91893853320467274f   // math.log(math.sqrt(2 * math.pi)) rounded once to fp32
#define PPO_ENT_CONST 1.4189385332046727f       // 0.5 + 0.5 * math.log(2 * math.pi), formed in double, rounded once
#define PPO_HEAD_BLOCKS 256                     // fixed grid of the loss heads: partial counts depend on nothing but the shape
#define PPO_GATHER_ROWS 64                      // minibatch rows per gather block (one advantage partial per block)

static int ppo_group_of(int A) {
  int G = 1;
  while (G < A) G <<= 1;
  return G;
}

// ------------------------------------------------------------------------------------------------
// GAE (ppo.py:88-124).  One thread per env column; TM > 0: all T loads of the column are issued before the reverse scan
// (register arrays, fully unrolled, T <= TM); TM == 0: the generic loop for long horizons.
__device__ __forceinline__ float gae_nnt2(float nnt, const float* __restrict__ tmo, int64_t off) {
  if (!tmo) return nnt;
  return ((nnt != 0.f) != (tmo[off] != 0.f)) ? 1.f : 0.f;   // torch.logical_xor(nnt, timeout[t]) as 0 / 1
}

template <int TM>
__global__ __launch_bounds__(256) void k_ppo_gae(const float* __restrict__ rew, const float* __restrict__ done,
                                                 const float* __restrict__ val, const float* __restrict__ next_val,
                                                 const float* __restrict__ next_done, const float* __restrict__ tmo, int T,
                                                 int64_t n, float gamma, float gl, int use_gae, float* __restrict__ adv,
                                                 float* __restrict__ ret) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float nv_last = next_val[i];
  const float nnt_last = 1.f - next_done[i];
  if constexpr (TM > 0) {
    float r[TM], d[TM], v[TM], to[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      if (t < T) {
        r[t] = rew[t * n + i];
        d[t] = done[t * n + i];
        v[t] = val[t * n + i];
        to[t] = tmo ? tmo[t * n + i] : 0.f;
      }
    }
    float last = 0.f;   // lastgaelam (GAE) / next_return (no GAE)
#pragma unroll
    for (int t = TM - 1; t >= 0; --t) {
      if (t < T) {
        const bool tail = (t == T - 1);
        const float nnt = tail ? nnt_last : (1.f - d[t + 1 < TM ? t + 1 : t]);
        const float nxv = tail ? nv_last : v[t + 1 < TM ? t + 1 : t];
        if (use_gae) {
          const float nnt2 = tmo ? (((nnt != 0.f) != (to[t] != 0.f)) ? 1.f : 0.f) : nnt;
          const float delta = (r[t] + (gamma * nxv) * nnt2) - v[t];
          last = delta + (gl * nnt) * last;
          adv[t * n + i] = last;
          ret[t * n + i] = last + v[t];
        } else {
          const float nr = tail ? nv_last : last;
          last = r[t] + (gamma * nnt) * nr;
          ret[t * n + i] = last;
          adv[t * n + i] = last - v[t];
        }
      }
    }
  } else {
    float last = 0.f;
    for (int t = T - 1; t >= 0; --t) {
      const bool tail = (t == T - 1);
      const float nnt = tail ? nnt_last : (1.f - done[(t + 1) * n + i]);
      const float vt = val[t * n + i];
      if (use_gae) {
        const float nxv = tail ? nv_last : val[(t + 1) * n + i];
        const float delta = (rew[t * n + i] + (gamma * nxv) * gae_nnt2(nnt, tmo, t * n + i)) - vt;
        last = delta + (gl * nnt) * last;
        adv[t * n + i] = last;
        ret[t * n + i] = last + vt;
      } else {
        const float nr = tail ? nv_last : last;
        last = rew[t * n + i] + (gamma * nnt) * nr;
        ret[t * n + i] = last;
        adv[t * n + i] = last - vt;
      }
    }
  }
}

extern "C" int pqlk_gae(const float* rew, const float* done, const float* val, const float* next_val, const float* next_done,
                        const float* timeout, int32_t T, int64_t n, double gamma, double lambda, int32_t use_gae, float* adv,
                        float* ret, pqlk_stream_t stream) {
  PQLK_REQUIRE(rew && done && val && next_val && next_done && adv && ret, PQLK_E_NULL);
  PQLK_REQUIRE(T > 0 && n > 0, PQLK_E_SHAPE);
  const float g = (float)gamma, gl = (float)(gamma * lambda);   // python: gamma * lambda in double, then one fp32 rounding
  const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
  const int ug = use_gae ? 1 : 0;
  if (T <= 8)
    hipLaunchKernelGGL(k_ppo_gae<8>, grid, blk, 0, pqlk_s(stream), rew, done, val, next_val, next_done, timeout, (int)T, n, g, gl, ug, adv, ret);
  else if (T <= 16)
    hipLaunchKernelGGL(k_ppo_gae<16>, grid, blk, 0, pqlk_s(stream), rew, done, val, next_val, next_done, timeout, (int)T, n, g, gl, ug, adv, ret);
  else if (T <= 32)
    hipLaunchKernelGGL(k_ppo_gae<32>, grid, blk, 0, pqlk_s(stream), rew, done, val, next_val, next_done, timeout, (int)T, n, g, gl, ug, adv, ret);
  else
    hipLaunchKernelGGL(k_ppo_gae<0>, grid, blk, 0, pqlk_s(stream), rew, done, val, next_val, next_done, timeout, (int)T, n, g, gl, ug, adv, ret);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

// ------------------------------------------------------------------------------------------------
// Diagonal-Gaussian head of the rollout: G = pow2 >= A lanes per row.  act = mean + exp(logstd) * eps (eps NULL: the mean);
// logp = sum_j in index order of Normal.log_prob; ent (optional) = sum_j (0.5 + 0.5 log 2pi + log scale_j).
__global__ __launch_bounds__(256) void k_ppo_gauss_head(const float* __restrict__ y, int64_t ld_y, const float* __restrict__ logstd,
                                                        const float* __restrict__ eps, int64_t b, int A, int G, float* __restrict__ act,
                                                        int64_t ld_act, float* __restrict__ logp, float* __restrict__ ent) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / G;
  const int j = (int)(t % G);
  const int base = (int)(threadIdx.x & 63) - j;   // lane of column 0 of this row inside the wave
  const bool ok = row < b && j < A;
  float lp = 0.f, en = 0.f;
  if (ok) {
    const float mu = y[row * ld_y + j];
    const float sc = expf(logstd[j]);
    const float a = eps ? mu + eps[row * A + j] * sc : mu;
    act[row * ld_act + j] = a;
    const float ls = logf(sc);   // Normal keeps scale = exp(logstd); log_prob / entropy take scale.log()
    const float d = a - mu;
    lp = -(d * d) / (2.f * (sc * sc)) - ls - PPO_LOG_SQRT_2PI;
    en = PPO_ENT_CONST + ls;
  }
  float slp = 0.f, sen = 0.f;
  for (int k = 0; k < A; ++k) {   // index-order row sums (every lane of the wave takes part in every shuffle)
    slp += __shfl(lp, base + k, 64);
    sen += __shfl(en, base + k, 64);
  }
  if (row < b && j == 0) {
    if (logp) logp[row] = slp;
    if (ent) ent[row] = sen;
  }
}

extern "C" int pqlk_ppo_gauss_head(const float* y, int64_t ld_y, const float* logstd, const float* eps, int64_t b, int32_t act_dim,
                                   float* act, int64_t ld_act, float* logp, float* ent, pqlk_stream_t stream) {
  PQLK_REQUIRE(y && logstd && act, PQLK_E_NULL);
  PQLK_REQUIRE(b > 0 && act_dim > 0 && act_dim <= 64 && ld_y >= act_dim && ld_act >= act_dim, PQLK_E_SHAPE);
  const int G = ppo_group_of(act_dim);
  const int64_t blocks = (b * G + 255) / 256;
  hipLaunchKernelGGL(k_ppo_gauss_head, dim3((unsigned)blocks), dim3(256), 0, pqlk_s(stream), y, ld_y, logstd, eps, b, (int)act_dim, G,
                     act, ld_act, logp, ent);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

// ------------------------------------------------------------------------------------------------
// Minibatch gather from the flat (T*N) trajectory (ppo.py:146-158).  64 minibatch rows per block: the scalars of a row by one
// lane of wave 0, then the block's obs / action elements; obs normalised by obs_rms without clamp into the padded GEMM tile
// (pad columns written as zero).  Advantage partials per block: { rows, sum, sum((x - block mean)^2) }.
// Indices are clamped into [0, rows): a bad permutation reads valid rows instead of leaving the trajectory.
__global__ __launch_bounds__(256) void k_ppo_gather(const int64_t* __restrict__ idx, int64_t mb, int64_t rows,
                                                    const float* __restrict__ obs, int O, const float* __restrict__ mean,
                                                    const float* __restrict__ var, float eps, float* __restrict__ x, int64_t ldx,
                                                    const float* __restrict__ act, int A, float* __restrict__ act_out,
                                                    const float* __restrict__ logp, const float* __restrict__ adv,
                                                    const float* __restrict__ ret, const float* __restrict__ val,
                                                    float* __restrict__ logp_o, float* __restrict__ adv_o, float* __restrict__ ret_o,
                                                    float* __restrict__ val_o, float* __restrict__ part) {
  __shared__ int64_t sidx[PPO_GATHER_ROWS];
  const int64_t r0 = (int64_t)blockIdx.x * PPO_GATHER_ROWS;
  const int64_t left = mb - r0;
  const int nr = left < PPO_GATHER_ROWS ? (int)left : PPO_GATHER_ROWS;
  if (threadIdx.x < PPO_GATHER_ROWS) {
    const int l = threadIdx.x;
    float a = 0.f;
    if (l < nr) {
      int64_t k = idx[r0 + l];
      k = k < 0 ? 0 : (k >= rows ? rows - 1 : k);
      sidx[l] = k;
      a = adv[k];
      const float lp = logp[k], rt = ret[k], vv = val[k];
      logp_o[r0 + l] = lp;
      adv_o[r0 + l] = a;
      ret_o[r0 + l] = rt;
      val_o[r0 + l] = vv;
    }
    const float s = wave_sum(a);
    const float m = s / (float)nr;
    const float dv = l < nr ? a - m : 0.f;
    const float m2 = wave_sum(dv * dv);
    if (l == 0) {
      part[3 * blockIdx.x + 0] = (float)nr;
      part[3 * blockIdx.x + 1] = s;
      part[3 * blockIdx.x + 2] = m2;
    }
  }
  __syncthreads();
  const int64_t nx = (int64_t)nr * ldx;
  for (int64_t e = threadIdx.x; e < nx; e += 256) {
    const int64_t r = e / ldx;
    const int c = (int)(e - r * ldx);
    float o = 0.f;
    if (c < O) {
      const float v = obs[sidx[r] * O + c];
      o = mean ? (v - mean[c]) / sqrtf(var[c] + eps) : v;
    }
    x[(r0 + r) * ldx + c] = o;
  }
  const int64_t na = (int64_t)nr * A;
  for (int64_t e = threadIdx.x; e < na; e += 256) {
    const int64_t r = e / A;
    const int c = (int)(e - r * A);
    act_out[(r0 + r) * A + c] = act[sidx[r] * A + c];
  }
}

extern "C" int32_t pqlk_ppo_gather_parts(int64_t mb) { return mb > 0 ? (int32_t)((mb + PPO_GATHER_ROWS - 1) / PPO_GATHER_ROWS) : 0; }

extern "C" int pqlk_ppo_gather(const int64_t* idx, int64_t mb, int64_t rows, const float* obs, int32_t obs_dim, const float* mean,
                               const float* var, float eps, float* x, int64_t ldx, const float* act, int32_t act_dim, float* act_out,
                               const float* logp, const float* adv, const float* ret, const float* val, float* logp_out,
                               float* adv_out, float* ret_out, float* val_out, float* adv_part, pqlk_stream_t stream) {
  PQLK_REQUIRE(idx && obs && x && act && act_out && logp && adv && ret && val && logp_out && adv_out && ret_out && val_out && adv_part,
               PQLK_E_NULL);
  PQLK_REQUIRE(!mean == !var, PQLK_E_NULL);
  PQLK_REQUIRE(mb > 0 && rows > 0 && obs_dim > 0 && act_dim > 0 && ldx >= obs_dim, PQLK_E_SHAPE);
  hipLaunchKernelGGL(k_ppo_gather, dim3((unsigned)pqlk_ppo_gather_parts(mb)), dim3(256), 0, pqlk_s(stream), idx, mb, rows, obs,
                     (int)obs_dim, mean, var, eps, x, ldx, act, (int)act_dim, act_out, logp, adv, ret, val, logp_out, adv_out,
                     ret_out, val_out, adv_part);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

// ------------------------------------------------------------------------------------------------
// Minibatch advantage mean and unbiased std from the gather's partials (identical bits in every block):
//   mean = sum(s_i) / n,  M2 = sum(M2_i + n_i (s_i / n_i - mean)^2),  std = sqrt(M2 / (n - 1)).  Wave 0 only.
//   A one-row minibatch gives std = sqrt(0 / 0) = NaN, as torch's std() of one element: the loss is NaN, as in the reference.
__device__ __forceinline__ void ppo_adv_stats(const float* __restrict__ part, int np, int64_t n, float& mean, float& std) {
  const int l = threadIdx.x & 63;
  float s = 0.f;
  for (int i = l; i < np; i += 64) s += part[3 * i + 1];
  s = wave_sum(s);
  const float m = s / (float)n;
  float q = 0.f;
  for (int i = l; i < np; i += 64) {
    const float c = part[3 * i], d = part[3 * i + 1] / c - m;
    q += part[3 * i + 2] + c * (d * d);
  }
  q = wave_sum(q);
  mean = m;
  std = sqrtf(q / (float)(n - 1));
}

// Policy head (ppo.py:156-175): per row logp, ratio = exp(logp - old), normalised advantage, max(-adv r, -adv clamp(r)); its
// gradient w.r.t. the mean block (dy) and per-block partial sums of d/dlogstd.  autograd's tie rules: max splits 50/50 on
// equal arguments, clamp passes the gradient on the closed interval.  Fixed grid-stride over row groups.
__global__ __launch_bounds__(256) void k_ppo_policy_head(const float* __restrict__ y, int64_t ld_y, const float* __restrict__ logstd,
                                                         const float* __restrict__ act, const float* __restrict__ old_logp,
                                                         const float* __restrict__ adv, const float* __restrict__ adv_part, int n_parts,
                                                         int64_t b, int A, int G, float lo, float hi, float* __restrict__ dy,
                                                         float* __restrict__ logp_out, float* __restrict__ part) {
  __shared__ float sh_stats[2];
  __shared__ float sh_ls[256];
  __shared__ float sh_loss[4];
  if (threadIdx.x < 64) {
    float m, s;
    ppo_adv_stats(adv_part, n_parts, b, m, s);
    if (threadIdx.x == 0) {
      sh_stats[0] = m;
      sh_stats[1] = s + 1e-8f;
    }
  }
  __syncthreads();
  const float am = sh_stats[0], ad = sh_stats[1];
  const int j = (int)(threadIdx.x % G);
  const int grp = (int)(threadIdx.x / G), groups = 256 / G;
  const int base = (int)(threadIdx.x & 63) - j;
  const bool col = j < A;
  const float sc = col ? expf(logstd[j]) : 1.f;
  const float var = sc * sc, ls = logf(sc);
  const float gB = 1.f / (float)b;
  float acc_ls = 0.f, acc_loss = 0.f;
  // the trip count is the same for every lane of the block (row - grp is the block's first row), so the shuffles stay uniform
  for (int64_t row = (int64_t)blockIdx.x * groups + grp; row - grp < b; row += (int64_t)gridDim.x * groups) {
    const bool live = row < b && col;
    float d = 0.f, lp = 0.f;
    if (live) {
      const float mu = y[row * ld_y + j];
      d = act[row * A + j] - mu;
      lp = -(d * d) / (2.f * var) - ls - PPO_LOG_SQRT_2PI;
    }
    float slp = 0.f;
    for (int k = 0; k < A; ++k) slp += __shfl(lp, base + k, 64);
    if (row < b) {
      const float ratio = expf(slp - old_logp[row]);
      const float na = (adv[row] - am) / ad;
      const float l1 = -na * ratio;
      const float cr = fminf(fmaxf(ratio, lo), hi);
      const float l2 = -na * cr;
      const float w1 = l1 > l2 ? gB : (l1 == l2 ? gB * 0.5f : 0.f);
      const float w2 = l2 > l1 ? gB : (l1 == l2 ? gB * 0.5f : 0.f);
      const bool in = ratio >= lo && ratio <= hi;
      const float dratio = w1 * -na + (in ? w2 * -na : 0.f);
      const float dlp = dratio * ratio;
      if (j == 0) {
        acc_loss += fmaxf(l1, l2);
        if (logp_out) logp_out[row] = slp;
      }
      if (col) {
        dy[row * ld_y + j] = dlp * (d / var);
        acc_ls += dlp * ((d * d) / var - 1.f);
      }
    }
  }
  sh_ls[threadIdx.x] = acc_ls;
  const float wl = wave_sum(acc_loss);
  if ((threadIdx.x & 63) == 0) sh_loss[threadIdx.x >> 6] = wl;
  __syncthreads();
  const int P = 1 + A;   // per block: [ loss sum | dlogstd (A) ]
  if (threadIdx.x == 0) part[blockIdx.x * P] = (sh_loss[0] + sh_loss[1]) + (sh_loss[2] + sh_loss[3]);
  if (threadIdx.x < A) {
    float s = 0.f;
    for (int g = 0; g < groups; ++g) s += sh_ls[g * G + threadIdx.x];
    part[blockIdx.x * P + 1 + threadIdx.x] = s;
  }
}

// one block: loss = sum(partials) / b - lambda_ent * H  (H = the state-independent row entropy, = mean(entropy)) into
// loss_ring[*slot % ring_len]; dlogstd[j] = sum of the block partials - lambda_ent  (d mean(entropy) / d logstd_j = 1)
__global__ __launch_bounds__(256) void k_ppo_policy_fold(const float* __restrict__ part, int nblk, int A, const float* __restrict__ logstd,
                                                         int64_t b, float lambda_ent, float* __restrict__ dlogstd,
                                                         float* __restrict__ ring, const int32_t* __restrict__ slot_dev, int ring_len) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int P = 1 + A;
  for (int c = w; c <= A; c += 4) {   // column 0 = loss, 1.. = dlogstd
    float s = 0.f;
    for (int i = l; i < nblk; i += 64) s += part[i * P + c];
    s = wave_sum(s);
    if (l == 0) {
      if (c > 0) {
        dlogstd[c - 1] = s - lambda_ent;
      } else if (ring) {
        float h = 0.f;
        for (int k = 0; k < A; ++k) h += PPO_ENT_CONST + logf(expf(logstd[k]));
        ring[slot_dev ? (slot_dev[0] % ring_len) : 0] = s / (float)b - lambda_ent * h;
      }
    }
  }
}

static int ppo_head_blocks(int64_t b, int G) {
  const int64_t groups = 256 / G;
  int64_t blocks = (b + groups - 1) / groups;
  if (blocks > PPO_HEAD_BLOCKS) blocks = PPO_HEAD_BLOCKS;
  return (int)blocks;
}

extern "C" int64_t pqlk_ppo_scratch_floats(int64_t b, int32_t act_dim) {
  if (b <= 0 || act_dim <= 0 || act_dim > 64) return 0;
  return (int64_t)ppo_head_blocks(b, ppo_group_of(act_dim)) * (1 + act_dim);
}

extern "C" int pqlk_ppo_policy_loss(const float* y, int64_t ld_y, const float* logstd, const float* act, const float* old_logp,
                                    const float* adv, const float* adv_part, int32_t n_parts, int64_t b, int32_t act_dim, float clip,
                                    float lambda_ent, float* dy, float* dlogstd, float* logp_out, float* scratch,
                                    int64_t scratch_floats, float* loss_ring, const int32_t* slot_dev, int32_t ring_len,
                                    pqlk_stream_t stream) {
  PQLK_REQUIRE(y && logstd && act && old_logp && adv && adv_part && dy && dlogstd && scratch, PQLK_E_NULL);
  PQLK_REQUIRE(b > 0 && act_dim > 0 && act_dim <= 64 && ld_y >= act_dim && n_parts > 0 && (!loss_ring || ring_len > 0), PQLK_E_SHAPE);
  PQLK_REQUIRE(clip >= 0.f, PQLK_E_RANGE);
  PQLK_REQUIRE(scratch_floats >= pqlk_ppo_scratch_floats(b, act_dim), PQLK_E_WORKSPACE);
  const int G = ppo_group_of(act_dim);
  const int blocks = ppo_head_blocks(b, G);
  const float lo = (float)(1.0 - (double)clip), hi = (float)(1.0 + (double)clip);   // python 1 -/+ ratio_clip, then fp32
  hipLaunchKernelGGL(k_ppo_policy_head, dim3(blocks), dim3(256), 0, pqlk_s(stream), y, ld_y, logstd, act, old_logp, adv, adv_part,
                     (int)n_parts, b, (int)act_dim, G, lo, hi, dy, logp_out, scratch);
  PQLK_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ppo_policy_fold, dim3(1), dim3(256), 0, pqlk_s(stream), scratch, blocks, (int)act_dim, logstd, b, lambda_ent,
                     dlogstd, loss_ring, slot_dev, (int)ring_len);
  PQLK_LAUNCH_CHECK();
  return PQLK_OK;
}

// ------------------------------------------------------------------------------------------------
// Value head (ppo.py:161-172): 0.5 mean((v - R)^2) or 0.5 mean(max((v - R)^2, (V + clamp(v - V, -c, c) - R)^2)), its dL/dv into
// column 0 of dy, per-block loss partials.  Fixed grid-stride over rows.
__global__ __launch_bounds__(256) void k_ppo_value_head(const float* __restrict__ v, int64_t ld_v, const float* __restrict__ ret,
                                                        const float* __restrict__ old_v, int64_t b, int clip_on, float clip,
                                                        float* __restrict__ dy, int64_t ld_dy, float* __restrict__ part) {
  __shared__ float sh[4];
  const float g = 0.5f * (1.f / (float)b);   // d(0.5 * mean(.)) / d elem
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < b; i += (int64_t)gridDim.x * 256) {
    const float nv = v[i * ld_v], R = ret[i];
    const float du = nv - R, lu = du * du;
    float dv;
    if (clip_on) {
      const float V = old_v[i], dd = nv - V;
      const float cd = fminf(fmaxf(dd, -clip), clip);
      const float dc = (V + cd) - R, lc = dc * dc;
      const float w1 = lu > lc ? g : (lu == lc ? g * 0.5f : 0.f);
      const float w2 = lc > lu ? g : (lu == lc ? g * 0.5f : 0.f);
      const bool in = dd >= -clip && dd <= clip;
      dv = w1 * (2.f * du) + (in ? w2 * (2.f * dc) : 0.f);
      acc += fmaxf(lu, lc);
    } else {
      dv = g * (2.f * du);
      acc += lu;
    }
    dy[i * ld_dy] = dv;
  }
  const float s = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(64) void k_ppo_value_fold(const float* __restrict__ part, int nblk, int64_t b, float* __restrict__ ring,
                                                       const int32_t* __restrict__ slot_dev, int ring_len) {
  float s = 0.f;
  for (int i = threadIdx.x; i < nblk; i += 64) s += part[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) ring[slot_dev ? (slot_dev[0] % ring_len) : 0] = 0.5f * (s / (float)b);
}

extern "C" int pqlk_ppo_value_loss(const float* v, int64_t ld_v, const float* ret, const float* old_v, int64_t b, int32_t clip_on,
                                   float clip, float* dy, int64_t ld_dy, float* scratch, int64_t scratch_floats, float* loss_ring,
                                   const int32_t* slot_dev, int32_t ring_len, pqlk_stream_t stream) {
  PQLK_REQUIRE(v && ret && dy && scratch && (!clip_on || old_v), PQLK_E_NULL);
  PQLK_REQUIRE(b > 0 && ld_v > 0 && ld_dy > 0 && (!loss_ring || ring_len > 0), PQLK_E_SHAPE);
  PQLK_REQUIRE(clip >= 0.f, PQLK_E_RANGE);
  int64_t blocks = (b + 255) / 256;
  if (blocks > PPO_HEAD_BLOCKS) blocks = PPO_HEAD_BLOCKS;
  PQLK_REQUIRE(scratch_floats >= blocks, PQLK_E_WORKSPACE);
  hipLaunchKernelGGL(k_ppo_value_head, dim3((unsigned)blocks), dim3(256), 0, pqlk_s(stream), v, ld_v, ret, old_v, b, clip_on ? 1 : 0,
                     clip, dy, ld_dy, scratch);
  PQLK_LAUNCH_CHECK();
  if (loss_ring) {
    hipLaunchKernelGGL(k_ppo_value_fold, dim3(1), dim3(64), 0, pqlk_s(stream), scratch, (int)blocks, b, loss_ring, slot_dev, (int)ring_len);
    PQLK_LAUNCH_CHECK();
  }
  return PQLK_OK;
}
