/*
 * pqlk.h -- C ABI of libpqlk.so, the MI355X (gfx950) kernel library for the
 * Parallel-Q-Learning learner hot path.
 *
 * The reference (supersglzc/pql) is pure Python on PyTorch: it has no FFI.  Its
 * plugin boundary is (i) class-name lookup of models/algos, (ii) the Python
 * signatures of the replay/learner objects and (iii) the Hydra key set
 * (SURVEY.md section 8b).  pql_amd/ keeps (i)-(iii) and calls the entry points below
 * through ctypes; every entry point names the reference code it replaces
 * (path:line under the reference tree).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / HIP types in signatures
 *     (pqlk_stream_t is a hipStream_t passed as void*; NULL = default stream).
 *   - All pointers are DEVICE pointers on the current HIP device unless a
 *     parameter is documented as host.  The caller owns every buffer; the
 *     library never allocates, frees or retains a pointer past the call.
 *   - Every call is asynchronous on the given stream and performs no host
 *     synchronisation, so calls can be captured into a hipGraph.
 *   - Return value: 0 = OK; >0 = PQLK_E_* argument error; <0 = -(hipError_t).
 *     pqlk_strerror() describes either.
 *   - Matrices are row-major fp32 with a leading dimension ("ld", in floats)
 *     that is a multiple of 32 (pqlk_ld()); pad columns must be zero on input
 *     and are written as zero on output.
 */
#ifndef PQLK_H
#define PQLK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pqlk_stream_t;

#define PQLK_VERSION 100 /* 0.1.0 */

enum {
  PQLK_OK = 0,
  PQLK_E_NULL = 1,     /* required pointer is NULL */
  PQLK_E_SHAPE = 2,    /* dimension <= 0 or inconsistent */
  PQLK_E_RANGE = 3,    /* index / pointer argument out of range */
  PQLK_E_ALIGN = 4,    /* leading dimension not a multiple of 32 / pointer not 16-B aligned */
  PQLK_E_UNSUPPORTED = 5,
  PQLK_E_WORKSPACE = 6 /* workspace too small */
};

int pqlk_version(void);
const char* pqlk_strerror(int rc);

/* Leading dimension used for a matrix with `cols` logical columns: round up to 32 floats (128 B). */
int64_t pqlk_ld(int64_t cols);

/* ------------------------------------------------------------------------------------------------
 * Replay ring  (reference: pql/replay/simple_replay.py:4-104, pql/algo/pql_p_learner.py:32-37,49-50,66-85)
 *
 * Storage is one array of fixed-stride records instead of the reference's five SoA tensors:
 *     record = [ obs(O) pad4 | next_obs(O) pad4 | action(A) pad4 | reward, done(0.0/1.0), 0, 0 | zero pad ]
 * (each field starts on a 16-B boundary so records move with dwordx4 accesses for any O, A).
 * rec_ld = pqlk_replay_rec_ld(O, A) floats (multiple of 32 => every record starts on a 128-B line, so
 * a random sample touches ceil(rec_bytes/128) HBM lines instead of ~10 for the SoA layout).
 * The obs-only ring of the P-learner is the same thing with A = -1 (record = obs, rec_ld = pqlk_ld(O)).
 *
 * Half-precision observation storage (obs_dtype = PQLK_OBS_F16; the reference's `reserve_space=True`,
 * simple_replay.py:9,15,91,94 -- kept in HBM here, not parked on the host):
 *     record = [ obs(O) f16 pad8 | next_obs(O) f16 pad8 | action(A) f32 pad4 | reward, done, 0, 0 | zero pad ]
 * Fields still start on 16-B boundaries and records on 128-B lines; a 16-B chunk of an observation field holds
 * 8 columns.  rec_ld stays in 4-byte words: 2 * (roundup(O, 8) / 2) + roundup(A, 4) + 4, rounded up to 32
 * (obs-only: roundup(O, 8) / 2, rounded up to 32) -- 512 B against 896 B at O = 88, A = 16.
 * Observations are rounded to nearest even ONCE, at insert (overflow -> +-inf, fp16 subnormals kept, NaN stays
 * NaN), and widened exactly when gathered: an fp16 ring fed x behaves bit for bit like an fp32 ring fed
 * (float)(half)x.  Actions, reward and done stay fp32.  fp16 and not bf16: it is the reference's dtype, and
 * bf16's 8 significand bits are too coarse for raw, not yet normalised observations.
 * Every entry point below dispatches on obs_dtype; an unknown value is PQLK_E_SHAPE.
 * ---------------------------------------------------------------------------------------------- */
enum {
  PQLK_OBS_F32 = 0, /* observations stored as fp32 (the default; a zeroed field means this) */
  PQLK_OBS_F16 = 1  /* observations stored as IEEE binary16 */
};

typedef struct {
  float* records;    /* (capacity, rec_ld) 4-byte words */
  int64_t capacity;  /* rows */
  int32_t obs_dim;   /* O */
  int32_t act_dim;   /* A, or -1 for an obs-only ring */
  int32_t rec_ld;    /* 4-byte words per record */
  int32_t obs_dtype; /* PQLK_OBS_F32 / PQLK_OBS_F16 (was `reserved`, always 0) */
} PqlReplayDesc;

int64_t pqlk_replay_rec_ld(int32_t obs_dim, int32_t act_dim);
/* The same for either storage format; pqlk_replay_rec_ld(O, A) == pqlk_replay_rec_ld_ex(O, A, PQLK_OBS_F32).
 * 0 for obs_dim <= 0 or an unknown obs_dtype. */
int64_t pqlk_replay_rec_ld_ex(int32_t obs_dim, int32_t act_dim, int32_t obs_dtype);

/* Ring insert of m rows at row `next_p` (host-side pointer law stays in Python, it is integer
 * bookkeeping: simple_replay.py:52-83).  Row r of the source goes to (dst_start + r) for r in
 * [0, m); the caller issues one call per contiguous segment (head, then wrapped tail).
 * done is canonicalised to 0.0/1.0 (reference: `.bool()` on ingest :51, `.float()` on sample :103).
 * act/rew/next_obs/done are ignored (may be NULL) for an obs-only ring.
 * src_ld_* are the source row strides in floats (contiguous tensors: O, A, 1, O, 1). */
int pqlk_replay_insert(const PqlReplayDesc* ring, int64_t dst_start, int64_t m,
                       const float* obs, int64_t ld_obs, const float* act, int64_t ld_act,
                       const float* rew, int64_t ld_rew, const float* next_obs, int64_t ld_nobs,
                       const float* done, int64_t ld_done, pqlk_stream_t stream);

/* Plain sample gather = ReplayBuffer.sample_batch with the index vector supplied
 * (simple_replay.py:98-104): five contiguous outputs (B,O),(B,A),(B,1),(B,O),(B,1) fp32. */
int pqlk_replay_gather(const PqlReplayDesc* ring, const int64_t* idx, int64_t b,
                       float* obs, float* act, float* rew, float* next_obs, float* done,
                       pqlk_stream_t stream);

/* Fused learner gather: sample + normalize (pql/utils/common.py:139-145:
 * clamp((x-mean)/sqrt(var+eps), -5, 5); mean == NULL => identity; clamp5 = 0 => no clamp, the DDPG
 * flavour ddpg.py:124-126) + torch.cat((obs, action)) (pql/models/mlp.py:197) in one pass.
 *   x_sa   (B, ld_sa)  : [ norm(obs) | action | 0 ]          critic input            (may be NULL)
 *   xn_sa  (B, ld_sa)  : [ norm(next_obs) | untouched | 0 ]  target-critic input; the action columns
 *                        are filled later by the target actor                        (may be NULL)
 *   xn_obs (B, ld_o)   : [ norm(next_obs) | 0 ]              target-actor input      (may be NULL)
 *   rew, done (B)                                                                    (may be NULL)
 * For an obs-only ring only x_sa (obs columns + zeroed action columns) and/or xn_obs (= norm(obs)
 * with ld_o) are written (pql_p_learner.py:49-52).
 * clamp5 is a flag word: bit 0 = apply the +-5 clamp; bit 1 (PQLK_GATHER_PADS_ZERO) = the caller guarantees that the pad
 * columns [O+A, ld_sa) / [O, ld_o) of the destinations are already zero (allocated zeroed, written by nothing else), so
 * the kernel does not re-zero them on every call (11 % fewer bytes stored at cfg 5).  Launch-shape overrides for
 * tools/bench_gather.py ride in the same word, so the library keeps no tuning state between calls: bit 2 = non-temporal
 * record loads, bits 8-11 = rows in flight per wave (1, 2, 4, 8; 0 = automatic), bits 12-17 = resident waves per CU
 * (0 = automatic). */
#define PQLK_GATHER_CLAMP5 1
#define PQLK_GATHER_PADS_ZERO 2
#define PQLK_GATHER_NT_LOADS 4
#define PQLK_GATHER_NT_STORES 8   /* experiment: non-temporal stores of the main 16-B tile writes */
#define PQLK_GATHER_ROWS_IN_FLIGHT(r) (((r) & 15) << 8)
#define PQLK_GATHER_WAVES_PER_CU(w) (((w) & 63) << 12)
int pqlk_replay_gather_fused(const PqlReplayDesc* ring, const int64_t* idx, int64_t b,
                             const float* mean, const float* var, float eps, int clamp5,
                             float* x_sa, int64_t ld_sa, float* xn_sa, float* xn_obs, int64_t ld_o,
                             float* rew, float* done, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * n-step assembler  (reference: pql/replay/nstep_replay.py:6-92)
 *
 * Circular per-env window instead of the reference's five torch.cat FIFO shifts per step.
 * window: (N, nstep, win_ld) fp32, win_ld = pqlk_replay_rec_ld(O, A), same record layout as the ring.
 * `count` = number of steps pushed before this call (host integer; slot of step s is s % nstep).
 * Inputs are the (N, T, .) slabs of PQLActor.explore_env (pql_actor.py:89-93,117-121).
 * Emits, for every step s = count + t with s + 1 >= nstep, one row per env in TIME-MAJOR order
 * (row = (s - first_emit_step) * N + env; nstep_replay.py:65), to five contiguous outputs.
 * gamma_pow: nstep floats (host pointer), gamma^j computed in double, rounded to fp32 (:24).
 * Reward sum, for every nstep up to 16: terms (r_j * g_j) * keep_j, j = 0 the oldest step, keep_j = 0 behind the first done;
 * four partial sums A_i over the j with j mod 4 == i, each in increasing j, then ((A0 + A1) + A2) + A3 (a lane without a term is
 * left out).  That is torch's CPU row sum `.sum(1)` for nstep <= 5 only (and plain left to right for nstep <= 4); from
 * nstep = 6 on it is this library's own order, stated in oracle NStepRef._emit and tests/rollout_cases.py.
 * nstep = 1 copies the inputs through (the window is still written).  A call with t_steps <= nstep - 1 - count emits nothing:
 * the outputs may then be NULL, the window is filled, *rows_out = 0.
 * PQLK_E_UNSUPPORTED: nstep outside [1, 16].
 * Returns the number of emitted rows through *rows_out (host pointer, may be NULL). */
int pqlk_nstep_push_emit(float* window, int64_t num_envs, int32_t nstep, int32_t obs_dim, int32_t act_dim,
                         int64_t count, int64_t t_steps,
                         const float* obs, const float* act, const float* rew, const float* next_obs,
                         const float* done, const float* gamma_pow /*host*/,
                         float* o_obs, float* o_act, float* o_rew, float* o_next_obs, float* o_done,
                         int64_t* rows_out /*host*/, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * MLP family  (reference: pql/models/mlp.py:15-40 MLPNet, :177-179 TanhMLPPolicy, :186-203 DoubleQ,
 * :244-267 DistributionalDoubleQ; backward = torch autograd of the same)
 *
 * One descriptor covers `n_nets` structurally identical nets evaluated on a shared input
 * (1 = actor, 2 = twin critic).  Parameters live in ONE flat fp32 arena:
 *   for net in 0..n_nets-1: for layer in 0..n_layers-1:
 *       W  (out_l, pqlk_ld(in_l))  row-major, y = x W^T + b  (same (out,in) orientation as nn.Linear)
 *       b  (pqlk_ld(out_l))
 * Gradients, Adam moments and Polyak targets use the same layout, so the optimiser is one pass over
 * the arena.  Hidden activation is ELU(alpha=1).
 * ---------------------------------------------------------------------------------------------- */
#define PQLK_MAX_LAYERS 8

enum { PQLK_ACT_NONE = 0, PQLK_ACT_TANH = 1, PQLK_ACT_TANH_NOISE = 2 };

typedef struct {
  int32_t n_layers;                 /* number of Linear layers (hidden + 1) */
  int32_t n_nets;                   /* 1 or 2 */
  int32_t dims[PQLK_MAX_LAYERS + 1]; /* in, h1, ..., out */
} PqlMlpDesc;

int64_t pqlk_mlp_param_floats(const PqlMlpDesc* d);                       /* arena size, all nets */
int64_t pqlk_mlp_net_stride(const PqlMlpDesc* d);                         /* floats between nets */
int pqlk_mlp_layer_offsets(const PqlMlpDesc* d, int32_t layer, int64_t* w_off, int64_t* b_off); /* within a net */
int64_t pqlk_mlp_acts_floats(const PqlMlpDesc* d, int64_t b);             /* activation stash, all nets */
int pqlk_mlp_act_offset(const PqlMlpDesc* d, int64_t b, int32_t net, int32_t layer, int64_t* off, int64_t* ld);
int64_t pqlk_mlp_bwd_ws_floats(const PqlMlpDesc* d, int64_t b, int32_t splits); /* backward workspace */

/* Fragment-ordered copy of the hidden layers' weights used by the fused forward path:
 *   packed[net][layer < L-1][tile n/32][k/8][lane (r,h)][j] = W[32 tile + r][8 (k/8) + 4 h + j]
 * pqlk_mlp_packed_floats() is 0 when the descriptor cannot take the fused path (a hidden width not a multiple of
 * 32, or wider than 636 so that two 32-row LDS activation buffers exceed 160 KB).  Call pqlk_mlp_pack() whenever
 * the arena changes (after the optimiser / Polyak step); it is one tiny launch per hidden layer. */
int64_t pqlk_mlp_packed_floats(const PqlMlpDesc* d);
int pqlk_mlp_pack(const PqlMlpDesc* d, const float* params, float* packed, pqlk_stream_t stream);

/* Forward.  x: (B, ldx) with ldx >= pqlk_ld(dims[0]).  acts: stash of every layer's post-activation
 * output (layer l of net n at pqlk_mlp_act_offset).  The last layer's output gets `out_act`:
 *   NONE       : logits / Q values
 *   TANH       : TanhMLPPolicy (mlp.py:179)
 *   TANH_NOISE : tanh, then target-policy smoothing a' = clamp(a + clamp(noise_std*draw, +-noise_clip), +-1)
 *                (pql/utils/noise.py:19-27 via pql_v_learner.py:63-71); draw: (B, dims[L]) contiguous N(0,1).
 * If out2 != NULL (n_nets must be 1) the final output is ALSO written to out2 with row stride ld_out2
 * (used to drop the actor's action into the action columns of a critic input: torch.cat for free).
 * packed != NULL (from pqlk_mlp_pack of the SAME params) selects the fused path: all hidden layers in one launch with
 * the activations of a 32- or 64-row tile resident in LDS; hidden activations are identical to the per-layer path (same
 * accumulation order).  An output layer of at most 32 columns runs inside the same launch with its reduction split over
 * the block's waves (a reassociation of the same products: ~1e-7 relative to the per-layer result).
 * stash_all = 0 on that path writes only what a forward-only caller needs: the output block, plus the last hidden layer
 * when the output layer is NOT fused; the other activation blocks are left untouched.  Backward needs stash_all = 1.  On the fused path columns [dims[0], ldx) of x are IGNORED (masked to zero while the
 * tile is staged), so x may alias a wider matrix; the per-layer path requires them to be zero.
 * stash_all = PQLK_STASH_OUTPUT_ONLY (2): forward-only call where `acts` IS the output block, (n_nets, B, pqlk_ld(out)) floats, and
 * nothing else is written -- the target policy's actions for the next K learner steps come from ONE launch over K x B rows
 * (the policy is fixed between two hand-offs, pql_v_learner.py:62-71,117-122) without a K x B activation stash.  Fused hidden stack
 * + fused output layer only (PQLK_E_UNSUPPORTED otherwise). */
#define PQLK_STASH_OUTPUT_ONLY 2
int pqlk_mlp_forward(const PqlMlpDesc* d, const float* params, const float* packed, int32_t stash_all,
                     const float* x, int64_t ldx, int64_t b,
                     int32_t out_act, const float* draw, float noise_std, float noise_clip,
                     float* acts, float* out2, int64_t ld_out2, pqlk_stream_t stream);

/* Forward-only stack on bf16 MFMA (pql_amd/csrc/fwd_bf16.hip): the V-learner's no-gradient target forwards with
 * algo.target_dtype=bfloat16.  The law, for every net: x~ = bf16(x[:, :dims[0]]) and W~_l = bf16(W_l) for EVERY layer, both round
 * to nearest even; z_l = sum_k a~_{l-1,k} W~_l[j,k] + b_l[j] accumulated in fp32 with fp32 biases; hidden a_l = bf16(elu(z_l)) with
 * the fp32 ELU of the fused path; the output layer's z stays fp32, gets `out_act` in fp32 exactly as pqlk_mlp_forward and is written
 * as fp32 with zero pad columns.  NaN / Inf propagate; a row's bits depend on neither b, its position, nor the launch.
 * Eligible (pqlk_mlp_bf16_ok): n_layers >= 2, hidden widths multiples of 32 and <= 1024, output width <= 64, and an input
 * width whose two 32-row bf16 images fit 160 KB of LDS (<= 1264).
 *   packed[net][layer][tile n/32][k/16][lane = 32 h + r][j] = bf16(W[32 tile + r][16 (k/16) + 8 h + j]),
 * every layer, K padded to 16 and N to 32 with zeros: pqlk_mlp_packed_bf16_elems() uint16 elements (0 when not eligible).  Call
 * pqlk_mlp_pack_bf16() (one launch) whenever the arena changes.  pqlk_mlp_forward_bf16: `params` supplies the biases; x, ldx, b,
 * out_act, draw, the noise arguments, out2 / ld_out2 as pqlk_mlp_forward; out is the (n_nets, b, pqlk_ld(out)) output block alone.
 * Columns [dims[0], ldx) of x are ignored, and out2 may point into the rows of x that the same call reads (the policy writes its
 * actions into the action columns of its own input tile).  PQLK_E_UNSUPPORTED when the descriptor is not eligible. */
int pqlk_mlp_bf16_ok(const PqlMlpDesc* d);                 /* 1 / 0 */
int64_t pqlk_mlp_packed_bf16_elems(const PqlMlpDesc* d);   /* uint16 elements; 0 when not ok */
int pqlk_mlp_pack_bf16(const PqlMlpDesc* d, const float* params, uint16_t* packed, pqlk_stream_t stream);
int pqlk_mlp_forward_bf16(const PqlMlpDesc* d, const float* params, const uint16_t* packed,
                          const float* x, int64_t ldx, int64_t b,
                          int32_t out_act, const float* draw, float noise_std, float noise_clip,
                          float* out, float* out2, int64_t ld_out2, pqlk_stream_t stream);

/* Backward.  dy: (n_nets, B, pqlk_ld(out)) gradient w.r.t. the last layer's PRE-activation output
 * (loss kernels below produce exactly that).  grads (arena layout) is overwritten with the full
 * parameter gradient when != NULL (deterministic split-batch partial sums through `ws`).
 * dx (B, ld_dx) receives the input gradient summed over nets when != NULL; if dx_tanh_of != NULL the
 * columns [dx_col0, dx_col0 + dx_cols) are multiplied by (1 - a^2) with a = dx_tanh_of (B, ld_tanh)
 * and ONLY those columns are written, compacted to column 0 of dx (DPG chain through the actor's
 * tanh, pql_p_learner.py:55-58). */
int pqlk_mlp_backward(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b,
                      const float* acts, const float* dy, float* grads, int32_t splits,
                      float* dx, int64_t ld_dx, int32_t dx_col0, int32_t dx_cols,
                      const float* dx_tanh_of, int64_t ld_tanh,
                      float* ws, int64_t ws_floats, pqlk_stream_t stream);

/* Same backward, with clip_grad_norm_'s first half folded into its last pass (pql_v_learner.py:128): the kernel that sums
 * the split slabs into `grads` also leaves per-block partials of sum(g^2) in sumsq_part[0, pqlk_mlp_norm_parts(d)) (room for
 * 2048 floats) and increments the optimiser's device step counter.  Follow with pqlk_adamw_polyak_fused(prenorm =
 * pqlk_mlp_norm_parts(d)).  Same gradient as pqlk_mlp_backward; the norm's partial sums are grouped differently from
 * pqlk_clip_adamw_polyak*'s own pass (last-bit differences in the clip factor).  Not for data parallel, where the gradient
 * all-reduce sits between backward and the norm. */
int pqlk_mlp_backward_norm(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b,
                           const float* acts, const float* dy, float* grads, int32_t splits,
                           float* dx, int64_t ld_dx, int32_t dx_col0, int32_t dx_cols,
                           const float* dx_tanh_of, int64_t ld_tanh,
                           float* ws, int64_t ws_floats, float* sumsq_part, int32_t* step_dev, pqlk_stream_t stream);
int32_t pqlk_mlp_norm_parts(const PqlMlpDesc* d);

/* Backward of a twin critic with scalar Q heads whose head pass forms dL/dQ itself: TD target y = r + (1-d) gamma^n
 * min(Q1', Q2') and the twin MSE loss of pql_v_learner.py:104-108 (replaces pqlk_td_mse_loss + pqlk_mlp_backward[_norm]: one
 * launch less, dL/dQ never goes through memory).  acts / acts_target: activation stashes of the online and the target
 * forward (only the target's head output is read).  loss_part receives pqlk_td_head_loss_parts(d, b) partial sums of
 * (Q - y)^2 over both nets: fold with scale 1 / b (pqlk_adamw_polyak_fused's loss_part).  sumsq_part / step_dev: both
 * non-NULL = as pqlk_mlp_backward_norm, both NULL = as pqlk_mlp_backward.  PQLK_E_UNSUPPORTED unless n_nets == 2, one
 * output, and the last hidden width is <= 1024. */
int pqlk_mlp_backward_td(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b,
                         const float* acts, const float* acts_target, const float* rew, const float* done, float gamma_n,
                         float* loss_part, float* grads, int32_t splits, float* ws, int64_t ws_floats,
                         float* sumsq_part, int32_t* step_dev, pqlk_stream_t stream);
int32_t pqlk_td_head_loss_parts(const PqlMlpDesc* d, int64_t b);   /* 0: this layout cannot take pqlk_mlp_backward_td */

/* The same scalar-head step with the head's backward inside the critic's FORWARD launch: pqlk_mlp_forward_td is
 * pqlk_mlp_forward(packed, stash_all = 1, PQLK_ACT_NONE) whose blocks, having formed Q for their rows, also form the TD error
 * (pql_v_learner.py:104-108), dL/dZ of the last hidden layer, the head's dW / db partials and the loss partials while that
 * layer's activations are still in LDS -- no head-backward launch, no second read of them (and no stash of them: that block of
 * `acts` is left unwritten).  bwd_ws / splits: the workspace and split count the backward will be called with.  Follow with
 * pqlk_mlp_backward_td_tail (same arguments as pqlk_mlp_backward_td minus the TD inputs): layers n_layers-2 .. 0 and the slab
 * reduction.  loss_part receives pqlk_td_forward_loss_parts(d, b) partials (0: this layout / batch cannot take the path: no
 * fused hidden stack, not a twin scalar head, or no room beside the last hidden layer in LDS). */
int32_t pqlk_td_forward_loss_parts(const PqlMlpDesc* d, int64_t b);
int pqlk_mlp_forward_td(const PqlMlpDesc* d, const float* params, const float* packed, const float* x, int64_t ldx, int64_t b,
                        float* acts, const float* acts_target, const float* rew, const float* done, float gamma_n,
                        float* loss_part, float* bwd_ws, int64_t bwd_ws_floats, int32_t splits, pqlk_stream_t stream);
int pqlk_mlp_backward_td_tail(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b,
                              const float* acts, float* grads, int32_t splits, float* ws, int64_t ws_floats,
                              float* sumsq_part, int32_t* step_dev, pqlk_stream_t stream);

/* Data-parallel buckets (the gradient all-reduce "overlapped with the last dW GEMMs"; the reference has no
 * counterpart, its learners are single-GPU -- pql_v_learner.py:110-113 is `backward(); step()`).  Layers layer_hi >= l >=
 * layer_lo of the backward above (dW_l, db_l, dX_l) and then the split-slab reduction of exactly those layers into `grads`:
 * what this call leaves in grads is final, so its all-reduce can be issued while the calls for the layers below still run.
 * Calls walk the layers downwards (first: layer_hi = n_layers - 1, last: layer_lo = 0) over the SAME workspace; their union
 * leaves in grads bit for bit what one pqlk_mlp_backward / pqlk_mlp_backward_td call leaves.  dy is read by the call holding
 * the last layer; give acts_target / rew / done / loss_part (all four or none) and that call forms the TD error in the head
 * pass as pqlk_mlp_backward_td does (dy is then ignored). */
int pqlk_mlp_backward_layers(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b,
                             const float* acts, const float* dy, const float* acts_target, const float* rew,
                             const float* done, float gamma_n, float* loss_part, float* grads, int32_t splits,
                             float* ws, int64_t ws_floats, int32_t layer_hi, int32_t layer_lo, pqlk_stream_t stream);

/* The learners' random draws with torch's own numbers (csrc/philox.hip; reference draws: pql/replay/simple_replay.py:87,
 * pql/utils/noise.py:20-21, pql/algo/pql_p_learner.py:49).  `chunks` consecutive learner steps in ONE launch: per step n_idx
 * int64 indices uniform on [0, range) into idx[chunk][n_idx], then n_normal standard normals into normal[chunk][n_normal]
 * (either part may be absent: n = 0 / NULL).  Chunk c holds exactly what
 *     torch.randint(range, (n_idx,), generator=g);  torch.empty(n_normal).normal_(generator=g)
 * return on a device generator g with this seed and Philox offset
 *     base_offset + (step - base_step + c) * (pqlk_philox_increment(n_idx) + pqlk_philox_increment(n_normal)),
 * step = step_dev[0] (a device step counter; NULL: base_step).  range < 2^28 (torch draws 64-bit values above).  contract:
 * Box-Muller's affine map of the angle as one fma (how torch's build of rocRAND compiles it) or as mul + add; which one
 * matches is checked against torch on the device by pql_amd/utils/rng.py, which falls back to ATen launches otherwise. */
int pqlk_philox_draws(uint64_t seed, int64_t base_offset, int32_t base_step, const int32_t* step_dev, int64_t range,
                      int64_t* idx, int64_t n_idx, float* normal, int64_t n_normal, int32_t chunks, int32_t contract,
                      pqlk_stream_t stream);
/* Philox offset increment of one torch draw of `numel` elements (4 values per counter block, at most 2048 x 256 threads). */
int64_t pqlk_philox_increment(int64_t numel);

/* DPG backward through the frozen twin critic (pql_p_learner.py:55-58): the input gradient of pqlk_mlp_backward's
 * (grads = NULL, dx + dx_tanh_of) form.  With scalar Q heads the gradient of min(Q1, Q2) reaches one net per sample, so the
 * samples are first partitioned by owning net and the dX chain runs over compact rows -- half the MFMA work, each sample's
 * values bit for bit those of the dense chain; other critics take the dense chain.  The compact chain overwrites dx (B, ld_dx)
 * fully (columns >= dx_cols with zero); the dense chain writes columns [0, dx_cols) alone and leaves the others untouched, as
 * pqlk_mlp_backward does, so a caller that wants them zero keeps them zero itself (the P-learner allocates dx zeroed).
 * ws >= pqlk_dpg_backward_ws_floats(d, b) floats. */
int64_t pqlk_dpg_backward_ws_floats(const PqlMlpDesc* d, int64_t b);
int pqlk_dpg_critic_backward(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b,
                             const float* acts, const float* dy, float* dx, int64_t ld_dx, int32_t dx_col0, int32_t dx_cols,
                             const float* dx_tanh_of, int64_t ld_tanh, const uint8_t* owner /* (B) from pqlk_dpg_loss_owner, or NULL */,
                             float* ws, int64_t ws_floats, pqlk_stream_t stream);

/* The P-learner's whole backward through the frozen critic in four launches (round 4; pql_p_learner.py:54-58: actor(obs) ->
 * -critic.get_q_min(obs, a).mean() -> .backward()).  Twin scalar-head critics whose forward is fused (hidden stack + head):
 *   pqlk_mlp_forward_qc        the critic's forward (as pqlk_mlp_forward, out_act none) that ALSO leaves the head outputs compact,
 *                              qc (2, B) = Q1 | Q2 (DoubleQ.get_q1_q2, mlp.py:197-199).  With x2 != NULL the input is
 *                              [ x[:, :x2_col0] | x2[:, :dims[0] - x2_col0] ] -- `torch.cat((state, action), dim=1)` (mlp.py:197) read
 *                              from where the two halves already lie (the actor's input tile, the actor's output block): the
 *                              P-learner's gather then writes the observations once instead of twice.  x2_col0 % 4 == 0.
 *   pqlk_dpg_backward_fused    (1) DPG loss partials, partition of the batch by the net that attained min(Q1, Q2) and the head's dX
 *                              over compact rows in ONE launch (replaces pqlk_dpg_loss_owner + two launches of
 *                              pqlk_dpg_critic_backward), (2) the compact dX GEMMs, (3) the action slice through tanh' TOGETHER
 *                              WITH the actor's last-layer backward (dX, dW / db partials per 32-row tile: replaces the actor
 *                              backward's head launch).  loss_part[pqlk_dpg_fused_loss_parts()] = partial sums of min(Q1, Q2):
 *                              fold with scale -1 / b.  dz_a (B, ld_dz): columns [0, A) of every row are written (A = the actor's
 *                              output width = the critic input's action columns [dx_col0, dx_col0 + A)), pad columns untouched.
 *   pqlk_mlp_backward_tail     the rest of the actor's backward (layers below the head, slab reduction incl. the head fold,
 *                              optional squared-norm partials as pqlk_mlp_backward_norm) over the SAME actor workspace;
 *                              head_parts = pqlk_dpg_fused_head_parts(b), head_parts_dev = critic_ws +
 *                              pqlk_dpg_fused_mn_offset(critic, b) floats (a device int[4]; only the partial tiles in use exist).
 * pqlk_dpg_fused_ok = 1 when this critic / actor pair can take the path (else use pqlk_dpg_loss_owner +
 * pqlk_dpg_critic_backward + pqlk_mlp_backward); every entry returns PQLK_E_UNSUPPORTED otherwise.  pqlk_dpg_backward_fused does not
 * read x (the critic's input): it may be NULL.
 * critic_ws >= pqlk_dpg_backward_ws_floats(critic, b), actor_ws >= pqlk_mlp_bwd_ws_floats(actor, b, splits) floats. */
int32_t pqlk_dpg_fused_ok(const PqlMlpDesc* critic, const PqlMlpDesc* actor, int64_t b);
int32_t pqlk_dpg_fused_loss_parts(void);
int32_t pqlk_dpg_fused_head_parts(int64_t b);
int64_t pqlk_dpg_fused_mn_offset(const PqlMlpDesc* critic, int64_t b);
int pqlk_mlp_forward_qc(const PqlMlpDesc* d, const float* params, const float* packed, int32_t stash_all, const float* x,
                        int64_t ldx, const float* x2 /* or NULL */, int64_t ldx2, int32_t x2_col0, int64_t b, float* acts, float* qc,
                        pqlk_stream_t stream);
int pqlk_dpg_backward_fused(const PqlMlpDesc* critic, const float* params, const float* x, int64_t ldx, int64_t b, const float* acts,
                            const float* qc, float* dz_a, int64_t ld_dz, int32_t dx_col0, const float* a_out, int64_t ld_tanh,
                            float* loss_part, float* critic_ws, int64_t critic_ws_floats, const PqlMlpDesc* actor,
                            const float* actor_params, const float* actor_acts, float* actor_ws, int64_t actor_ws_floats,
                            int32_t actor_splits, pqlk_stream_t stream);
int pqlk_mlp_backward_tail(const PqlMlpDesc* d, const float* params, const float* x, int64_t ldx, int64_t b, const float* acts,
                           float* grads, int32_t splits, float* ws, int64_t ws_floats, float* sumsq_part, int32_t* step_dev,
                           int32_t head_parts, const int32_t* head_parts_dev, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Losses.  Each writes dy (2, B, ld) for pqlk_mlp_backward and one scalar loss (device), via per-block
 * partials in `scratch` (>= 1024 floats) reduced in fixed order.  The scalar lands in
 * loss_out[slot_dev[0] % ring_len] when slot_dev != NULL (a device int32 counter, normally the optimiser's
 * step counter: gives a graph-replay-safe ring of the last `ring_len` losses, replacing the reference's
 * per-step `.item()` host sync, pql_v_learner.py:111), else in loss_out[0].  loss_out = NULL leaves the per-block
 * partials in scratch[0, pqlk_loss_parts(b, k)) for pqlk_adamw_polyak_fused to fold (one launch less).
 * ---------------------------------------------------------------------------------------------- */

/* TD target + twin MSE (pql_v_learner.py:104-108): y = r + (1-d) * gamma_n * min(qt1, qt2);
 * loss = mean((q1-y)^2) + mean((q2-y)^2).  q, qt: (2, B, ld) with the value in column 0. */
int pqlk_td_mse_loss(const float* q, const float* qt, int64_t ld, const float* rew, const float* done,
                     float gamma_n, int64_t b, float* dy, float* loss_out, const int32_t* slot_dev, int32_t ring_len,
                     float* scratch, pqlk_stream_t stream);

/* C51: softmax of target logits, categorical projection x2 (pql/utils/distl_util.py:4-20), elementwise
 * min (pql_v_learner.py:83-102), softmax of current logits, twin BCE (mean over B*K, log clamped at
 * -100 like torch) and its gradient w.r.t. the current logits.  logits: (2, B, ld), 2 <= K <= PQLK_C51_MAX_ATOMS atoms
 * (more: PQLK_E_UNSUPPORTED); dy's pad columns [K, ld) are written as zero;
 * support = DistributionalDoubleQ.z_atoms (mlp.py:253), passed in so its fp32 values are torch.linspace's.
 * If proj_out != NULL the (B, K) target pmf is also stored (tests); it changes no other output.
 *
 * Projection law, every K: per atom k, tz = clamp(r + ((1 - d) * gamma_n) * z_k, v_min, v_max), bpos = (tz - v_min) / dz with
 * dz = (v_max - v_min) / (K - 1) formed in double and rounded once, lo = floor(bpos), up = ceil(bpos), then
 * `if (up > 0 && lo == up) lo -= 1; if (lo < K - 1 && lo == up) up += 1;`, w_lo = p_k * (up - bpos), w_up = p_k * (bpos - lo),
 * in fp32 without contraction.  Bin j receives every w_lo with lo == j in increasing atom order, then every w_up with up == j
 * in increasing atom order, as one plain left-to-right fp32 sum: the order of the reference's two index_add_ passes.
 * Precondition for K > 64: support increasing, 0 <= done <= 1, gamma_n >= 0 (then lo and up are non-decreasing in k, which the
 * kernels for K > 64 rely on to find a bin's atoms; K <= 64 does not need it).  A non-finite reward can drop mass from a row at
 * any K; it never makes a kernel read or write out of bounds. */
#define PQLK_C51_MAX_ATOMS 256
int pqlk_c51_bce_loss(const float* logits, const float* logits_t, int64_t ld, int32_t k,
                      const float* rew, const float* done, const float* support /*(K) z atoms*/, float gamma_n,
                      float v_min, float v_max, int64_t b, float* dy, float* loss_out, const int32_t* slot_dev,
                      int32_t ring_len, float* proj_out, float* scratch, pqlk_stream_t stream);

/* Stand-alone projection = projection() of distl_util.py:4-20 on a given pmf (B, K) contiguous, 2 <= K <= PQLK_C51_MAX_ATOMS;
 * law and precondition as above. */
int pqlk_c51_project(const float* p, const float* rew, const float* done, const float* support, float gamma_n,
                     float v_min, float v_max, int32_t k, int64_t b, float* out, pqlk_stream_t stream);

/* DPG actor loss (pql_p_learner.py:56-57): L = -mean(min(Q1,Q2)); dy = dL/dQ (ties split evenly, as
 * torch.min's backward).  k == 1: q (2,B,ld) scalar heads.  k > 1: logits of the distributional critic,
 * Q_i = sum softmax(logits_i) * z (mlp.py:256-260), dy = gradient w.r.t. the logits, pad columns [K, ld) written as zero;
 * K <= PQLK_C51_MAX_ATOMS (more: PQLK_E_UNSUPPORTED). */
int pqlk_dpg_loss_owner(const float* q, int64_t ld, int32_t k, const float* support, int64_t b, float* dy, float* loss_out,
                        const int32_t* slot_dev, int32_t ring_len, float* scratch,
                        uint8_t* owner /* (B), k == 1: bit 0 / bit 1 = the gradient of min(Q1, Q2) reaches net 0 / net 1 */,
                        pqlk_stream_t stream);
int pqlk_dpg_loss(const float* q, int64_t ld, int32_t k, const float* support /*(K), NULL when k == 1*/, int64_t b,
                  float* dy, float* loss_out, const int32_t* slot_dev, int32_t ring_len, float* scratch,
                  pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Prioritized experience replay (Schaul et al. 2016, proportional variant) on a device sum tree.  The reference has no
 * prioritized replay; the formulas below are the paper's.
 *
 * `tree` is ONE flat fp32 device buffer of pqlk_per_tree_floats(capacity) floats, zeroed once by the caller, that holds a
 * radix-64 sum tree over the ring's rows:
 *     level 0    : n_0 = capacity leaves, leaf r = priority_r ^ alpha (0 for a row never written);
 *     level l + 1: n_{l+1} = ceil(n_l / 64) nodes, node j = the sum of nodes [64 j, 64 j + 64) of level l;
 *     levels go on until one has at most 64 nodes: pqlk_per_levels(capacity) of them (5 000 000 rows: 4); the total is the sum
 *     of that top level, formed where it is needed and stored nowhere.
 * Every level is padded with zeros to a multiple of 64 floats and the levels lie one after the other, level 0 first:
 * pqlk_per_tree_floats = sum_l roundup(n_l, 64).  Pads are never written.  Every sum of 64 is one wave's xor-butterfly (offsets
 * 32, 16, 8, 4, 2, 1; pql_amd/csrc/per.hip's header writes the association out), so the upper levels after any sequence of
 * calls are a pure function of the leaves: pqlk_per_rebuild of the same leaves gives the same bits.
 * `pmax` is one device float beside the tree: the largest priority ever assigned, before ^alpha; the caller sets it to 1 once.
 * x ^ e below means: e == 0 -> 1, e == 1 -> x, e == -1 -> 1.0f / x (one IEEE division), e == 0.5 -> sqrtf(x), else powf(x, e).
 * Errors, before any launch: PQLK_E_NULL a NULL pointer; PQLK_E_SHAPE capacity <= 0, m <= 0, b <= 0 or n_valid <= 0;
 * PQLK_E_RANGE dst_start < 0, dst_start + m > capacity or n_valid > capacity.  An index outside [0, capacity) in `idx` is
 * skipped by the kernels (weight 0), never dereferenced.  No float atomic adds anywhere: results are bitwise reproducible.
 * ---------------------------------------------------------------------------------------------- */
int32_t pqlk_per_levels(int64_t capacity);       /* 0 for capacity <= 0.  Host only: no GPU needed. */
int64_t pqlk_per_tree_floats(int64_t capacity);  /* 0 for capacity <= 0.  Host only. */

/* New rows enter with the largest priority seen so far (Schaul et al., algorithm 1 line 6: p_t = max_{i<t} p_i):
 * leaf[r] = pmax ^ alpha for r in [dst_start, dst_start + m), pmax read on the device; then every ancestor of that range is
 * recomputed, one launch per level.  One call per ring_plan segment, like pqlk_replay_insert. */
int pqlk_per_insert(float* tree, int64_t capacity, const float* pmax, int64_t dst_start, int64_t m, float alpha,
                    pqlk_stream_t stream);

/* Every node of every upper level from its 64 children, bottom up (node j of level l + 1 = sum of level l's [64 j, 64 j + 64)). */
int pqlk_per_rebuild(float* tree, int64_t capacity, pqlk_stream_t stream);

/* Stratified proportional sampling (Schaul et al. 3.3 / appendix B.2.1: P(i) = p_i^alpha / sum_k p_k^alpha, one draw from each
 * of b equal segments of the total mass).  u: b floats in [0, 1).  Sample k, one wave: seg = total / (float)b,
 * t_k = ((float)k + u[k]) * seg; residual = t_k; from the top level down, lane j loads child j of the current node (at the top:
 * node j of the top level), an inclusive prefix over the 64 lanes is formed (Hillis-Steele: for d = 1, 2, 4, 8, 16, 32,
 * lane j >= d adds lane j - d's value of the previous round), the chosen child is the first with a non-zero sum whose inclusive
 * prefix exceeds the residual, or, when rounding leaves none, the last child with a non-zero sum; the residual drops by the
 * chosen child's exclusive prefix.  idx_out[k] (int64) = the leaf reached: never a row whose leaf is 0 while total > 0. */
int pqlk_per_sample(const float* tree, int64_t capacity, const float* u, int64_t b, int64_t* idx_out, pqlk_stream_t stream);

/* Importance weights (Schaul et al. 3.4: w_i = (N P(i))^-beta, normalised by the batch maximum where they are used):
 * w_out[i] = (((float)n_valid * leaf[idx[i]]) / total) ^ (-beta); wmax_out[0] = max_i w_out[i], taken with an integer atomic
 * max on the bit patterns of the non-negative floats (wmax_out is zeroed on the stream first).  beta == 0: exactly 1.0. */
int pqlk_per_weights(const float* tree, int64_t capacity, const int64_t* idx, int64_t b, int64_t n_valid, float beta,
                     float* w_out, float* wmax_out, pqlk_stream_t stream);

/* pqlk_per_sample and pqlk_per_weights for `steps` batches of b in ONE launch, all on the tree as it stands (the PQL V-learner's
 * run of steps between two hand-offs: the distribution is frozen for the run).  r: steps * b integers in [0, 2^24)
 * (torch.randint(1 << 24) draws).  Step s, sample k, one wave: u = (float)r[s b + k] * 2^-24 (exact); then pqlk_per_sample's walk
 * for stratum k of b -- seg = total / (float)b, t = ((float)k + u) * seg, the same prefix, ballot and choice of child -- and
 * pqlk_per_weights' w = (((float)n_valid * leaf) / total) ^ (-beta) on the leaf value the wave loaded at level 0, with the same
 * total and the same x ^ e.  idx_out, w_out: steps * b entries, step-major.  wmax_out: `steps` floats, wmax_out[s] = the maximum
 * of step s's b weights (integer atomic max on the bit patterns; steps * 4 bytes are zeroed on the stream first).  Bit-equal, on
 * one device, to `steps` pairs of pqlk_per_sample (given u) and pqlk_per_weights.  Errors, before any launch: PQLK_E_NULL a NULL
 * pointer; PQLK_E_SHAPE capacity, b, steps or n_valid <= 0, or steps > 65535; PQLK_E_RANGE n_valid > capacity. */
int pqlk_per_sample_steps(const float* tree, int64_t capacity, const int64_t* r, int64_t b, int64_t steps, int64_t n_valid,
                          float beta, int64_t* idx_out, float* w_out, float* wmax_out, pqlk_stream_t stream);

/* pqlk_td_mse_loss with the per-sample weight wh_i = w[i] / wmax[0] (Schaul et al. algorithm 1 lines 10-12):
 * loss = mean(wh (q1-y)^2) + mean(wh (q2-y)^2), dy = ((2/B) wh) (q-y), abs_td_out[i] = max(|q1-y|, |q2-y|) (the new priority,
 * before eps and ^alpha).  Grid, partials, fold order and loss-ring semantics are pqlk_td_mse_loss's; with every w and wmax 1.0
 * dy and the loss are its bits. */
int pqlk_td_mse_loss_per(const float* q, const float* qt, int64_t ld, const float* rew, const float* done, float gamma_n,
                         int64_t b, float* dy, float* loss_out, const int32_t* slot_dev, int32_t ring_len, float* scratch,
                         const float* w, const float* wmax, float* abs_td_out, pqlk_stream_t stream);

/* Priority write-back (Schaul et al. algorithm 1 line 11, proportional: p_i = |delta_i| + eps):
 * leaf[idx[i]] = (abs_td[i] + eps) ^ alpha; pmax = max(pmax, max_i(abs_td[i] + eps)); then every touched ancestor is recomputed
 * from its 64 children, one launch per level (recomputed redundantly, a node gets identical bits).  A row drawn more than once ends
 * with the largest of its candidates whatever order the threads run in: the sampled leaves are cleared in one launch and raised
 * with an integer atomic max on the bit pattern in the next.  abs_td >= 0. */
int pqlk_per_update(float* tree, int64_t capacity, float* pmax, const int64_t* idx, const float* abs_td, int64_t b, float eps,
                    float alpha, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Quantile-regression twin critic (QR-DQN, Dabney et al. 2018).  The reference has no such critic; the formulas below are the
 * paper's, adapted to twin critics.  No support, no projection, no v_min / v_max: a head learns the locations of N quantiles of
 * fixed probability.
 *
 * Inputs.  N = n quantiles, 2 <= N <= PQLK_QR_MAX_QUANTILES; kappa > 0, the Huber threshold; tau_j = (2 j + 1) / (2 N), formed
 * in fp32 as (float)(2 j + 1) / (float)(2 N).  theta: the current heads, (2, B, ld) with quantile j in column j, ld = pqlk_ld(N)
 * (any multiple of 32 >= N is taken); theta_t: the target heads, same layout.
 * Target net.  S_i = sum_j theta_t[i, b, j], one wave butterfly over 64 lanes (offsets 32, 16, 8, 4, 2, 1; lanes >= N hold 0).
 * i* = 1 if S_1 < S_0, else 0: a tie takes net 0.  Clipped double-Q at the level of the means: one choice per row, no sorting.
 * Target quantiles.  T_k = r + ((1 - d) * gamma_n) * theta_t[i*, b, k], in this order (pqlk_td_mse_loss's).
 * Loss.  u_ijk = T_k - theta[i, b, j];  rho(u; tau) = |tau - 1{u < 0}| * H(u) / kappa;  H(u) = 0.5 u^2 for |u| <= kappa, else
 * kappa (|u| - 0.5 kappa);  L = sum_i (1 / (B N)) sum_{b, j, k} rho(u_ijk; tau_j): the paper's sum over current quantiles and mean
 * over target quantiles, then a batch mean, then the twin nets added.  Per (i, b, j) the k terms |tau_j - 1{u < 0}| * H(u) are
 * added in increasing k; per (b, j) the two nets' sums are added and divided by kappa once.  Each per-block partial is a plain sum
 * of these; the fold scale is 1 / (B N), formed as 1.0f / ((float)B * (float)N): the convention of pqlk_loss_parts(b, k > 1).
 * Gradient.  dy[i, b, j] = -(1 / (B N)) * sum_k |tau_j - 1{u_ijk < 0}| * clamp(u_ijk, -kappa, kappa) / kappa: the k terms
 * |tau_j - 1{u < 0}| * clamp(u) are added in increasing k, the sum is divided by kappa, multiplied by 1 / (B N) and negated.
 * Pad columns [N, ld) of dy are written as zero.
 * Prioritized variant (_per).  wh = w[b] / wmax[0] multiplies the row's loss terms ((l_0 + l_1) / kappa, before it joins the
 * partial) and the row's dy (before the negation); abs_td_out[b] = max_i |mean_k T_k - mean_j theta[i, b, j]|, each mean a wave
 * butterfly times 1.0f / (float)N.  The plain entry never reads w, wmax or abs_td_out; with every w and wmax 1.0 the weighted one
 * gives its bits.
 * DPG.  Q_i = (sum_j theta[i, b, j]) * (1 / N);  L = -(1 / B) sum_b min(Q_0, Q_1);  dy[i, b, j] = -share_i / (B N), share_i = 1
 * for the smaller net and 0 for the other, 0.5 each on a tie (torch.min's backward, as pqlk_dpg_loss); pad columns zero.
 *
 * loss_out / slot_dev / ring_len / scratch: as for every loss above; loss_out = NULL leaves pqlk_loss_parts(b, n) partials in
 * scratch.  No float atomics, every reduction in a fixed order: two launches on the same inputs give the same bits.
 * Errors, before any launch: PQLK_E_NULL a NULL pointer; PQLK_E_SHAPE b <= 0, kappa <= 0 or a ring without a length;
 * PQLK_E_UNSUPPORTED n < 2 or n > PQLK_QR_MAX_QUANTILES; PQLK_E_ALIGN ld not a multiple of 32 or ld < n.
 * ---------------------------------------------------------------------------------------------- */
#define PQLK_QR_MAX_QUANTILES 64
int pqlk_qr_huber_loss(const float* theta, const float* theta_t, int64_t ld, int32_t n, const float* rew, const float* done,
                       float gamma_n, float kappa, int64_t b, float* dy, float* loss_out, const int32_t* slot_dev,
                       int32_t ring_len, float* scratch, pqlk_stream_t stream);
int pqlk_qr_huber_loss_per(const float* theta, const float* theta_t, int64_t ld, int32_t n, const float* rew, const float* done,
                           float gamma_n, float kappa, int64_t b, float* dy, float* loss_out, const int32_t* slot_dev,
                           int32_t ring_len, float* scratch, const float* w, const float* wmax, float* abs_td_out,
                           pqlk_stream_t stream);
int pqlk_dpg_loss_quantile(const float* theta, int64_t ld, int32_t n, int64_t b, float* dy, float* loss_out,
                           const int32_t* slot_dev, int32_t ring_len, float* scratch, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Truncated pooled targets for the quantile twin critic (TQC, Kuznetsov et al. 2020).  The reference has no such critic; the law
 * is the paper's, adapted to twin heads, in the conventions of the block above: N, kappa, tau_j, theta, theta_t, ld as there;
 * drop = d, 0 <= d <= N - 1, the atoms dropped per net; M = 2 (N - d) of the 2 N pooled atoms are kept; c = (1 - done_b) * gamma_n.
 * Pool.  p = i * N + k for target net i and quantile k;  z_p = theta_t[i, b, k].
 * Rank.  rank(p) = #{q : z_q < z_p} + #{q < p : z_q = z_p}: on the raw theta_t (comparisons only, no rounding); ties are broken
 * by the pool index, so the ranks are a permutation of 0 ... 2 N - 1 whatever the values, also on a row with done = 1, whose
 * targets are all equal.  Inputs are finite.
 * Kept set.  Atom p is kept iff rank(p) < M: the M smallest, the largest 2 d are dropped.  d = 0 keeps all atoms of both nets
 * (which is not the law above: that one takes one whole net per row).
 * Targets.  T_p = r + c * z_p, formed as r + ((1 - d) * gamma_n) * z_p (pqlk_td_mse_loss's order).
 * Loss.  u_ijp = T_p - theta[i, b, j];  L = sum_i (1 / (B M)) sum_{b, j, kept p} rho(u_ijp; tau_j), rho and H as above.  Per
 * (i, b, j) the terms |tau_j - 1{u < 0}| * H(u) of the kept atoms are added in increasing pool index p (dropped atoms skipped);
 * per (b, j) the two nets' sums are added and divided by kappa once.  Each per-block partial is a plain sum of these; the fold
 * scale is 1 / (B M), formed as 1.0f / ((float)B * (float)M).  The partial count stays pqlk_loss_parts(b, n).
 * Gradient.  dy[i, b, j] = -(1 / (B M)) * sum_{kept p} |tau_j - 1{u_ijp < 0}| * clamp(u_ijp, -kappa, kappa) / kappa: the terms
 * added in increasing p, dropped atoms skipped; the sum is divided by kappa, multiplied by 1 / (B M) and negated.  Pad columns
 * [N, ld) of dy are written as zero.
 * Prioritized variant (_per).  wh = w[b] / wmax[0] multiplies the row's loss terms and the row's dy, as above;
 * abs_td_out[b] = max_i |mean_{kept p} T_p - mean_j theta[i, b, j]|: the first mean is a wave butterfly over the per-lane sums
 * (T_k if kept, else 0) + (T_{N + k} if kept, else 0), times 1.0f / (float)M; the second as above.  With every w and wmax 1.0 the
 * weighted entry gives the plain one's bits.
 * The actor's loss stays pqlk_dpg_loss_quantile.
 *
 * loss_out / slot_dev / ring_len / scratch, determinism: as above.  Errors, before any launch: those of pqlk_qr_huber_loss, and
 * PQLK_E_SHAPE drop < 0 or drop >= n (checked after n's own range).
 * ---------------------------------------------------------------------------------------------- */
int pqlk_tqc_huber_loss(const float* theta, const float* theta_t, int64_t ld, int32_t n, const float* rew, const float* done,
                        float gamma_n, float kappa, int64_t b, float* dy, float* loss_out, const int32_t* slot_dev,
                        int32_t ring_len, float* scratch, int32_t drop, pqlk_stream_t stream);
int pqlk_tqc_huber_loss_per(const float* theta, const float* theta_t, int64_t ld, int32_t n, const float* rew, const float* done,
                            float gamma_n, float kappa, int64_t b, float* dy, float* loss_out, const int32_t* slot_dev,
                            int32_t ring_len, float* scratch, const float* w, const float* wmax, float* abs_td_out, int32_t drop,
                            pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * TQC as the paper defines it: a maximum-entropy actor-critic on the truncated pooled target (algo=tqc_algo).  Notation of the
 * block above: N, kappa, tau_j, theta, theta_t, d, M = 2 (N - d), pool index p = i * N + k, z_p = theta_t[i, b, k],
 * c = (1 - done_b) * gamma_n.  logp: (B,), log pi(a'_b | s'_b) of the next action the target heads were evaluated at; log_alpha:
 * (1,), the log of the temperature, read on the device.
 *
 * Soft truncated target (pqlk_tqc_huber_loss_soft, pqlk_tqc_huber_loss_soft_per).
 * Shift.  s_b = alpha * logp[b], alpha = expf(log_alpha[0]): pqlk_sac_entropy_shift's expression, one fp32 product.
 * Rank, kept set.  Those of the block above, computed on the RAW theta_t.  The shift is the same for every atom of a row, so in
 * real arithmetic it changes no order; ranking the raw atoms means that rounding after the shift can never create or break a tie.
 * Targets.  T_p = r + c * (z_p - s_b), in this order: the subtraction, the product with c = fl((1 - d) * gamma_n), the addition;
 * no contraction, each step rounds.  The entropy bonus sits inside every target atom; on a row with done = 1 every T_p is r.
 * Loss, gradient, pad columns, the fold scale 1.0f / ((float)B * (float)M), the prioritized weighting wh = w[b] / wmax[0]: as
 * above, with these T_p.  abs_td_out[b] = max_i |mean_{kept p} T_p - mean_j theta[i, b, j]| with the soft T_p.
 * With logp = 0 everywhere the entries give the bits of pqlk_tqc_huber_loss{,_per}, whatever log_alpha (z - 0 = z); with every w
 * and wmax 1.0 the weighted entry gives the plain one's bits.  The shift rides in the loss launch: the target heads are not
 * rewritten, and a critic step has the launch count of the one above.
 *
 * Mean-of-critics actor objective (pqlk_dpg_loss_quantile_mean; arguments of pqlk_dpg_loss_quantile).
 * Qbar_b = (1 / (2 N)) sum_i sum_j theta[i, b, j]: per lane j theta[0, b, j] + theta[1, b, j], one wave butterfly, times
 * 1.0f / (float)(2 N).  L_q = -(1 / B) sum_b Qbar_b: lane 0 adds Qbar_b to the block's partial, the fold scale is -1 / B.
 * dy[i, b, j] = -(1.0f / ((float)B * (float)(2 * N))) for j < N, pad columns [N, ld) zero: no min, so no share and no tie rule.
 * The agent's actor loss is L_q + alpha * mean_b logp_b: the second term is added to the ring by pqlk_sac_alpha_terms, and the
 * gradient reaches the policy head through pqlk_sg_head_backward with glp_scale = 1 / B, as in SAC.
 *
 * Errors, before any launch: those of pqlk_tqc_huber_loss{,_per} and of pqlk_dpg_loss_quantile; PQLK_E_NULL for logp or
 * log_alpha NULL.  No float atomics; two launches on the same inputs give the same bits.
 * ---------------------------------------------------------------------------------------------- */
int pqlk_tqc_huber_loss_soft(const float* theta, const float* theta_t, int64_t ld, int32_t n, const float* rew, const float* done,
                             float gamma_n, float kappa, int64_t b, float* dy, float* loss_out, const int32_t* slot_dev,
                             int32_t ring_len, float* scratch, const float* logp, const float* log_alpha, int32_t drop,
                             pqlk_stream_t stream);
int pqlk_tqc_huber_loss_soft_per(const float* theta, const float* theta_t, int64_t ld, int32_t n, const float* rew,
                                 const float* done, float gamma_n, float kappa, int64_t b, float* dy, float* loss_out,
                                 const int32_t* slot_dev, int32_t ring_len, float* scratch, const float* w, const float* wmax,
                                 float* abs_td_out, const float* logp, const float* log_alpha, int32_t drop, pqlk_stream_t stream);
int pqlk_dpg_loss_quantile_mean(const float* theta, int64_t ld, int32_t n, int64_t b, float* dy, float* loss_out,
                                const int32_t* slot_dev, int32_t ring_len, float* scratch, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * HL-Gauss loss for the categorical twin critic (Farebrother et al. 2024, "Stop regressing").  The reference has no such loss; the
 * formulas below are the paper's, adapted to twin critics and clipped double-Q.  Network, support, layout and the actor's loss
 * (pqlk_dpg_loss with k > 1) are those of pqlk_c51_bce_loss: logits, logits_t (2, B, ld), 2 <= K <= PQLK_C51_MAX_ATOMS atoms,
 * support = z (K).  Every operation is fp32 without contraction unless stated.
 *
 * Target value.  For each target net i: P = softmax(logits_t[i, b, :K]) and E_i = sum_k P_k z_k (the softmax and the dot product
 * of pqlk_dpg_loss: per lane over its atoms lane + 64 j in increasing j, then a wave butterfly).
 * y = r + ((1 - d) * gamma_n) * fminf(E_0, E_1), in this order (pqlk_td_mse_loss's); then y = fminf(fmaxf(y, v_min), v_max).
 * Bins.  dz = (v_max - v_min) / (K - 1), formed in double and rounded once, as in C51.  Edge e_k = v_min + ((float)k - 0.5f) * dz
 * for k = 0 ... K.  inv = (float)(1.0 / ((double)sigma_ratio * (double)dz * sqrt(2.0))), formed in double on the host from the
 * fp32 sigma_ratio and the rounded fp32 dz: 1 / (sigma sqrt 2) with sigma = sigma_ratio bin widths.  u_k = (e_k - y) * inv.
 * c(u) = 1 if u >= 4, -1 if u <= -4, else erff(u): what a correctly rounded erf returns there, so that the saturated bits do not
 * depend on the math library.
 * Target pmf.  t_k = (c(u_{k+1}) - c(u_k)) / (c(u_K) - c(u_0)): the mass of N(y, sigma^2) in bin k over its mass on the support.
 * Each lane evaluates its own two edges and the two outer ones; there is no cross-lane sum in the target.
 * Loss.  Per net i: m = max_k x_k, s = sum_k expf(x_k - m), lse = m + logf(s) with x = logits[i, b, :K] (the reduction order of the
 * softmax above); l_ib = sum_k t_k * (lse - x_k), where a term with t_k == 0 contributes 0 (per lane in increasing j, then a wave
 * butterfly).  The row adds wh * (l_0b + l_1b) to its block's partial (wh = 1: l_0b + l_1b); the fold scale is 1 / B, formed as
 * 1.0f / (float)B -- not C51's 1 / (B K).  The partial count stays pqlk_loss_parts(b, k).
 * Gradient.  dy[i, b, k] = (wh * (1 / B)) * (p_k - t_k) with p_k = expf(x_k - m) / s; pad columns [K, ld) are written as zero.
 * Prioritized variant (_per).  wh = w[b] / wmax[0]; abs_td_out[b] = max_i |sum_k p_ik z_k - y|.  The plain entry never reads w,
 * wmax or abs_td_out; with every w and wmax 1.0 the weighted entry gives its bits.
 * target_out: optional (B, K), receives t (tests); it changes no other output.
 * Non-finite inputs.  A row whose reward, done flag or any of whose 4 K logits is not finite takes y = NaN: its dy, its target_out,
 * its abs_td_out and the loss are NaN.  No value ever becomes an address: such a row cannot make a kernel read or write out of
 * bounds.
 *
 * loss_out / slot_dev / ring_len / scratch: as for every loss above.  No float atomics, every reduction in a fixed order: two
 * launches on the same inputs give the same bits.
 * Errors, before any launch: PQLK_E_NULL a NULL pointer; PQLK_E_SHAPE b <= 0, k < 2, sigma_ratio not > 0, v_max <= v_min or a ring
 * without a length; PQLK_E_UNSUPPORTED k > PQLK_C51_MAX_ATOMS; PQLK_E_ALIGN ld not a multiple of 32 or ld < k.
 * ---------------------------------------------------------------------------------------------- */
int pqlk_hlgauss_ce_loss(const float* logits, const float* logits_t, int64_t ld, int32_t k, const float* rew, const float* done,
                         const float* support /*(K) z atoms*/, float gamma_n, float v_min, float v_max, float sigma_ratio, int64_t b,
                         float* dy, float* loss_out, const int32_t* slot_dev, int32_t ring_len, float* target_out, float* scratch,
                         pqlk_stream_t stream);
int pqlk_hlgauss_ce_loss_per(const float* logits, const float* logits_t, int64_t ld, int32_t k, const float* rew, const float* done,
                             const float* support, float gamma_n, float v_min, float v_max, float sigma_ratio, int64_t b, float* dy,
                             float* loss_out, const int32_t* slot_dev, int32_t ring_len, float* target_out, float* scratch,
                             const float* w, const float* wmax, float* abs_td_out, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Critic diagnostics (opt-in, algo.diag.enabled; the reference logs none).  Read-only on every input; no gradient, no loss.
 *
 * pqlk_critic_stats.  q: the twin heads' output, qt: the target heads' output, both (2, B, ld) as the loss entries take them.
 * head / k: PQLK_HEAD_SCALAR with k = 1; PQLK_HEAD_CATEGORICAL with 2 <= k <= PQLK_C51_MAX_ATOMS, z_atoms (k), v_min < v_max;
 * PQLK_HEAD_QUANTILE with 2 <= k <= PQLK_QR_MAX_QUANTILES (z_atoms, v_min, v_max are not looked at off the categorical head).
 * Every operation is fp32 without contraction.
 * Row value V_i of net i (V'_i: of target net i, the same law on qt):
 *   scalar       column 0;
 *   categorical  E_i[z] = sum_k P_k z_k, P = softmax(q[i, b, :k]): the softmax and the dot product of pqlk_dpg_loss and
 *                pqlk_hlgauss_ce_loss (per lane over its atoms lane + 64 j in increasing j, then a wave butterfly): their bits;
 *   quantile     (sum_j q[i, b, j]) * (1.0f / (float)k), the sum a wave butterfly over the 64 lanes (lanes >= k hold 0): the Q of
 *                pqlk_dpg_loss_quantile.
 * Target: y = r + ((1 - d) * gamma_n) * fminf(V'_0, V'_1), in this order (pqlk_td_mse_loss's).  On the categorical head y is then
 * clamped, fminf(fmaxf(y, v_min), v_max) as pqlk_hlgauss_ce_loss does, except that a NaN stays a NaN.
 * out[0 .. PQLK_CRITIC_STATS), over the B rows:
 *   0 mean V_0    1 mean V_1    2 min of fminf(V_0, V_1)    3 max of fmaxf(V_0, V_1)    4 mean y
 *   5 mean of (V_0 + V_1) * 0.5f - y (bias)       6 mean of td = fmaxf(fabsf(V_0 - y), fabsf(V_1 - y))       7 max of td
 *   8 mean of fabsf(V_0 - V_1) (twin gap)         9 the number of rows where V_0, V_1 or the unclamped y is not finite, as a float
 *                                                   (exact below 2^24 rows)
 * A mean is the sum times 1.0f / (float)B -- one multiplication by the rounded reciprocal, the fold scale of the loss entries -- and
 * the sums start from 0.f.  Non-finite values are not filtered out of the sums: they propagate into the means; out[9] says how many
 * rows carried them.  The min and the max are fminf / fmaxf folds from +inf / -inf: they keep an infinity and drop a NaN operand.
 * Geometry: pqlk_loss_parts(b, k) blocks, as the loss entries (scalar: one row per thread, 256 per block; wider heads: one wave per
 * row, four per block; a row loop above 1024 blocks); PQLK_CRITIC_STATS partials per block in scratch, folded by a second launch of
 * one block: per thread a chain over blocks t, t + 256, ..., a wave butterfly, the four waves as (w0 + w1) + (w2 + w3).  No float
 * atomics: two calls on the same inputs give the same bits.
 * scratch: >= pqlk_critic_stats_scratch_floats(b, k) floats (PQLK_CRITIC_STATS * pqlk_loss_parts(b, k)).
 * Errors, before any launch: PQLK_E_NULL a NULL q, qt, rew, done, out, scratch, or z_atoms on the categorical head; PQLK_E_UNSUPPORTED
 * an unknown head or k above the head's maximum; PQLK_E_SHAPE b <= 0, k != 1 on the scalar head, k < 2 on the others, v_max <= v_min
 * on the categorical head; PQLK_E_ALIGN ld < 32, ld not a multiple of 32 or ld < k.
 *
 * pqlk_unit_stats.  h (rows, ld): one layer's post-ELU activations with `cols` valid columns (a stash block addressed through
 * pqlk_mlp_act_offset, or a per-layer critic's own matrix); columns >= cols are never read.  0 <= tau < 1.
 *   a_c = (sum_r fabsf(h[r, c])) / (float)rows;   A = (sum_c a_c) / (float)cols;   unit c is dormant iff a_c <= tau * A
 *   (Sokar et al. 2023, "The dormant neuron phenomenon"; tau * A one fp32 product);   s(x) = x > 0 ? 1 : x + 1 (ELU' from ELU's output)
 *   out[0] = (number of dormant units) / (float)cols      out[1] = A      out[2] = (sum_c sum_r s(h[r, c])) / ((float)rows * (float)cols)
 * Order of the sums: rows are cut into min(rows, PQLK_UNIT_CHUNKS) chunks of ceil(rows / chunks) consecutive rows; within a chunk wave
 * w of the block adds rows w, w + 4, ... of its column, the four waves join as (w0 + w1) + (w2 + w3); a second launch of one block
 * adds a column's chunks in index order; thread t of it then adds its columns t, t + 256, ... in increasing c (a_c and the slope sums
 * alike), and the 256 threads join by a wave butterfly and (w0 + w1) + (w2 + w3).  No float atomics.
 * scratch: >= pqlk_unit_stats_scratch_floats(cols) floats ((2 * PQLK_UNIT_CHUNKS + 1) * cols).
 * Errors, before any launch: PQLK_E_NULL a NULL h, out or scratch; PQLK_E_SHAPE rows <= 0, cols <= 0, ld < cols, or tau outside
 * [0, 1) (a NaN included).
 * ---------------------------------------------------------------------------------------------- */
#define PQLK_CRITIC_STATS 10
#define PQLK_UNIT_CHUNKS 64
enum { PQLK_HEAD_SCALAR = 0, PQLK_HEAD_CATEGORICAL = 1, PQLK_HEAD_QUANTILE = 2 };
int64_t pqlk_critic_stats_scratch_floats(int64_t b, int32_t k);   /* 0 for b <= 0 or k < 1.  Host only. */
int pqlk_critic_stats(const float* q, const float* qt, int64_t ld, int32_t head, int32_t k, const float* z_atoms, float v_min,
                      float v_max, const float* rew, const float* done, float gamma_n, int64_t b, float* out, float* scratch,
                      pqlk_stream_t stream);
int64_t pqlk_unit_stats_scratch_floats(int32_t cols);             /* 0 for cols <= 0.  Host only. */
int pqlk_unit_stats(const float* h, int64_t ld, int64_t rows, int32_t cols, float tau, float* out, float* scratch,
                    pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Optimiser: clip_grad_norm_ + AdamW (+ Polyak) over flat arenas
 * (pql_v_learner.py:124-133, pql_p_learner.py:87-96, pql/utils/torch_util.py:9-12).
 *   g *= grad_scale   (1/world_size after a data-parallel sum all-reduce; 1.0 otherwise)
 *   total = ||g||_2 ; g *= min(1, max_norm / (total + 1e-6))   (max_norm <= 0 disables clipping)
 *   p *= 1 - lr*wd ; m += (g-m)(1-b1) ; v = b2 v + (1-b2) g^2
 *   p -= (lr / (1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 *   target = p*tau + target*(1-tau)                              (target may be NULL)
 * lr, b1, b2, eps, wd, tau are doubles, as torch holds them: 1 - b2, 1 - lr*wd, 1 - tau and the bias corrections are
 * formed in double and rounded once.
 * step_dev: device int32 counter t, incremented by the call (graph-replay safe).
 * scratch: >= 2048 floats.  gnorm_out (device, may be NULL) receives the pre-clip norm.
 * ---------------------------------------------------------------------------------------------- */
int pqlk_clip_adamw_polyak(float* p, float* g, float* m, float* v, float* target, int64_t n, float grad_scale,
                           float max_norm, double lr, double b1, double b2, double eps, double wd, double tau,
                           int32_t* step_dev, float* gnorm_out, float* scratch, pqlk_stream_t stream);

/* Same update for the arena of the MLP `d`, which ALSO refreshes the fragment-ordered weight copies of the fused
 * forward path while each new value is in a register (packed_p for the parameters, packed_t -- may be NULL -- for the
 * Polyak target), replacing the separate pqlk_mlp_pack launches. */
int pqlk_clip_adamw_polyak_pack(const PqlMlpDesc* d, float* p, float* g, float* m, float* v, float* target,
                                float* packed_p, float* packed_t, float grad_scale, float max_norm, double lr, double b1,
                                double b2, double eps, double wd, double tau, int32_t* step_dev, float* gnorm_out,
                                float* scratch, pqlk_stream_t stream);

/* The optimiser launch of a fused learner step (pql_v_learner.py:124-133 + :109-111, pql_p_learner.py:87-96): the same
 * update as pqlk_clip_adamw_polyak_pack (packed_p may be NULL: nothing to re-pack), plus
 *   prenorm > 0  : `scratch` already holds that many squared-norm partials and step_dev is already incremented (both left
 *                  by pqlk_mlp_backward_norm; prenorm = pqlk_mlp_norm_parts(d)), so no separate norm launch;
 *   loss_part    : per-block loss partials left in a loss kernel's scratch (pqlk_td_mse_loss / pqlk_c51_bce_loss /
 *                  pqlk_dpg_loss called with loss_out = NULL; count = pqlk_loss_parts(b, k)): block 0 folds them, times
 *                  loss_scale (1/B, 1/(B K), -1/B), into loss_ring[(t - 1) % ring_len], t = the incremented step --
 *                  the slot and the bits the stand-alone fold writes.  NULL = no fold. */
int pqlk_adamw_polyak_fused(const PqlMlpDesc* d, float* p, float* g, float* m, float* v, float* target,
                            float* packed_p, float* packed_t, float grad_scale, float max_norm, double lr, double b1,
                            double b2, double eps, double wd, double tau, int32_t* step_dev, float* gnorm_out,
                            float* scratch, int32_t prenorm, const float* loss_part, int32_t loss_parts,
                            float loss_scale, float* loss_ring, int32_t ring_len, pqlk_stream_t stream);
/* Number of per-block partials a loss entry point leaves in `scratch` (k = atoms; 1 for scalar heads). */
int32_t pqlk_loss_parts(int64_t b, int32_t k);

/* soft_update alone (torch_util.py:9-12): target = cur*tau + target*(1-tau). */
int pqlk_polyak(float* target, const float* cur, int64_t n, float tau, pqlk_stream_t stream);

/* RunningMeanStd.update batch moments (torch_util.py:77-81): mean and UNBIASED variance over rows of
 * x (N, ldx) for `cols` columns -> mean_out, var_out (cols).  The Chan merge (:87-103) stays on host.
 * scratch: >= 64 * cols * 3 floats (per-chunk count / mean / M2). */
int pqlk_batch_moments(const float* x, int64_t ldx, int64_t n, int32_t cols, float* mean_out, float* var_out,
                       float* scratch, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * SAC on the same kernels (reference pql/algo/sac.py:138-156, pql/models/mlp.py:144-174,
 * pql/utils/torch_util.py:15-65).
 *
 * Squashed-Gaussian policy head.  y (B, ld_y) = [ mu(A) | log_std(A) | pad ] is the policy MLP's output
 * (pqlk_mlp_forward with PQLK_ACT_NONE), eps (B, A) contiguous the standard-normal draw of Normal.rsample:
 *     std = exp(clamp(log_std, -5, 5));  u = mu + eps * std;  a = tanh(u)
 *     logp = sum_j [ -((u - mu)^2) / (2 std^2) - log(std) - log(sqrt(2 pi)) - 2 (log 2 - u - softplus(-2u)) ]
 * act (B, ld_act) receives a in columns [0, A) (pass a pointer into the critic's [obs | action] tile); logp (B).
 * eps == NULL => the deterministic action tanh(mu) (get_actions(sample=False)); logp is not written.  A <= 64. */
int pqlk_sg_head_forward(const float* y, int64_t ld_y, const float* eps, int64_t b, int32_t act_dim,
                         float* act, int64_t ld_act, float* logp, pqlk_stream_t stream);

/* Backward of the head: dy (B, ld_y) <- d loss / d [mu | log_std] (pad columns written as zero) given
 * da (B, ld_da) = d loss / d a and d loss / d logp = glp_scale * exp(*log_alpha) for every row
 * (log_alpha: device scalar, NULL => factor 1).  dy feeds pqlk_mlp_backward of the policy MLP. */
int pqlk_sg_head_backward(const float* y, int64_t ld_y, const float* eps, const float* act, int64_t ld_act,
                          const float* da, int64_t ld_da, const float* log_alpha, float glp_scale,
                          int64_t b, int32_t act_dim, float* dy, pqlk_stream_t stream);

/* Entropy term of the SAC target (sac.py:140-142): column 0 of each target-critic net,
 * qt[n * net_stride + r * ld] -= exp(*log_alpha) * logp[r]; pqlk_td_mse_loss then forms
 * r + (1 - d) gamma^n (min(q1, q2) - alpha logp). */
int pqlk_sac_entropy_shift(float* qt, int64_t ld, int64_t net_stride, int32_t n_nets, const float* logp,
                           const float* log_alpha, int64_t b, pqlk_stream_t stream);

/* Temperature terms (sac.py:146-156), one launch: with m = mean(logp) and alpha = exp(*log_alpha),
 *   grad_out[0] = alpha_loss_out[0] = alpha * (-m - target_entropy)   (the alpha loss and its gradient w.r.t. log_alpha
 *                                                                      have the same value; either may be NULL)
 *   actor_loss_ring[*slot_dev % ring_len] += alpha * m                (completes mean(alpha logp - Q) after pqlk_dpg_loss) */
int pqlk_sac_alpha_terms(const float* logp, int64_t b, const float* log_alpha, float target_entropy,
                         float* grad_out, float* alpha_loss_out, float* actor_loss_ring,
                         const int32_t* slot_dev, int32_t ring_len, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm1d + ELU blocks of the CrossQ critic (reference pql/models/mlp.py:15-24,224-241,
 * pql/algo/crossQ.py:144-166).  The Linear layers run as one-layer PqlMlpDesc calls of pqlk_mlp_forward / _backward; the
 * batch statistics come from pqlk_batch_moments (mean, UNBIASED variance over the m rows).
 *
 * Forward: y = ELU(z * w + b), w = gamma * invstd, b = beta - mean * w, invstd = 1/sqrt(var + eps) (ATen's order).
 * training != 0: mean / var = the batch statistics (biased variance = var_unbiased * (m-1)/m) and, when running_mean is
 * not NULL, running_{mean,var} <- (1 - momentum) * running + momentum * (mean, var_unbiased) (torch: momentum 0.1,
 * eps 1e-5).  training == 0: the running statistics normalise and nothing is updated.  z, y: (m, ld), cols <= ld. */
int pqlk_bn_elu_forward(const float* z, int64_t ld, int64_t m, int32_t cols, const float* mean, const float* var_unbiased,
                        const float* gamma, const float* beta, float eps, int32_t training, float momentum,
                        float* running_mean, float* running_var, float* y, pqlk_stream_t stream);

/* Backward of the training-mode block: dy = d loss / d y (post-ELU), y and z as stored by the forward ->
 * dz = gamma * invstd * (g - mean_rows(g) - xhat * mean_rows(g * xhat)), g = dy * ELU'(pre) with ELU' taken from y,
 * dgamma = sum_rows(g * xhat), dbeta = sum_rows(g) (either may be NULL).  dz may alias dy.
 * scratch: >= 128 * cols floats (64 row chunks x 2 column sums, folded in chunk order: deterministic). */
int pqlk_bn_elu_backward(const float* dy, const float* y, const float* z, int64_t ld, int64_t m, int32_t cols,
                         const float* mean, const float* var_unbiased, const float* gamma, float eps, float* dz,
                         float* dgamma, float* dbeta, float* scratch, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm + ELU blocks of the LayerNorm twin critic (pql_amd/models/layernorm.py; the reference only hints at it, a
 * commented-out critic at pql/models/mlp.py:288-310).  Row-local: any m >= 1, no batch statistics, no train / eval difference.
 * The Linear layers run as one-layer PqlMlpDesc calls like the BatchNorm critic's.
 *
 * The law.  Everything is fp32 and every written operation is ONE rounding (no contraction, correctly rounded division and
 * sqrtf, no rsqrt, no fast-math builtin, not E[z^2] - mean^2).  Per row of n = cols values:
 *   mean   = (sum_j z_j) / (float)n
 *   var    = (sum_j (z_j - mean)^2) / (float)n            (biased; second pass over the row)
 *   rstd   = 1.0f / sqrtf(var + eps)
 *   xhat_j = (z_j - mean) * rstd
 *   y_j    = elu(xhat_j * gamma_j + beta_j),   elu(x) = x > 0 ? x : expm1f(x)
 * and the forward also writes mean[r], rstd[r] (m floats each).  Backward, per row, with y / z / mean / rstd of the forward:
 *   g_j  = dy_j * (y_j > 0 ? 1 : y_j + 1)
 *   h_j  = g_j * gamma_j
 *   c1   = (sum_j h_j) / n,   c2 = (sum_j h_j * xhat_j) / n
 *   dz_j = rstd * (h_j - c1 - xhat_j * c2)                (left to right)
 * and, down the columns, dbeta_j = sum_r g_rj, dgamma_j = sum_r g_rj * xhat_rj.
 * Summation orders (fixed: the same input gives the same bits, no float atomics).  A row sum: each lane adds its values in
 * register order, then a 64-lane xor butterfly.  A column sum: each wave adds its rows in row order, a block adds its 4 waves in
 * wave order, and pqlk_ln_elu_backward's second launch adds the blocks' partial rows ("chunks") in 16 groups of consecutive chunks,
 * each in chunk order, then the groups in group order.
 *
 * Dispatch.  One wavefront per row, 4 rows per 256-thread block.  cols <= 128 / 256 / 512 / 1024: the row is held in 2 / 4 / 8 /
 * 16 registers per lane (seams at 128|129, 256|257, 512|513); cols > 1024: a strided path that re-reads the row (seam 1024|1025),
 * whose column sums run down the columns over min(m, PQLK_LN_CHUNKS) row chunks.  16-byte accesses when z, y, gamma, beta (backward:
 * dy, y, z, gamma, dz) are 16-B aligned and ld % 4 == 0, scalar ones otherwise.
 * Grid caps.  PQLK_LN_ROW_BLOCKS: blocks of a launch that forms no column sum (the forward; the backward without parameter
 * gradients); past 4 * PQLK_LN_ROW_BLOCKS rows a wave takes several rows.  PQLK_LN_CHUNKS: blocks of the backward that forms column
 * sums = partial rows in scratch; past 4 * PQLK_LN_CHUNKS rows a wave takes several rows.
 *
 * Contract: m >= 1, cols >= 1, ld >= cols, any float-aligned pointers; columns [cols, ld) of y and dz are left untouched and
 * nothing past column cols (of z, dy, y) or element cols (of gamma, beta) is read.  PQLK_E_NULL: a required pointer is NULL.
 * PQLK_E_SHAPE: m <= 0, cols <= 0, ld < cols. */
#define PQLK_LN_ROW_BLOCKS 4096
#define PQLK_LN_CHUNKS 512

/* floats of pqlk_ln_elu_backward's scratch: 2 * PQLK_LN_CHUNKS * cols (0 for cols <= 0) */
int64_t pqlk_ln_scratch_floats(int32_t cols);

int pqlk_ln_elu_forward(const float* z, int64_t ld, int64_t m, int32_t cols, const float* gamma, const float* beta, float eps,
                        float* y, float* mean, float* rstd, pqlk_stream_t stream);

/* dz may alias dy.  dgamma == dbeta == NULL: no parameter gradient is formed, one launch, scratch may be NULL (and is not touched);
 * otherwise scratch >= pqlk_ln_scratch_floats(cols) floats and either output may still be NULL. */
int pqlk_ln_elu_backward(const float* dy, const float* y, const float* z, int64_t ld, int64_t m, int32_t cols, const float* mean,
                         const float* rstd, const float* gamma, float* dz, float* dgamma, float* dbeta, float* scratch,
                         pqlk_stream_t stream);

/* The skip connection of the residual LayerNorm critic (BroNet; pql_amd/models/bronet.py) inside the LayerNorm rows: a block is
 * h_k = h_{k-1} + LN(zb), so the forward adds the skip to the normalised row it already holds, and the backward takes its incoming
 * gradient as a sum of two addends (the gradient through the block's successor and the running skip gradient) and hands the sum on.
 * No stand-alone add launch, no extra pass over the (m, cols) activations.
 *
 * pqlk_ln_res_forward: LayerNorm WITHOUT activation, plus the skip.  Per row:
 *   mean, var, rstd, xhat_j : as in the LayerNorm + ELU law above
 *   t_j = xhat_j * gamma_j
 *   t_j = t_j + beta_j
 *   y_j = res_j + t_j
 * res has the layout of z ((m, ld), columns [cols, ld) never read).  y aliases neither z nor res.  mean[r], rstd[r] are written.
 *
 * pqlk_ln_sum_backward: the LayerNorm backward above with the incoming gradient dy + dy2, with or without the ELU.  Per row:
 *   g0_j   = dy2 ? dy_j + dy2_j : dy_j
 *   dsum_j = g0_j                                          (only if dsum != NULL)
 *   g_j    = y ? g0_j * (y_j > 0 ? 1 : y_j + 1) : g0_j     (y == NULL: no activation behind the norm, the block's second half)
 *   h_j, c1, c2, dz_j, dgamma_j, dbeta_j : as in the law above, from g
 * dy2, y, dsum, dgamma, dbeta are optional (NULL).  dy2 and dsum have the layout of dy.  With dy2 == dsum == NULL and y given the
 * entry runs the operations of pqlk_ln_elu_backward in its order: the same bits.
 * Aliasing.  dz may alias dy; dsum may alias dy2 (the running skip gradient is updated in place); both at once is allowed.  Nothing
 * else may overlap: dz and dsum are distinct, and neither aliases y, z or the other input.  (A row held in registers is read whole
 * before anything of it is written; in the strided path every element of dy and dy2 is read by the lane that then writes dsum and
 * dz at that element, after the row sums, and the column-sum launch runs before the launch that writes.)
 * scratch, and the launches: as for pqlk_ln_elu_backward (pqlk_ln_scratch_floats(cols) floats when dgamma or dbeta is wanted).
 *
 * Dispatch, alignment modes, grid caps and summation orders: those of pqlk_ln_elu_* (the same row bodies); 16-byte accesses need
 * res (backward: dy2, dsum, where given) 16-B aligned too.  Columns [cols, ld) of y, dz and dsum are left untouched.
 * Errors: as for pqlk_ln_elu_*; res is required, and so are dy, z, mean, rstd, gamma, dz. */
int pqlk_ln_res_forward(const float* z, int64_t ld, int64_t m, int32_t cols, const float* gamma, const float* beta, float eps,
                        const float* res, float* y, float* mean, float* rstd, pqlk_stream_t stream);

int pqlk_ln_sum_backward(const float* dy, const float* dy2, const float* y, const float* z, int64_t ld, int64_t m, int32_t cols,
                         const float* mean, const float* rstd, const float* gamma, float* dsum, float* dz, float* dgamma, float* dbeta,
                         float* scratch, pqlk_stream_t stream);

/* Dropout fused into the LayerNorm + ELU rows: the `Linear -> Dropout(p) -> LayerNorm -> ELU` blocks of the DroQ critic
 * (Hiraoka et al. 2022; pql_amd/models/droq.py).  The mask is generated inside the row launches, forward and backward, from a
 * counter-based generator: no mask tensor is written or read, no extra pass over the (m, cols) activations, no extra workspace.
 *
 * The mask law: a pure function of (seed, tag, row r, column c), r the row index in the whole (m, cols) matrix.
 *   x(r, c)    = component (c & 3) of the Philox4x32-10 block with key (seed & 0xffffffff, seed >> 32) and counter words
 *                (c >> 2, r, tag & 0xffffffff, tag >> 32)
 *   thr        = (uint32_t) floor((double)p * 4294967296.0)          (on the host)
 *   keep(r, c) = x(r, c) >= thr
 *   s          = 1.0f / (1.0f - p)                                   (on the host; one rounding each)
 *   u_j        = keep ? z_j * s : 0.0f
 * Forward: the LayerNorm + ELU law above applied to u instead of z; mean and rstd are those of u.  Backward: the law above with
 * xhat re-formed from u -- from z and the regenerated mask, never a stored one -- gives du; then dz_j = keep ? du_j * s : 0.0f;
 * dgamma and dbeta are unchanged in form.  dz may alias dy.
 * p == 0: thr = 0 and s = 1.0f, so u = z bit for bit and both entries give the bits of pqlk_ln_elu_forward / _backward.
 *
 * Dispatch, alignment modes, grid caps and summation orders: those of pqlk_ln_elu_* (the same row bodies).  In the 16-byte layout
 * a lane's chunk of four consecutive columns is one Philox block, generated once per chunk (the 8-byte layout at cols <= 128: half a
 * block per chunk); the scalar layout and the strided path for cols > 1024 spend one block per element, the strided path once per
 * pass over the row.
 * Errors: as for pqlk_ln_elu_*, and PQLK_E_SHAPE for p < 0, p >= 1, a non-finite p, or m > 2^32 (r is one counter word). */

/* keep(r, c) as bytes (1 keep, 0 drop) into keep[r * ld_keep + c], c < cols <= ld_keep: the law alone, for tests and inspection. */
int pqlk_drop_mask(uint64_t seed, uint64_t tag, float p, int64_t m, int32_t cols, uint8_t* keep, int64_t ld_keep,
                   pqlk_stream_t stream);

int pqlk_drop_ln_elu_forward(const float* z, int64_t ld, int64_t m, int32_t cols, const float* gamma, const float* beta, float eps,
                             float p, uint64_t seed, uint64_t tag, float* y, float* mean, float* rstd, pqlk_stream_t stream);

/* y / mean / rstd of pqlk_drop_ln_elu_forward with the same (p, seed, tag); z the forward's input.  NULL outputs and scratch as for
 * pqlk_ln_elu_backward. */
int pqlk_drop_ln_elu_backward(const float* dy, const float* y, const float* z, int64_t ld, int64_t m, int32_t cols, const float* mean,
                              const float* rstd, const float* gamma, float p, uint64_t seed, uint64_t tag, float* dz, float* dgamma,
                              float* dbeta, float* scratch, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Synthetic vectorised environment step (the Isaac-Gym stand-in of BASELINE.json; not a reference component).
 * Counter-based: outputs depend only on (seed, env_offset + env, t, column), so shards of the env axis reproduce
 * slices of the global env.  next_obs ~ N(0,1) (N, obs_dim); reward = N(0,1) - 0.1 mean(action^2) (N);
 * done ~ Bernoulli(p_done) as bytes (N).  Same arithmetic as pql_amd/envs/synthetic.py's torch-op definition. */
int pqlk_synth_env_step(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset, uint32_t t,
                        float p_done, const float* action, float* next_obs, float* reward, uint8_t* done,
                        pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * PointMass vectorised environment step (the learnable task of pql_amd/envs/pointmass.py; not a reference component).
 * Replaces the ~40 elementwise / masked-select torch launches of `PointMassVecEnv._step_torch`, to which every output is
 * bit-equal (one fp32 rounding per operation, no contraction, the sums over act_dim taken in index order, no atomics):
 *   a = clamp(action, -1, 1); v' = 0.8 v + 0.2 a; x' = x + 0.25 v'; k' = k + 1; oob = any |x'| > 1.5;
 *   reward = -mean_j (x' - g)^2 - 0.01 mean_j a^2 - oob; truncated = k' >= episode_length && !oob; done = oob || truncated.
 * State (x, v, g: (N, act_dim) floats; k, ep: (N) int32) is updated IN PLACE; a done env moves to episode ep + 1 and is reset
 * from the counter-based uniform of the synthetic env keyed by (seed, env_offset + env, ep + 1), v = 0, k = 0.
 * next_obs (N, obs_dim) = [x | v | g | 0 ...] AFTER the reset (16-byte stores when obs_dim % 4 == 0 and next_obs is 16-byte
 * aligned); reward (N) floats; done / truncated (N) bytes.
 * PQLK_E_NULL: any pointer NULL.  PQLK_E_SHAPE: n <= 0, act_dim <= 0, obs_dim < 3 * act_dim. */
int pqlk_pointmass_step(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                        int32_t episode_length, const float* action, float* x, float* v, float* g, int32_t* k, int32_t* ep,
                        float* next_obs, float* reward, uint8_t* done, uint8_t* truncated, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * SwingUp vectorised environment step (the nonlinear learnable task of pql_amd/envs/swingup.py; not a reference component):
 * act_dim independent torque-limited pendulums per env, each held as (c, s) = (cos, sin) of its angle from upright and its
 * angular velocity w.  Replaces the ~200 elementwise torch launches of `SwingUpVecEnv._step_torch`, to which every output
 * is bit-equal (one fp32 rounding per operation, no contraction, the sum over act_dim taken in index order, no atomics, no
 * transcendental function, division or square root):
 *   rot(c, s, d): d2 = d d; cd = 1 - d2 (0.5 - d2 / 24); sd = d (1 - d2 (1/6 - d2 / 120)); cn = c cd - s sd; sn = s cd + c sd;
 *                 m = 1.5 - 0.5 (cn cn + sn sn); return (cn m, sn m)          (the three fractions as fp32 literals)
 *   a = clamp(action, -1, 1); w' = clamp(w + 0.05 (15 s + 6 a), -8, 8); (c', s') = rot(c, s, 0.05 w'); k' = k + 1;
 *   reward = -0.05 mean_j ((1 - c') + 0.01 w'^2 + 0.01 a^2); truncated = k' >= episode_length; done = truncated.
 * State (c, s, w: (N, act_dim) floats; k, ep: (N) int32) is updated IN PLACE; a done env moves to episode ep + 1 and is reset
 * from the counter-based uniform u of the synthetic env keyed by (seed, env_offset + env, ep + 1): (c, s) = rot applied four
 * times to (-1, 0) with d = 0.5 (2 u_13 - 1), w = 2 u_14 - 1, k = 0.
 * next_obs (N, obs_dim) = [c | s | 0.125 w | 0 ...] AFTER the reset (16-byte stores when obs_dim % 4 == 0 and next_obs is
 * 16-byte aligned); reward (N) floats; done / truncated (N) bytes.
 * PQLK_E_NULL: any pointer NULL.  PQLK_E_SHAPE: n <= 0, act_dim <= 0, obs_dim < 3 * act_dim. */
int pqlk_swingup_step(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                      int32_t episode_length, const float* action, float* c, float* s, float* w, int32_t* k, int32_t* ep,
                      float* next_obs, float* reward, uint8_t* done, uint8_t* truncated, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Reacher vectorised environment step (the coupled learnable task of pql_amd/envs/reacher.py; not a reference component): a
 * planar arm of act_dim links of length 1 / act_dim per env, joint j held as (c, s) = (cos, sin) of its angle relative to the
 * link before it (joint 0: to the world x axis) and its angular velocity w; the tip has to reach (0.6, 0).  Every output is
 * bit-equal to `ReacherVecEnv._step_torch` (one fp32 rounding per operation, no contraction, the sums over act_dim taken in
 * index order, no atomics, no transcendental function or square root), rot as for SwingUp:
 *   a = clamp(action, -1, 1); w' = clamp(0.9 w + 0.3 a, -3, 3); (c', s') = rot(c, s, 0.05 w'); k' = k + 1;
 *   tip(c, s): C = c_0, S = s_0, x = C, y = S; for j = 1 .. act_dim - 1: (C, S) = (C c_j - S s_j, S c_j + C s_j), x += C, y += S;
 *              ex = x / act_dim - 0.6, ey = y / act_dim        (a product with the fp32 constant 1.0f / act_dim)
 *   (ex, ey) = tip(c', s'); d2 = ex ex + ey ey; reward = -0.05 ((d2 + 0.01 mean_j w'^2) + 0.01 mean_j a^2);
 *   truncated = k' >= episode_length; done = truncated.
 * State (c, s, w: (N, act_dim) floats; k, ep: (N) int32) is updated IN PLACE; a done env moves to episode ep + 1 and is reset
 * from the counter-based uniform u of the synthetic env keyed by (seed, env_offset + env, ep + 1): (c, s) = rot applied six
 * times to (1, 0) with d = 0.5 (2 u_15 - 1), w = 0.5 (2 u_16 - 1), k = 0.
 * next_obs (N, obs_dim) = [c | s | 0.25 w | ex | ey | 0 ...] AFTER the reset, (ex, ey) = tip of the state the row holds (16-byte
 * stores when obs_dim % 4 == 0 and next_obs is 16-byte aligned); reward (N) floats; done / truncated (N) bytes.
 * PQLK_E_NULL: any pointer NULL.  PQLK_E_SHAPE: n <= 0, act_dim <= 0, obs_dim < 3 * act_dim + 2. */
int pqlk_reacher_step(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                      int32_t episode_length, const float* action, float* c, float* s, float* w, int32_t* k, int32_t* ep,
                      float* next_obs, float* reward, uint8_t* done, uint8_t* truncated, pqlk_stream_t stream);

/* The three steps above with the task's info channels (pql_amd/envs/base.py `info_keys`): the same launch, the same argument list
 * plus `info` in front of the stream, every other output bit-identical.  info is channel-major (n_info, N) floats with row stride
 * N; row c holds channel c of the step just taken, for a finished env the value BEFORE its reset:
 *   pointmass: 0 = dist2 = mean_j (x' - g)^2, the very value of the reward; 1 = oob = 1.0 where the step left the box, else 0.0;
 *   swingup:   0 = upright = mean_j c'; 1 = effort = mean_j a^2 of the clamped action; both sums in index order from the j = 0 term.
 *   reacher:   0 = tip_dist2 = d2 of the reward; 1 = effort = mean_j a^2 of the clamped action, summed in index order;
 *              2 = reached = 1.0 where d2 < 0.01, else 0.0.
 * PQLK_E_NULL: info NULL, besides the errors of the plain entries. */
int pqlk_pointmass_step_info(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                             int32_t episode_length, const float* action, float* x, float* v, float* g, int32_t* k, int32_t* ep,
                             float* next_obs, float* reward, uint8_t* done, uint8_t* truncated, float* info, pqlk_stream_t stream);
int pqlk_swingup_step_info(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                           int32_t episode_length, const float* action, float* c, float* s, float* w, int32_t* k, int32_t* ep,
                           float* next_obs, float* reward, uint8_t* done, uint8_t* truncated, float* info, pqlk_stream_t stream);
int pqlk_reacher_step_info(int64_t n, int32_t obs_dim, int32_t act_dim, uint32_t seed, uint32_t env_offset,
                           int32_t episode_length, const float* action, float* c, float* s, float* w, int32_t* k, int32_t* ep,
                           float* next_obs, float* reward, uint8_t* done, uint8_t* truncated, float* info, pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Per-env-step bookkeeping of the rollout in one launch (pql_actor.py:104-114 slab writes, :129-135 update_tracker,
 * common.py:195-202 handle_timeout): column t of the (N, horizon, .) trajectory slabs <- (obs, action, reward, next_obs,
 * done * !truncated); cur_return += reward, cur_length += 1; the finished envs' values are appended IN ENV ORDER to the two
 * moving windows of win_len floats (the last win_len of them when more finish in one step, like deque.extend) behind the
 * windows' device write pointers, and their accumulators reset.  done / truncated are bytes (truncated may be NULL). */
int pqlk_rollout_step(int64_t n, int32_t obs_dim, int32_t act_dim, int32_t horizon, int32_t t, const float* obs,
                      const float* action, const float* next_obs, const float* reward, const uint8_t* done,
                      const uint8_t* truncated, float* slab_obs, float* slab_act, float* slab_rew, float* slab_nobs,
                      float* slab_done, float* cur_return, float* cur_length, float* win_return, float* win_length,
                      int64_t* win_return_ptr, int64_t* win_length_ptr, int32_t win_len, pqlk_stream_t stream);

/* The info trackers of one env step in one launch (`info_track_keys` / `info_track_step`: pql/algo/pql_actor.py:28-33,138-151,
 * pql/algo/ac_base.py:54-59,88-101, pql/utils/evaluator.py:56-61,89-111, where every key costs a `torch.where(done)[0]`, a `.cpu()`
 * and a `deque.extend` per env step).  One 1024-thread block per key; per key, with value(e) = values[e] (PQLK_INFO_F32) or
 * values[e] != 0 as 0.0 / 1.0 (PQLK_INFO_U8: bool / uint8 bytes):
 *   PQLK_INFO_LAST         value(e) of the envs with done[e] != 0 is appended IN ENV ORDER to the key's window;
 *   PQLK_INFO_ALL_EPISODE  acc[e] += value(e) for every env, then acc[e] of the done envs is appended and set to zero;
 *   PQLK_INFO_ALL_STEP     value(e) of every env is appended;
 * appended = written behind the window's device write pointer ring_ptr[0] (in [0, win_len)), which advances by the number of
 * appended values modulo win_len; when one step appends more than win_len values only the last win_len stay, like deque.extend
 * (and like the windows of pqlk_rollout_step, whose ordered block-wide append this is).  ring holds win_len floats, acc (N)
 * floats (read only by ALL_EPISODE, may be NULL otherwise), done (N) bytes.  Keys must not share rings, pointers or accumulators.
 * Deterministic: no atomics, no host sync; bit-equal to the torch form in pql_amd/utils/info_track.py.
 * PQLK_E_NULL: done, keys, or a key's values / ring / ring_ptr NULL, acc NULL under ALL_EPISODE.  PQLK_E_SHAPE: n <= 0,
 * win_len <= 0, n_keys outside [1, PQLK_INFO_MAX_KEYS].  PQLK_E_UNSUPPORTED: an unknown dtype or mode. */
#define PQLK_INFO_MAX_KEYS 8
enum { PQLK_INFO_F32 = 0, PQLK_INFO_U8 = 1 };
enum { PQLK_INFO_LAST = 0, PQLK_INFO_ALL_EPISODE = 1, PQLK_INFO_ALL_STEP = 2 };
typedef struct PqlInfoKey {
  const void* values; /* (N) this step's values of the key */
  float* acc;         /* (N) per-env running sum (ALL_EPISODE) */
  float* ring;        /* window of win_len floats */
  int64_t* ring_ptr;  /* the window's write pointer */
  int32_t dtype;      /* PQLK_INFO_F32 / PQLK_INFO_U8 */
  int32_t mode;       /* PQLK_INFO_LAST / _ALL_EPISODE / _ALL_STEP */
} PqlInfoKey;
int pqlk_rollout_info(int64_t n, const uint8_t* done, int32_t win_len, int32_t n_keys, const PqlInfoKey* keys,
                      pqlk_stream_t stream);

/* The remaining per-env-step elementwise work of the rollout, one launch each (the reference issues 12 + 4 + 4 ATen launches):
 * RunningMeanStd.update_from_moments (pql/utils/torch_util.py:91-103): Chan merge of one batch's moments into the running
 * ones, op for op in fp32 (count / batch_count / total = the python scalars rounded to fp32 as torch rounds them), written to
 * mean_out / var_out (may alias mean / var); RunningMeanStd.normalize (:83-85): (x - mean) / sqrt(var + eps) of a contiguous
 * (rows, cols) matrix into rows of stride ld_out (columns past cols untouched), IEEE division, no clamp; add_normal_noise / add_mixed_normal_noise (pql/utils/noise.py:19-41):
 * out = clamp(act + draw * sigma, lo, hi) with sigma = std_rows[row] (one per env) when std_rows != NULL, else std_scalar. */
int pqlk_rms_merge(const float* mean, const float* var, const float* batch_mean, const float* batch_var, float count,
                   float batch_count, float total, int32_t cols, float* mean_out, float* var_out, pqlk_stream_t stream);
int pqlk_rms_normalize(const float* x, int64_t rows, int32_t cols, const float* mean, const float* var, float eps, float* out,
                       int64_t ld_out, pqlk_stream_t stream);
int pqlk_action_noise(const float* act, const float* draw, const float* std_rows, float std_scalar, int64_t rows, int32_t cols,
                      float lo, float hi, float* out, pqlk_stream_t stream);

/* Temporally correlated exploration noise (algo.noise.color = ar1 | pink, pql_amd/utils/noise.py `ColoredNoise`): per element
 * (e, a) of a (rows, cols) action matrix, R = octaves unit-variance AR(1) states s_k are advanced by one step and their scaled sum
 * takes the place of pqlk_action_noise's white draw.  Everything is fp32, every written operation one rounding (no contraction).
 * With E = env_offset + e the row's GLOBAL env index and g = E mod groups its correlation group:
 *   eps_k = draw[e, k * cols + a]                                                     draw is (rows, R * cols), standard normal
 *   s_k   = fresh[e] ? eps_k : (rho[g, k] * s_k) + (coef[g, k] * eps_k)               for k = 0 ... R-1, in index order
 *   n     = (((s_0 + s_1) + s_2) + ...) * w
 *   out   = clamp(act + n * sigma_e, lo, hi)                                          sigma_e = std_rows[e], or std_scalar when NULL
 * with pqlk_action_noise's expression order in the last line: with R = 1, w = 1 and rho = 0, coef = 1 `out` has its bits.
 * rho, coef: (groups, R) tables; the caller builds coef = fp32(sqrt(1 - rho^2)) (evaluated in float64) and w = fp32(1 / sqrt(R)), so
 * every s_k and n have stationary variance 1.  ar1: R = 1, groups = corr_groups, rho = linspace(corr_min, corr_max, groups);
 * pink: groups = 1, rho[0] = 0, rho[k] = 1 - 2^-k.  fresh (rows) bytes: non-zero = the row's process starts over from this draw (an
 * env's first step, and the step after one that ended an episode).  state (rows, R, cols) is updated in place.
 * Contract: act, draw, rho, coef, fresh, state, out non-NULL (PQLK_E_NULL); rows > 0, cols > 0, 1 <= octaves <=
 * PQLK_NOISE_MAX_OCTAVES, groups >= 1, env_offset >= 0, lo <= hi (PQLK_E_SHAPE); float-aligned pointers suffice; out may not
 * overlap state (PQLK_E_RANGE).  Nothing outside [0, rows) x [0, cols) of out and [0, rows) x [0, R * cols) of state is written.
 * One launch of one thread per element (grid-stride past 4096 blocks of 256), no LDS, no atomics: deterministic. */
#define PQLK_NOISE_MAX_OCTAVES 8
int pqlk_action_noise_colored(const float* act, const float* draw, const float* std_rows, float std_scalar, const float* rho,
                              const float* coef, int32_t groups, int32_t octaves, int64_t env_offset, const uint8_t* fresh,
                              float* state, int64_t rows, int32_t cols, float w, float lo, float hi, float* out,
                              pqlk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * On-policy PPO baseline (reference pql/algo/ppo.py:79-183, pql/models/mlp.py:43-75).  All reductions in a fixed order.
 *
 * GAE / plain discounted returns over a (T, N) trajectory, one column per env, the reference's operation order:
 *   use_gae: delta = r[t] + (gamma * nv) * nnt2 - v[t];  lastgaelam = delta + ((float)(gamma * lambda) * nnt) * lastgaelam;
 *            adv[t] = lastgaelam, ret[t] = adv[t] + v[t];  nnt = 1 - (t == T-1 ? next_done : done[t+1]), nv likewise from
 *            next_val / val[t+1];  nnt2 = logical_xor(nnt, timeout[t]) when timeout (T, N) != NULL, else nnt.
 *   else:    ret[t] = r[t] + (gamma * nnt) * (t == T-1 ? next_val : ret[t+1]);  adv = ret - v  (time-outs ignored).
 * rew / done / val / timeout / adv / ret are (T, N) contiguous, next_val / next_done (N); done and timeout hold 0 / 1. */
int pqlk_gae(const float* rew, const float* done, const float* val, const float* next_val, const float* next_done,
             const float* timeout, int32_t T, int64_t n, double gamma, double lambda, int32_t use_gae, float* adv, float* ret,
             pqlk_stream_t stream);

/* Diagonal-Gaussian head of DiagGaussianMLPPolicy: y (B, ld_y) = the MLP's mean block, logstd (A), eps (B, A) the standard-
 * normal draw (NULL = the mean itself).  act[r * ld_act + j] = mean + exp(logstd_j) * eps; logp (B) = sum over j in index order
 * of -((a - mu)^2) / (2 scale^2) - log(scale) - log(sqrt(2 pi)); ent (B) = sum_j 0.5 + 0.5 log(2 pi) + log(scale).  logp / ent
 * may be NULL.  A <= 64. */
int pqlk_ppo_gauss_head(const float* y, int64_t ld_y, const float* logstd, const float* eps, int64_t b, int32_t act_dim,
                        float* act, int64_t ld_act, float* logp, float* ent, pqlk_stream_t stream);

/* Minibatch gather from the flat (rows = T*N) trajectory: for r < mb and k = idx[r] (clamped into [0, rows)):
 *   x[r] (ld ldx) = (obs[k] - mean) / sqrt(var + eps) (no clamp; raw when mean == var == NULL), pad columns [O, ldx) zero;
 *   act_out[r] (A, contiguous) = act[k];  logp / adv / ret / val _out[r] = the trajectory's value at k;
 *   adv_part (3 * pqlk_ppo_gather_parts(mb)) = per-block { rows, sum, sum of squared deviations from the block mean } of the
 *   gathered advantages, read by pqlk_ppo_policy_loss for the minibatch's mean and unbiased std.  mb may be < the batch size. */
int32_t pqlk_ppo_gather_parts(int64_t mb);
int pqlk_ppo_gather(const int64_t* idx, int64_t mb, int64_t rows, const float* obs, int32_t obs_dim, const float* mean,
                    const float* var, float eps, float* x, int64_t ldx, const float* act, int32_t act_dim, float* act_out,
                    const float* logp, const float* adv, const float* ret, const float* val, float* logp_out, float* adv_out,
                    float* ret_out, float* val_out, float* adv_part, pqlk_stream_t stream);

/* Clipped-surrogate policy loss and its gradient.  With the minibatch's advantage mean m and unbiased std s (from adv_part),
 *   logp = as pqlk_ppo_gauss_head at act (B, A contiguous), ratio = exp(logp - old_logp), na = (adv - m) / (s + 1e-8),
 *   loss = mean(max(-na ratio, -na clamp(ratio, 1 - clip, 1 + clip))) - lambda_ent * mean(entropy)
 * into loss_ring[*slot_dev % ring_len] (loss_ring may be NULL); dy (B, ld_y) columns [0, A) = d loss / d mean (pad columns
 * untouched), dlogstd (A) = d loss / d logstd; logp_out (B, may be NULL).  autograd's tie rules: max splits the gradient 50/50 on
 * equal arguments, clamp passes it on the closed interval.  scratch >= pqlk_ppo_scratch_floats(b, A) floats.  Two launches.
 * b == 1 (a one-row last minibatch) is accepted: the unbiased std is NaN and so are the loss and gradient, as in the reference. */
int64_t pqlk_ppo_scratch_floats(int64_t b, int32_t act_dim);
int pqlk_ppo_policy_loss(const float* y, int64_t ld_y, const float* logstd, const float* act, const float* old_logp,
                         const float* adv, const float* adv_part, int32_t n_parts, int64_t b, int32_t act_dim, float clip,
                         float lambda_ent, float* dy, float* dlogstd, float* logp_out, float* scratch, int64_t scratch_floats,
                         float* loss_ring, const int32_t* slot_dev, int32_t ring_len, pqlk_stream_t stream);

/* Value loss: clip_on ? 0.5 mean(max((v - R)^2, (V + clamp(v - V, -clip, clip) - R)^2)) : 0.5 mean((v - R)^2), with v = column 0
 * of the critic's output rows (stride ld_v), R = ret, V = old_v.  dy[r * ld_dy] = d loss / d v (same tie rules); the loss into
 * loss_ring[*slot_dev % ring_len] when loss_ring != NULL.  scratch >= pqlk_ppo_scratch_floats(b, 1) floats. */
int pqlk_ppo_value_loss(const float* v, int64_t ld_v, const float* ret, const float* old_v, int64_t b, int32_t clip_on, float clip,
                        float* dy, int64_t ld_dy, float* scratch, int64_t scratch_floats, float* loss_ring,
                        const int32_t* slot_dev, int32_t ring_len, pqlk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PQLK_H */
