/*
 * iqlhip.h -- C-ABI of libiqlhip.so, the MI355X (gfx950) implementation of the
 * IQL-with-preference-reward hot path of ml4ai/iqlpref.
 *
 * The reference has no FFI: its boundary for this path is the Python module
 * surface of algorithms/offline/iql.py.  Each entry point
 * below names the reference lines it replaces ("ref:" = that file).  The Python
 * package iqlpref_amd mirrors the reference classes on top of these calls via
 * ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain C types only; every pointer documented "device" is a HIP device
 *     pointer owned by the caller (borrowed for the duration stated);
 *   - every function returns 0 on success and a negative iqlhip_status on
 *     failure; iqlhip_last_error() returns a thread-local message;
 *   - all work is enqueued on the hipStream_t passed as `stream` (void*), nothing
 *     synchronises the host unless stated;
 *   - one trainer <-> one stream <-> one host thread (not re-entrant per trainer).
 */
#ifndef IQLHIP_H
#define IQLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  IQLHIP_OK = 0,
  IQLHIP_ERR_INVALID = -1,     /* bad argument (Python raises ValueError)        */
  IQLHIP_ERR_HIP = -2,         /* HIP runtime error (Python raises RuntimeError) */
  IQLHIP_ERR_UNSUPPORTED = -3, /* shape outside what the kernels are built for   */
  IQLHIP_ERR_NOMEM = -4
} iqlhip_status;

const char *iqlhip_last_error(void);
/* ABI version of this header; bumped on any incompatible change. */
int iqlhip_abi_version(void);
/* 16 hex digits: sha256 prefix of the sources (csrc/ + this header + compiler flags) the
 * library was built from, stamped by iqlpref_amd/build.py.  The Python binding refuses a
 * library whose tag differs from the sources beside it.                                  */
const char *iqlhip_build_tag(void);

/* ------------------------------------------------------------------------ */
/* Shape envelope (everything outside returns IQLHIP_ERR_UNSUPPORTED with a   */
/* message; every YAML under the reference's configs/offline/iql/ fits):      */
/*   trainer   ReLU hidden activations, one width for all hidden layers,       */
/*             n_hidden 1..6, hidden_dim 1..1024, any batch_size >= 1 (the     */
/*             kernels pad it to whole 16-row slabs and count only the real    */
/*             rows; every array of the caller keeps batch_size rows; a step   */
/*             may count fewer rows still: iqlhip_train_steps_valid),          */
/*             state_dim + action_dim <= 128, action_dim <= 32, 2..8 critics,  */
/*             plain Adam (no weight decay / amsgrad), one (beta1, beta2, eps) */
/*             for the three optimisers.  n_hidden = 2 with hidden_dim 64, 128 */
/*             or 256 (the reference's default and every shipped YAML) runs on */
/*             the tuned three-kernel step; every other shape on the general   */
/*             layer-wise step (csrc/iql_deep.hip: same arithmetic, graph      */
/*             replay and seed groups of one shape as on the tuned step; no    */
/*             CU-slice sub-groups);                                           */
/*   online    iqlhip_explore_action: every trainer shape above at precision     */
/*             fp32; iqlhip_replay_append: any ring of >= 1 rows, n <= capacity;  */
/*             iqlhip_np_randint_growing: growth 0 or 1, bounds up to 2^32;       */
/*             iqlhip_explore_action_group / iqlhip_replay_append_group: the same */
/*             for one row of each of 1..16 trainers / rings in one launch;       */
/*   MLP fwd   1..8 layers, every width in [1, 1024] (beyond 256: a plain      */
/*             one-wave-per-16-rows variant);                                  */
/*   CVaR      1 <= n_tail <= S <= 2400;                                       */
/*   PT        tuned (iqlhip_pt_relabel): embd_dim 64, ONE GPT-2 block,        */
/*             num_heads a power of two <= 16, inter_dim a multiple of 256 up  */
/*             to 1024, state_dim + action_dim <= 192, query_length such that  */
/*             the window fits the 160 KiB LDS.  General layer-wise path       */
/*             (iqlhip_pt_relabel_general, csrc/pt_general.hip): 1..8 blocks,  */
/*             embd_dim a multiple of 64 up to 256, num_heads a power of two   */
/*             with embd_dim / num_heads >= 4, inter_dim a multiple of 64 up   */
/*             to 1024, state_dim + action_dim <= 256, query_length <= 4096.  */
/* ------------------------------------------------------------------------ */

/* ------------------------------------------------------------------------ */
/* Replay buffer  (ref:164-226 ReplayBuffer)                                 */
/*                                                                           */
/* Storage is ONE row-major fp32 matrix [capacity][row_stride]; row i holds  */
/* transition i as  [ s(S) | a(A) | r | d | pad | s'(S) | pad ]  with s' on a */
/* 16-byte boundary (float offset iqlhip_replay_next_offset), so that one    */
/* sample is one contiguous read of aligned 16-byte pieces instead of five.  */
/* ------------------------------------------------------------------------ */
typedef struct {
  const float *rows;  /* device, [n_rows][row_stride]          */
  int64_t n_rows;     /* min(_size,_pointer) of ref:212         */
  int32_t row_stride; /* floats, multiple of 4                  */
  int32_t state_dim;
  int32_t action_dim;
  uint64_t generation; /* changes whenever the CONTENTS of rows change (a Python ReplayBuffer
                          bumps it on every load).  A call whose view equals the previous
                          call's (rows, n_rows, generation), with on-device indices and no
                          per-step outputs, continues that call: the batch its last step
                          prefetched is used and nothing is re-sent.  0 is a valid value for
                          callers that never rewrite rows in place.                        */
} iqlhip_replay_view;

/* Float offset of s' inside a row: S+A+2 rounded up to a multiple of 4; row stride (floats):
 * that offset + S, rounded up to a multiple of 4.  Views must carry exactly this stride.  */
int32_t iqlhip_replay_next_offset(int32_t state_dim, int32_t action_dim);
int32_t iqlhip_replay_row_stride(int32_t state_dim, int32_t action_dim);

/* ref:193-209 load_d4rl_dataset: interleave the five device arrays
 * obs[n][S], act[n][A], rew[n], next_obs[n][S], done[n] (fp32) into
 * rows[first_row .. first_row+n).                                           */
int iqlhip_replay_pack(float *rows, int32_t row_stride, int32_t state_dim,
                       int32_t action_dim, int64_t first_row, int64_t n,
                       const float *obs, const float *act, const float *rew,
                       const float *next_obs, const float *done, void *stream);

/* The same with the state z-scoring of ref:1438-1448 fused in: s and s' columns are written as
 * (x - mean[c]) / std[c] (fp32, the arithmetic of normalize_states ref:138-139); mean / std are
 * device fp32 [S] (iqlhip_prep_state_stats, or compute_mean_std results uploaded).            */
int iqlhip_replay_pack_normalized(float *rows, int32_t row_stride, int32_t state_dim,
                                  int32_t action_dim, int64_t first_row, int64_t n,
                                  const float *obs, const float *act, const float *rew,
                                  const float *next_obs, const float *done, const float *mean,
                                  const float *std, void *stream);

/* ------------------------------------------------------------------------ */
/* Dataset preparation on the device (the Python loops over the N transitions */
/* that run before training starts).  All pointers are device pointers unless  */
/* stated; terminals / timeouts are uint8 (0 / 1).                             */
/* ------------------------------------------------------------------------ */
/* ref:701-716 (= ref:938-951, 1127-1141, 1236-1253): keep[i] and the episode-step counter
 * ep_steps[i] seen by transition i, for i < n - 1.  timeouts == NULL: `final` is
 * (counter == max_episode_steps - 1) as in the reference.  Integer outputs: exact.          */
int iqlhip_prep_keep_mask(const uint8_t *terminals, const uint8_t *timeouts, int64_t n,
                          int32_t max_episode_steps, int32_t terminate_on_end, uint8_t *keep,
                          int64_t *ep_steps, void *stream);
/* ref:344-360 return_reward_range: an episode ends at a terminal or after max_episode_steps
 * transitions.  *min_ret / *max_ret (HOST doubles) over the complete episodes -- every return
 * is summed in double in transition order, so they equal the reference's bit for bit;
 * trj_lens[i] (device double [n]) = length of the episode transition i belongs to.
 * Synchronises `stream`.  IQLHIP_ERR_INVALID when no episode is complete.                   */
int iqlhip_prep_reward_range(const float *rewards, const uint8_t *terminals, int64_t n,
                             int32_t max_episode_steps, double *trj_lens, double *min_ret,
                             double *max_ret, void *stream);
/* ref:363-401 modify_reward, in place, with numpy's in-place float32 arithmetic:
 *   sub_first 1: r -= min_ret (fp32)   2: r = fp32(double(r) - min_ret / trj_lens[i])
 *   scale      : r /= fp32(max_ret - min_ret); r *= fp32(max_episode_steps)
 *   sub_one    : r -= 1
 * (which of them apply to which env / normalize_reward value is host logic).                */
int iqlhip_prep_modify_reward(float *rewards, int64_t n, const double *trj_lens, int32_t sub_first,
                              int32_t scale, int32_t sub_one, double min_ret, double max_ret,
                              int32_t max_episode_steps, void *stream);
/* ref:132-135 compute_mean_std: mean[c], std[c] + eps of obs[n][state_dim] (state_dim <= 256),
 * accumulated in double in a fixed order (deterministic; differs from numpy's fp32 row-order
 * sums at the 1e-6 level).                                                                  */
int iqlhip_prep_state_stats(const float *obs, int64_t n, int32_t state_dim, double eps, float *mean,
                            float *std, void *stream);

/* algorithms/offline/any_percent_bc.py:206-239 keep_best_trajectories, the part that walks every row.
 * A trajectory ends at a row whose terminal is set or when it has max_len rows (iqlhip_prep_reward_range's
 * rule); a trailing run that reaches neither is no trajectory.  For the complete trajectories, in dataset
 * order: starts[t] = first row, lengths[t] = rows, returns[t] = the discounted return (device arrays of n
 * entries each: max_len = 1 makes every row a trajectory; entries from the count on are not written);
 * *n_traj (HOST) = their count.  returns[t] = sum over k of fp32(scale[k] * rewards[starts[t] + k]), products
 * and sums each rounded to fp32, in row order from 0 -- what numpy 2 computes for
 * `cur_return += reward_scale * reward` on float32 rewards when scale[k] = fp32(the Python float after k
 * multiplications by the discount): bit-identical to the reference's returns.  scale: device fp32
 * [min(max_len, n)] (a trajectory has at most n rows: entry k is read only by a trajectory with a row k).
 * Synchronises `stream` (the count comes back).  Refused before any launch: a null pointer, n < 1,
 * max_len < 1 (IQLHIP_ERR_INVALID), max_len > 2^20 (IQLHIP_ERR_UNSUPPORTED).  IQLHIP_ERR_INVALID when no
 * trajectory is complete: nothing has been written to starts / lengths / returns / *n_traj then.           */
int iqlhip_prep_trajectory_returns(const float *rewards, const uint8_t *terminals, int64_t n,
                                   int32_t max_len, const float *scale, int64_t *starts, int64_t *lengths,
                                   float *returns, int64_t *n_traj, void *stream);
/* The same function's `dataset[k][order]` (:231-239) for one array: src [n][width] fp32; chosen [m] = numbers of
 * trajectories (indices into starts / lengths of the call above, n_traj of them), in the order they are to
 * lie in dst; dst_offsets [m] = the exclusive prefix sum of their lengths; dst [total_rows][width] with
 * total_rows = the sum of their lengths.  Whole trajectories are copied, in 16-byte pieces where both ends lie
 * on 16-byte boundaries and in floats otherwise; rows of no chosen trajectory are not read.  An entry of
 * chosen outside [0, n_traj), or whose rows would not fit src or dst, is skipped on the device.  All arrays are
 * device arrays; no host wait.  Refused before the launch (IQLHIP_ERR_INVALID): a null pointer, n < 1,
 * width < 1, n_traj outside 1..n, m outside 1..n_traj, total_rows outside m..n.                              */
int iqlhip_prep_gather_trajectories(const float *src, int64_t n, int32_t width, const int64_t *starts,
                                    const int64_t *lengths, int64_t n_traj, const int64_t *chosen,
                                    const int64_t *dst_offsets, int64_t m, int64_t total_rows, float *dst,
                                    void *stream);

/* ref:211-221 sample.  idx == NULL: indices are drawn on device,
 * idx[b] = philox4x32_10(key=seed, ctr=(b, step, stream 0)).x % n_rows
 * (oracle/philox.py); otherwise idx is a device int64[batch] that is used as
 * given (parity runs).  Outputs are dense device fp32 tensors
 * s[B][S] a[B][A] r[B][1] s2[B][S] d[B][1]; idx_out (optional) receives the
 * indices used.                                                             */
int iqlhip_replay_sample(const iqlhip_replay_view *view, int32_t batch,
                         const int64_t *idx, uint64_t seed, uint64_t step, float *s,
                         float *a, float *r, float *s2, float *d, int64_t *idx_out,
                         void *stream);

/* ------------------------------------------------------------------------ */
/* Trainer  (ref:546-688 ImplicitQLearning; nets ref:408-543)                 */
/* ------------------------------------------------------------------------ */
#define IQLHIP_PREC_FP32 0 /* autocast disabled: exact fp32 MFMA (16x16x4 f32)    */
#define IQLHIP_PREC_BF16 1 /* ref:650 autocast: bf16 MFMA, fp32 accumulate        */

typedef struct {
  int32_t state_dim, action_dim;
  int32_t hidden_dim;    /* 1..1024 (ref:417-449 MLP: one width for all hidden layers) */
  int32_t batch_size;    /* any batch_size >= 1 (padded to 16 rows inside)        */
  int32_t deterministic; /* 1: DeterministicPolicy (ref:485), 0: Gaussian (ref:452)*/
  int32_t precision;     /* IQLHIP_PREC_*                                         */
  float dropout_p;       /* actor dropout (ref:436-437); < 0 = none               */
  float discount, tau, beta, iql_tau; /* ref:558-562                             */
  double lr_q, lr_v, lr_actor;        /* Adam lr; lr_actor = cosine base lr       */
  double adam_beta1, adam_beta2, adam_eps;
  int64_t cosine_t_max;  /* CosineAnnealingLR T_max = max_steps (ref:571)         */
  uint64_t seed;         /* Philox key for on-device indices and dropout          */
  int32_t n_critics;     /* 0 or 2: TwinQ (ref:517-533); 3..8: E-way critic ensemble,
                            the same MLP E times, q_target = min over E, q_loss =
                            sum(mse)/E (ref:606 generalised; SURVEY 8 "config 5")    */
  int32_t polyak_form;   /* target update: 0 = tp.lerp_(sp, tau) (offline/iql.py:127-129),
                            1 = (1 - tau) tp + tau sp (custom_offline/iql.py:85-87)      */
  int32_t n_hidden;      /* hidden layers per network (ref:458-459, 519, 538: n_hidden);
                            0 = the reference's default 2; 1..6                           */
} iqlhip_trainer_config;

/* Number of fp32 elements of the arenas (n_params, n_target: they include the
 * alignment padding, every tensor starts on a 128-byte line; padding elements
 * are never read or written) and the element offset of every tensor in the
 * parameter arena.  Order of the 2 L (E+2) + 1 offsets, L = n_hidden + 1 Linear
 * layers (25 offsets for TwinQ with two hidden layers): for net in (q1, .., qE, v,
 * actor): W_1[H][in] b_1[H] W_2[H][H] b_2[H] ... W_L[out][H] b_L[out]; then actor
 * log_std[A] (offset -1 when deterministic); unused slots are -1.
 * Torch [out][in] row-major layouts.  The target arena uses the q1..qE part of
 * the same layout.                                                           */
#define IQLHIP_MAX_CRITICS 8
#define IQLHIP_MAX_HIDDEN 6
#define IQLHIP_N_TENSORS (2 * (IQLHIP_MAX_HIDDEN + 1) * (IQLHIP_MAX_CRITICS + 2) + 1)
int iqlhip_arena_layout(const iqlhip_trainer_config *cfg, int64_t offsets[IQLHIP_N_TENSORS],
                        int64_t *n_params, int64_t *n_target);

typedef struct {
  float *params;  /* device fp32 [n_params]  master weights (torch-owned)       */
  float *exp_avg; /* device fp32 [n_params]  Adam m                             */
  float *exp_avg_sq; /* device fp32 [n_params]  Adam v                          */
  float *target;  /* device fp32 [n_target]  q_target (ref:565)                 */
  float *grads;   /* optional device fp32 [n_params]; when non-NULL every step
                     also stores the parameter gradients (tests)               */
} iqlhip_arenas;

typedef struct iqlhip_trainer iqlhip_trainer;

/* Borrows the arenas for the trainer's lifetime; allocates its own workspace
 * (compute-precision weight copies, activations) on the current device.      */
int iqlhip_trainer_create(iqlhip_trainer **out, const iqlhip_trainer_config *cfg,
                          const iqlhip_arenas *arenas);
int iqlhip_trainer_destroy(iqlhip_trainer *t);

/* Which step runs this trainer's shape: 0 = the tuned three-kernel step (csrc/iql_step.hip),
 * 1 = the general layer-wise step (csrc/iql_deep.hip).  See the shape envelope above.        */
int iqlhip_trainer_step_kind(iqlhip_trainer *t, int32_t *kind);

/* Rebuild the compute-precision weight copies from the fp32 masters (call
 * after the arenas were written from outside: init, load_state_dict).        */
int iqlhip_trainer_sync_weights(iqlhip_trainer *t, void *stream);

/* total_it (ref:575,640) = optimiser steps taken = Adam `step` = scheduler
 * last_epoch.                                                                */
int iqlhip_trainer_set_step(iqlhip_trainer *t, int64_t total_it);
int iqlhip_trainer_get_step(iqlhip_trainer *t, int64_t *total_it, double *actor_lr);
int iqlhip_trainer_set_lr(iqlhip_trainer *t, double lr_q, double lr_v, double lr_actor_base);

/* ref:1533-1536 the hot loop body, n_steps times, without host round trips:
 *   sample (ref:211-221) -> ImplicitQLearning.train (ref:639-662).
 * idx: NULL (on-device Philox indices) or device int64[n_steps][batch].
 * dropout_keep: NULL (on-device Philox masks) or device uint8
 *   [n_steps][n_hidden][batch][hidden] (1 = keep); ignored without actor dropout.
 * losses_out: NULL or device fp32[n_steps][3] = value_loss, q_loss, actor_loss
 *   of each step (ref:589,607,633).
 * graph_unroll: > 0 replays a captured hipGraph of that many steps per launch
 *   (the general step caps it at 1024, the steps of one upload of its arguments);
 *   0: plain kernel launches, three per step, from this call's loop (one seed: the
 *   faster mode, a graph launch costs ~5 us of device time; seed groups: graphs of 50).
 * Asynchronous on `stream`, except that a call never leaves more than
 * IQLHIP_MAX_INFLIGHT kernel dispatches (environment, default 6144, 0 = no bound;
 * 3 per step) queued: beyond that it waits for the oldest third of them.      */
int iqlhip_train_steps(iqlhip_trainer *t, const iqlhip_replay_view *view, int64_t n_steps,
                       const int64_t *idx, const uint8_t *dropout_keep, float *losses_out,
                       int32_t graph_unroll, void *stream);

/* iqlhip_train_steps with a per-step count of the rows that count: n_valid is NULL (every step uses
 * its whole batch: this IS iqlhip_train_steps, bit for bit) or a device int32[n_steps] with
 * 1 <= n_valid[i] <= batch_size (values outside are clamped into that range on the device).
 * Step i then forms its three losses, their gradients and the logged means over rows [0, n_valid[i])
 * of its batch only, dividing by n_valid[i]; rows beyond it are gathered like any other (their
 * indices must point into the buffer) and contribute nothing.  A step with n_valid[i] == batch_size
 * equals the step without counts bit for bit.  This is the short last batch of an epoch of
 * algorithms/custom_offline/iql_bb.py (RandomBatchSampler, drop_last=False).
 * Supported on the tuned three-kernel step at precision fp32, plain launches and graph replay (a
 * k_backward instantiation of its own: calls without counts run the kernels they always ran).  On
 * the general layer-wise step, or at precision bf16, a non-NULL n_valid returns
 * IQLHIP_ERR_UNSUPPORTED before anything is launched (the counts live on the device: the call
 * cannot see whether they all equal batch_size).  Seed groups of such trainers take counts through
 * iqlhip_group_train_steps_valid.                                                               */
int iqlhip_train_steps_valid(iqlhip_trainer *t, const iqlhip_replay_view *view, int64_t n_steps,
                             const int64_t *idx, const int32_t *n_valid, const uint8_t *dropout_keep,
                             float *losses_out, int32_t graph_unroll, void *stream);

/* ------------------------------------------------------------------------ */
/* Seed groups: K independent trainers of ONE shape (dims, hidden layers,      */
/* batch, precision, critics, policy kind, dropout on/off) stepped by one      */
/* launch sequence -- the three kernels of a step run once for all K members.  */
/* All members run on the tuned step or all on the general step (a mix is      */
/* IQLHIP_ERR_INVALID).  The seeds share nothing;                              */
/* each one's arithmetic is bit-identical to stepping it alone.  This is the   */
/* path's sharding unit (one (seed, dataset) run, ensemble_sweeps/launch.sh:   */
/* 12 AGENTS_PER_GPU, :84-94) used inside one GPU.                              */
/* While a trainer is a member, its own iqlhip_train_* calls keep working;     */
/* destroy the group before its members.  views[k], idx[k], dropout_keep[k],   */
/* losses_out[k] belong to member k (idx / dropout_keep / losses_out may be    */
/* NULL as a whole or per member; meaning as in iqlhip_train_steps).           */
/* ------------------------------------------------------------------------ */
#define IQLHIP_MAX_GROUP 16
typedef struct iqlhip_group iqlhip_group;
int iqlhip_group_create(iqlhip_group **out, iqlhip_trainer *const *trainers, int32_t n);
int iqlhip_group_destroy(iqlhip_group *g);
int iqlhip_group_train_steps(iqlhip_group *g, const iqlhip_replay_view *views, int64_t n_steps,
                             const int64_t *const *idx, const uint8_t *const *dropout_keep,
                             float *const *losses_out, int32_t graph_unroll, void *stream);

/* iqlhip_group_train_steps with per-step valid-row counts: n_valid is NULL as a whole (this IS
 * iqlhip_group_train_steps, bit for bit) or an array of K entries, each NULL (that member uses its whole
 * batch in every step) or a device int32[n_steps] with the meaning and the clamping of
 * iqlhip_train_steps_valid; members may share one array.  Every member stays bit-identical to the same
 * trainer stepped alone by iqlhip_train_steps_valid.  With any non-NULL entry the one launch of k_backward
 * is its counted instantiation for all members; the group's captured graph is keyed on that, and a call
 * with counts never continues the previous call (its arguments are always sent).  Plain launches and graph
 * replay.  A non-NULL entry for a group on the general layer-wise step, or at precision bf16, returns
 * IQLHIP_ERR_UNSUPPORTED before anything is launched.                                               */
int iqlhip_group_train_steps_valid(iqlhip_group *g, const iqlhip_replay_view *views, int64_t n_steps,
                                   const int64_t *const *idx, const int32_t *const *n_valid,
                                   const uint8_t *const *dropout_keep, float *const *losses_out,
                                   int32_t graph_unroll, void *stream);

/* A HIP stream confined to one slice of the compute units: bit i of the CU mask belongs to
 * slice i % n_slices.  The mask enumerates the CUs round-robin over the 8 XCDs, so two slices
 * are the even and the odd XCDs: each sub-group keeps four L2s to itself and all memory channels
 * (slices that split every XCD in half instead measured 180k steps/s against 209k).  Two seed
 * groups stepped on the two slices overlap one group's HBM-bound update with the other's
 * latency-bound forward / backward: 8 seeds as 2 x 4 measured 205k steps/s against 171k as one
 * group of 8 on the whole chip (tools/group_streams.py).  No counterpart in the reference (its
 * AGENTS_PER_GPU processes share the GPU unmanaged).  Destroy with iqlhip_stream_destroy.   */
int iqlhip_stream_create_cu_slice(void **stream, int32_t slice, int32_t n_slices);
int iqlhip_stream_destroy(void *stream);

/* Which path ran: steps issued as plain launches (three per step; a group step counts once) and
 * hipGraph replays issued since the handle was created.  Either pointer may be NULL.          */
int iqlhip_trainer_launch_counts(iqlhip_trainer *t, int64_t *eager_steps, int64_t *graph_launches);
int iqlhip_group_launch_counts(iqlhip_group *g, int64_t *eager_steps, int64_t *graph_launches);

/* Per-kernel HIP-event timing of a group's launches (as iqlhip_trainer_set/get_timing). */
int iqlhip_group_set_timing(iqlhip_group *g, int32_t enable);
int iqlhip_group_get_timing(iqlhip_group *g, double avg_ms[3], int64_t *n_launches);

/* ref:639-662 train(batch) on an explicit batch of dense device tensors
 * (shapes as iqlhip_replay_sample produces them).                           */
int iqlhip_train_batch(iqlhip_trainer *t, const float *s, const float *a, const float *r,
                       const float *s2, const float *d, const uint8_t *dropout_keep,
                       float *losses_out, void *stream);

/* Forward passes on the live weights (ref:452-543), n rows (any n >= 1):
 *   which = 0: q1..qE -> out[n][E]   (needs a; E = 2 for TwinQ)
 *   which = 1: v     -> out[n]
 *   which = 2: actor mean (tanh)  -> out[n][A]   (eval mode: no dropout)
 *   which = 3: q_target1..E -> out[n][E]   (needs a)
 * out is dense and row-major: critic e of row i is out[i * E + e].  Exactly the first n rows of out
 * are written (a larger buffer keeps what it held beyond them) and n rows of s / a are read.  The
 * actor runs in eval mode whatever the trainer's dropout_p and however many training steps have
 * drawn masks: two calls on the same weights give the same bits.  which outside 0..3, n <= 0, a
 * NULL s / out (or a NULL a where it is needed) return IQLHIP_ERR_INVALID and write nothing.
 * Pinned over the whole shape envelope by tests/test_gpu_forward_envelope.py.                  */
int iqlhip_forward(iqlhip_trainer *t, int32_t which, const float *s, const float *a,
                   int64_t n, float *out, void *stream);

/* ------------------------------------------------------------------------ */
/* Stand-alone fp32 MLP forward (exact f32 MFMA)                              */
/*   - nn.Module.forward() of MLP/TwinQ/ValueFunction/policies outside the   */
/*     autocast region (ref:408-543; eval_actor ref:306-319);                 */
/*   - the Markovian reward model forward of the relabel paths               */
/*     (ref:719-724 MR, ref:986-991 BNN, ref:1176-1178 MR ensemble).          */
/* ------------------------------------------------------------------------ */
#define IQLHIP_MLP_MAX_LAYERS 8
typedef struct {
  int32_t n_layers;                          /* Linear layers, 1..8                */
  int32_t dims[IQLHIP_MLP_MAX_LAYERS + 1];   /* in, hidden..., out; each <= 1024    */
  const float *weights[IQLHIP_MLP_MAX_LAYERS]; /* device fp32                      */
  const float *biases[IQLHIP_MLP_MAX_LAYERS];  /* device fp32 [out]                */
  int32_t w_in_out;   /* 0: W[out][in] (torch nn.Linear); 1: W[in][out] (x @ W)  */
  int32_t hidden_act; /* 0 relu, 1 tanh; 8 + i: entry i of reward_models/q_mlp.py:121-130
                         (cos, tanh, relu, softplus, sin, leaky_relu, swish, none)  */
  int32_t out_act;    /* 0 none, 1 tanh; 8 + i as above                          */
  /* nn.Dropout(p) behind every hidden activation, as a module in train mode applies it
   * (ref:436-437; GaussianPolicy.act in train mode, ref:476-482): dropout_p <= 0 disables.
   * Masks: Philox4x32-10 keyed by dropout_seed, counter (row, dropout_call, unit / 4 | layer << 16,
   * stream 3) -- oracle/philox.py:mlp_dropout_keep; a caller passes a fresh dropout_call per
   * forward.  Kept values are multiplied by float(1 / (1 - p)) (ATen _dropout_impl).            */
  float dropout_p;
  uint32_t dropout_call;
  uint64_t dropout_seed;
} iqlhip_mlp_desc;

/* out[n][out_stride] (first dims[n_layers] columns) = MLP(x[n][x_stride]).  */
int iqlhip_mlp_forward(const iqlhip_mlp_desc *d, const float *x, int64_t n, int32_t x_stride,
                       float *out, int32_t out_stride, void *stream);

/* A frozen set of M MLPs of one shape, for one launch over rows of their own (the post-hoc
 * checkpoint evaluation, iqlpref_amd/posthoc.py: M checkpoints x R environments per lock step).
 *
 * iqlhip_mlp_set_create writes every member's fragment-major weight images and biases into ONE device
 * allocation of the current device that the set owns, and waits for `stream`: the set is a snapshot,
 * the source tensors may change or go afterwards.  All members share n_layers, dims, the activation
 * codes and w_in_out (else IQLHIP_ERR_INVALID); every width is <= 256 and dropout_p <= 0 (an eval-mode
 * forward), else IQLHIP_ERR_UNSUPPORTED: iqlhip_mlp_forward takes those.  M outside
 * 1..IQLHIP_MLP_SET_MAX, a null pointer anywhere, n_layers or an activation code outside
 * iqlhip_mlp_forward's range: IQLHIP_ERR_INVALID.  Every refusal happens before any HIP call and
 * leaves *out as it was.
 *
 * iqlhip_mlp_set_forward is one launch: no allocation, no host wait, no repack.
 *   out[(m R + r) out_stride + c] = MLP_m(x[(m R + r) x_stride + 0 .. dims[0]))[c],  m < M, r < R
 * with the bits iqlhip_mlp_forward(descs[m], that row, 1, ...) writes (both run the same row-tile
 * body).  Exactly M R rows and dims[n_layers] columns are written.  R < 1, a null pointer or a stride
 * below the width: IQLHIP_ERR_INVALID, nothing is launched; so is a call while another device than the
 * set's (the one current at create) is current.
 * Pinned by tests/test_gpu_posthoc.py.                                                            */
typedef struct iqlhip_mlp_set iqlhip_mlp_set;
#define IQLHIP_MLP_SET_MAX 1024
int iqlhip_mlp_set_create(const iqlhip_mlp_desc *const *descs, int32_t M, iqlhip_mlp_set **out, void *stream);
int iqlhip_mlp_set_destroy(iqlhip_mlp_set *set);
int iqlhip_mlp_set_forward(const iqlhip_mlp_set *set, const float *x, int32_t R, int32_t x_stride,
                           float *out, int32_t out_stride, void *stream);

/* ------------------------------------------------------------------------ */
/* Ensemble CVaR  (ref:1003-1011 BNN, ref:1185-1187 MR snapshots)             */
/*   out[c] = mean of the n_tail smallest of preds[0..S)[c],  c < N           */
/* preds: device fp32 [S][N] row-major (one row per posterior sample /         */
/* snapshot, filled with iqlhip_mlp_forward using out_stride = 1 into row k). */
/* n_tail = max(1, floor((1 - alpha) S)) (ref:935,1152); S <= 2400.           */
/* ------------------------------------------------------------------------ */
int iqlhip_cvar_tail_mean(const float *preds, int32_t S, int64_t N, int32_t n_tail, float *out,
                          void *stream);

/* ------------------------------------------------------------------------ */
/* Preference-transformer relabel  (ref:1223-1309 qlearning_dataset_pt)        */
/* Architecture: reward_models/pref_transformer.py:170-277 (PT), ops.py:6-117.  */
/* iqlhip_pt_relabel: one GPT-2 block, embd_dim 64 (the tuned streaming      */
/* kernel, csrc/pt.hip); iqlhip_pt_relabel_general: any depth and width of the */
/* envelope above (layer-wise, csrc/pt_general.hip).  Every pointer is device  */
/* fp32; "T" = stored transposed ([in][out]) relative to the torch /           */
/* state-dict [out][in] layout.                                                */
/* ------------------------------------------------------------------------ */
typedef struct {
  int32_t state_dim, action_dim;
  int32_t embd_dim;   /* must be 64                                             */
  int32_t num_heads;  /* power of two <= 16                                     */
  int32_t inter_dim;  /* GPT2MLP width, multiple of 256, <= 1024                */
  int32_t num_layers; /* must be 1                                              */
  int32_t n_temb;     /* rows of timestep_embed (max_episode_steps + 1)         */
  float eps;          /* LayerNorm epsilon                                      */
  const float *state_wT, *state_b;   /* state_linear  [S][64] T, [64]          */
  const float *action_wT, *action_b; /* action_linear [A][64] T, [64]          */
  const float *temb;                 /* timestep_embed.weight [n_temb][64]     */
  const float *sln_w, *sln_b;        /* stacked_layer_norm                     */
  const float *ln0_w, *ln0_b;        /* gpt.layers.0.layer_norm_0              */
  const float *qkv_w, *qkv_b;        /* attention.in_linear [192][64], [192]   */
  const float *attn_out_w, *attn_out_b; /* attention.out_linear.weight [64][64], [64] */
  const float *ln1_w, *ln1_b;        /* layer_norm_1                           */
  const float *mlp_in_w, *mlp_in_b;   /* mlp.in_linear.weight  [I][64], [I]   */
  const float *mlp_out_w, *mlp_out_b; /* mlp.out_linear.weight [64][I], [64]  */
  const float *lnf_w, *lnf_b;        /* gpt.layer_norm                         */
  const float *pref_w_last;          /* LAST row of pref_linear.weight [64]    */
  float pref_b_last;                 /* last element of pref_linear.bias       */
} iqlhip_pt_weights;

/* out[w] = value[:, 0, -1, 0] (ref:1301) of the window of win_len[w] consecutive
 * transitions obs/act[win_start[w] .. +win_len[w]), right-aligned in a
 * query_length window (ref:1269-1292); the timestep of the window's k-th transition is
 * win_t0[w] + k.  win_t0 == NULL: 0 for every window (ref:1281,1291: timesteps 0..len-1);
 * custom_offline/iql.py:183-211 passes the true episode step (win_t0[w] + len <= n_temb is the
 * caller's to guarantee).  Because attention is causal, the value at position i of ONE forward
 * over a window (custom_offline:172-192) equals the last-token value of its prefix of length
 * i + 1: per-position values are windows of growing length.
 * obs [n_rows][S], act [n_rows][A], win_start int64 [n_win], win_len int32
 * [n_win] (1 <= len <= query_length), win_t0 int32 [n_win] or NULL, all device.
 * Precondition (the window arrays live on the device, the entry point cannot read them):
 * win_start[w] >= 0, win_start[w] + win_len[w] <= n_rows, win_t0[w] >= 0,
 * win_t0[w] + win_len[w] <= n_temb.  The kernel clamps every window into these bounds, so a
 * window that violates them yields a value for the clamped window, never an out-of-bounds read. */
int iqlhip_pt_relabel(const iqlhip_pt_weights *w, const float *obs, const float *act, int64_t n_rows,
                      const int64_t *win_start, const int32_t *win_len, const int32_t *win_t0,
                      int64_t n_win, int32_t query_length, float *out, void *stream);

/* The general path: the weights of one GPT-2 block gpt.layers.{l} (E = embd_dim, I = inter_dim),
 * all device fp32 in the torch [out][in] layout.                                              */
typedef struct {
  const float *ln0_w, *ln0_b;           /* layer_norm_0 [E], [E]                        */
  const float *qkv_w, *qkv_b;           /* attention.in_linear [3E][E], [3E]            */
  const float *attn_out_w, *attn_out_b; /* attention.out_linear [E][E], [E]             */
  const float *ln1_w, *ln1_b;           /* layer_norm_1 [E], [E]                        */
  const float *mlp_in_w, *mlp_in_b;     /* mlp.in_linear [I][E], [I]                    */
  const float *mlp_out_w, *mlp_out_b;   /* mlp.out_linear [E][I], [E]                   */
} iqlhip_pt_block;

/* A whole PT for the general path.  The embedding, stacked-LN, final-LN and value-head pointers
 * are those of iqlhip_pt_weights, with E = embd_dim in place of 64; `blocks` is a HOST array of
 * num_layers block structs, read during the call only.                                        */
typedef struct {
  int32_t state_dim, action_dim;
  int32_t embd_dim;   /* multiple of 64, <= 256                                      */
  int32_t num_heads;  /* power of two, embd_dim / num_heads >= 4                     */
  int32_t inter_dim;  /* multiple of 64, <= 1024                                     */
  int32_t num_layers; /* 1..8                                                        */
  int32_t n_temb;     /* rows of timestep_embed (max_episode_steps + 1)              */
  float eps;          /* LayerNorm epsilon                                           */
  const float *state_wT, *state_b;   /* state_linear  [S][E] T, [E]                  */
  const float *action_wT, *action_b; /* action_linear [A][E] T, [E]                  */
  const float *temb;                 /* timestep_embed.weight [n_temb][E]            */
  const float *sln_w, *sln_b;        /* stacked_layer_norm                           */
  const float *lnf_w, *lnf_b;        /* gpt.layer_norm                               */
  const float *pref_w_last;          /* LAST row of pref_linear.weight [E]           */
  float pref_b_last;                 /* last element of pref_linear.bias             */
  const iqlhip_pt_block *blocks;     /* host [num_layers]                            */
} iqlhip_pt_model;

/* Device workspace (bytes) that lets iqlhip_pt_relabel_general take min(n_win, chunk cap)
 * windows of query_length in one pass; the chunk cap keeps the figure under 1 GiB.  Pure host
 * code; the shape checks are those of iqlhip_pt_relabel_general.                              */
int iqlhip_pt_general_workspace_bytes(const iqlhip_pt_model *m, int32_t query_length, int64_t n_win,
                                      size_t *bytes);

/* iqlhip_pt_relabel for every shape of the general envelope: the same windows, timesteps,
 * clamping and output, computed layer by layer over chunks of windows whose token matrices live in
 * `workspace` (device, workspace_bytes long, 16-byte aligned).  A workspace smaller than
 * iqlhip_pt_general_workspace_bytes(m, query_length, n_win) is used in several chunks; one that
 * holds no window is IQLHIP_ERR_INVALID.  Shapes outside the envelope return
 * IQLHIP_ERR_UNSUPPORTED before any HIP call.  Same arithmetic (bf16 q.k logits, fp32
 * elsewhere) as the tuned kernel.                                                              */
int iqlhip_pt_relabel_general(const iqlhip_pt_model *m, const float *obs, const float *act, int64_t n_rows,
                              const int64_t *win_start, const int32_t *win_len, const int32_t *win_t0,
                              int64_t n_win, int32_t query_length, void *workspace, size_t workspace_bytes,
                              float *out, void *stream);

/* ------------------------------------------------------------------------ */
/* numpy's legacy RandomState.randint (algorithms/custom_offline/iql.py:277-284 */
/* samples replay indices with it), bit for bit, on the device (np_sampler.hip) */
/* ------------------------------------------------------------------------ */
/* numpy RandomState.randint(0, hi[k], size=(n_batches, batch)) for K legacy MT19937 states.
 * state: device uint32 [K][625] = key[624], pos; read and advanced in place.
 * out[k]: device int64 [n_batches][batch].  1 <= hi[k] <= 2^32, 0 <= pos <= 624.
 * hi and out are host arrays of K entries.  Synchronises `stream` once, before the launch, to
 * read and check the K pos words; the draw itself is asynchronous.  1 <= K <= IQLHIP_MAX_GROUP,
 * batch >= 1, n_batches >= 0 (0 draws nothing).                                               */
int iqlhip_np_randint(uint32_t *state, const int64_t *hi, int32_t K, int32_t batch,
                      int64_t n_batches, int64_t *const *out, void *stream);

/* ------------------------------------------------------------------------ */
/* Online fine-tuning, algorithms/finetune/iql.py ("fref"): the three kernels   */
/* around the training step of one online tick (csrc/online.hip).  The tick     */
/* itself is a host loop (iqlpref_amd/finetune.py): act, env.step, append, one  */
/* iqlhip_train_steps call of one step.  fref runs without autocast: fp32 only. */
/* ------------------------------------------------------------------------ */
/* fref:164-180 add_transition, n >= 1 transitions at once: row (pointer + i) % capacity of the ring
 * rows[capacity][row_stride] receives transition i of the device fp32 staging arrays obs[n][S], act[n][A],
 * rew[n], next_obs[n][S], done[n], in the layout of iqlhip_replay_pack -- padding zeros and the 16-byte
 * aligned s' included, bit for bit what packing the same data into those rows writes.  Every other row
 * keeps its contents.  rows on a 16-byte boundary (whole rows are written as 16-byte pieces).
 * n > capacity, pointer outside [0, capacity), n < 1: IQLHIP_ERR_INVALID, nothing is launched.  The
 * caller advances its pointer / size (fref:179-180) and the generation of its views.                 */
int iqlhip_replay_append(float *rows, int32_t row_stride, int32_t state_dim, int32_t action_dim,
                         int64_t capacity, int64_t pointer, int64_t n, const float *obs, const float *act,
                         const float *rew, const float *next_obs, const float *done, void *stream);

/* numpy's RandomState.randint(0, hi_t, batch) for t = 0 .. n_steps - 1 as ONE stream, with
 * hi_t = min(hi0[k] + t * growth, cap[k]): the index draws of n_steps online ticks, whose buffer grows by
 * `growth` (0 or 1) rows per tick until it is full (fref:155-156, 180).  The values, and the MT19937 key and
 * position left behind, are those of n_steps successive host calls; a step with hi_t == 1 consumes no word
 * and yields zeros.  growth == 0 is iqlhip_np_randint.  state, K, out[k] (device int64 [n_steps][batch]), the
 * one synchronisation of `stream` before the launch and the pos check are as for iqlhip_np_randint; hi0 and
 * cap are host arrays of K entries, 1 <= hi0[k] <= cap[k] <= 2^32.  IQLHIP_ERR_INVALID before any launch
 * otherwise (the states are then untouched).  n_steps == 0 draws nothing.                            */
int iqlhip_np_randint_growing(uint32_t *state, const int64_t *hi0, const int64_t *cap, int32_t growth,
                              int32_t K, int32_t batch, int64_t n_steps, int64_t *const *out, void *stream);

/* fref:681-693, the action the online phase proposes, for rows >= 1 states s[rows][state_dim] at once:
 * the actor's forward on the LIVE fp32 master weights of the parameter arena (no copy is kept), then
 *   Gaussian policy        a = mean + exp(clamp(log_std, -20, 2)) * eps            (fref:687 dist.sample())
 *   deterministic policy   a = out + clamp(expl_noise * eps, -noise_clip, noise_clip)   (fref:689-692)
 *   out[rows][action_dim]  = clamp(max_action * a, -max_action, max_action)        (fref:693)
 * fref never takes the actor out of train mode for this forward (only eval_actor does, and it switches
 * back, fref:223,240): a trainer without actor dropout (fref's default 0.0 builds no Dropout layer) runs
 * the plain forward; one with dropout_p > 0 drops hidden units here too, as fref's actor(state) does --
 * masks of iqlhip_mlp_forward's convention keyed by the trainer's seed with dropout_call = call.
 * eps: device fp32 [rows][action_dim] standard normals as given (parity tests), or NULL: drawn from the
 * trainer's Philox key, block (row, call, column / 4, stream 4), words (x, y) and (z, w) one Box-Muller
 * pair each: u1 = (x + 1) 2^-32, u2 = y 2^-32, sqrt(-2 ln u1) (cos, sin)(2 pi u2).  `call`: a number the
 * caller never repeats for one trainer (the tick).  Two launches on `stream`, no synchronisation.  Every
 * trainer shape of the envelope, tuned or general step; precision bf16 is IQLHIP_ERR_UNSUPPORTED.    */
int iqlhip_explore_action(iqlhip_trainer *t, const float *s, int64_t rows, const float *eps,
                          float expl_noise, float noise_clip, float max_action, uint32_t call, float *out,
                          void *stream);

/* The tick of K seeds that train side by side (finetune.train(seeds_per_gpu = K)): the act and the append
 * of all members as ONE launch each, 1 <= K <= IQLHIP_MAX_GROUP.
 *
 * iqlhip_explore_action_group: row k of out[K][action_dim] is what
 *   iqlhip_explore_action(trainers[k], s + k * s_stride, 1, eps ? eps + k * action_dim : NULL, expl_noise,
 *                         noise_clip, max_action, calls[k], ...)
 * writes, BIT FOR BIT, over the trainer's whole envelope (either summation order of the stand-alone MLP
 * kernels, dropout masks, drawn or given noise): one work-group per member on the live fp32 masters, no
 * scratch, no second launch.  trainers and calls are host arrays of K entries (read during the call only);
 * s is device fp32 [K][s_stride], s_stride >= state_dim; eps is NULL or device fp32 [K][action_dim].  All
 * members are precision fp32 (bf16: IQLHIP_ERR_UNSUPPORTED) on one device with equal state_dim and
 * action_dim (else IQLHIP_ERR_INVALID); depth, width, policy kind, dropout and seed are each member's own.
 * Nothing is launched when a check fails.  No synchronisation.
 *
 * iqlhip_replay_append_group: one transition into each of K rings of one geometry.  stage is device fp32
 * [K][2 S + A + 2], transition k in the order s | a | r | s' | d; row pointer[k] % capacity[k] of
 * rows[k][capacity[k]][row_stride] receives what iqlhip_replay_append(n = 1) writes there, padding zeros
 * included; every other row keeps its contents.  rows, capacity and pointer are host arrays of K entries;
 * rows[k] distinct and on 16-byte boundaries, 0 <= pointer[k] < capacity[k], else IQLHIP_ERR_INVALID
 * before the launch.  The caller advances its pointers, sizes and generations.                       */
int iqlhip_explore_action_group(iqlhip_trainer *const *trainers, int32_t K, const float *s, int32_t s_stride,
                                const float *eps, float expl_noise, float noise_clip, float max_action,
                                const uint32_t *calls, float *out, void *stream);
int iqlhip_replay_append_group(float *const *rows, int32_t row_stride, int32_t state_dim, int32_t action_dim,
                               const int64_t *capacity, const int64_t *pointer, int32_t K, const float *stage,
                               void *stream);

/* ------------------------------------------------------------------------ */
/* Block-shuffled epochs of algorithms/custom_offline/iql_bb.py:208-267        */
/* (RandomBatchSampler: contiguous blocks of `batch` rows in ONE permuted       */
/* order that every epoch repeats, the rows left over as a short last batch)    */
/* ------------------------------------------------------------------------ */
/* For steps t0 .. t0 + n_steps - 1 of that walk: with nb = n_rows / batch whole blocks and
 * slots = ceil(n_rows / batch) steps per epoch, step t uses slot t % slots;
 *   slot <  nb: idx[i][j] = perm[slot] * batch + j,                 n_valid[i] = batch
 *   slot == nb: idx[i][j] = min(nb * batch + j, n_rows - 1),        n_valid[i] = n_rows % batch.
 * perm: device int64 [nb], a permutation of 0..nb-1 (values outside are clamped into it; may be
 * NULL when nb == 0).  idx: device int64 [n_steps][batch]; n_valid: device int32 [n_steps] -- what
 * iqlhip_train_steps_valid takes.  One launch on `stream`, no synchronisation.                    */
int iqlhip_block_epoch_indices(const int64_t *perm, int64_t n_rows, int32_t batch, int64_t t0,
                               int64_t n_steps, int64_t *idx, int32_t *n_valid, void *stream);

/* The same walk for the K members of a seed group, 1 <= K <= IQLHIP_MAX_GROUP, in ONE launch: perm and idx
 * are HOST arrays of K device pointers (read during the call only; they travel by value in the kernel's
 * argument block), idx[k] receives what iqlhip_block_epoch_indices writes for perm[k].  All members walk
 * the same n_rows and batch, so the short slot falls on the same step for all of them: n_valid is ONE
 * device int32 [n_steps], what every entry of iqlhip_group_train_steps_valid's n_valid may point to.
 * perm (or an entry of it) may be NULL only when there is no whole block.  No synchronisation.        */
int iqlhip_block_epoch_indices_group(const int64_t *const *perm, int64_t n_rows, int32_t batch, int64_t t0,
                                     int64_t n_steps, int64_t *const *idx, int32_t *n_valid, int32_t K,
                                     void *stream);

/* ------------------------------------------------------------------------ */
/* The BB flavour's evaluation simulator, algorithms/custom_offline/iql_bb.py   */
/* :675-867, on the device (csrc/bb_sim.hip): the state of ONE episode lives in  */
/* device memory, the actor's forward and one simulator step alternate on one    */
/* stream, and the host waits for nothing between them.  The host draws the      */
/* set-up and the whole drift table from numpy's generator and uploads them.     */
/* ------------------------------------------------------------------------ */
typedef struct {
  int32_t n_obs;       /* obstacles, 1..1024 (the levels have 50 / 100 / 150)                     */
  int32_t n_near;      /* obstacles in an observation, 1..min(n_obs, 16)                          */
  int32_t state_dim;   /* 2 + 3 n_near + 6: agent x y, (x y heading) per obstacle, goal x y, tail */
  int32_t action_dim;  /* 2: speed, heading in degrees                                            */
  int32_t max_horizon; /* >= 1                                                                    */
  int32_t actor_out_stride; /* 0: step t reads actor_out[0 .. 2) (the forward's live output row);
                               >= 2: it reads actor_out[t * stride ..), a table of injected rows  */
  double *state;       /* device f64 [8 + 3 n_obs]: agent x y, goal x y, level, ai, attempt, day,
                          ox[n_obs], oy[n_obs], oang[n_obs]; uploaded per episode, advanced in place */
  const double *drift; /* device f64 [max_horizon][n_obs]: the obstacles' drift of every step     */
  int32_t *ctl;        /* device int32 [2]: steps taken, done flag; once done (or at max_horizon)
                          [0] is the episode's length                                             */
  float *obs_hist;     /* device fp32 [max_horizon + 1][state_dim]: raw observations              */
  float *act_hist;     /* device fp32 [max_horizon][2]: clamped actions                           */
  double *record;      /* device f64 [max_horizon + 1][state_dim]: every observation, unrounded   */
  float *actor_in;     /* device fp32 [state_dim]: (observation - mean) / std, formed in double and
                          rounded once: the row the next forward reads                            */
  float *actor_out;    /* device fp32: see actor_out_stride                                       */
  const double *state_mean, *state_std; /* device f64 [state_dim]                                 */
  const float *min_actions, *max_actions; /* device fp32 [2]: the clamp of bref:344-350           */
} iqlhip_bb_sim;

/* Observation row 0 (record, obs_hist, actor_in) from the set-up in `state`; ctl = {0, 0}.  One launch. */
int iqlhip_bb_sim_reset(const iqlhip_bb_sim *sim, void *stream);
/* One simulator step, one launch: with t = ctl[0], nothing at all is written when ctl[1] is set or
 * t == max_horizon; otherwise the action row is clamped per component in fp32 (torch.clamp) and stored as
 * act_hist[t]; the agent moves by speed * (cos, sin)(heading) in numpy's float32 arithmetic (what the
 * reference's scalar expressions evaluate to, see csrc/bb_sim.hip) and the obstacles by drift[t] along
 * their headings in float64, one that leaves the disc of radius 50 re-entering at its mirrored OLD
 * position; the goal counts as reached when the closest point of the agent's segment lies within
 * (0.3 + 1)^2 of it (np.isclose included); observation row t + 1 and the next actor input are written,
 * ctl[0] = t + 1 and ctl[1] = reached.  The nearest obstacles are taken in ascending distance, ties by
 * lowest index.                                                                                      */
int iqlhip_bb_sim_step(const iqlhip_bb_sim *sim, void *stream);
/* n_steps >= 1 times { iqlhip_mlp_forward(actor, actor_in, 1 row) -> actor_out; iqlhip_bb_sim_step }
 * on `stream`, no synchronisation: steps queued behind the end of the episode write nothing.  `actor`
 * maps state_dim inputs to 2 outputs (the policy's net in eval mode: dropout_p <= 0 is the caller's
 * to set); actor_out_stride must be 0.
 * All three refuse, before any launch: a null pointer (IQLHIP_ERR_INVALID), n_obs outside 1..1024,
 * n_near outside 1..min(n_obs, 16), action_dim != 2 (IQLHIP_ERR_UNSUPPORTED), state_dim !=
 * 2 + 3 n_near + 6, max_horizon < 1, actor_out_stride 1 or negative (IQLHIP_ERR_INVALID).           */
int iqlhip_bb_sim_rollout(const iqlhip_bb_sim *sim, const iqlhip_mlp_desc *actor, int32_t n_steps,
                          void *stream);

/* n whole episodes in ONE launch (k_bb_episodes, csrc/bb_sim.hip), one work-group per episode: what
 * iqlhip_bb_sim_reset and then max_horizon times { forward of actors[k] on actor_in; iqlhip_bb_sim_step }
 * leave behind for sims[k] -- ctl, record, obs_hist, act_hist, actor_in, state bit for bit, nothing past
 * the episode's last row -- without a launch between the steps.  The forward is the arithmetic of
 * iqlhip_mlp_forward for one row: equal input rows give equal action bits on both paths.  1 <= n <=
 * IQLHIP_MAX_GROUP; the episodes share nothing (the members of a seed group, each with its own buffers).
 * A sim with actor_out_stride != 0 reads row t of its injected table at step t and runs no forward;
 * its actors[k] may be NULL.
 * scratch: device memory the caller owns, 16-byte aligned, at least iqlhip_bb_sim_episodes_scratch_bytes
 * long: the per-episode argument blocks and one fragment-major weight image per actor, written once per
 * call, on `stream`; it stays in use until the work queued on `stream` has finished.  No allocation, no
 * synchronisation.
 * Refused before any HIP call: a null sims / actors / scratch, n out of range, what the three calls above
 * refuse for any sims[k], a NULL actors[k] without an injected table, an actor that does not map
 * state_dim -> 2 or has a null weight pointer, too little scratch (IQLHIP_ERR_INVALID); an actor outside
 * the fused forward's envelope -- a width above 256, an activation code other than 0 / 1, dropout_p > 0
 * (IQLHIP_ERR_UNSUPPORTED: iqlhip_bb_sim_rollout takes those).                                        */
int iqlhip_bb_sim_episodes_scratch_bytes(const iqlhip_mlp_desc *const *actors, int32_t n, size_t *bytes);
int iqlhip_bb_sim_episodes(const iqlhip_bb_sim *sims, const iqlhip_mlp_desc *const *actors, int32_t n,
                           void *scratch, size_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------ */
/* Posterior relabel of algorithms/custom_offline/iql_br.py:179-253: per       */
/* transition, n_samps draws of np.random.choice over the S posterior          */
/* predictions on numpy's legacy generator, reduced on the device              */
/* (posterior_choice.hip)                                                      */
/* ------------------------------------------------------------------------ */
#define IQLHIP_CHOICE_MEAN 0
#define IQLHIP_CHOICE_MEDIAN 1

/* Device workspace (bytes) with which iqlhip_posterior_choice runs at its full chunk size: a ring of
 * uint16 index chunks, O(chunk) -- it does not grow with N beyond one chunk.  Pure host code; the
 * envelope checks are those of iqlhip_posterior_choice.                                         */
int iqlhip_posterior_choice_workspace_bytes(int32_t S, int64_t N, int32_t n_samps, size_t *bytes);

/* out[c] = mean or median over j < n_samps of preds[idx[c][j]][c], where idx is
 * RandomState.randint(0, S, size=(N, n_samps)) continued from `state` -- what N consecutive
 * np.random.choice(preds[:, c], n_samps) calls draw (iql_br.py:179-186).
 * state: device uint32 [625] = key[624], pos (the layout of iqlhip_np_randint); read and advanced
 * in place; afterwards pos sits one past the word that produced the last accepted value.
 * preds: device fp32 [S][N] row-major (the layout iqlhip_cvar_tail_mean takes).
 * mode: IQLHIP_CHOICE_MEAN (fp32 sum / n_samps; n_samps == 1 is the single posterior draw, exact)
 * or IQLHIP_CHOICE_MEDIAN (numpy's: the middle value, or (a + b) * 0.5f of the two middle ones).
 * out: device fp32 [N].  idx_out: device uint16 [N][n_samps] or NULL; it receives the drawn indices
 * (tests pin the stream with it, production passes NULL: the indices then never exist in full).
 * workspace: device, 16-byte aligned, workspace_bytes long.  One smaller than
 * iqlhip_posterior_choice_workspace_bytes is used in smaller chunks; one that holds no 32-row
 * chunk is IQLHIP_ERR_INVALID.  It stays in use until the work queued on `stream` has finished.
 * Envelope, refused with IQLHIP_ERR_INVALID before anything is launched: 2 <= S <= 2400,
 * 1 <= n_samps <= 1024, N >= 1, pos <= 624.  Synchronises `stream` once, before the first launch,
 * to read and check pos.  The index draw runs on an internal stream, the reductions on `stream`;
 * when the call returns, `stream` is ordered behind both.                                        */
int iqlhip_posterior_choice(uint32_t *state, const float *preds, int32_t S, int64_t N, int32_t n_samps,
                            int32_t mode, float *out, uint16_t *idx_out, void *workspace,
                            size_t workspace_bytes, void *stream);

/* Algorithmic traffic and work of one step for this configuration
 * (SURVEY.md section 8d): bytes = 4B(2S+A+2) + 32 P_train + 8 P_q.          */
int iqlhip_step_cost(const iqlhip_trainer_config *cfg, double *bytes, double *flops);

/* HIP-event timing of the kernels of the most recent iqlhip_train_steps call
 * made with timing enabled (bench.py roofline leg).  enable != 0 brackets
 * every launch of the dominant kernel with events on `stream`.              */
int iqlhip_trainer_set_timing(iqlhip_trainer *t, int32_t enable);
/* avg_ms[3] = mean duration of the forward / backward / update kernels, with
 * the cost of an empty event pair (measured in the same pass) subtracted.    */
int iqlhip_trainer_get_timing(iqlhip_trainer *t, double avg_ms[3], int64_t *n_launches);

/* ------------------------------------------------------------------------ */
/* Any-percent behaviour cloning (algorithms/minari/any_percent_bc.py,        */
/* "bcref"; csrc/bc_step.hip): ONE network, Actor [S,256] ReLU [256,256] ReLU  */
/* [256,A] Tanh times max_action (bcref:195-209), F.mse_loss(pi, action)       */
/* (bcref:235-236), plain Adam (bcref:330).  Two launches per step.            */
/* Envelope (anything else: IQLHIP_ERR_UNSUPPORTED before any HIP call):       */
/* precision fp32, hidden_dim 256, n_hidden 0 or 2, state_dim <= 128,          */
/* action_dim <= 32, no dropout, any batch_size >= 1 (padded to whole 16-row   */
/* slabs inside, the mean counts the batch_size x action_dim real elements),   */
/* 1..IQLHIP_MAX_GROUP members per group.                                      */
/* Of iqlhip_trainer_config these fields are read: state_dim, action_dim,      */
/* hidden_dim, n_hidden, batch_size, precision, dropout_p, lr_actor (the Adam  */
/* lr, no schedule), adam_beta1, adam_beta2, adam_eps.  Of iqlhip_arenas:      */
/* params, exp_avg, exp_avg_sq, grads (optional); target is ignored.           */
/* ------------------------------------------------------------------------ */
/* Element offsets of W_1[256][S] b_1[256] W_2[256][256] b_2[256] W_3[A][256] b_3[A] (torch
 * [out][in] row-major, packed in this order) in the arenas, and their length.               */
int iqlhip_bc_arena_layout(const iqlhip_trainer_config *cfg, int64_t offsets[6], int64_t *n_params);

typedef struct iqlhip_bc iqlhip_bc;
/* Borrows the arenas for the trainer's lifetime; allocates its workspace (the padded copy of
 * every weight matrix that the forward reads, the transposed copies of W_2 and W_3 that the
 * backward reads, the feature-major activation and dz planes) on the current device and builds
 * the copies from the masters.  Synchronises the default stream once.                        */
int iqlhip_bc_create(iqlhip_bc **out, const iqlhip_trainer_config *cfg, float max_action,
                     const iqlhip_arenas *arenas);
int iqlhip_bc_destroy(iqlhip_bc *t);
/* Rebuild the copies from the masters (after the arenas were written from outside).          */
int iqlhip_bc_sync_weights(iqlhip_bc *t, void *stream);
/* Optimiser steps taken so far = Adam `step` (the bias corrections of the next step).        */
int iqlhip_bc_set_step(iqlhip_bc *t, int64_t total_it);
int iqlhip_bc_set_lr(iqlhip_bc *t, double lr);
/* bcref:339-341 n_steps times: gather rows idx[i][0..batch) of the view (its s and a columns),
 * forward, mse loss, backward, Adam.  idx: device int64[n_steps][batch], required (the index
 * stream is the caller's: numpy's, custom_offline.NumpyIndexStream); values outside the view
 * are clamped into it.  losses_out: NULL or device fp32[n_steps] (actor_loss of each step).
 * Plain launches on `stream`; at most ~2048 steps are left queued ahead of the device.       */
int iqlhip_bc_train_steps(iqlhip_bc *t, const iqlhip_replay_view *view, int64_t n_steps,
                          const int64_t *idx, float *losses_out, void *stream);
/* One of the copies the kernels read, device to device into dst (tests): which = 0 W_1 copy
 * [256][S padded to 16], 1 W_2 copy [256][256], 2 W_3 copy [A padded to 16][256], 3 W_2
 * transposed [256][256], 4 W_3 transposed [256][A padded to 16].  Padding is zero.           */
int iqlhip_bc_copy_out(iqlhip_bc *t, int32_t which, float *dst, void *stream);

/* K trainers of one shape (dims, batch size, max_action) stepped by the same two launches per
 * step, the member as a launch coordinate.  Each member is bit-identical to stepping it alone.
 * views[k], idx[k], losses_out[k] belong to member k (losses_out NULL as a whole or per member).
 * Destroy the group before its members.                                                      */
typedef struct iqlhip_bc_group iqlhip_bc_group;
int iqlhip_bc_group_create(iqlhip_bc_group **out, iqlhip_bc *const *members, int32_t n);
int iqlhip_bc_group_destroy(iqlhip_bc_group *g);
int iqlhip_bc_group_train_steps(iqlhip_bc_group *g, const iqlhip_replay_view *views, int64_t n_steps,
                                const int64_t *const *idx, float *const *losses_out, void *stream);

/* ------------------------------------------------------------------------ */
/* Offline AWAC (algorithms/offline/awac.py, "awac"; csrc/awac_step.hip): an   */
/* actor Linear(S,H) ReLU Linear(H,H) ReLU Linear(H,H) ReLU Linear(H,A) with a */
/* _log_std[A] parameter, two critics of the same shape on (s | a) ending in   */
/* Linear(H,1), their two Polyak targets (awac:134-215); update() as           */
/* awac:301-310: critics (MSE against r + gamma (1 - d) min Q_target(s', a'),  */
/* a' sampled from the live actor), then the actor (mean of                    */
/* -min(exp((q - v) / lambda), exp_adv_max) log_prob(a | s) at the critics     */
/* just updated), then the targets.  Plain Adam, four launches per step.       */
/* Envelope (anything else: IQLHIP_ERR_UNSUPPORTED before any HIP call):       */
/* precision fp32, n_hidden 3, hidden_dim a multiple of 16 in 16..256,         */
/* state_dim <= 128, action_dim <= 32, no dropout, batch_size 1..65536 (padded */
/* to whole 16-row slabs inside, the means count the batch_size real rows),    */
/* 1..IQLHIP_MAX_GROUP members per group.                                      */
/* Of iqlhip_trainer_config these fields are read: state_dim, action_dim,      */
/* hidden_dim, n_hidden, batch_size, precision, dropout_p, discount (gamma),   */
/* beta (awac_lambda),      lr_q (critic 1), lr_v (critic 2), lr_actor,        */
/* adam_beta1, adam_beta2, adam_eps (one set for the three optimisers), seed   */
/* (the Philox key of the action noise).  Of iqlhip_arenas: all five (grads    */
/* optional).                                                                  */
/* ------------------------------------------------------------------------ */
/* Element offsets in the parameter arena, every tensor on a 128-byte line, torch [out][in]
 * row-major: actor W_1 b_1 .. W_4 b_4, _log_std, critic 1 W_1 b_1 .. W_4 b_4, critic 2 the same
 * (25 offsets), and the arena lengths.  The target arena holds the two critics' part of the
 * layout: a target tensor sits at its critic's offset minus offsets[9] (critic 1's W_1).       */
int iqlhip_awac_arena_layout(const iqlhip_trainer_config *cfg, int64_t offsets[25], int64_t *n_params,
                             int64_t *n_target);

typedef struct iqlhip_awac iqlhip_awac;
/* Borrows the arenas for the trainer's lifetime; allocates its workspace (padded forward copies
 * of every weight matrix of the five networks, transposed copies of layers 2..4 of the three
 * trained ones, the feature-major activation and dz planes, the last step's eps) on the current
 * device and builds the copies from the masters.  Synchronises the default stream once.
 * tau: the Polyak coefficient in double -- awac:215 multiplies by float32(1 - tau) and float32(tau)
 * of the Python double, and 1 - cfg->tau (already fp32) can be one ulp away from the former; cfg->tau
 * is not read.                                                                                 */
int iqlhip_awac_create(iqlhip_awac **out, const iqlhip_trainer_config *cfg, double tau, float exp_adv_max,
                       const iqlhip_arenas *arenas);
int iqlhip_awac_destroy(iqlhip_awac *t);
/* Rebuild the copies from the masters and targets (after the arenas were written from outside). */
int iqlhip_awac_sync_weights(iqlhip_awac *t, void *stream);
/* Updates taken so far = Adam `step` of the three optimisers and the step of the noise streams. */
int iqlhip_awac_set_step(iqlhip_awac *t, int64_t total_it);
int iqlhip_awac_set_lr(iqlhip_awac *t, double lr_actor, double lr_critic_1, double lr_critic_2);
/* awac:301-310 n_steps times on rows idx[i][0..batch) of the view.  idx: device int64
 * [n_steps][batch], required (the index stream is the caller's); values outside the view are
 * clamped into it.  eps: device fp32 [n_steps][2][batch][action_dim] -- [i][0] the standard
 * normals of a' (awac:269), [i][1] those of pi (awac:250) -- or NULL: drawn from the Philox key
 * `seed`, Box-Muller on block (row * 8 + column / 4, step lo, step hi, stream 5 | 6), words
 * (x, y) and (z, w) one pair each: u1 = (x + 1) 2^-32, u2 = y 2^-32 -> sqrt(-2 ln u1)
 * (cos, sin)(2 pi u2) in double; step = the update's zero-based count.  losses_out: NULL or
 * device fp32 [n_steps][2] (critic_loss, actor_loss).  Plain launches on `stream`; at most
 * ~1024 steps are left queued ahead of the device.                                            */
int iqlhip_awac_train_steps(iqlhip_awac *t, const iqlhip_replay_view *view, int64_t n_steps,
                            const int64_t *idx, const float *eps, float *losses_out, void *stream);
/* Device to device into dst (tests, replays): which = 0 the eps of the last step
 * [2][batch][action_dim]; 1 + 7 net + c, net = 0 actor, 1 critic 1, 2 critic 2, 3 target 1,
 * 4 target 2: c = 0..3 the forward copy of Linear c + 1 [out padded to 16][in padded to 16],
 * c = 4..6 the transposed copy of Linear c - 2 [in padded][out padded] (trained nets only; a
 * critic's single output is padded to 16).  Padding is zero.                                  */
int iqlhip_awac_copy_out(iqlhip_awac *t, int32_t which, float *dst, void *stream);

/* K trainers of one shape (dims, width, batch size, gamma, tau, lambda, exp_adv_max) stepped by
 * the same four launches per step, the member as a launch coordinate.  Each member is
 * bit-identical to stepping it alone.  views[k], idx[k], eps[k], losses_out[k] belong to member k
 * (eps and losses_out NULL as a whole or per member).  Destroy the group before its members.  */
typedef struct iqlhip_awac_group iqlhip_awac_group;
int iqlhip_awac_group_create(iqlhip_awac_group **out, iqlhip_awac *const *members, int32_t n);
int iqlhip_awac_group_destroy(iqlhip_awac_group *g);
int iqlhip_awac_group_train_steps(iqlhip_awac_group *g, const iqlhip_replay_view *views, int64_t n_steps,
                                  const int64_t *const *idx, const float *const *eps, float *const *losses_out,
                                  void *stream);

/* ------------------------------------------------------------------------ */
/* Offline TD3+BC (algorithms/offline/td3_bc.py, "tdbc"; csrc/td3_bc_step.hip): */
/* an actor Linear(S,H) ReLU Linear(H,H) ReLU Linear(H,A) Tanh times           */
/* max_action, two critics Linear(S+A,H) ReLU Linear(H,H) ReLU Linear(H,1), a  */
/* Polyak target of each of the three (tdbc:244-282); train() as tdbc:324-380: */
/* the critics every step (MSE against r + (1 - d) discount min Q_target(s',   */
/* a'), a' the target actor plus clipped noise), and when total_it %           */
/* policy_freq == 0 the actor (-lmbda mean Q1(s, pi) + mse(pi, a), lmbda =     */
/* alpha / mean|Q1(s, pi)| at the critic 1 just updated) and the three         */
/* targets.  Plain Adam; two launches per step, five on an actor step.         */
/* Envelope (anything else: IQLHIP_ERR_UNSUPPORTED before any HIP call):       */
/* precision fp32, n_hidden 2, hidden_dim a multiple of 16 in 16..256,         */
/* state_dim <= 128, action_dim <= 32, no dropout, batch_size 1..65536 (padded */
/* to whole 16-row slabs inside, the means count the batch_size real rows),    */
/* policy_freq >= 1, 1..IQLHIP_MAX_GROUP members per group.                    */
/* Of iqlhip_trainer_config these fields are read: state_dim, action_dim,      */
/* hidden_dim, n_hidden, batch_size, precision, dropout_p, discount, lr_q      */
/* (critic 1), lr_v (critic 2), lr_actor, adam_beta1, adam_beta2, adam_eps     */
/* (one set for the three optimisers), seed (the Philox key of the noise).     */
/* Of iqlhip_arenas: all five (grads optional).                                */
/* ------------------------------------------------------------------------ */
/* Element offsets in the parameter arena, every tensor on a 128-byte line, torch [out][in]
 * row-major: actor W_1 b_1 .. W_3 b_3, critic 1 the same, critic 2 the same (18 offsets), and the
 * arena length.  The target arena has the same length and layout: a target tensor sits at the
 * offset of the tensor it follows.                                                              */
int iqlhip_td3bc_arena_layout(const iqlhip_trainer_config *cfg, int64_t offsets[18], int64_t *n_params);

typedef struct iqlhip_td3bc iqlhip_td3bc;
/* Borrows the arenas for the trainer's lifetime; allocates its workspace (padded forward copies
 * of every weight matrix of the six networks, transposed copies of Linear 2 and 3 of the three
 * trained ones and of critic 1's Linear 1, the feature-major activation and dz planes, the last
 * step's eps) on the current device and builds the copies from the masters.  Synchronises the
 * default stream once.  tau in double, as iqlhip_awac_create takes it (cfg->tau is not read).
 * policy_noise and noise_clip arrive already multiplied by max_action (tdbc:473-474).          */
int iqlhip_td3bc_create(iqlhip_td3bc **out, const iqlhip_trainer_config *cfg, double tau, float policy_noise,
                        float noise_clip, float max_action, float alpha, int64_t policy_freq,
                        const iqlhip_arenas *arenas);
int iqlhip_td3bc_destroy(iqlhip_td3bc *t);
/* Rebuild the copies from the masters and targets (after the arenas were written from outside). */
int iqlhip_td3bc_sync_weights(iqlhip_td3bc *t, void *stream);
/* total_it: train() calls so far = Adam `step` of the two critic optimisers, the step of the noise
 * stream, and what decides the actor steps; actor_it: Adam `step` of the actor's optimiser (its
 * own count: total_it / policy_freq for a fresh trainer).                                      */
int iqlhip_td3bc_set_step(iqlhip_td3bc *t, int64_t total_it, int64_t actor_it);
int iqlhip_td3bc_set_lr(iqlhip_td3bc *t, double lr_actor, double lr_critic_1, double lr_critic_2);
/* tdbc:324-380 n_steps times on rows idx[i][0..batch) of the view.  idx: device int64
 * [n_steps][batch], required; values outside the view are clamped into it.  eps: device fp32
 * [n_steps][batch][action_dim], the standard normals of tdbc:333, or NULL: drawn from the Philox
 * key `seed` as iqlhip_awac_train_steps draws them, on stream 7.  losses_out: NULL or device fp32
 * [n_steps][2] (critic_loss, actor_loss; actor_loss is 0 on a step without an actor update).
 * Plain launches on `stream`; at most ~1024 steps are left queued ahead of the device.         */
int iqlhip_td3bc_train_steps(iqlhip_td3bc *t, const iqlhip_replay_view *view, int64_t n_steps,
                             const int64_t *idx, const float *eps, float *losses_out, void *stream);
/* Device to device into dst (tests, replays): which = 0 the eps of the last step
 * [batch][action_dim]; 1 + 6 net + c, net = 0 actor, 1 critic 1, 2 critic 2, 3 actor target,
 * 4 target 1, 5 target 2: c = 0..2 the forward copy of Linear c + 1 [out padded to 16][in padded
 * to 16], c = 3..5 the transposed copy of Linear c - 2 [in padded][out padded] (Linear 2 and 3 of
 * the trained nets, Linear 1 of critic 1 only).  Padding is zero.                              */
int iqlhip_td3bc_copy_out(iqlhip_td3bc *t, int32_t which, float *dst, void *stream);

/* K trainers of one shape (dims, width, batch size) stepped by the same launches, the member as
 * a launch coordinate; every hyperparameter, policy_freq and the step counts are the member's
 * own, and the actor launches are issued on a step on which any member's actor steps.  Each
 * member is bit-identical to stepping it alone.  views[k], idx[k], eps[k], losses_out[k] belong
 * to member k (eps and losses_out NULL as a whole or per member).  Destroy the group before its
 * members.                                                                                    */
typedef struct iqlhip_td3bc_group iqlhip_td3bc_group;
int iqlhip_td3bc_group_create(iqlhip_td3bc_group **out, iqlhip_td3bc *const *members, int32_t n);
int iqlhip_td3bc_group_destroy(iqlhip_td3bc_group *g);
int iqlhip_td3bc_group_train_steps(iqlhip_td3bc_group *g, const iqlhip_replay_view *views, int64_t n_steps,
                                   const int64_t *const *idx, const float *const *eps, float *const *losses_out,
                                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* IQLHIP_H */
