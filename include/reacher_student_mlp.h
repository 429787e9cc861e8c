/* reacher_student_mlp.h -- C ABI of the reference's own MLP student: forward and one
 * distillation training step on a batch of rows, and its closed-loop evaluation over whole
 * episodes (rdm_evaluate), and its batched on-policy distillation over persistent envs
 * (rdm_step_envs) (libreacher.so).
 *
 * Graph: student_mlp_graph (reference src/distilation/student_nn.py:51-57)
 *     x[16] -> dense 24, tanh -> dense 128, tanh -> dense 128 -> dense 32, tanh -> dense 4
 * x row = dropout(ob)[11] | prev_pdflat[4] | prev_rew[1]   (mlp_train.py:38-52; the caller
 * assembles rows, keep_prob = 1), output = s_pdflat = mean[2] | logstd[2] (a state-dependent
 * log-std, unlike MlpPolicy's free logstd).
 * Flat parameters (RDM_PARAMS = 24,380 floats), tf.layers.dense order per layer:
 *     kernel W[in][out] row-major, then bias[out];  layers 16x24, 24x128, 128x128, 128x32, 32x4.
 * Loss: kl_loss(s_pdflat, t_pdflat) (reference loss.py:3-13: sum over rows of KL(s||t)),
 * or action-MSE: sum over rows of |mu_s - mu_t|^2 / (2 n_global).
 * Optimiser: TF1 Adam (mlp_train.py:73-80), f32 master weights and slots.
 *
 * Arithmetic (the dtype of rdm_create_dtype).  RDM_DTYPE_F32 (rdm_create): exact f32 products everywhere.
 * RDM_DTYPE_BF16, mixed precision: master weights, Adam slots, biases, tanh, the loss, db and every
 * accumulation stay f32.  Layers 0 (16->24) and 4 (32->4), 2.1 % of the MACs, keep the f32 products
 * (forward, dW, db, layer 4's dgrad), so neither the raw inputs nor the emitted mean and log-std are
 * cut to 8 bits.  Layers 1, 2, 3 (24->128, 128->128, 128->32) round their matrix operands to bf16,
 * bf = round-to-nearest-even (v_cvt_pk_bf16_f32), products exact, sums f32:
 *     forward  z  = b + sum_k bf(x_k) bf(W_kc)
 *     dgrad    dH = sum_m bf(dZ_m) bf(W_cm),  dZ = dH (1 - H^2) with the f32 activation H
 *     wgrad    dW = sum_rows bf(H) bf(dZ),    db = sum_rows dZ (unrounded)
 * The bf16 weights are roundings of the master, re-formed by rdm_set_params and every Adam step.
 * Every path of the handle runs the same forward: rdm_forward, the training launch, rdm_evaluate
 * and the envs calls, so the bitwise contracts below hold in either mode.  The teacher stays f32.
 *
 * Conventions as in reacher.h: device pointers (x 16-byte aligned), asynchronous on the
 * handle's stream, 0 = OK, RD_EINVAL, -(hipError_t).  Multi-GPU: rows sharded by the
 * caller; per step rdm_rollout(), all-reduce(SUM) rdm_grad_buffer(), rdm_apply().
 */
#ifndef REACHER_STUDENT_MLP_H
#define REACHER_STUDENT_MLP_H
#include <stdint.h>

#include "reacher.h"
#include "reacher_action_noise.h"   /* rd_action_noise: rdm_envs_set_action_noise, rdm_evaluate_noisy */
#include "reacher_obs_faults.h"     /* rd_obs_faults: rdm_envs_set_obs_faults, rdm_evaluate_faulty */
#include "reacher_replay.h"   /* rd_replay: rd_replay_push_rows_flags, below */

#ifdef __cplusplus
extern "C" {
#endif

#define RDM_PARAMS 24380
#define RDM_IN 16
#define RDM_OUT 4
#define RDM_LOSS_MSE 0
#define RDM_LOSS_KL 1
#define RDM_DTYPE_F32 0
#define RDM_DTYPE_BF16 1

typedef struct {
    int32_t loss;                  /* RDM_LOSS_*                                         */
    float lr, beta1, beta2, eps;   /* Adam (reference: 1e-4, .9, .999, 1e-8)             */
    int32_t grid;                  /* workgroups (64 rows each per pass); 0 = one per CU */
    int32_t metrics_len;           /* per-step metrics ring length; 0 = 4096             */
    float keep_prob;               /* dropout on the 11 ob inputs while training
                                      (tf.nn.dropout, mlp_train.py:50; reference KEEP_PROB =
                                      0.5); 1 = off.  Mask of input k of global row r at
                                      optimiser step S: keep iff u < keep_prob, u = word k%4
                                      of Philox4x32-10(ctr = {r lo, r hi, S, k/4}, key = seed),
                                      u = (word >> 8) * 2^-24; kept inputs are x / keep_prob */
    uint64_t seed;                 /* dropout key                                        */
    int64_t row_base;              /* global index of this rank's row 0 (sharded batches) */
} rdm_config;

typedef struct rdm_trainer rdm_trainer;

int rdm_param_count(void);
/* the 'MLP' scope: student graph, loss and Adam (mlp_train.py:35-80), in f32 */
int rdm_create(rdm_trainer** out, const rdm_config* cfg, int device, void* hip_stream);
/* rdm_create with the arithmetic of layers 1-3 chosen (RDM_DTYPE_*, "Arithmetic" above); RD_EINVAL for
 * another value.  rdm_config keeps its layout, so callers of rdm_create need no rebuild, and
 * rdm_create(cfg) == rdm_create_dtype(cfg, RDM_DTYPE_F32). */
int rdm_create_dtype(rdm_trainer** out, const rdm_config* cfg, int32_t dtype, int device, void* hip_stream);
int rdm_destroy(rdm_trainer* t);
int rdm_set_stream(rdm_trainer* t, void* hip_stream);
/* variable initialisation / restore (mlp_train.py:82-99): params [RDM_PARAMS] */
int rdm_set_params(rdm_trainer* t, const float* params);
int rdm_get_params(rdm_trainer* t, float* params);
/* Adam slots, beta powers and step counter to zero (mlp_train.py:93) */
int rdm_reset(rdm_trainer* t);
/* sess.run(s_pdflat_slice) (mlp_train.py:170-183), all rows: x [n][16] -> pdflat [n][4] */
int rdm_forward(rdm_trainer* t, const float* x, int64_t n, float* pdflat);
/* forward + loss + backward of n rows (of n_global over all ranks): gradient into
 * rdm_grad_buffer(); metrics (loss, sum |mu_s - mu_t|^2, rows) into the ring at apply */
int rdm_rollout(rdm_trainer* t, const float* x, const float* t_pdflat, int64_t n, int64_t n_global);
/* Adam on rdm_grad_buffer() (after an optional all-reduce), step counter + 1 */
int rdm_apply(rdm_trainer* t);
/* sess.run([loss, minimize_adam]) (mlp_train.py:145-160) == rollout + apply */
int rdm_step(rdm_trainer* t, const float* x, const float* t_pdflat, int64_t n);
float* rdm_grad_buffer(rdm_trainer* t);
int rdm_bind_grad_buffer(rdm_trainer* t, float* grad);
int rdm_get_counter(rdm_trainer* t, int64_t* opt_steps);
/* last `count` optimiser steps, oldest first: [count][4] = loss, sq err, rows, 0 */
int rdm_read_metrics(rdm_trainer* t, int64_t count, double* out);

/* The teacher of rdm_evaluate: the 2x64 MlpPolicy with its observation filter, same arguments as
 * rdd_set_teacher (device pointers: params [rdd_param_count()], ob_mean [11], ob_std [11]).  The
 * handle keeps its own copy of the net, from which every evaluation launch packs the LDS image
 * rdd_forward's kernel packs (the same function). */
int rdm_set_teacher(rdm_trainer* t, const float* params, const float* ob_mean, const float* ob_std);

/* Whole-episode evaluation of the reference student in one launch: n_envs evaluation envs (their
 * own states, kept in registers; no trainer's envs exist or are touched) run `episodes` consecutive
 * 50-step episodes, stepped with the student's unclipped mean.  It is the driver's phase-2 loop
 * (mlp_train.train(student="mlp"), reference mlp_train.py:143-204) without the optimiser steps.
 * Episode e of env i starts from reset draw draws[(e n_envs + i) 6 ..] (the table layout of
 * rd_set_reset_mode) or, with draws NULL, from Philox(seed, env_base + i, first_episode + e).
 * Step s = 0..49 of an episode, per env:
 *   ob_s  = observe(state)
 *   T_s   = the teacher's mean[2] | logstd[2] on ob_s (rdd_forward's teacher output)
 *   row_s = ob_s[11] | prevT[4] | prevR[1]   (the x row of rdm_forward):
 *           s = 0: prevT = 0 and prevR = 0;
 *           s > 0: prevT = T_{s-1}, prevR = the reward FIELD of record s-1 (below), i.e. the
 *           reward returned by step s-2 of this episode, and for s = 1 the reward carried over
 *           the reset: the one the previous episode's last step returned (0 in the call's first
 *           episode).  Consecutive episodes of one env are therefore not independent.
 *   S_s   = student(row_s) = mean[2] | logstd[2], dropout off (rdm_forward)
 *   reward r_s = env.step(S_s[0..1])
 * Same arithmetic as the stepwise path: the outputs are bitwise those of rd_reset, then 50 x
 * { rdd_forward (teacher) on the observation, rdm_forward on the assembled row, rd_step with the
 * student's mean }, for every block size and grid.
 * Outputs (device, caller-owned; final_dist and records may be NULL):
 *   returns    [episodes][n_envs]  r_0 + ... + r_49, f32, summed in step order
 *   final_dist [episodes][n_envs]  |fingertip - target| after the episode's last step
 *   records    [episodes][n_envs][50][21]  one record per step in the dataset's layout
 *              ob[11] | reward | t_pdflat[4] | s_pdflat[4] | stepped_with:
 *              ob = ob_s; reward = the one this env's PREVIOUS step of this call returned (0 for
 *              episode 0 step 0; for a later episode's step 0 the previous episode's r_49, carried
 *              over the reset); t_pdflat = T_s; s_pdflat = S_s; stepped_with = 1.
 * No side effects on the trainer (parameters, Adam state and counter, gradient, metrics).
 * Asynchronous on the handle's stream, no host sync, no allocation, no workspace: capturable.
 * RD_EINVAL: NULL trainer, config or returns; n_envs < 1 (or > 2^31); episodes < 1; negative
 * env_base, first_episode or grid (all checked before any device call and before the handle is
 * read); no teacher set. */
typedef struct {
    int64_t n_envs;          /* evaluation envs (their own states)                          */
    int64_t env_base;        /* global id of evaluation env 0 (Philox key)                  */
    uint64_t seed;           /* Philox reset seed                                           */
    int32_t episodes;        /* E >= 1 consecutive episodes per env                         */
    int32_t first_episode;   /* Philox episode index of the first one                       */
    int32_t grid;            /* workgroups; 0 = the trainer's (rdm_config.grid, one per CU)  */
    const float* draws;      /* NULL: Philox; else device table [E][n_envs][6] (q0 q1 v0 v1 tx ty) */
} rdm_eval_config;
int rdm_evaluate(rdm_trainer* t, const rdm_eval_config* cfg, float* returns, float* final_dist, float* records);

/* Batched on-policy distillation of the reference student: the handle keeps n_envs persistent envs
 * in lockstep, and one call takes them through K env steps, labels every step with the teacher
 * (rdm_set_teacher), and trains on the K n_envs rows: the driver's loops (mlp_train.py:120-204)
 * over many envs, as rdd_step is for the 2x64 MlpPolicy student.
 * Per env the device keeps the state, the clock (step 0..49 of the episode, episode), the reward
 * its last step returned, and the previous record's fields (the teacher's pdflat, the reward field).
 * One env step is exactly rdm_evaluate's:
 *   ob_s  = observe(state);  T_s = the teacher's pdflat on ob_s
 *   row_s = ob_s[11] | T_{s-1}[4] | the reward field of record s-1 (zeros at an episode's step 0;
 *           the carried reward survives the reset and reaches step 1's row)
 *   S_s   = student(row_s), dropout off;  r_s = env.step(mean)
 * with mean = S_s[0..1] (RDM_ACT_STUDENT) or T_s[0..1] (RDM_ACT_TEACHER: the driver's phase 1; the
 * student is not evaluated and s_pdflat is written as 0).  After its step 49 an env resets, inside
 * that step as rd_step does, from Philox(seed, env_base + i, episode + 1).  The clock is on the
 * device: no host-side count enters a launch, so a captured call replays the NEXT K steps.
 * Outputs (device, caller-owned, step-major: row k n_envs + i is env i's k-th step of the call):
 *   x        [K][n_envs][16]  the undropped rows (16-byte aligned, required)
 *   t_pdflat [K][n_envs][4]   T_s (16-byte aligned, required)
 *   s_pdflat [K][n_envs][4]   S_s, or 0 under RDM_ACT_TEACHER (may be NULL)
 *   reward   [K][n_envs]      r_s (may be NULL)
 * Same arithmetic as the stepwise path: the outputs are bitwise those of rd_reset, then K x
 * { rdd_forward (teacher), rdm_forward on the assembled row, rd_step }, for every block size, grid
 * and split of the steps over calls; rdm_step_envs leaves the parameters, gradient, metrics and
 * counter of rdm_step on those K n_envs rows (the same two launches on (x, t_pdflat, K n_envs)), so
 * the dropout mask of env i's k-th row is keyed (row_base + k n_envs + i, optimiser step).
 * Asynchronous on the handle's stream; no allocation outside rdm_envs_attach: capturable.
 * rdm_destroy frees the envs.  Multi-GPU is out of scope: there is no rank-sharded variant of these
 * calls (a caller may still all-reduce rdm_grad_buffer() between rdm_rollout_envs and rdm_apply,
 * but n_global is this rank's K n_envs).
 * RD_EINVAL, naming the function and the field: NULL trainer, config, x or t_pdflat; x or t_pdflat
 * not 16-byte aligned; n_envs < 1 (or > 2^31); steps < 1; unknown act_with; negative env_base or
 * grid (all before any device call and before the handle is read); then, from the handle: no envs
 * attached; steps x n_envs > 2^31; no teacher set. */
#define RDM_ACT_TEACHER 0
#define RDM_ACT_STUDENT 1
typedef struct {
    int64_t n_envs;          /* persistent envs of the handle                               */
    int64_t env_base;        /* global id of env 0 (Philox key)                             */
    uint64_t seed;           /* Philox reset seed                                           */
    int32_t grid;            /* workgroups; 0 = the trainer's (rdm_config.grid, one per CU)  */
} rdm_envs_config;

/* allocate (or replace) the handle's envs, then reset them */
int rdm_envs_attach(rdm_trainer* t, const rdm_envs_config* cfg);
/* episode 0 of every env; clocks, carried reward and prev fields to 0 */
int rdm_envs_reset(rdm_trainer* t);
/* K env steps, no training, no side effect on params / Adam / grad / metrics */
int rdm_envs_act(rdm_trainer* t, int act_with, int steps, float* x, float* t_pdflat, float* s_pdflat, float* reward);
/* act, then the training launch on these K n rows (n_global = K n): gradient in rdm_grad_buffer() */
int rdm_rollout_envs(rdm_trainer* t, int act_with, int steps, float* x, float* t_pdflat, float* s_pdflat,
                     float* reward);
/* rdm_rollout_envs + rdm_apply: one optimiser step */
int rdm_step_envs(rdm_trainer* t, int act_with, int steps, float* x, float* t_pdflat, float* s_pdflat, float* reward);
/* state [8][n_envs] SoA as rd_get_state (device); env 0's clock; host-synchronising */
int rdm_envs_get_state(rdm_trainer* t, float* state, int32_t* step, int32_t* episode);

/* DAgger's beta-mixture pi_i = beta pi* + (1 - beta) pi^_i in the RDM_ACT_STUDENT calls above: the
 * handle has a teacher share beta in [0, 1] and a 64-bit coin seed; the default beta = 0 leaves every
 * call exactly as described above (the same launch of the same kernel).  RDM_ACT_TEACHER ignores
 * beta.  In a mixed call an env step is the student step -- T_s and S_s both computed, S_s written to
 * s_pdflat -- and only the action handed to env.step differs, by a coin per env and step:
 *   e    = env_base + i
 *   w    = word 0 of Philox4x32-10(ctr = {e lo, e hi, episode, 0x80000000 | s}, key = {coin_seed lo, hi})
 *   coin = (w >> 8) 2^-24 < beta             (the teacher acts)
 *   mean = coin ? T_s[0..1] : S_s[0..1];   stepped_with = coin ? 0 : 1
 * s and episode are the env's device clock, so the coin is a function of (coin seed, env, episode,
 * step) alone: it does not depend on the grid, the block size or the split of the steps over calls,
 * and a captured call replays the NEXT steps' coins.  Counter word 3 has its top bit set: the stream
 * is disjoint from the reset draws' (word 3 = 0, 1) even under equal seeds.  beta and the coin seed
 * are kernel arguments: a captured call keeps the values it was captured with, whatever is set later.
 * Training is unchanged: rdm_rollout_envs / rdm_step_envs train on all K n_envs rows, every visited
 * state carrying its teacher label whoever stepped it.  Multi-GPU stays out of scope, as above.
 * rdm_envs_set_teacher_share is host-only (no device call, no allocation, no synchronisation); the
 * next call takes the new setting; it may precede rdm_envs_attach and survives attach and reset.
 * RD_EINVAL, naming the function and the field, before the handle is read: NULL trainer; beta NaN,
 * < 0 or > 1.  rdm_envs_teacher_share returns beta, -1 for a NULL trainer. */
int rdm_envs_set_teacher_share(rdm_trainer* t, float beta, uint64_t coin_seed);
float rdm_envs_teacher_share(const rdm_trainer* t);
/* Where the per-row stepped_with goes: buf = a caller-owned device buffer [K][n_envs] of `rows`
 * floats, step-major as reward.  Every later RDM_ACT_STUDENT call fills its steps x n_envs rows with
 * 1 (the student stepped) or 0 (the teacher's coin fell; all 1 at beta = 0), an RDM_ACT_TEACHER call
 * with 0.  buf = NULL unbinds.  Host-only.  While a buffer is bound a call with steps x n_envs > rows
 * is RD_EINVAL naming `rows`; so are a NULL trainer and rows < 1 with a buffer here. */
int rdm_envs_bind_stepped_with(rdm_trainer* t, float* buf, int64_t rows);
/* The replay ring's push for that buffer: rd_replay_push_rows (reacher_replay.h) with a stepped_with
 * per row, stepped_with_rows [K][n] (required), step-major as reward, in place of the scalar.  The same
 * copies, counter bump and argument checks; also RD_EINVAL for NULL stepped_with_rows. */
int rd_replay_push_rows_flags(rd_replay* h, const float* x, const float* t_pdflat, const float* s_pdflat,
                              const float* reward, const float* carry, int64_t steps, int64_t n_envs,
                              const float* stepped_with_rows);

/* Action noise in the envs calls above (reacher_action_noise.h has the definition): the handle has an
 * rd_action_noise; the default mode = RD_NOISE_NONE, and a set back to it, with no actions buffer
 * bound leaves every call exactly as described above (the same launch of the same kernel).
 * Otherwise, in rdm_envs_act / rdm_rollout_envs / rdm_step_envs under BOTH RDM_ACT_STUDENT (with the
 * beta-coin as it is) and RDM_ACT_TEACHER (DART's noisy expert; the student is still not evaluated),
 * the action handed to env.step is the perturbed mean of whoever acts at that step -- S_s, T_s under
 * RDM_ACT_TEACHER, T_s where the coin fell -- at e = env_base + i and the env's device clock
 * (episode, s).  ONLY that action changes: x, t_pdflat, s_pdflat, stepped_with and the training on
 * every row are as without noise.  The noise is a function of (seed, env, episode, step) alone: it
 * does not depend on the grid, the block size or the split of the steps over calls, and a captured
 * call replays the NEXT steps' noise.  Mode, scale and seed are kernel arguments: a captured call
 * keeps the values it was captured with, whatever is set later.
 * rdm_envs_set_action_noise is host-only (no device call, no allocation, no synchronisation); the
 * next call takes the new setting; it may precede rdm_envs_attach and survives attach and reset.
 * rdm_evaluate never reads it.  RD_EINVAL, naming the function and the field, before the handle is
 * read: NULL trainer or struct; unknown mode; scale NaN, negative or infinite.
 * rdm_envs_action_noise copies the setting to *out (RD_EINVAL for a NULL trainer or out). */
int rdm_envs_set_action_noise(rdm_trainer* t, const rd_action_noise* nz);
int rdm_envs_action_noise(const rdm_trainer* t, rd_action_noise* out);
/* Where the action that stepped each env goes: buf = a caller-owned device buffer [K][n_envs][2] of
 * `rows` rows, step-major as reward; every later call of either actor fills its steps x n_envs rows
 * (the acting means when the noise is off).  buf = NULL unbinds.  Host-only; `rows` is checked as
 * rdm_envs_bind_stepped_with checks it. */
int rdm_envs_bind_actions(rdm_trainer* t, float* buf /*[K][n][2] step-major*/, int64_t rows);

/* rdm_evaluate with the student's action perturbed by *nz (RD_NOISE_POLICY or RD_NOISE_FIXED) at
 * Philox episode first_episode + e, with or without a draws table: the records, returns and final_dist
 * of the noisy trajectory (records keep S_s, not the action).  Bitwise the stepwise loop with
 * rd_perturb_actions between rdm_forward and rd_step.  Independent of the envs' noise setting.
 * RD_EINVAL as rdm_evaluate, and before it: NULL nz, unknown mode, a bad scale, mode = RD_NOISE_NONE
 * (call rdm_evaluate). */
int rdm_evaluate_noisy(rdm_trainer* t, const rdm_eval_config* cfg, const rd_action_noise* nz,
                       float* returns, float* final_dist, float* records);

/* Sensor faults on what the student reads in the envs calls above (reacher_obs_faults.h has the
 * definition): the handle has an rd_obs_faults; the default mode = RD_OBS_CLEAN, and a set back to it,
 * leaves every call exactly as described above (the same launch of the same kernel).  Otherwise, in
 * rdm_envs_act / rdm_rollout_envs / rdm_step_envs under RDM_ACT_STUDENT, the student's forward reads
 * ob masked at e = env_base + i and the env's device clock (episode, s) in place of ob; prev_pdflat and
 * prev_rew of its row are untouched.  ONLY S_s, and through it the trajectory, changes: the teacher
 * reads the clean ob, and x, t_pdflat, s_pdflat's meaning, stepped_with, reward, actions and the
 * training on every (clean) row with its own keep_prob dropout are as without faults.  They compose
 * with the beta-coin and the action noise.  RDM_ACT_TEACHER calls evaluate no student: they ignore the
 * setting and launch what they launch without it.  The mask is a function of (seed, env, episode,
 * step, component) alone: it does not depend on the grid, the block size or the split of the steps
 * over calls, and a captured call replays the NEXT steps' mask.  Mode, keep_prob and seed are kernel
 * arguments: a captured call keeps the values it was captured with, whatever is set later.
 * rdm_envs_set_obs_faults is host-only (no device call, no allocation, no synchronisation); the next
 * call takes the new setting; it may precede rdm_envs_attach and survives attach and reset.
 * rdm_evaluate never reads it.  RD_EINVAL, naming the function and the field, before the handle is
 * read: NULL struct; unknown mode; keep_prob NaN, <= 0 or > 1; then a NULL trainer.
 * rdm_envs_obs_faults copies the setting to *out (RD_EINVAL for a NULL trainer or out). */
int rdm_envs_set_obs_faults(rdm_trainer* t, const rd_obs_faults* of);
int rdm_envs_obs_faults(const rdm_trainer* t, rd_obs_faults* out);

/* rdm_evaluate with the student reading its observation through *of (RD_OBS_DROPOUT or RD_OBS_MISSING)
 * at Philox episode first_episode + e, with or without a draws table, and, with nz, its action
 * perturbed as rdm_evaluate_noisy perturbs it (nz = NULL or mode RD_NOISE_NONE: the mean acts): the
 * records (clean ob, T_s from the clean ob, S_s from the masked one), returns and final_dist of that
 * trajectory.  Bitwise the stepwise loop { rdd_forward, rd_mask_obs, rdm_forward on the masked row,
 * [rd_perturb_actions], rd_step }.  Independent of the envs' settings; capturable.
 * RD_EINVAL as rdm_evaluate, and before it: NULL of, unknown mode, a bad keep_prob, mode =
 * RD_OBS_CLEAN (call the plain function); a bad *nz as rdm_evaluate_noisy names it. */
int rdm_evaluate_faulty(rdm_trainer* t, const rdm_eval_config* cfg, const rd_obs_faults* of, const rd_action_noise* nz,
                        float* returns, float* final_dist, float* records);

#ifdef __cplusplus
}
#endif
#endif
