/* reacher_student_lstm.h -- C ABI of the reference's LSTM student: forward over unrolled
 * windows and one truncated-BPTT distillation training step (libreacher.so).
 *
 * Graph: student_lstm_graph (reference src/distilation/student_nn.py:21-49), T unrolled steps
 * (STEPS_UNROLLED = 10, config.py:25) over B windows (LSTM_BATCH_SIZE = 20, config.py:26):
 *     p_t = dense(prev_pdflat_t, 32)                         linear
 *     x_t = [dropout(ob_t)[11], p_t[32]]
 *     (c_t, h_t) = LSTMCell(200)(x_t, (c_{t-1}, h_{t-1}))     TF1: gates i, j, f, o of
 *                                                             [x_t, h_{t-1}] . Wl + bl,
 *                                                             forget_bias 1, tanh
 *     pdflat_t = dense(tanh dense 32(tanh dense 64(tanh dense 128(tanh dense 64(h_t))))), 4)
 * with ONE HEAD PER UNROLLED STEP: the reference calls tf.layers.dense inside its Python loop
 * over the T steps without reuse (student_nn.py:40-47), so step t's five layers are their own
 * variables (dense_{5t+1} .. dense_{5t+5}); the LSTMCell and the prev-pdflat dense are shared.
 * Flat parameters (RDL_PARAMS_T(T) floats; RDL_PARAMS at the reference's T = 10) in
 * variable-creation order, each kernel W[in][out] row-major then its bias:
 *     Wp[4][32] bp | Wl[243][800] bl | head_0 | ... | head_{T-1},
 *     head_t = W1[200][64] b1 | W2[64][128] b2 | W3[128][64] b3 | W4[64][32] b4 | W5[32][4] b5
 * Tensors: ob [T][B][11], prev_pdflat [T][B][4], t_pdflat / pdflat [T][B][4], LSTM state
 * [2][B][200] = (c, m) as the reference's initial_state_batch_ph (lstm_train.py:51).
 * Loss: kl_loss summed over T and B (loss.py:3-13), or action-MSE over T x rows_global.
 * Optimiser: TF1 Adam (reference lr 1e-3, lstm_train.py:73-79).
 *
 * Arithmetic.  RDL_DTYPE_F32 (rdl_create): every product on v_mfma_f32_16x16x4_f32, exact f32
 * products and f32 sums.  RDL_DTYPE_BF16 (rdl_create_dtype) is mixed precision.  These stay f32:
 * the master weights and the Adam slots; every bias; the prev_pdflat projection (Wp, bp); the gate
 * nonlinearities; c and h, the stored gates and the cell's backward point-wise arithmetic; the five
 * head layers of every step, forward and backward; the loss, dbl, dWp, dbp and every accumulation.
 * The three products of the cell matrix Wl[243][800] (86 % of the multiply-adds per row) round their
 * operands to bf16, to nearest even (v_cvt_pk_bf16_f32); products are exact, sums f32, bf() below:
 *     forward  z_t         = bl + sum_k bf([x_t | h_{t-1}]_k) bf(Wl_kc)
 *     dgrad    [dx_t | dh] = sum_c bf(dz_t,c) bf(Wl_kc)     (dx's columns 11..42 feed dWp, dbp; dh
 *                                                            feeds step t-1)
 *     wgrad    dWl         = sum_{t,rows} bf([x_t | h_{t-1}]) bf(dz_t),   dbl = sum dz_t (unrounded)
 * dz_t comes from the f32 cell backward on the unrounded stored gates and c.  The handle keeps two
 * bf16 images of Wl (the second transposed, for the dgrad), roundings of the master, re-formed on
 * the stream and without allocation by rdl_create_dtype, rdl_set_params and every Adam step
 * (rdl_apply, rdl_step, rdl_step_envs).  The weight gradient is split over the rows and summed in a
 * fixed order from a workspace sized at create from max_windows: no floating-point atomics, no
 * hand-off between workgroups, no allocation after create; a bf16 step is capturable.
 * Which calls run it: the window passes -- rdl_forward, rdl_rollout / rdl_step and the training
 * pass inside rdl_rollout_envs / rdl_step_envs.  A bf16 handle always takes the per-step recurrence
 * path: the persistent kernels (at most 32 windows, latency bound) are f32 only and never launched
 * by it, so RDL_KERNELS_STEP_RECURRENCE has no effect on it; RDL_KERNELS_LAYER_HEAD and
 * rdl_head_path work as on an f32 handle (the head is f32 on either path).
 * The closed-loop query -- the one-record-per-env query of rdl_evaluate, rdl_envs_act and the act
 * phase of rdl_rollout_envs / rdl_step_envs -- has its own setting, rdl_set_query_dtype:
 *   RDL_DTYPE_F32 (the default of every handle): the query stays f32, on the master weights.  On a
 *     bf16 handle these calls are then bitwise what an f32 handle with the same parameters returns
 *     (evaluate measures the checkpointed f32 policy), while the training pass sees the rounded
 *     operands: the student that acts is not quite the student that is trained.
 *   RDL_DTYPE_BF16 (bf16 handles only): one query step is exactly one rdl_forward of the handle on
 *     that env's window from its carried (c, h): x formed in f32, z = bl + sum_k bf([x | h]_k)
 *     bf(Wl_kc) from the handle's forward image (no per-call pack of Wl), the f32 cell, the f32 head
 *     T-1; teacher, physics and records unchanged.  rdl_evaluate and rdl_envs_act are then bitwise
 *     the stepwise loop { rdd_forward (teacher), rdl_forward on the window, rd_step } run with that
 *     bf16 handle, whatever the grid; evaluate measures the policy as deployed in bf16.
 * Under either setting rdl_step_envs equals rdl_envs_act, then rdl_step on the windows written.
 *
 * Conventions as in reacher.h: device pointers, asynchronous on the handle's stream,
 * 0 = OK, RD_EINVAL, -(hipError_t).  Multi-GPU: windows sharded by the caller (row_base =
 * this rank's first global window); rdl_rollout, all-reduce(SUM) rdl_grad_buffer(), rdl_apply.
 */
#ifndef REACHER_STUDENT_LSTM_H
#define REACHER_STUDENT_LSTM_H
#include <stdint.h>

#include "reacher.h"
#include "reacher_action_noise.h"   /* rd_action_noise: rdl_envs_set_action_noise, rdl_evaluate_noisy */
#include "reacher_obs_faults.h"     /* rd_obs_faults: rdl_envs_set_obs_faults, rdl_evaluate_faulty */

#ifdef __cplusplus
extern "C" {
#endif

#define RDL_CELL_PARAMS 195360                                   /* Wp bp Wl bl          */
#define RDL_HEAD_PARAMS 31652                                    /* one step's head      */
#define RDL_PARAMS_T(T) (RDL_CELL_PARAMS + (T) * RDL_HEAD_PARAMS)
#define RDL_PARAMS RDL_PARAMS_T(10)                              /* 511,880              */
#define RDL_UNITS 200
#define RDL_LOSS_MSE 0
#define RDL_LOSS_KL 1

typedef struct {
    int32_t loss;                  /* RDL_LOSS_*                                             */
    float lr, beta1, beta2, eps;   /* Adam (reference: 1e-3, .9, .999, 1e-8)                 */
    int32_t steps;                 /* T, unrolled steps per window (reference 10)            */
    int32_t max_windows;           /* capacity: largest B passed to any call                 */
    int32_t metrics_len;           /* per-step metrics ring length; 0 = 4096                 */
    float keep_prob;               /* dropout on ob while training (reference KEEP_PROB 0.5);
                                      mask of ob[t][b][k] at optimiser step S: keep iff
                                      u < keep_prob, u = word k%4 of Philox4x32-10(ctr =
                                      {w lo, w hi, S, 4t + k/4}, key = seed), w = row_base + b */
    uint64_t seed;
    int64_t row_base;              /* global index of this rank's window 0                  */
    int32_t kernels;               /* 0 = automatic kernel selection; RDL_KERNELS_* bits force
                                      the general path (same results, tests compare them)    */
} rdl_config;

/* rdl_config.kernels: by default at most 32 windows run the whole recurrence / BPTT as one
 * persistent launch each and at most 16,384 rows run the heads as one launch each way (when
 * their backward's partial rows fit 512 MB at max_windows: rdl_head_path reports it); these
 * bits keep the per-step recurrence launches / the per-layer head GEMMs at any size. */
#define RDL_KERNELS_STEP_RECURRENCE 1
#define RDL_KERNELS_LAYER_HEAD 2

typedef struct rdl_trainer rdl_trainer;

/* flat parameters of a trainer with `steps` unrolled steps (RDL_PARAMS_T(steps)), -1 if steps <= 0 */
int64_t rdl_param_count(int32_t steps);
/* the 'LSTM' scope: graph, kl_loss and Adam (lstm_train.py:35-79) */
int rdl_create(rdl_trainer** out, const rdl_config* cfg, int device, void* hip_stream);
/* rdl_create with the arithmetic of the cell matrix's products chosen ("Arithmetic" above):
 * rdl_create(cfg) == rdl_create_dtype(cfg, RDL_DTYPE_F32); any other dtype than these two is
 * RD_EINVAL before any device call */
#define RDL_DTYPE_F32 0
#define RDL_DTYPE_BF16 1
int rdl_create_dtype(rdl_trainer** out, const rdl_config* cfg, int32_t dtype, int device, void* hip_stream);
/* arithmetic of the closed-loop query (rdl_evaluate, rdl_envs_act, the act phase of
 * rdl_rollout_envs / rdl_step_envs): RDL_DTYPE_F32 (the default) or RDL_DTYPE_BF16
 * ("Arithmetic" above).  Host-only: no device call, no allocation, no synchronisation; the next
 * call takes it, a captured call keeps the kernel it was captured with.  RD_EINVAL (the setting
 * unchanged) for a null handle, an unknown dtype, and RDL_DTYPE_BF16 on a handle that was not
 * created with RDL_DTYPE_BF16: it keeps no bf16 image, and its training would not match the query */
int rdl_set_query_dtype(rdl_trainer* t, int32_t dtype);
int rdl_query_dtype(const rdl_trainer* t);      /* RDL_DTYPE_*; -1 for NULL */
int rdl_destroy(rdl_trainer* t);
int rdl_set_stream(rdl_trainer* t, void* hip_stream);
/* initialisation / saver.restore (lstm_train.py:82-107): params [RDL_PARAMS_T(steps)] */
int rdl_set_params(rdl_trainer* t, const float* params);
int rdl_get_params(rdl_trainer* t, float* params);
/* Adam slots, beta powers, step counter to zero (lstm_train.py:99) */
int rdl_reset(rdl_trainer* t);
/* the Adam slots m, v [RDL_PARAMS_T(steps)] (device pointers): with the params, what the reference's
 * tf.train.Saver over the 'LSTM' scope checkpoints every episode and restores with -r
 * (lstm_train.py:86-87,102-107,199); the beta powers are not in that scope, so a restore
 * starts them afresh (rdl_reset, then rdl_set_params + rdl_set_slots) */
int rdl_get_slots(rdl_trainer* t, float* m, float* v);
int rdl_set_slots(rdl_trainer* t, const float* m, const float* v);
/* sess.run((s_action, s_pdflat_slice, final_state)) (lstm_train.py:171-183), all T x B outputs:
 * state0 may be null (zero state); state_out may be null */
int rdl_forward(rdl_trainer* t, const float* ob, const float* prev_pdflat, const float* state0, int64_t windows,
                float* pdflat, float* state_out);
/* forward + loss + BPTT of B windows (of windows_global over all ranks) from state0 (null =
 * zeros, as lstm_train.py:159): gradient into rdl_grad_buffer() */
int rdl_rollout(rdl_trainer* t, const float* ob, const float* prev_pdflat, const float* t_pdflat,
                const float* state0, int64_t windows, int64_t windows_global);
int rdl_apply(rdl_trainer* t);
/* final_state_batch of the last forward pass (rdl_forward / rdl_rollout / rdl_step) of
 * `windows` windows, as [2][windows][200] = (c, h): the truncated-BPTT driver feeds it back as
 * the next window's initial state (backup/lstm_bbpt.py:141-155 fetches it in the training
 * sess.run); RD_EINVAL if the last pass had another window count */
int rdl_final_state(rdl_trainer* t, int64_t windows, float* state_out);
/* sess.run([loss, minimize_adam]) (lstm_train.py:145-160) == rollout + apply */
int rdl_step(rdl_trainer* t, const float* ob, const float* prev_pdflat, const float* t_pdflat,
             const float* state0, int64_t windows);
float* rdl_grad_buffer(rdl_trainer* t);
int rdl_bind_grad_buffer(rdl_trainer* t, float* grad);
/* optimiser steps taken; RD_EINVAL if a persistent recurrence launch (<= 32 windows) gave up
 * at its grid barrier since the trainer was created (its steps are invalid) */
int rdl_get_counter(rdl_trainer* t, int64_t* opt_steps);
/* 1: batches of at most 16,384 rows run the fused head kernels (their backward's partial rows,
 * T x workgroups x 31,652 floats at max_windows, were allocated: at most 512 MB); 0: the
 * per-layer head GEMMs at every size (RDL_KERNELS_LAYER_HEAD, or the rows would not fit). */
int rdl_head_path(const rdl_trainer* t);
/* [count][4] = loss, sum |mu_s - mu_t|^2, rows (T x B), 0 */
int rdl_read_metrics(rdl_trainer* t, int64_t count, double* out);

/* The teacher of rdl_evaluate: the 2x64 MlpPolicy with its observation filter, same arguments as
 * rdd_set_teacher / rdm_set_teacher (device pointers: params [rdd_param_count()], ob_mean [11],
 * ob_std [11]).  The handle keeps its own copy of the net, from which every evaluation launch
 * packs the LDS image rdd_forward's kernel packs (the same function). */
int rdl_set_teacher(rdl_trainer* t, const float* params, const float* ob_mean, const float* ob_std);

/* Whole-episode evaluation of the LSTM student in one rollout launch: n_envs evaluation envs (their
 * own states; no trainer's envs exist or are touched) run `episodes` consecutive 50-step episodes,
 * stepped with the student's unclipped mean.  It is the query loop of lstm_train.train (reference
 * lstm_train.py:163-204) without the optimiser steps, one env being column B-1 of the driver's
 * query batch.  Episode e of env i starts from reset draw draws[(e n_envs + i) 6 ..] or, with draws
 * NULL, from Philox(seed, env_base + i, first_episode + e) (as rdm_evaluate).  With T =
 * rdl_config.steps, step s = 0..49 of an episode, per env:
 *   ob_s = observe(state)
 *   T_s  = the teacher's mean[2] | logstd[2] on ob_s (rdd_forward's teacher output)
 *   window: position p = 0..T-1 holds record j = s - (T-1) + p of this episode:
 *           j >= 0: ob_j[11] | prev = T_{j-1} (0 at j = 0);  j < 0: ob = 0, prev = 0
 *   S_s  = pdflat of unrolled position T-1 (head T-1) of rdl_forward on that window, dropout off,
 *          from the final (c, h) of this env's previous query: carried over episode boundaries,
 *          state0 (zeros when NULL) at the call's first step
 *   reward r_s = env.step(S_s[0..1])
 * Same arithmetic as the stepwise path: the outputs are bitwise those of rd_reset, then 50 x
 * { rdd_forward (teacher), rdl_forward on the windows, rd_step with the student's mean }, for every
 * grid -- rdl_forward being an f32 handle's under the f32 query and this bf16 handle's under the bf16
 * query (rdl_set_query_dtype, "Arithmetic" above).  T is at most RDL_EVAL_MAX_STEPS, the records of history the kernel keeps on chip per env.
 * Outputs (device, caller-owned; final_dist, records and state_out may be NULL):
 *   returns    [episodes][n_envs]  r_0 + ... + r_49, f32, summed in step order
 *   final_dist [episodes][n_envs]  |fingertip - target| after the episode's last step
 *   records    [episodes][n_envs][50][21]  ob[11] | reward | t_pdflat[4] | s_pdflat[4] | stepped_with:
 *              reward = the one this env's PREVIOUS step of this call returned (0 at the call's first
 *              step); t_pdflat = T_s; s_pdflat = S_s; stepped_with = 1
 *   state_out  [2][n_envs][200] = (c, h) after the call's last query; state0 has the same layout
 * No side effects on the trainer: parameters, Adam state and counter, gradient, metrics, the
 * activations rdl_final_state reads, the persistent kernels' barrier words and granule generation.
 * Asynchronous on the handle's stream, no host sync, no allocation (the packed image of the cell's
 * weights is the handle's, rebuilt on the stream by every call; the bf16 query reads the handle's
 * bf16 image, no launch): capturable.
 * RD_EINVAL: NULL trainer, config or returns; n_envs < 1 (or > 2^31); episodes < 1; negative
 * env_base, first_episode or grid (all checked before any device call and before the handle is
 * read); no teacher set; rdl_config.steps > RDL_EVAL_MAX_STEPS. */
#define RDL_EVAL_MAX_STEPS 16
typedef struct {
    int64_t n_envs;          /* evaluation envs (their own states)                          */
    int64_t env_base;        /* global id of evaluation env 0 (Philox key)                  */
    uint64_t seed;           /* Philox reset seed                                           */
    int32_t episodes;        /* E >= 1 consecutive episodes per env                         */
    int32_t first_episode;   /* Philox episode index of the first one                       */
    int32_t grid;            /* workgroups (16 envs each per pass); 0 = one per CU          */
    const float* draws;      /* NULL: Philox; else device table [E][n_envs][6] (q0 q1 v0 v1 tx ty) */
} rdl_eval_config;
int rdl_evaluate(rdl_trainer* t, const rdl_eval_config* cfg, const float* state0, float* returns, float* final_dist,
                 float* records, float* state_out);

/* Batched on-policy distillation of the LSTM student: the handle keeps n_envs persistent envs in
 * lockstep, and one call takes them through K env steps under the teacher's or the student's mean
 * action, labels every step with the teacher (rdl_set_teacher), emits the training windows that lie
 * wholly inside an episode and trains on them: the driver's loop (lstm_train.py:120-204) over many
 * envs, the counterpart of rdm_envs_* (reacher_student_mlp.h).
 * Per env the device keeps (rdl_envs_attach allocates, rdl_destroy frees): the physics state, the
 * reward its last step returned, the clock (step 0..49 of the episode, episode), the query state
 * (c, h), the teacher's last pdflat, and the raw fields ob[11] | prev[4] of the open episode's last
 * T records (T = rdl_config.steps).  One env step is exactly one step of rdl_evaluate:
 *   ob_s = observe(state);  T_s = the teacher's pdflat on ob_s
 *   window: the last T records of this episode (zero rows before its step 0), prev of record j =
 *           T_{j-1}, 0 at j = 0
 *   RDL_ACT_STUDENT: S_s = head T-1 of the forward on that window from the env's carried (c, h),
 *           which it replaces; r_s = env.step(S_s[0..1])
 *   RDL_ACT_TEACHER: r_s = env.step(T_s[0..1]); the student is not evaluated, (c, h) stays as it
 *           was, s_pdflat and stepped_with are written as 0 (the drivers' warm-up)
 * After its step 49 an env resets, inside that step as rd_step does, from Philox(seed, env_base + i,
 * episode + 1); (c, h) and the carried reward survive the reset.  The x rows of the carried records
 * are re-formed from the raw fields with the parameters each call finds, so an optimiser step or
 * rdl_set_params between calls acts on the next query as it does in the stepwise loop.  The clock is
 * on the device: no host-side count enters a launch, so a captured call replays the NEXT K steps.
 * Outputs (device, caller-owned, step-major: row k n_envs + i is env i's k-th step of the call):
 *   records [K][n_envs][21]  ob[11] | reward | t_pdflat[4] | s_pdflat[4] | stepped_with (the dataset's
 *           record): reward = the one the env's previous step returned (0 after attach / reset,
 *           carried over episode resets), stepped_with = 1 (student) or 0 (teacher)
 *   reward  [K][n_envs]      r_s (may be NULL)
 * Training windows: the query windows of the steps whose episode step s >= T-1, i.e. records
 * s-T+1 .. s of one episode (the windows training_batches can draw, start = s-T+1 in [0, 50-T]),
 * ordered by k among the qualifying steps, then by env, in the trainer's layout with B windows:
 *   ob_w [T][B][11], prev_w [T][B][4] (prev of the record), t_w [T][B][4] (its own t_pdflat).
 * The first windows of a call reach into records of earlier calls (the carried history).
 * Any 50 consecutive lockstep steps hold exactly 51-T qualifying steps, so rdl_rollout_envs and
 * rdl_step_envs, which require steps % 50 == 0 (and T <= 50), write B = n_envs (steps/50) (51-T)
 * windows, then run rdl_rollout(ob_w, prev_w, t_w, NULL, B, B) [+ rdl_apply]: zero initial state,
 * dropout keep_prob keyed (row_base + window, optimiser step); they leave the parameters, gradient,
 * metrics, counter and rdl_final_state of rdl_step on those windows.  rdl_envs_act takes any steps
 * >= 1 and writes windows only if the three window buffers are given, with stride and capacity
 * B = `windows`: as many as the clock yields (windows past B are dropped; fewer leave the rest of
 * the buffers untouched), n_envs (steps/50) (51-T) when steps is a multiple of 50.
 * rdl_envs_act has no side effect on parameters, Adam state, gradient, metrics or counter.
 * Asynchronous on the handle's stream; no allocation outside rdl_envs_attach: capturable.
 * SINGLE GPU ONLY: there is no rank-sharded variant of these calls.
 * RD_EINVAL, naming the function and the field: NULL trainer, config or records; n_envs < 1 (or >
 * 2^31); steps < 1; unknown act_with; negative env_base or grid; window buffers given in part (or
 * missing from a training call) (all before any device call and before the handle is read); then,
 * from the handle: no envs attached; no teacher set; rdl_config.steps > RDL_EVAL_MAX_STEPS; steps x
 * n_envs > 2^31; for the training calls steps % 50 != 0, rdl_config.steps > 50, B > max_windows. */
#define RDL_ACT_TEACHER 0
#define RDL_ACT_STUDENT 1
typedef struct {
    int64_t n_envs;          /* persistent envs of the handle                               */
    int64_t env_base;        /* global id of env 0 (Philox key)                             */
    uint64_t seed;           /* Philox reset seed                                           */
    int32_t grid;            /* workgroups (16 envs each per pass); 0 = one per CU          */
} rdl_envs_config;

/* allocate (or replace) the handle's envs, then reset them */
int rdl_envs_attach(rdl_trainer* t, const rdl_envs_config* cfg);
/* episode 0 of every env; clock, carried reward, (c, h) and history to 0 */
int rdl_envs_reset(rdl_trainer* t);
/* K env steps, no training; ob_w, prev_w, t_w all NULL (no windows) or all given with B = windows */
int rdl_envs_act(rdl_trainer* t, int act_with, int steps, float* records, float* reward, float* ob_w, float* prev_w,
                 float* t_w, int64_t windows);
/* act, then rdl_rollout on the B windows written: gradient in rdl_grad_buffer() */
int rdl_rollout_envs(rdl_trainer* t, int act_with, int steps, float* records, float* reward, float* ob_w,
                     float* prev_w, float* t_w);
/* rdl_rollout_envs + rdl_apply: one optimiser step */
int rdl_step_envs(rdl_trainer* t, int act_with, int steps, float* records, float* reward, float* ob_w, float* prev_w,
                  float* t_w);
/* state [8][n_envs] SoA as rd_get_state (device); env 0's clock; host-synchronising */
int rdl_envs_get_state(rdl_trainer* t, float* state, int32_t* step, int32_t* episode);
/* the envs' query state [2][n_envs][200] = (c, h) (device), asynchronous */
int rdl_envs_get_query_state(rdl_trainer* t, float* state_out);

/* DAgger's beta-mixture pi_i = beta pi* + (1 - beta) pi^_i in the RDL_ACT_STUDENT calls above: the
 * handle has a teacher share beta in [0, 1] and a 64-bit coin seed; the default beta = 0 leaves every
 * call exactly as described above (the same launch of the same kernel).  RDL_ACT_TEACHER ignores
 * beta.  In a mixed call an env step is the student step -- T_s and S_s both computed, S_s in the
 * record, (c, h) read and replaced, the ring kept and the windows written -- and only the action
 * handed to env.step differs, by a coin per env and step:
 *   e    = env_base + i
 *   w    = word 0 of Philox4x32-10(ctr = {e lo, e hi, episode, 0x80000000 | s}, key = {coin_seed lo, hi})
 *   coin = (w >> 8) 2^-24 < beta             (the teacher acts)
 *   mean = coin ? T_s[0..1] : S_s[0..1];   the record's stepped_with = coin ? 0 : 1
 * s and episode are the env's device clock, so the coin is a function of (coin seed, env, episode,
 * step) alone: it does not depend on the grid or the split of the steps over calls, and a captured
 * call replays the NEXT steps' coins.  Counter word 3 has its top bit set: the stream is disjoint from
 * the reset draws' (word 3 = 0, 1) even under equal seeds.  beta and the coin seed are kernel
 * arguments: a captured call keeps the values it was captured with, whatever is set later.
 * Training is unchanged: rdl_rollout_envs / rdl_step_envs train on all the in-episode windows, every
 * visited state carrying its teacher label whoever stepped it.  SINGLE GPU ONLY, as above.
 * rdl_envs_set_teacher_share is host-only, like rdl_set_query_dtype (no device call, no allocation,
 * no synchronisation); the next call takes the new setting; it may precede rdl_envs_attach and
 * survives attach and reset.  RD_EINVAL, naming the function and the field, before the handle is
 * read: NULL trainer; beta NaN, < 0 or > 1.  rdl_envs_teacher_share returns beta, -1 for NULL. */
int rdl_envs_set_teacher_share(rdl_trainer* t, float beta, uint64_t coin_seed);
float rdl_envs_teacher_share(const rdl_trainer* t);

/* Action noise in the envs calls above (reacher_action_noise.h has the definition): the handle has an
 * rd_action_noise; the default mode = RD_NOISE_NONE, and a set back to it, with no actions buffer
 * bound leaves every call exactly as described above (the same launch of the same kernel).
 * Otherwise, in rdl_envs_act / rdl_rollout_envs / rdl_step_envs under BOTH RDL_ACT_STUDENT (with the
 * beta-coin as it is) and RDL_ACT_TEACHER (DART's noisy expert; the student is still not evaluated),
 * the action handed to env.step is the perturbed mean of whoever acts at that step -- S_s, T_s under
 * RDL_ACT_TEACHER, T_s where the coin fell -- at e = env_base + i and the env's device clock
 * (episode, s).  ONLY that action changes: the records (both pdflats, stepped_with), (c, h), the
 * history ring, the windows and the training on every window are as without noise.  The noise is a
 * function of (seed, env, episode, step) alone: it does not depend on the grid or the split of the
 * steps over calls, and a captured call replays the NEXT steps' noise.  Mode, scale and seed are
 * kernel arguments: a captured call keeps the values it was captured with, whatever is set later.
 * rdl_envs_set_action_noise is host-only, like rdl_envs_set_teacher_share; the next call takes the new
 * setting; it may precede rdl_envs_attach and survives attach and reset.  rdl_evaluate never reads
 * it.  RD_EINVAL, naming the function and the field, before the handle is read: NULL trainer or
 * struct; unknown mode; scale NaN, negative or infinite.
 * rdl_envs_action_noise copies the setting to *out (RD_EINVAL for a NULL trainer or out). */
int rdl_envs_set_action_noise(rdl_trainer* t, const rd_action_noise* nz);
int rdl_envs_action_noise(const rdl_trainer* t, rd_action_noise* out);
/* Where the action that stepped each env goes: buf = a caller-owned device buffer [K][n_envs][2] of
 * `rows` rows, step-major as reward; every later call of either actor fills its steps x n_envs rows
 * (the acting means when the noise is off).  buf = NULL unbinds.  Host-only.  While a buffer is bound
 * a call with steps x n_envs > rows is RD_EINVAL naming `rows`; so are a NULL trainer and rows < 1
 * with a buffer here. */
int rdl_envs_bind_actions(rdl_trainer* t, float* buf /*[K][n][2] step-major*/, int64_t rows);

/* rdl_evaluate with the student's action perturbed by *nz (RD_NOISE_POLICY or RD_NOISE_FIXED) at
 * Philox episode first_episode + e, with or without a draws table: the records, returns, final_dist
 * and state_out of the noisy trajectory (records keep S_s, not the action).  Bitwise the stepwise loop
 * with rd_perturb_actions between rdl_forward and rd_step.  Independent of the envs' noise setting.
 * RD_EINVAL as rdl_evaluate, and before it: NULL nz, unknown mode, a bad scale, mode = RD_NOISE_NONE
 * (call rdl_evaluate). */
int rdl_evaluate_noisy(rdl_trainer* t, const rdl_eval_config* cfg, const rd_action_noise* nz, const float* state0,
                       float* returns, float* final_dist, float* records, float* state_out);

/* Sensor faults on what the student reads in the envs calls above (reacher_obs_faults.h has the
 * definition): the handle has an rd_obs_faults; the default mode = RD_OBS_CLEAN, and a set back to it,
 * leaves every call exactly as described above (the same launch of the same kernel).  Otherwise, in
 * rdl_envs_act / rdl_rollout_envs / rdl_step_envs under RDL_ACT_STUDENT, the student's query reads
 * every record of its window masked: record j of the open episode carries the mask of (e = env_base +
 * i, episode, j) at every position and in every later query that still holds it -- a reading once lost
 * stays lost -- whichever call recorded it (a teacher call's records and those of an earlier call are
 * masked the same: the mask is a pure function and the handle's history keeps the clean readings).
 * Zero-padding records stay zero and prev is untouched.  ONLY S_s, and through it (c, h) and the
 * trajectory, changes: the teacher reads the clean ob, and the records' layout, the windows (ob_w,
 * prev_w, t_w hold the clean readings), stepped_with, reward, actions and the training on every window
 * with its own keep_prob dropout are as without faults.  They compose with the beta-coin and the
 * action noise.  RDL_ACT_TEACHER calls evaluate no student: they ignore the setting and launch what
 * they launch without it.  The mask does not depend on the grid or the split of the steps over calls;
 * a captured call replays the NEXT steps' mask and keeps the mode, keep_prob and seed it was captured
 * with.  rdl_envs_set_obs_faults is host-only, like rdl_envs_set_action_noise; it may precede
 * rdl_envs_attach and survives attach and reset.  rdl_evaluate never reads it.  RD_EINVAL, naming the
 * function and the field, before the handle is read: NULL struct; unknown mode; keep_prob NaN, <= 0 or
 * > 1; then a NULL trainer.
 * rdl_envs_obs_faults copies the setting to *out (RD_EINVAL for a NULL trainer or out). */
int rdl_envs_set_obs_faults(rdl_trainer* t, const rd_obs_faults* of);
int rdl_envs_obs_faults(const rdl_trainer* t, rd_obs_faults* out);

/* rdl_evaluate with the student reading its windows through *of (RD_OBS_DROPOUT or RD_OBS_MISSING) at
 * Philox episode first_episode + e, with or without a draws table, and, with nz, its action perturbed
 * as rdl_evaluate_noisy perturbs it (nz = NULL or mode RD_NOISE_NONE: the mean acts): the records
 * (clean ob), returns, final_dist and state_out of that trajectory.  Bitwise the stepwise loop with
 * rd_mask_obs on every record as it enters the window.  Independent of the envs' settings; capturable.
 * RD_EINVAL as rdl_evaluate, and before it: NULL of, unknown mode, a bad keep_prob, mode =
 * RD_OBS_CLEAN (call the plain function); a bad *nz as rdl_evaluate_noisy names it. */
int rdl_evaluate_faulty(rdl_trainer* t, const rdl_eval_config* cfg, const rd_obs_faults* of, const rd_action_noise* nz,
                        const float* state0, float* returns, float* final_dist, float* records, float* state_out);

#ifdef __cplusplus
}
#endif
#endif
