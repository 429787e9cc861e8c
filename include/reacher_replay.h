/* reacher_replay.h -- C ABI of the device-resident episode replay ring: whole episodes pushed by
 * the envs / evaluation calls, training batches of any size drawn from them ON THE DEVICE
 * (libreacher.so).
 *
 * It is the aggregate half of the reference's DAgger loop for the batched paths: every step record
 * enters a Dataset of past episodes and every optimiser step trains on a random batch of windows
 * drawn from that aggregate (reference src/distilation/dataset.py:166-194).  The single-env drivers
 * have it as DeviceDataset, whose windows a host RNG draws and whose index tensor is built on the
 * host and copied over per batch.  Here the episodes stay on the device, the draw is a counter-based
 * Philox stream evaluated by the sampling launch itself, and the batch goes straight to rdl_step /
 * rdm_step: no host RNG, no index upload, no sync, so push + sample + step can sit in one hipGraph,
 * and the batch size no longer follows from the env count.
 *
 * Storage
 *   ring    rec[capacity][50][21] f32, the dataset's record layout
 *           ob[11] | rew | t_pdflat[4] | s_pdflat[4] | stepped_with
 *           (rew = the reward the env's PREVIOUS step returned, as every record-writing call has it).
 *   header  two int64 counters on the device:
 *           pushed  episodes ever pushed.  Episode g lives in slot g % capacity; the stored count is
 *                   min(pushed, capacity).
 *           draws   sample launches so far; its low 32 bits are the Philox draw index d.
 *   The kernels read the counters FROM THE DEVICE when they run, and a 1-thread launch behind each
 *   push or sample adds to them, ordered by the stream: no atomics, no grid-wide sync, and no
 *   host-side count enters a launch.  A captured call therefore replays the NEXT push or draw, as the
 *   envs calls' device clock does (reacher_student_mlp.h).  The handle also keeps a host mirror of
 *   `pushed`, advanced when a push is ISSUED; it is used for one thing only, to refuse a sample from a
 *   ring nothing was ever pushed to.  (A captured sample replayed after rd_replay_reset finds count =
 *   0 on the device and reads slot 0; it stays inside the ring.)
 *
 * Pushes are pure copies: one launch plus the counter bump.  Every float is copied unchanged.
 *
 * Draws.  With d = the low 32 bits of `draws` as the launch finds it and w = window_base + b for
 * window (row) b of the batch:
 *   (r0, r1, ., .) = Philox4x32-10(ctr = {w lo, w hi, d, 0}, key = {seed lo, seed hi})
 *   count = min(pushed, capacity), or min(count, recent) when recent > 0: the `recent` newest episodes
 *   rank  r = (r0 * count) >> 32, counted from the oldest eligible episode
 *   slot  = (pushed - count + r) % capacity
 *   start (windows), RD_REPLAY_START_PER_WINDOW: (r1 * (51 - T)) >> 32
 *                    RD_REPLAY_START_COMMON (one start for the batch, the reference's training_batches):
 *                    (c0 * (51 - T)) >> 32, c0 = word 0 of Philox4x32-10({0xFFFFFFFF, 0xFFFFFFFF, d, 1}, key)
 *   step  (rows):    (r1 * 50) >> 32
 * The multiply-high map of a 32-bit word onto [0, m) gives each value a probability within 2^-32 of
 * 1/m: a relative bias of at most m / 2^32 per episode (count / 2^32; 2e-6 at 8,192 episodes).
 * Record semantics are DeviceDataset._prev's: the prev fields of record j are record j-1's t_pdflat and
 * rew, zeros at j = 0, and record j-1 is never read across an episode boundary.  All outputs are
 * bitwise functions of the ring, the counters and the sample struct.
 *
 * Conventions as in reacher.h: device pointers, asynchronous on the handle's stream (capturable: no
 * allocation and no host sync outside create / destroy / rd_replay_counters), 0 = OK, RD_EINVAL for a
 * bad argument (checked before any device call; rd_last_error() names the function and the field),
 * -(hipError_t) for a HIP error.  One handle per stream; not thread-safe per handle.
 * Multi-GPU is out of scope: one ring per process, filled by that process's envs; ranks that want
 * disjoint draw streams from equal seeds give each its own window_base range.
 */
#ifndef REACHER_REPLAY_H
#define REACHER_REPLAY_H
#include <stdint.h>

#include "reacher.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RD_REPLAY_EPISODE_STEPS 50
#define RD_REPLAY_RECORD 21
#define RD_REPLAY_MAX_BATCH 4194304      /* 2^22: the largest max_batch (flat output indices stay in 32 bits) */
#define RD_REPLAY_START_PER_WINDOW 0
#define RD_REPLAY_START_COMMON 1

typedef struct {
    int64_t capacity;    /* episodes the ring holds, 1 .. 2^31 - 1                 */
    int64_t max_batch;   /* largest B of any sample, 1 .. RD_REPLAY_MAX_BATCH      */
} rd_replay_config;

typedef struct rd_replay rd_replay;

/* ring NULL: the library allocates (and zeroes, and frees) the ring; else a caller-owned device
 * buffer [capacity][50][21] that outlives the handle.  Counters start at 0.
 * RD_EINVAL: NULL out or config; capacity or max_batch out of range. */
int rd_replay_create(rd_replay** out, const rd_replay_config* cfg, float* ring, int device, void* hip_stream);
int rd_replay_destroy(rd_replay* h);
int rd_replay_set_stream(rd_replay* h, void* hip_stream);
/* both counters (and the host mirror) to 0; the ring's floats stay */
int rd_replay_reset(rd_replay* h);
/* the ring's device pointer (NULL for a NULL handle) */
float* rd_replay_ring(rd_replay* h);
/* the device counters, read back: HOST-SYNCHRONISING on the handle's stream (either may be NULL) */
int rd_replay_counters(rd_replay* h, int64_t* pushed, int64_t* draws);

/* records [K][n_envs][21], the step-major block rdl_envs_act / rdl_step_envs write.  The caller
 * guarantees that row 0 is an episode's step 0 (lockstep envs after attach or reset, and after any
 * multiple of 50 steps).  Episode q = (k / 50) n_envs + i gets global index pushed + q; pushed +=
 * (K / 50) n_envs.  RD_EINVAL: NULL handle or records; steps < 1 or steps % 50 != 0; n_envs < 1;
 * (K / 50) n_envs > capacity (one call never overwrites its own episodes). */
int rd_replay_push_steps(rd_replay* h, const float* records, int64_t steps, int64_t n_envs);
/* records [E][50][21], the episode-major form of rdm_evaluate / rdl_evaluate records ([E][n] flattened)
 * and of the collected teacher episodes.  RD_EINVAL: NULL handle or records; E < 1 or E > capacity. */
int rd_replay_push_episodes(rd_replay* h, const float* records, int64_t episodes);
/* the outputs of rdm_envs_act: x [K][n][16], t_pdflat [K][n][4], s_pdflat [K][n][4] (NULL: zeros),
 * reward [K][n], carry [n] (NULL: zeros).  Record (k, i): ob = x[k][i][0..10], t, s, stepped_with, and
 * rew = the reward the env's previous step returned: reward[k-1][i], or carry[i] at k = 0 (the last
 * reward row of the previous call).  K and capacity rules as rd_replay_push_steps; also RD_EINVAL for
 * NULL x, t_pdflat or reward. */
int rd_replay_push_rows(rd_replay* h, const float* x, const float* t_pdflat, const float* s_pdflat,
                        const float* reward, const float* carry, int64_t steps, int64_t n_envs, float stepped_with);
/* (The form with a stepped_with per row, rd_replay_push_rows_flags, is declared beside the call that
 * fills its flags, rdm_envs_bind_stepped_with in reacher_student_mlp.h: this header's list of names is
 * as it was.) */

typedef struct {
    int32_t steps;        /* T, 1 .. 50 (rd_replay_sample_rows ignores it)          */
    int32_t start_mode;   /* RD_REPLAY_START_*                                      */
    int64_t windows;      /* B, 1 .. max_batch                                      */
    int64_t window_base;  /* global index of window 0 (>= 0): the Philox counter    */
    int64_t recent;       /* 0 = every stored episode; else the newest `recent`     */
    uint64_t seed;        /* Philox key                                             */
} rd_replay_sample;

/* B windows of T consecutive records, position-major as rdl_step takes them:
 *   ob_w [T][B][11]  ob of record start + p
 *   prev_w [T][B][4] t_pdflat of record start + p - 1 (zeros at record 0)
 *   t_w [T][B][4]    t_pdflat of record start + p
 *   prew_w [T][B][1] rew of record start + p - 1 (zeros at record 0); may be NULL
 *   idx [B][2] int32 (slot, start) of each window; may be NULL
 * draws += 1.  RD_EINVAL: NULL handle, sample, ob_w, prev_w or t_w; steps outside 1..50; windows < 1;
 * unknown start_mode; negative window_base or recent (all before the handle is read); then windows >
 * max_batch; a ring never pushed to. */
int rd_replay_sample_windows(rd_replay* h, const rd_replay_sample* s, float* ob_w, float* prev_w, float* t_w,
                             float* prew_w, int32_t* idx);
/* B single records as the rows rdm_step takes (exactly the row rdm_envs_act emitted for that step):
 *   x [B][16] = ob_s | t_pdflat of record s-1 | rew of record s-1 (zeros at s = 0); 16-byte aligned
 *   t_pdflat [B][4] of record s;  idx [B][2] int32 (slot, step), may be NULL
 * draws += 1.  RD_EINVAL as above (steps and start_mode are not read), and for a misaligned x. */
int rd_replay_sample_rows(rd_replay* h, const rd_replay_sample* s, float* x, float* t_pdflat, int32_t* idx);

#ifdef __cplusplus
}
#endif
#endif
