/* Sensor faults on the student's observation in the closed loop: ONE definition, used by the
 * persistent-env calls (rdm_ / rdl_envs_set_obs_faults), by the faulty evaluations
 * (rdm_ / rdl_evaluate_faulty) and by the stepwise primitive below.
 *
 * Both reference students are trained with tf.nn.dropout on the observation (keep_prob).  The question
 * that dropout exists for is how the student acts when its sensors actually fail: here the student,
 * and only the student, reads a masked observation while it steps the envs.  The teacher reads the
 * clean one, and every record, row and window keeps the clean one.
 *
 * For env e = env_base + i, the record of step s (0..49) of Philox episode `episode`, component
 * k = 0..10 of the observation:
 *   w^q    = Philox4x32-10(ctr = {e lo, e hi, episode, 0x20000000 | (q << 8) | s}, key = {seed lo, seed hi}),
 *            q = k / 4
 *   u_k    = (w^q[k % 4] >> 8) 2^-24
 *   keep_k = u_k < keep_prob
 *   seen_k = keep_k ? (DROPOUT ? ob_k / keep_prob : ob_k) : 0
 * scaled(ob_k) = ob_k / keep_prob is ONE f32 division, the arithmetic the training kernels' dropout
 * applies to a kept component (no reciprocal is formed): a DROPOUT query is exactly the transform the
 * student was trained under.  Counter word 3 has bit 29 set and bits 30 and 31 clear: the stream is
 * disjoint from the reset draws' (word 3 = 0, 1), the action noise's (bit 30) and the beta-mixture's
 * coins' (bit 31) even under equal seeds.  The mask is a function of (seed, env, episode, step,
 * component) alone.  keep_prob is in (0, 1]; at keep_prob = 1 every u_k < 1 is kept and x / 1 = x, so
 * seen is bitwise ob in both modes. */
#ifndef REACHER_OBS_FAULTS_H
#define REACHER_OBS_FAULTS_H

#include <stdint.h>

#include "reacher.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RD_OBS_CLEAN   0   /* the student reads ob                                            */
#define RD_OBS_DROPOUT 1   /* tf.nn.dropout: kept readings scaled by 1/keep_prob, lost = 0    */
#define RD_OBS_MISSING 2   /* a dead sensor: kept readings as they are, lost = 0              */
typedef struct {
    int32_t mode;            /* RD_OBS_*                                              */
    float keep_prob;         /* in (0, 1]                                             */
    uint64_t seed;           /* the mask's Philox key                                 */
} rd_obs_faults;

/* The stepwise primitive: seen[i] = what the student reads of ob[i], the observation of env
 * env_base + i at (episode, step), under *of; kept (optional) receives keep_k as 0 / 1.
 * One small launch on hip_stream of `device`, asynchronous; all three buffers are device memory.
 * mode = RD_OBS_CLEAN copies ob to seen (kept is still the draws' keep_k).
 * RD_EINVAL, naming the function and the field, before any device call: NULL of, ob or seen; unknown
 * mode; keep_prob NaN, <= 0 or > 1; n < 1; negative env_base, episode or step; step > 49. */
int rd_mask_obs(const rd_obs_faults* of, int64_t env_base, int64_t n, int32_t episode, int32_t step,
                const float* ob /*[n][11]*/, float* seen /*[n][11]*/, uint8_t* kept /*[n][11] or NULL*/,
                int device, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
