/* Action noise of the acting policy in the students' closed loop: ONE definition, used by the
 * persistent-env calls (rdm_ / rdl_envs_set_action_noise), by the noisy evaluations
 * (rdm_ / rdl_evaluate_noisy) and by the stepwise primitive below.
 *
 * Both reference students and the PPO teacher emit a pdflat = mean[2] | logstd[2].  Without noise the
 * mean acts.  With noise the action handed to env.step is a sample around the mean of whoever acts
 * at that step -- the policy's own Gaussian (what baselines calls stochastic=True), or an isotropic
 * one of a fixed sigma (DART's noise injection, Laskey et al. 2017).
 *
 * For env e = env_base + i at step s (0..49) of Philox episode `episode`:
 *   w   = Philox4x32-10(ctr = {e lo, e hi, episode, 0x40000000 | s}, key = {seed lo, seed hi})
 *   u1  = ((w0 >> 8) + 1) 2^-24        in (0, 1]
 *   u2  = (w1 >> 8) 2^-24
 *   rad = sqrtf(-2 logf(u1));  ang = 6.283185307179586f u2
 *   xi0 = rad cosf(ang);       xi1 = rad sinf(ang)
 *   g_c = scale (POLICY ? expf(logstd_c) : 1);   a_c = fmaf(g_c, xi_c, mean_c)
 * Every operation is one f32 operation in this order, nothing contracted but the stated fmaf, so
 * every caller computes the same bits.  Counter word 3 has bit 30 set and bit 31 clear: the stream is
 * disjoint from the reset draws' (word 3 = 0, 1) and from the beta-mixture's coins' (bit 31 set) even
 * under equal seeds.  The noise is a function of (seed, env, episode, step) alone.
 * env.step clips the control to +-1 and charges the control cost on the unclipped action, as it does
 * for a mean: noise cannot drive the dynamics outside the range saturated means already reach. */
#ifndef REACHER_ACTION_NOISE_H
#define REACHER_ACTION_NOISE_H

#include <stdint.h>

#include "reacher.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RD_NOISE_NONE   0   /* the mean acts                                          */
#define RD_NOISE_POLICY 1   /* a_c = mean_c + scale * exp(logstd_c) * xi_c            */
#define RD_NOISE_FIXED  2   /* a_c = mean_c + scale * xi_c  (DART's isotropic sigma)  */
typedef struct {
    int32_t mode;            /* RD_NOISE_*                                            */
    float scale;             /* >= 0, finite                                          */
    uint64_t seed;           /* the noise's Philox key                                */
} rd_action_noise;

/* The stepwise primitive: actions[i] = the action of env env_base + i at (episode, step) under *nz,
 * given its acting pdflat[i] = mean[2] | logstd[2]; xi (optional) receives the two normal draws.
 * One small launch on hip_stream of `device`, asynchronous; all three buffers are device memory.
 * mode = RD_NOISE_NONE copies the means (xi is still the draws).
 * RD_EINVAL, naming the function and the field, before any device call: NULL nz, pdflat or actions;
 * unknown mode; scale NaN, negative or infinite; n < 1; negative env_base, episode or step;
 * step > 49. */
int rd_perturb_actions(const rd_action_noise* nz, int64_t env_base, int64_t n, int32_t episode, int32_t step,
                       const float* pdflat /*[n][4]*/, float* actions /*[n][2]*/, float* xi /*[n][2] or NULL*/,
                       int device, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
