"""The action noise of the students' closed loop (include/reacher_action_noise.h) from NumPy:
oracle/refnet_np.philox4x32_10 and the header's definition -- for env e = env_base + i at step s of
Philox episode `episode`

    w   = Philox4x32-10(ctr = {e lo, e hi, episode, 0x40000000 | s}, key = seed)
    u1  = ((w0 >> 8) + 1) 2^-24,  u2 = (w1 >> 8) 2^-24
    xi  = sqrt(-2 log u1) (cos, sin)(2 pi u2)
    a_c = mean_c + scale (POLICY ? exp(logstd_c) : 1) xi_c

in float32.  Shared by tests/test_action_noise_host.py and the *_noise_gpu.py suites, with the seeds
and shapes of the GPU runs, so that the host suite can check the draws' moments over exactly those."""
import numpy as np

from oracle import refnet_np as rn

EPISODE = 50
NONE, POLICY, FIXED = 0, 1, 2
MODES = {"none": NONE, "policy": POLICY, "fixed": FIXED}
NOISE_BIT = 0x40000000
# (noise seed, env_base, n_envs, lockstep steps from the attach) of the GPU suites' runs against the
# stepwise loop; the moments are checked over the largest, 83 envs x 100 steps x 2 draws
RUNS = [(11, 5, 1, 100), (11, 5, 17, 100), (11, 5, 83, 100)]
# rd_perturb_actions against this model: env ids across 2^32, a seed with a high word
WIDE_SEED, WIDE_BASE = 0x9E3779B97F4A7C15, 2 ** 32 - 40


def counters(env_base, n, episode, step):
    """the four Philox counter words [4][n] (uint64 holding 32-bit values)"""
    e = np.arange(n, dtype=np.uint64) + np.uint64(env_base)
    return [e & rn.M32, e >> np.uint64(32), np.full(n, episode, np.uint64), np.full(n, NOISE_BIT | int(step), np.uint64)]


def normal_draws(seed, env_base, n, episode, step):
    """xi float32 [n, 2] of envs env_base .. env_base + n - 1 at (episode, step)"""
    w = rn.philox4x32_10(counters(env_base, n, episode, step), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    f = np.float32
    u1 = ((w[0] >> np.uint32(8)) + np.uint32(1)).astype(f) * f(2.0 ** -24)
    u2 = (w[1] >> np.uint32(8)).astype(f) * f(2.0 ** -24)
    rad = np.sqrt(f(-2.0) * np.log(u1)).astype(f)
    ang = (f(6.283185307179586) * u2).astype(f)
    return np.stack([rad * np.cos(ang).astype(f), rad * np.sin(ang).astype(f)], axis=1).astype(f)


def draw_table(seed, env_base, n, steps, start=0):
    """xi [steps, n, 2] for lockstep envs from global step `start` (episode g // 50, step g % 50)"""
    return np.stack([normal_draws(seed, env_base, n, g // EPISODE, g % EPISODE) for g in range(start, start + steps)])


def perturb(pdflat, xi, mode, scale):
    """actions float32 [n, 2] from the acting pdflat [n, 4] = mean | logstd and the draws"""
    f = np.float32
    p = np.asarray(pdflat, f)
    if mode == NONE:
        return p[:, :2].copy()
    g = f(scale) * (np.exp(p[:, 2:4]).astype(f) if mode == POLICY else f(1.0))
    return (g * np.asarray(xi, f) + p[:, :2]).astype(f)
