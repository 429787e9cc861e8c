"""The expected coins of DAgger's beta-mixture in the students' persistent envs (rdm_ / rdl_
envs_set_teacher_share), from NumPy: oracle/refnet_np.philox4x32_10 and the rule of
include/reacher_student_mlp.h -- the teacher steps env e = env_base + i at step s of its episode iff
(word 0 of Philox(ctr = {e lo, e hi, episode, 0x80000000 | s}, key = coin seed) >> 8) 2^-24 < beta.
Shared by tests/test_envs_teacher_share_host.py and the two *_envs_mix_gpu.py suites, with the (coin
seed, env_base, n, steps) of every mixed GPU run, so that the host suite can check their premise:
at beta = 0.5 both actors occur for some env inside one episode."""
import numpy as np

from oracle import refnet_np as rn

EPISODE = 50
BETA = 0.5
# (coin seed, env_base, n_envs, lockstep steps from the attach): every beta = 0.5 run of the GPU suites
MLP_RUNS = [(11, 5, 1, 100), (11, 5, 17, 100), (11, 5, 83, 100),   # against the stepwise loop
            (7, 0, 595, 50),                                       # 64-env against 16-env blocks
            (11, 5, 83, 56),                                       # step_envs, 8 x K = 7
            (9, 5, 17, 50)]                                        # the ring's flags; an explicit coin seed
LSTM_RUNS = [(11, 5, 1, 100), (11, 5, 17, 100), (11, 5, 35, 100)]


def teacher_coins(coin_seed, env_base, n, episode, step, beta):
    """bool [n]: the teacher steps env env_base + i at (episode, step)"""
    e = np.arange(n, dtype=np.uint64) + np.uint64(env_base)
    ctr = [e & rn.M32, e >> np.uint64(32), np.full(n, episode, np.uint64),
           np.full(n, 0x80000000 | int(step), np.uint64)]
    w = rn.philox4x32_10(ctr, int(coin_seed) & 0xFFFFFFFF, (int(coin_seed) >> 32) & 0xFFFFFFFF)[0]
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u < np.float32(beta)


def coin_table(coin_seed, env_base, n, steps, beta, start=0):
    """bool [steps, n] for lockstep envs from global step `start` (episode g // 50, step g % 50)"""
    return np.stack([teacher_coins(coin_seed, env_base, n, g // EPISODE, g % EPISODE, beta)
                     for g in range(start, start + steps)])
