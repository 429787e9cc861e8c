"""Batched on-policy distillation of the reference MLP student: one optimiser step of K env steps
per env as StudentMlpTrainer.step_envs (one env launch, the training launch, Adam) against the
stepwise composition of the calls that existed before it -- K x {DistillTrainer.forward (teacher),
student_mlp.rows, StudentMlpTrainer.forward, BatchedReacher.step}, then StudentMlpTrainer.step on
the K n concatenated rows -- in one process.

For each case (n envs, K): 64, 4,096 and 65,536 envs at K = 50, and 4,096 envs at K = 1.  Two
trainers with the same config (kl, lr 1e-4, keep_prob 0.5) take the same optimiser steps, one per
side; the first step's rows and the parameters after every warm-up step and after the last timed
step are asserted bitwise equal.  Each optimiser step is timed with device events, alternating the
two sides for ``--reps`` repetitions (>= 20).  Reports median, quartiles, min and max per side; no
speed-up is asserted.  Also records the loss curve of mlp_train.train_envs at the smoke test's
settings.  Writes one JSON file (default profiles/student_mlp_envs_fused_vs_stepwise.json) and
prints it.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reacherdistilation_amd import mlp_train  # noqa: E402
from reacherdistilation_amd.config import ACSPACE_SHAPE, EPISODE_STEPS  # noqa: E402
from reacherdistilation_amd.distill import DistillConfig, DistillTrainer  # noqa: E402
from reacherdistilation_amd.env import BatchedReacher  # noqa: E402
from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer, rows  # noqa: E402

DEV = "cuda:0"


class Stepwise:
    """The persistent state of the stepwise loop: the env, its observation, the last reward, the
    previous record's fields and the episode clock."""

    def __init__(self, tr, sm, n):
        self.tr, self.sm, self.n = tr, sm, n
        self.env = BatchedReacher(n, seed=0, device=DEV)
        self.ob = self.env.reset()
        self.reward = torch.zeros(n, 1, device=DEV)
        self.prev_t, self.prev_r = torch.zeros(n, 4, device=DEV), torch.zeros(n, 1, device=DEV)
        self.zt, self.zr = torch.zeros(n, 4, device=DEV), torch.zeros(n, 1, device=DEV)
        self.s = 0

    def opt_step(self, K):
        """K env steps under the student's mean, then one optimiser step on their K n rows."""
        xs, ts = [], []
        for _ in range(K):
            t, _ = self.tr.forward(self.ob, student=False)
            first = self.s == 0
            x = rows(self.ob, self.zt if first else self.prev_t, self.zr if first else self.prev_r)
            s = self.sm.forward(x)
            self.prev_t, self.prev_r = t, self.reward
            self.ob, rew, _, _ = self.env.step(s[:, :ACSPACE_SHAPE].contiguous())
            self.reward = rew.clone().view(self.n, 1)
            self.s = (self.s + 1) % EPISODE_STEPS
            xs.append(x)
            ts.append(t)
        x, t = (xs[0], ts[0]) if K == 1 else (torch.cat(xs), torch.cat(ts))
        self.sm.step(x, t)
        return x, t


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3   # us


def stats(us):
    q = statistics.quantiles(us, n=4)
    return dict(median_us=statistics.median(us), q1_us=q[0], q3_us=q[2], iqr_us=q[2] - q[0], min_us=min(us),
                max_us=max(us), reps=len(us))


def run(n, K, reps, warmup):
    tr = DistillTrainer(DistillConfig(n_envs=64, seed=0), device=DEV)
    cfg = StudentMlpConfig(loss="kl", lr=1e-4, keep_prob=0.5, seed=0)
    fused, twin = StudentMlpTrainer(cfg, device=DEV), StudentMlpTrainer(cfg, device=DEV)
    fused.set_teacher(tr.teacher)
    fused.attach_envs(n, seed=0, accum_steps=K)
    loop = Stepwise(tr, twin, n)
    same = True
    for k in range(max(warmup, 1)):   # same bits first: the rows of the first step, the parameters of each
        r = fused.step_envs()
        x, t = loop.opt_step(K)
        if k == 0:
            same = same and bool(torch.equal(r.x.reshape(-1, 16), x) and torch.equal(r.t_pdflat.reshape(-1, 4), t))
        same = same and bool(torch.equal(fused.params(), twin.params()))
    assert same, f"n = {n}, K = {K}: step_envs and the stepwise loop differ"
    torch.cuda.synchronize()
    f_us, s_us = [], []
    for _ in range(reps):   # alternating, so that both sides see the same machine
        s_us.append(timed(lambda: loop.opt_step(K)))
        f_us.append(timed(fused.step_envs))
    same = bool(torch.equal(fused.params(), twin.params())) and fused.counter() == twin.counter()
    assert same, f"n = {n}, K = {K}: the parameters differ after the timed steps"
    loop.env.close()
    fused.close()
    twin.close()
    tr.close()
    f, s = stats(f_us), stats(s_us)
    return dict(n_envs=n, env_steps_per_opt_step=K, rows_per_opt_step=n * K, bitwise_equal_params=same, fused=f,
                stepwise=s, fused_iqr_below_stepwise=f["q3_us"] < s["q1_us"],
                stepwise_iqr_below_fused=s["q3_us"] < f["q1_us"], speedup_median=s["median_us"] / f["median_us"],
                fused_env_steps_per_s=n * K / (f["median_us"] * 1e-6), fused_launches=3, stepwise_launches=4 * K + 2)


def curve():
    """mlp_train.train_envs at tests/test_student_mlp_envs_gpu.py::test_train_envs_smoke's settings."""
    sm, history = mlp_train.train_envs(64, 20, keep_prob=0.5, lr=1e-3, accum_steps=50)
    sm.close()
    return dict(n_envs=64, accum_steps=50, opt_steps=20, keep_prob=0.5, lr=1e-3, loss="kl",
                columns=["opt_step", "loss_sum_over_rows", "action_mse", "mean_step_reward"], history=history)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, nargs="*", default=[64, 50, 4096, 50, 65536, 50, 4096, 1],
                    help="pairs: n_envs K")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "student_mlp_envs_fused_vs_stepwise.json"))
    a = ap.parse_args()
    if a.reps < 20 or len(a.cases) % 2:
        ap.error("--reps >= 20 and --cases in pairs")
    res = dict(device=torch.cuda.get_device_name(0),
               method="device events around one optimiser step (K env steps per env, training launch, Adam), "
                      "alternating sides; quartiles by statistics.quantiles",
               results=[run(n, K, a.reps, a.warmup) for n, K in zip(a.cases[::2], a.cases[1::2])],
               train_envs_curve=curve())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
