"""Batched on-policy distillation of the LSTM student: one optimiser step of K = 50 env steps per env
as StudentLstmTrainer.step_envs (the image pack, one env launch, the training pass, Adam) -- and the
env steps alone as act_envs -- against the stepwise composition of the calls that existed before it:
K x {DistillTrainer.forward (teacher), the query window formed on the device, StudentLstmTrainer.forward
from the carried state, BatchedReacher.step}, the training windows gathered on the device, then
StudentLstmTrainer.step on them -- in one process.

For each n (16, 64, 1,024 and 4,096 envs; T = 10, so 41 n windows per optimiser step) two trainers with
the same config (kl, lr 1e-3, keep_prob 0.5) take the same optimiser steps, one per side; the first
step's windows and the parameters after every warm-up step and after the last timed step are asserted
bitwise equal.  Each call is timed with device events, alternating the two sides for ``--reps``
repetitions (>= 20).  Reports median, quartiles, min and max per side; no speed-up is asserted.  Also
records a loss curve of lstm_train.train_envs.  Writes one JSON file (default
profiles/student_lstm_envs_fused_vs_stepwise.json) and prints it.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reacherdistilation_amd import lstm_train  # noqa: E402
from reacherdistilation_amd.config import ACSPACE_SHAPE, EPISODE_STEPS  # noqa: E402
from reacherdistilation_amd.distill import DistillConfig, DistillTrainer  # noqa: E402
from reacherdistilation_amd.env import BatchedReacher  # noqa: E402
from reacherdistilation_amd.student_lstm import StudentLstmConfig, StudentLstmTrainer  # noqa: E402

DEV = "cuda:0"
T = 10


class Stepwise:
    """The persistent state of the stepwise loop: the env, its observation, the carried query state,
    the episode clock, and the records of the last T-1 + K steps (ob, prev, the teacher's pdflat) in
    device buffers whose first T-1 rows are the call before's last."""

    def __init__(self, tr, st, n, K):
        self.tr, self.st, self.n, self.K = tr, st, n, K
        self.env = BatchedReacher(n, seed=0, device=DEV)
        self.ob = self.env.reset()
        self.state = None
        self.s = 0
        kw = dict(device=DEV)
        self.b_ob, self.b_prev, self.b_t = (torch.zeros(T - 1 + K, n, d, **kw) for d in (11, 4, 4))
        self.zero4 = torch.zeros(n, 4, **kw)

    def act(self, K=None):
        """K env steps under the student's mean; returns the buffer rows of the qualifying steps."""
        K = self.K if K is None else K
        for b in (self.b_ob, self.b_prev, self.b_t):   # the call before's last T-1 records
            b[:T - 1] = b[K:K + T - 1].clone()
        ends = []
        for k in range(K):
            t, _ = self.tr.forward(self.ob, student=False)
            j = T - 1 + k
            self.b_ob[j] = self.ob
            self.b_prev[j] = self.b_t[j - 1] if self.s else self.zero4
            self.b_t[j] = t
            ob_w, prev_w = self.b_ob[k:j + 1].clone(), self.b_prev[k:j + 1].clone()
            if self.s < T - 1:   # zero rows before the episode's first record
                ob_w[:T - 1 - self.s] = 0
                prev_w[:T - 1 - self.s] = 0
            else:
                ends.append(j)
            out, self.state = self.st.forward(ob_w, prev_w, self.state)
            self.ob, _, _, _ = self.env.step(out[T - 1, :, :ACSPACE_SHAPE].contiguous())
            self.s = (self.s + 1) % EPISODE_STEPS
        return ends

    def opt_step(self):
        """K env steps, then one optimiser step on the windows that lie inside an episode."""
        ends = self.act()
        idx = torch.tensor([[j - T + 1 + p for j in ends] for p in range(T)], device=DEV)
        w = tuple(b[idx].reshape(T, len(ends) * self.n, -1) for b in (self.b_ob, self.b_prev, self.b_t))
        self.st.step(*w)
        return w


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


def side(f_us, s_us):
    f, s = stats(f_us), stats(s_us)
    return dict(fused=f, stepwise=s, fused_iqr_below_stepwise=f["q3_us"] < s["q1_us"],
                stepwise_iqr_below_fused=s["q3_us"] < f["q1_us"], speedup_median=s["median_us"] / f["median_us"])


def run(n, K, reps, warmup):
    B = n * (K // EPISODE_STEPS) * (EPISODE_STEPS + 1 - T)
    tr = DistillTrainer(DistillConfig(n_envs=64, seed=0), device=DEV)
    cfg = StudentLstmConfig(loss="kl", lr=1e-3, keep_prob=0.5, seed=0, steps=T, max_windows=B)
    fused, twin = StudentLstmTrainer(cfg, device=DEV), StudentLstmTrainer(cfg, device=DEV)
    fused.set_teacher(tr.teacher)
    fused.attach_envs(n, seed=0, accum_steps=K)
    loop = Stepwise(tr, twin, n, K)
    same = True
    for k in range(max(warmup, 1)):   # same bits first: the windows of the first step, the parameters of each
        r = fused.step_envs()
        w = loop.opt_step()
        if k == 0:
            same = same and all(bool(torch.equal(a, b)) for a, b in zip((r.ob_w, r.prev_w, r.t_w), w))
        same = same and bool(torch.equal(fused.params(), twin.params()))
    assert same, f"n = {n}, K = {K}: step_envs and the stepwise loop differ"
    torch.cuda.synchronize()
    f_us, s_us, fa_us, sa_us = [], [], [], []
    for _ in range(reps):   # alternating, so that both sides see the same machine
        s_us.append(timed(loop.opt_step))
        f_us.append(timed(fused.step_envs))
        sa_us.append(timed(loop.act))
        fa_us.append(timed(fused.act_envs))
    same = bool(torch.equal(fused.params(), twin.params())) and fused.counter() == twin.counter()
    same = same and bool(torch.equal(fused.query_state(), loop.state))
    assert same, f"n = {n}, K = {K}: the parameters or the query state differ after the timed steps"
    loop.env.close()
    fused.close()
    twin.close()
    tr.close()
    res = dict(n_envs=n, env_steps_per_opt_step=K, steps_unrolled=T, windows_per_opt_step=B, bitwise_equal_params=same,
               step_envs=side(f_us, s_us), act_envs=side(fa_us, sa_us))
    res["fused_env_steps_per_s"] = n * K / (res["step_envs"]["fused"]["median_us"] * 1e-6)
    return res


def curve(n, steps):
    st, history = lstm_train.train_envs(n, steps, keep_prob=0.5, warmup_steps=2)
    st.close()
    return dict(n_envs=n, accum_steps=50, opt_steps=steps, warmup_steps=2, keep_prob=0.5, lr=1e-3, loss="kl",
                columns=["opt_step", "loss_sum_over_rows", "action_mse", "mean_step_reward"], history=history)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="*", default=[16, 64, 1024, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--curve", type=int, nargs=2, default=[256, 40], help="n_envs opt_steps of the train_envs curve")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "student_lstm_envs_fused_vs_stepwise.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps >= 20")
    res = dict(device=torch.cuda.get_device_name(0),
               method="device events around one call (step_envs: 50 env steps per env, the training pass, Adam; "
                      "act_envs: the env steps alone), alternating sides; quartiles by statistics.quantiles",
               results=[run(n, EPISODE_STEPS, a.reps, a.warmup) for n in a.envs],
               train_envs_curve=curve(*a.curve))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
