"""Whole-episode evaluation of the reference MLP student: the fused launch
(StudentMlpTrainer.evaluate) against the stepwise loop it replaces (per step: the teacher's
DistillTrainer.forward, student_mlp.rows, StudentMlpTrainer.forward, BatchedReacher.step), in one
process.

For each size (n = 4,096 and 262,144 by default; E = 1, Philox resets) both sides are first
asserted to return the same bits, warmed up, then timed with device events around one whole
episode, alternating the two sides for ``--reps`` repetitions (>= 20).  Reports median, quartiles,
min and max per side.  Writes one JSON file (default
profiles/evaluate_student_mlp_fused_vs_stepwise.json), prints it, and fails if at 4,096 envs the
fused launch's interquartile range does not lie entirely below the stepwise loop's.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reacherdistilation_amd.config import ACSPACE_SHAPE, EPISODE_STEPS  # noqa: E402
from reacherdistilation_amd.distill import DistillConfig, DistillTrainer  # noqa: E402
from reacherdistilation_amd.env import BatchedReacher  # noqa: E402
from reacherdistilation_amd.student_mlp import StudentMlpTrainer, rows  # noqa: E402

DEV = "cuda:0"


def stepwise_episode(tr, sm, env):
    """One episode of every env under the student's mean; f32 returns summed in step order.  The
    reward field of a record is the previous step's reward (0 before an env's first step)."""
    n = env.n
    ob = env.reset()
    ret = torch.zeros(n, dtype=torch.float32, device=DEV)
    field = torch.zeros(n, 1, device=DEV)                       # record s's reward field
    prev_t, prev_r = torch.zeros(n, 4, device=DEV), torch.zeros(n, 1, device=DEV)
    for _ in range(EPISODE_STEPS):
        t, _ = tr.forward(ob, student=False)
        s = sm.forward(rows(ob, prev_t, prev_r))
        prev_t, prev_r = t, field
        ob, rew, _, _ = env.step(s[:, :ACSPACE_SHAPE].contiguous())
        ret = ret + rew
        field = rew.clone().view(n, 1)
    return ret


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


def run(n, reps, warmup):
    tr = DistillTrainer(DistillConfig(n_envs=64, seed=0), device=DEV)
    sm = StudentMlpTrainer(device=DEV)
    sm.set_teacher(tr.teacher)
    env = BatchedReacher(n, seed=0, device=DEV)
    # same bits first: the stepwise env's first episode is Philox episode 0
    same = bool(torch.equal(stepwise_episode(tr, sm, env), sm.evaluate(n, 1, seed=0).returns[0]))
    assert same, f"n = {n}: the fused launch and the stepwise loop differ"
    for _ in range(warmup):
        stepwise_episode(tr, sm, env)
        sm.evaluate(n, 1, seed=0)
    torch.cuda.synchronize()
    fused, step = [], []
    for _ in range(reps):   # alternating, so that both sides see the same machine
        step.append(timed(lambda: stepwise_episode(tr, sm, env)))
        fused.append(timed(lambda: sm.evaluate(n, 1, seed=0)))
    env.close()
    sm.close()
    tr.close()
    f, s = stats(fused), stats(step)
    return dict(n_envs=n, episodes=1, bitwise_equal=same, fused=f, stepwise=s,
                fused_iqr_below_stepwise=f["q3_us"] < s["q1_us"],
                speedup_median=s["median_us"] / f["median_us"],
                fused_env_steps_per_s=n * EPISODE_STEPS / (f["median_us"] * 1e-6), fused_launches=1)


def block_sizes(reps):
    """The fused launch alone by its block of envs (rdm_evaluate's eval_small_rows rule: 16-env
    blocks while each has a workgroup of the grid to itself, else 64-env blocks).  A grid cap below
    / at the count of 16-env blocks forces the other size; the bits are the same."""
    tr = DistillTrainer(DistillConfig(n_envs=64, seed=0), device=DEV)
    sm = StudentMlpTrainer(device=DEV)
    sm.set_teacher(tr.teacher)
    out = []
    for n in (4096, 8192):
        blocks16 = (n + 15) // 16
        auto = sm.evaluate(n, 1, seed=0).returns
        for rows, grid in ((16, blocks16), (64, blocks16 - 1)):
            assert torch.equal(sm.evaluate(n, 1, seed=0, grid=grid).returns, auto)
            torch.cuda.synchronize()
            us = [timed(lambda: sm.evaluate(n, 1, seed=0, grid=grid)) for _ in range(reps)]
            out.append(dict(n_envs=n, block_envs=rows, grid_cap=grid, **stats(us)))
    sm.close()
    tr.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 262144])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_student_mlp_fused_vs_stepwise.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps >= 20")
    res = dict(device=torch.cuda.get_device_name(0),
               method="device events around one 50-step episode, alternating sides; quartiles by statistics.quantiles",
               results=[run(n, a.reps, a.warmup) for n in a.sizes], fused_by_block_size=block_sizes(a.reps))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    for r in res["results"]:
        if r["n_envs"] == 4096:
            assert r["fused_iqr_below_stepwise"], "4,096 envs: the fused interquartile range is not below the stepwise one"
