"""Whole-episode evaluation of the reference LSTM student: the fused rollout launch
(StudentLstmTrainer.evaluate) against the stepwise loop it replaces (per step: the teacher's
DistillTrainer.forward, the window assembled on the device, StudentLstmTrainer.forward,
BatchedReacher.step), in one process.

For each size (n = 1, the driver's case, 64 and 4,096 by default; E = 1, T = 10, Philox resets, zero
initial state) both sides are first asserted to return the same bits, warmed up, then timed with
device events around one whole episode, alternating the two sides for ``--reps`` repetitions
(>= 20).  Reports median, quartiles, min and max per side and which side is faster; no ratio is
required.  Writes one JSON file (default profiles/evaluate_student_lstm_fused_vs_stepwise.json) and
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
from reacherdistilation_amd.config import ACSPACE_SHAPE, EPISODE_STEPS, STEPS_UNROLLED  # noqa: E402
from reacherdistilation_amd.distill import DistillConfig, DistillTrainer  # noqa: E402
from reacherdistilation_amd.env import BatchedReacher  # noqa: E402
from reacherdistilation_amd.student_lstm import StudentLstmConfig, StudentLstmTrainer  # noqa: E402

DEV = "cuda:0"


def stepwise_episode(tr, st, env):
    """One episode of every env under the student's mean, from a zero LSTM state; f32 returns summed
    in step order.  The window slides on the device: rows T-1-s.. hold the episode's records so far
    (ob | the previous record's teacher pdflat), zero rows in front."""
    n, T = env.n, st.T
    ob = env.reset()
    ret = torch.zeros(n, dtype=torch.float32, device=DEV)
    ob_w, prev_w = torch.zeros(T, n, 11, device=DEV), torch.zeros(T, n, 4, device=DEV)
    prev_t = torch.zeros(n, 4, device=DEV)
    state = None
    for _ in range(EPISODE_STEPS):
        t, _ = tr.forward(ob, student=False)
        ob_w, prev_w = torch.cat((ob_w[1:], ob[None])), torch.cat((prev_w[1:], prev_t[None]))
        out, state = st.forward(ob_w, prev_w, state)
        prev_t = t
        ob, rew, _, _ = env.step(out[T - 1, :, :ACSPACE_SHAPE].contiguous())
        ret = ret + rew
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
    st = StudentLstmTrainer(StudentLstmConfig(steps=STEPS_UNROLLED, max_windows=n), device=DEV)
    st.set_teacher(tr.teacher)
    env = BatchedReacher(n, seed=0, device=DEV)
    # same bits first: the stepwise env's first episode is Philox episode 0
    same = bool(torch.equal(stepwise_episode(tr, st, env), st.evaluate(n, 1, seed=0).returns[0]))
    assert same, f"n = {n}: the fused launch and the stepwise loop differ"
    for _ in range(warmup):
        stepwise_episode(tr, st, env)
        st.evaluate(n, 1, seed=0)
    torch.cuda.synchronize()
    fused, step = [], []
    for _ in range(reps):   # alternating, so that both sides see the same machine
        step.append(timed(lambda: stepwise_episode(tr, st, env)))
        fused.append(timed(lambda: st.evaluate(n, 1, seed=0)))
    env.close()
    st.close()
    tr.close()
    f, s = stats(fused), stats(step)
    return dict(n_envs=n, episodes=1, steps_unrolled=STEPS_UNROLLED, bitwise_equal=same, fused=f, stepwise=s,
                fused_iqr_below_stepwise=f["q3_us"] < s["q1_us"], stepwise_iqr_below_fused=s["q3_us"] < f["q1_us"],
                speedup_median=s["median_us"] / f["median_us"],
                fused_env_steps_per_s=n * EPISODE_STEPS / (f["median_us"] * 1e-6),
                fused_launches=2)   # the image pack and the rollout


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 64, 4096])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_student_lstm_fused_vs_stepwise.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps >= 20")
    res = dict(device=torch.cuda.get_device_name(0),
               method="device events around one 50-step episode, alternating sides; quartiles by statistics.quantiles",
               results=[run(n, a.reps, a.warmup) for n in a.sizes])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
