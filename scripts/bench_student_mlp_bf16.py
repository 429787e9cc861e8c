"""The reference MLP student in bf16 mixed precision (StudentMlpConfig(dtype="bf16")) against the
f32 student, in one process: two trainers that differ in nothing but the dtype (kl, lr 1e-4,
keep_prob 0.5) take the same calls.

  * ``step``: the training launch + Adam on 200, 204,800 and 3,276,800 caller rows;
  * ``step_envs``: one optimiser step of K = 50 env steps per env at 4,096 and 65,536 envs (the env
    launch, the training launch on the K n rows, Adam).

Each call is timed with device events, alternating the two sides for ``--reps`` repetitions (>= 20)
after ``--warmup`` calls per side.  Reports median, quartiles, min and max per side, and whether one
side's interquartile range lies wholly below the other's; no speed-up is asserted.  With
``--parent FILE --here FILE`` (the JSONs scripts/bench_student_mlp_envs.py wrote at the parent commit
and at this one in the same session: the same script, so the same interleaving with its stepwise
side) each f32 step_envs median of this commit is compared with the parent's quartiles widened by
one IQR.  Writes one JSON file (default profiles/student_mlp_bf16_vs_f32.json) and prints it.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reacherdistilation_amd.distill import DistillConfig, DistillTrainer  # noqa: E402
from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer  # noqa: E402

DEV = "cuda:0"
SIDES = ("f32", "bf16")


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


def compare(calls, reps, warmup):
    """calls: {side: fn}.  Alternating timed calls after the warm-up; the per-side stats and verdicts."""
    for _ in range(max(warmup, 1)):
        for side in SIDES:
            calls[side]()
    torch.cuda.synchronize()
    us = {side: [] for side in SIDES}
    for _ in range(reps):   # alternating, so that both sides see the same machine
        for side in SIDES:
            us[side].append(timed(calls[side]))
    f, b = stats(us["f32"]), stats(us["bf16"])
    return dict(f32=f, bf16=b, bf16_iqr_below_f32=b["q3_us"] < f["q1_us"], f32_iqr_below_bf16=f["q3_us"] < b["q1_us"],
                speedup_median=f["median_us"] / b["median_us"])


def trainers(**kw):
    return {side: StudentMlpTrainer(StudentMlpConfig(loss="kl", lr=1e-4, keep_prob=0.5, seed=0, dtype=side, **kw),
                                    device=DEV) for side in SIDES}


def run_step(n, reps, warmup):
    g = torch.Generator(device=DEV).manual_seed(n)
    x = torch.rand(n, 16, device=DEV, generator=g) * 2 - 1
    t = torch.cat([torch.randn(n, 2, device=DEV, generator=g) * 0.5,
                   torch.rand(n, 2, device=DEV, generator=g) * 0.2 - 3.4], 1).contiguous()
    sm = trainers()
    res = compare({side: (lambda s=sm[side]: s.step(x, t)) for side in SIDES}, reps, warmup)
    loss = {side: float(sm[side].metrics(1)[0, 0]) for side in SIDES}
    for s in sm.values():
        s.close()
    return dict(call="step", rows=n, last_loss=loss, **res)


def run_envs(n, K, reps, warmup, tr):
    sm = trainers()
    for s in sm.values():
        s.set_teacher(tr.teacher)
        s.attach_envs(n, seed=0, accum_steps=K)
    res = compare({side: sm[side].step_envs for side in SIDES}, reps, warmup)
    loss = {side: float(sm[side].metrics(1)[0, 0]) for side in SIDES}
    for s in sm.values():
        s.close()
    return dict(call="step_envs", n_envs=n, env_steps_per_opt_step=K, rows_per_opt_step=n * K, last_loss=loss, **res)


def fused_of(path):
    with open(path) as fh:
        return {(r["n_envs"], r["env_steps_per_opt_step"]): r["fused"] for r in json.load(fh)["results"]}


def against_parent(parent_path, here_path):
    """bench_student_mlp_envs.py's fused (f32) step_envs at this commit against the parent commit's
    quartiles widened by one IQR."""
    parent, here = fused_of(parent_path), fused_of(here_path)
    out = []
    for key in sorted(set(parent) & set(here)):
        p, h = parent[key], here[key]
        lo, hi = p["q1_us"] - p["iqr_us"], p["q3_us"] + p["iqr_us"]
        out.append(dict(n_envs=key[0], env_steps_per_opt_step=key[1], parent_fused=p, here_fused=h, window_us=[lo, hi],
                        here_median_within_window=lo <= h["median_us"] <= hi))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[200, 204800, 3276800])
    ap.add_argument("--envs", type=int, nargs="*", default=[4096, 65536])
    ap.add_argument("--accum-steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent", default=None, help="bench_student_mlp_envs.py's JSON at the parent commit")
    ap.add_argument("--here", default=None, help="bench_student_mlp_envs.py's JSON at this commit, same session")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "student_mlp_bf16_vs_f32.json"))
    a = ap.parse_args()
    if a.reps < 20 or bool(a.parent) != bool(a.here):
        ap.error("--reps >= 20; --parent and --here together")
    tr = DistillTrainer(DistillConfig(n_envs=64, seed=0), device=DEV)
    results = [run_step(n, a.reps, a.warmup) for n in a.rows]
    results += [run_envs(n, a.accum_steps, a.reps, a.warmup, tr) for n in a.envs]
    tr.close()
    res = dict(device=torch.cuda.get_device_name(0),
               method="device events around one call, f32 and bf16 alternating in one process; quartiles by "
                      "statistics.quantiles; kl, lr 1e-4, keep_prob 0.5",
               results=results)
    if a.parent:
        res["f32_against_parent"] = against_parent(a.parent, a.here)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
