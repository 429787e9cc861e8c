"""What the sensor faults cost in the students' persistent-env optimiser step (step_envs) and in the
fused evaluation, against the parent commit in the same run, and the experiment the faults are for.

Timing.  Cases: the MLP student at 4,096 envs, K = 50, f32 and bf16; the LSTM student at 4,096 envs
(K = 50, T = 10: 167,936 windows per step); and, on this checkout only, the MLP student (f32) at
65,536 envs.  Variants:

  off  no faults set: the launch the library made before the faults (in this checkout measured after a
       set back to "none": the same launch);
  on   set_obs_faults("missing", 0.5): the faulty instances (no noise, beta = 0).

The driver (no GPU work of its own) runs ``--rounds`` rounds, each of three child processes in turn:
one on the parent checkout (``--parent DIR``: a tree of the parent commit with its library built;
variant off, which uses nothing but step_envs -- or ``--parent-variants off,on`` for a parent that has the
faults already, which it then runs as this checkout's third process does), one on this checkout that likewise never touches the
faults (off: the default), and one on this checkout with off and on, one step of each in turn per
repetition -- parent, here, here, parent, here, here, ...  Each step is timed with device events.
Reported per case and variant: median, quartiles and interquartile range over the pooled repetitions of
all rounds, the per-round medians, and the medians' ratios.  No difference is asserted.

Evaluate.  StudentMlpTrainer.evaluate(4096, 1) plain and with faults=("missing", 0.5), one of each in
turn per repetition, device events.

Experiment (``--train-steps`` > 0).  mlp_train.train_envs at 4,096 envs, K = 50, the same number of
optimiser steps at training keep_prob 1.0 and 0.5 (clean acting); then each student's evaluate() mean
return over 4,096 fresh envs, one episode, under "missing" at keep_prob 1, 0.9 and 0.5.  A record, not a
threshold: nothing is asserted beyond finiteness.

Writes one JSON file (default profiles/envs_obs_faults.json) and prints it.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
K, T = 50, 10
FAULTS = ("missing", 0.5)


def stats(us):
    q = statistics.quantiles(us, n=4)
    return dict(median_us=statistics.median(us), q1_us=q[0], q3_us=q[2], iqr_us=q[2] - q[0], min_us=min(us),
                max_us=max(us), reps=len(us))


def timed(torch, fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3   # us


# ------------------------------------------------------------------ a child: one checkout, one process
def child(a):
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from reacherdistilation_amd.distill import DistillConfig, DistillTrainer
    from reacherdistilation_amd.student_lstm import StudentLstmConfig, StudentLstmTrainer
    from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer
    variants = a.variants.split(",")
    here = variants != ["off"]   # a checkout from before the faults has nothing to select
    own = os.path.abspath(a.root) == HERE_ROOT   # the cases beyond the comparison run on this checkout only

    def run(trainer, info):
        def select(v):
            if here:
                trainer.set_obs_faults(*(FAULTS if v == "on" else ("none", 1.0)))

        for _ in range(max(a.warmup, 1)):
            for v in variants:
                select(v)
                trainer.step_envs()
        torch.cuda.synchronize()
        us = {v: [] for v in variants}
        for _ in range(a.reps):   # one step of each variant in turn, so that all see the same machine
            for v in variants:
                select(v)
                us[v].append(timed(torch, trainer.step_envs))
        trainer.close()
        return dict(info, us=us)

    def mlp(n, dtype):
        sm = StudentMlpTrainer(StudentMlpConfig(loss="kl", lr=1e-4, keep_prob=0.5, seed=0, dtype=dtype), device=DEV)
        sm.set_teacher(tr.teacher)
        sm.attach_envs(n, seed=0, accum_steps=K)
        return run(sm, dict(student="mlp", n_envs=n, dtype=dtype, env_steps_per_opt_step=K))

    tr = DistillTrainer(DistillConfig(n_envs=64, seed=0), device=DEV)
    n = a.envs
    out = [mlp(n, "f32"), mlp(n, "bf16")]
    B = n * (51 - T)
    st = StudentLstmTrainer(StudentLstmConfig(loss="kl", lr=1e-4, keep_prob=0.5, seed=0, steps=T, max_windows=B), device=DEV)
    st.set_teacher(tr.teacher)
    st.attach_envs(n, seed=0, accum_steps=K)
    out.append(run(st, dict(student="lstm", n_envs=n, dtype="f32", env_steps_per_opt_step=K, windows_per_opt_step=B)))
    res = dict(device=torch.cuda.get_device_name(0), results=out)
    if here and own:
        out.append(mlp(a.big_envs, "f32"))
        sm = StudentMlpTrainer(device=DEV)
        sm.set_teacher(tr.teacher)
        ev = {"plain": [], "faulty": []}
        for rep in range(a.warmup + a.reps):
            for v, kw in (("plain", {}), ("faulty", dict(faults=FAULTS))):
                us = timed(torch, lambda: sm.evaluate(n, 1, seed=1, **kw))
                if rep >= a.warmup:
                    ev[v].append(us)
        sm.close()
        res["evaluate"] = dict(student="mlp", n_envs=n, dtype="f32", episodes=1, us=ev)
    tr.close()
    with open(a.out, "w") as fh:
        json.dump(res, fh)


def experiment(a):
    sys.path.insert(0, HERE_ROOT)
    import torch
    from reacherdistilation_amd import mlp_train
    S, n = a.train_steps, a.envs
    out = []
    for keep_prob in (1.0, 0.5):
        sm, hist = mlp_train.train_envs(n, S, keep_prob=keep_prob, lr=1e-3, accum_steps=K, seed=0, device=DEV)
        row = dict(train_keep_prob=keep_prob, last_loss=hist[-1][1], last_action_mse=hist[-1][2],
                   clean_eval_mean_return=float(sm.evaluate(4096, 1, seed=1).returns.mean()), missing={})
        for kp in (1.0, 0.9, 0.5):
            row["missing"][str(kp)] = float(sm.evaluate(4096, 1, seed=1, faults=("missing", kp)).returns.mean())
        assert all(math.isfinite(v) for v in row["missing"].values()) and math.isfinite(row["last_loss"])
        out.append(row)
        sm.close()
    with open(a.out, "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), n_envs=n, opt_steps=S, env_steps=S * K * n, lr=1e-3,
                       student="mlp f32, glorot init seed 2, the student acting on clean sensors while it trains",
                       teacher="the default synthetic teacher",
                       evaluation="StudentMlpTrainer.evaluate(4096, 1, seed=1, faults=(\"missing\", keep_prob)), mean return",
                       runs=out), fh)


# ------------------------------------------------------------------ the driver
def spawn(mode, root, out, extra):
    cmd = [sys.executable, os.path.abspath(__file__), mode, "--root", root, "--out", out, *extra]
    subprocess.run(cmd, check=True, cwd=root)
    with open(out) as fh:
        return json.load(fh)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="driver", choices=["driver", "child", "experiment"])
    ap.add_argument("--parent", help="a tree of the parent commit with its library built")
    ap.add_argument("--parent-variants", default="off", help="off,on: the parent has the faults too")
    ap.add_argument("--root", default=HERE_ROOT)
    ap.add_argument("--variants", default="off,on")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--big-envs", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=400)
    ap.add_argument("--tmp", default=os.path.join(HERE_ROOT, "bench_out"))
    ap.add_argument("--out", default=os.path.join(HERE_ROOT, "profiles", "envs_obs_faults.json"))
    a = ap.parse_args()
    if a.mode == "child":
        child(a)
        sys.exit(0)
    if a.mode == "experiment":
        experiment(a)
        sys.exit(0)
    if not a.parent:
        ap.error("--parent DIR: the parent commit's tree with its library built")
    a.tmp = os.path.abspath(a.tmp)   # the children run in their checkout's directory
    os.makedirs(a.tmp, exist_ok=True)
    common =["--envs", str(a.envs), "--big-envs", str(a.big_envs), "--reps", str(a.reps), "--warmup", str(a.warmup)]
    pooled, rounds, device, ev = {}, [], None, {"plain": [], "faulty": []}
    for r in range(a.rounds):   # parent, here (default), here (off and on in turn), parent, ...
        for label, root, variants in (("parent", os.path.abspath(a.parent), a.parent_variants), ("here_default", HERE_ROOT, "off"),
                                      ("here", HERE_ROOT, "off,on")):
            got = spawn("child", root, os.path.join(a.tmp, f"faults_{label}_{r}.json"), common + ["--variants", variants])
            device = got["device"]
            for case in got["results"]:
                key = (case["student"], case["n_envs"], case["dtype"])
                for v, us in case["us"].items():
                    pooled.setdefault(key, {}).setdefault(f"{label}_{v}", []).extend(us)
                    rounds.append(dict(round=r, checkout=label, variant=v, student=key[0], n_envs=key[1], dtype=key[2],
                                       median_us=statistics.median(us)))
            for v, us in got.get("evaluate", {}).get("us", {}).items():
                ev[v].extend(us)
    results = []
    for (student, n, dtype), by in pooled.items():
        row = dict(student=student, n_envs=n, dtype=dtype, env_steps_per_opt_step=K,
                   variants={v: stats(us) for v, us in by.items()})
        med = {v: s["median_us"] for v, s in row["variants"].items()}
        if "parent_off" in med:
            row["median_here_default_off_over_parent_off"] = med["here_default_off"] / med["parent_off"]
            row["median_here_off_over_parent_off"] = med["here_off"] / med["parent_off"]
        if "parent_on" in med:
            row["median_here_on_over_parent_on"] = med["here_on"] / med["parent_on"]
        row["median_here_on_over_here_off"] = med["here_on"] / med["here_off"]
        results.append(row)
    res = dict(device=device,
               method="device events around one step_envs call (K env steps per env in one launch, the training pass, "
                      "Adam); per round one process on the parent commit's checkout (off), one on this checkout that "
                      "never touches the faults (off), one on this checkout (off, on: one step of each in turn per "
                      "repetition); repetitions pooled over the rounds; quartiles by statistics.quantiles",
               variants=dict(parent_off="the parent commit, step_envs as it was",
                             parent_on="the parent commit under --parent-variants off,on: as here_on",
                             here_default_off="this checkout, step_envs alone: the faults never set",
                             here_off="this checkout, faults \"none\" (set back from \"missing\")",
                             here_on="this checkout, set_obs_faults(\"missing\", 0.5), no noise, beta = 0"),
               rounds=a.rounds, reps_per_round=a.reps, results=results, per_round_medians=rounds)
    if ev["plain"]:
        e = dict(student="mlp", n_envs=a.envs, dtype="f32", episodes=1,
                 variants=dict(plain=stats(ev["plain"]), faulty=stats(ev["faulty"])))
        e["median_faulty_over_plain"] = e["variants"]["faulty"]["median_us"] / e["variants"]["plain"]["median_us"]
        res["evaluate"] = e
    if a.train_steps > 0:
        res["experiment"] = spawn("experiment", HERE_ROOT, os.path.join(a.tmp, "faults_experiment.json"),
                                  ["--train-steps", str(a.train_steps), "--envs", str(a.envs)])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
