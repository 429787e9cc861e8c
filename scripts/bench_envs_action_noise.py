"""What the action noise costs in the students' persistent-env optimiser step (step_envs), against the
parent commit in the same run, and one quality reading of DART's noisy expert.

Timing.  Cases: the MLP student at 4,096 envs, K = 50, f32 and bf16; the LSTM student at 4,096 envs
(K = 50, T = 10: 167,936 windows per step).  Variants:

  off  no noise set, nothing bound: the launch the library made before the noise (in this checkout
       measured after a set back to "none": the same launch);
  on   set_action_noise("policy", 1.0): the noisy instances.

The driver (no GPU work of its own) runs ``--rounds`` rounds, each of three child processes in turn:
one on the parent checkout (``--parent DIR``: a tree of the parent commit with its library built;
variant off, which uses nothing but step_envs), one on this checkout that likewise never touches the
noise (off: the default), and one on this checkout with off and on, one step of each in turn per
repetition -- parent, here, here, parent, here, here, ...  Each step is timed with device events.  Reported per
case and variant: median, quartiles and interquartile range over the pooled repetitions of all
rounds, the per-round medians, and the medians' ratios.  No difference is asserted.

Quality (``--quality-steps`` > 0).  mlp_train.train_envs at 64 envs, K = 50, the same number of
optimiser steps -- so the same env-step budget -- under (a) the teacher acting, no noise (behaviour
cloning on the expert's own states), (b) the teacher acting under FIXED noise at a few sigma (DART),
(c) DAgger's beta schedule beta = 0.5 x 0.99^k, (d) the student acting (the hard switch, for scale);
recorded: the noiseless evaluate() mean return over 4,096 fresh envs, one episode.  Nothing is asserted
beyond finiteness.

Writes one JSON file (default profiles/envs_action_noise.json) and prints it.
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


def stats(us):
    q = statistics.quantiles(us, n=4)
    return dict(median_us=statistics.median(us), q1_us=q[0], q3_us=q[2], iqr_us=q[2] - q[0], min_us=min(us),
                max_us=max(us), reps=len(us))


# ------------------------------------------------------------------ a child: one checkout, one process
def child(a):
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from reacherdistilation_amd.distill import DistillConfig, DistillTrainer
    from reacherdistilation_amd.student_lstm import StudentLstmConfig, StudentLstmTrainer
    from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer
    variants = a.variants.split(",")

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e3   # us

    def run(trainer, info):
        def select(v):
            if variants != ["off"]:   # a checkout from before the noise has nothing to select
                trainer.set_action_noise("policy" if v == "on" else "none", 1.0)

        for _ in range(max(a.warmup, 1)):
            for v in variants:
                select(v)
                trainer.step_envs()
        torch.cuda.synchronize()
        us = {v: [] for v in variants}
        for _ in range(a.reps):   # one step of each variant in turn, so that all see the same machine
            for v in variants:
                select(v)
                us[v].append(timed(trainer.step_envs))
        trainer.close()
        return dict(info, us=us)

    tr = DistillTrainer(DistillConfig(n_envs=64, seed=0), device=DEV)
    out = []
    n = a.envs
    for dtype in ("f32", "bf16"):
        sm = StudentMlpTrainer(StudentMlpConfig(loss="kl", lr=1e-4, keep_prob=0.5, seed=0, dtype=dtype), device=DEV)
        sm.set_teacher(tr.teacher)
        sm.attach_envs(n, seed=0, accum_steps=K)
        out.append(run(sm, dict(student="mlp", n_envs=n, dtype=dtype, env_steps_per_opt_step=K)))
    B = n * (51 - T)
    st = StudentLstmTrainer(StudentLstmConfig(loss="kl", lr=1e-4, keep_prob=0.5, seed=0, steps=T, max_windows=B), device=DEV)
    st.set_teacher(tr.teacher)
    st.attach_envs(n, seed=0, accum_steps=K)
    out.append(run(st, dict(student="lstm", n_envs=n, dtype="f32", env_steps_per_opt_step=K, windows_per_opt_step=B)))
    tr.close()
    with open(a.out, "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=out), fh)


def quality(a):
    sys.path.insert(0, HERE_ROOT)
    import torch
    from reacherdistilation_amd import mlp_train
    S, n = a.quality_steps, 64
    runs = [("a: teacher acts, no noise", dict(warmup_steps=S)),
            *[(f"b: teacher acts, fixed noise sigma = {s}", dict(warmup_steps=S, noise="fixed", noise_scale=s))
              for s in (0.1, 0.3, 0.6)],
            ("c: beta = 0.5 x 0.99^k", dict(beta0=0.5, beta_decay=0.99)),
            ("d: student acts", dict())]
    out = []
    for name, kw in runs:
        sm, hist = mlp_train.train_envs(n, S, lr=1e-3, accum_steps=K, seed=0, device=DEV, **kw)
        ret = float(sm.evaluate(4096, 1, seed=1).returns.mean())
        assert math.isfinite(ret) and all(math.isfinite(h[1]) for h in hist)
        out.append(dict(run=name, settings=kw, eval_mean_return=ret, last_loss=hist[-1][1], last_action_mse=hist[-1][2]))
        sm.close()
    from reacherdistilation_amd.distill import DistillConfig
    from reacherdistilation_amd.policy import synthetic_teacher
    from reacherdistilation_amd.student_mlp import StudentMlpTrainer
    fresh = StudentMlpTrainer(device=DEV)   # the same glorot initialisation, untrained
    fresh.set_teacher(synthetic_teacher(DistillConfig().teacher_seed))
    untrained = float(fresh.evaluate(4096, 1, seed=1).returns.mean())
    fresh.close()
    with open(a.out, "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), n_envs=n, opt_steps=S, env_steps=S * K * n, lr=1e-3,
                       student="mlp f32, glorot init seed 2", teacher="the default synthetic teacher",
                       evaluation="StudentMlpTrainer.evaluate(4096, 1, seed=1), noiseless, mean return",
                       untrained_eval_mean_return=untrained, runs=out), fh)


# ------------------------------------------------------------------ the driver
def spawn(mode, root, out, extra):
    cmd = [sys.executable, os.path.abspath(__file__), mode, "--root", root, "--out", out, *extra]
    subprocess.run(cmd, check=True, cwd=root)
    with open(out) as fh:
        return json.load(fh)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="driver", choices=["driver", "child", "quality"])
    ap.add_argument("--parent", help="a tree of the parent commit with its library built")
    ap.add_argument("--root", default=HERE_ROOT)
    ap.add_argument("--variants", default="off,on")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quality-steps", type=int, default=400)
    ap.add_argument("--tmp", default=os.path.join(HERE_ROOT, "bench_out"))
    ap.add_argument("--out", default=os.path.join(HERE_ROOT, "profiles", "envs_action_noise.json"))
    a = ap.parse_args()
    if a.mode == "child":
        child(a)
        sys.exit(0)
    if a.mode == "quality":
        quality(a)
        sys.exit(0)
    if not a.parent:
        ap.error("--parent DIR: the parent commit's tree with its library built")
    os.makedirs(a.tmp, exist_ok=True)
    common = ["--envs", str(a.envs), "--reps", str(a.reps), "--warmup", str(a.warmup)]
    pooled, rounds, device = {}, [], None
    for r in range(a.rounds):   # parent, here (default), here (off and on in turn), parent, ...
        for label, root, variants in (("parent", os.path.abspath(a.parent), "off"), ("here_default", HERE_ROOT, "off"),
                                      ("here", HERE_ROOT, "off,on")):
            got = spawn("child", root, os.path.join(a.tmp, f"noise_{label}_{r}.json"), common + ["--variants", variants])
            device = got["device"]
            for case in got["results"]:
                key = (case["student"], case["n_envs"], case["dtype"])
                for v, us in case["us"].items():
                    pooled.setdefault(key, {}).setdefault(f"{label}_{v}", []).extend(us)
                    rounds.append(dict(round=r, checkout=label, variant=v, student=key[0], n_envs=key[1], dtype=key[2],
                                       median_us=statistics.median(us)))
    results = []
    for (student, n, dtype), by in pooled.items():
        row = dict(student=student, n_envs=n, dtype=dtype, env_steps_per_opt_step=K,
                   variants={v: stats(us) for v, us in by.items()})
        med = {v: s["median_us"] for v, s in row["variants"].items()}
        row["median_here_default_off_over_parent_off"] = med["here_default_off"] / med["parent_off"]
        row["median_here_off_over_parent_off"] = med["here_off"] / med["parent_off"]
        row["median_here_on_over_here_off"] = med["here_on"] / med["here_off"]
        row["median_here_on_over_parent_off"] = med["here_on"] / med["parent_off"]
        results.append(row)
    res = dict(device=device,
               method="device events around one step_envs call (K env steps per env in one launch, the training pass, "
                      "Adam); per round one process on the parent commit's checkout (off), one on this checkout that "
                      "never touches the noise (off), one on this checkout (off, on: one step of each in turn per "
                      "repetition); repetitions pooled over the rounds; "
                      "quartiles by statistics.quantiles",
               variants=dict(parent_off="the parent commit, step_envs as it was",
                             here_default_off="this checkout, step_envs alone: the noise never set",
                             here_off="this checkout, noise \"none\" (set back from \"policy\"), nothing bound",
                             here_on="this checkout, set_action_noise(\"policy\", 1.0)"),
               rounds=a.rounds, reps_per_round=a.reps, results=results, per_round_medians=rounds)
    if a.quality_steps > 0:
        res["quality"] = spawn("quality", HERE_ROOT, os.path.join(a.tmp, "noise_quality.json"),
                               ["--quality-steps", str(a.quality_steps)])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
