"""The LSTM student's closed-loop query on its bf16 cell (StudentLstmConfig(dtype="bf16",
query_dtype="bf16"), rdl_set_query_dtype) against the f32 query of the same bf16 trainer, in one
process (kl, lr 1e-3, keep_prob 0.5, T = 10):

  * ``evaluate``: one 50-step episode of 64, 1,024 and 4,096 envs, ONE trainer whose setting is
    switched between the timed calls (set_query_dtype is host-only);
  * ``step_envs``: one optimiser step of 50 env steps per env at 4,096 envs (the act phase under either
    query, then the same bf16 training pass on 41 n windows and Adam), two trainers that differ in
    nothing but the setting;
  * ``train_envs``: lstm_train.train_envs(replay_capacity=8192, replay_windows=16384) at 4,096 envs,
    ms per optimiser step from the wall time of whole calls of two lengths, differenced.

The first two are timed with device events around one call, the two sides alternating for ``--reps``
repetitions (>= 20) after ``--warmup`` calls per side; median, quartiles, min and max per side, and
whether one side's interquartile range lies wholly below the other's.  No speed-up is asserted.
``--f32-evaluate N`` times nothing but the default (f32) query's evaluate at N envs through calls the
parent commit has too; its JSONs from the parent commit and from this one, same session, go in with
``--parent-f32 / --here-f32`` and are compared with the run-to-run spread.  Writes one JSON file
(default profiles/student_lstm_query_bf16_vs_f32.json) and prints it.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reacherdistilation_amd import lstm_train  # noqa: E402
from reacherdistilation_amd.distill import DistillConfig, DistillTrainer  # noqa: E402
from reacherdistilation_amd.student_lstm import StudentLstmConfig, StudentLstmTrainer  # noqa: E402

DEV = "cuda:0"
SIDES = ("f32", "bf16")   # the query's arithmetic; the trainer is bf16 on both sides
T = 10


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
    return dict(f32_query=f, bf16_query=b, bf16_iqr_below_f32=b["q3_us"] < f["q1_us"],
                f32_iqr_below_bf16=f["q3_us"] < b["q1_us"], speedup_median=f["median_us"] / b["median_us"])


def trainer(max_windows, **kw):
    return StudentLstmTrainer(StudentLstmConfig(loss="kl", lr=1e-3, keep_prob=0.5, seed=0, steps=T,
                                                max_windows=max_windows, dtype="bf16", **kw), device=DEV)


def run_evaluate(n, reps, warmup, tr):
    st = trainer(64)
    st.set_teacher(tr.teacher)

    def call(side):
        st.set_query_dtype(side)
        st.evaluate(n, 1, seed=0)
    res = compare({side: (lambda s=side: call(s)) for side in SIDES}, reps, warmup)
    ret = {}
    for side in SIDES:
        st.set_query_dtype(side)
        ret[side] = float(st.evaluate(n, 1, seed=0).returns.mean())
    st.close()
    return dict(call="evaluate", n_envs=n, episodes=1, mean_return=ret, **res)


def run_f32_evaluate(n, reps, warmup, tr):
    """The default query's evaluate alone, through calls the parent commit has too."""
    st = trainer(64)
    st.set_teacher(tr.teacher)
    for _ in range(max(warmup, 1)):
        st.evaluate(n, 1, seed=0)
    torch.cuda.synchronize()
    us = [timed(lambda: st.evaluate(n, 1, seed=0)) for _ in range(2 * reps)]
    st.close()
    return dict(call="evaluate", query="f32 (default)", n_envs=n, episodes=1, **stats(us))


def run_step_envs(n, reps, warmup, tr):
    B = n * (51 - T)
    st = {side: trainer(B, query_dtype=side) for side in SIDES}
    for s in st.values():
        s.set_teacher(tr.teacher)
        s.attach_envs(n, seed=0, accum_steps=50)
    res = compare({side: st[side].step_envs for side in SIDES}, reps, warmup)
    loss = {side: float(st[side].metrics(1)[0, 0]) for side in SIDES}
    for s in st.values():
        s.close()
    return dict(call="step_envs", n_envs=n, env_steps_per_opt_step=50, windows_per_opt_step=B, last_loss=loss, **res)


def run_train_envs(n, capacity, windows, lengths, rounds):
    """ms per optimiser step of lstm_train.train_envs with a replay ring (scripts/bench_replay.py's method):
    wall time of two whole calls, differenced; the two sides alternating, after one untimed call each."""
    def wall(side, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st, _ = lstm_train.train_envs(n, steps, dtype="bf16", query_dtype=side, device=DEV, replay_capacity=capacity,
                                      replay_windows=windows)   # ends in a metrics read
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st.close()
        return dt

    a, b = lengths
    for side in SIDES:
        wall(side, a)   # code objects, allocator
    ms = {side: [] for side in SIDES}
    for _ in range(rounds):
        for side in SIDES:
            ta, tb = wall(side, a), wall(side, b)
            ms[side].append(1e3 * (tb - ta) / (b - a))
    out = {f"{side}_query": dict(ms_per_opt_step=statistics.median(ms[side]), each_round=ms[side], min_ms=min(ms[side]),
                                 max_ms=max(ms[side])) for side in SIDES}
    f, q = out["f32_query"], out["bf16_query"]
    return dict(call="train_envs", n_envs=n, replay_capacity=capacity, replay_windows=windows, lengths=list(lengths),
                rounds=rounds, bf16_range_below_f32=q["max_ms"] < f["min_ms"], f32_range_below_bf16=f["max_ms"] < q["min_ms"],
                speedup_median=f["ms_per_opt_step"] / q["ms_per_opt_step"], **out)


def against_parent(parent, here):
    """This commit's f32 evaluate against the parent's: its median inside the parent's quartiles widened by
    one IQR is agreement within the run-to-run spread."""
    p, h = json.load(open(parent))["result"], json.load(open(here))["result"]
    lo, hi = p["q1_us"] - p["iqr_us"], p["q3_us"] + p["iqr_us"]
    return dict(parent=p, here=h, window_us=[lo, hi], here_median_within_window=lo <= h["median_us"] <= hi,
                here_over_parent_median=h["median_us"] / p["median_us"])


def verdict(results):
    """Where the bf16 query wins by more than the spread, and where it does not."""
    wins, keep = [], []
    for r in results:
        name = f"{r['call']} at {r['n_envs']} envs"
        won = r.get("bf16_iqr_below_f32", r.get("bf16_range_below_f32"))
        (wins if won else keep).append(f"{name} ({r['speedup_median']:.2f}x)")
    return dict(bf16_query_faster_beyond_the_spread=wins, keep_f32_there=keep)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 1024, 4096])
    ap.add_argument("--envs", type=int, default=4096, help="step_envs and train_envs; 0: neither")
    ap.add_argument("--replay", type=int, nargs=2, default=[8192, 16384], help="replay_capacity replay_windows")
    ap.add_argument("--lengths", type=int, nargs=2, default=[10, 40], help="train_envs optimiser steps, two lengths")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--f32-evaluate", type=int, default=0, help="only the default query's evaluate at this many envs")
    ap.add_argument("--parent-f32", default=None, help="--f32-evaluate's JSON at the parent commit")
    ap.add_argument("--here-f32", default=None, help="--f32-evaluate's JSON at this commit, same session")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "student_lstm_query_bf16_vs_f32.json"))
    a = ap.parse_args()
    if a.reps < 20 or bool(a.parent_f32) != bool(a.here_f32):
        ap.error("--reps >= 20; --parent-f32 and --here-f32 together")
    tr = DistillTrainer(DistillConfig(n_envs=64, seed=0), device=DEV)
    res = dict(device=torch.cuda.get_device_name(0))
    if a.f32_evaluate:
        res.update(method="device events around one evaluate call of one 50-step episode; bf16 trainer, default query",
                   result=run_f32_evaluate(a.f32_evaluate, a.reps, a.warmup, tr))
    else:
        results = [run_evaluate(n, a.reps, a.warmup, tr) for n in a.sizes]
        if a.envs:
            results.append(run_step_envs(a.envs, a.reps, a.warmup, tr))
            results.append(run_train_envs(a.envs, a.replay[0], a.replay[1], tuple(a.lengths), a.rounds))
        res.update(method="bf16 trainers (kl, lr 1e-3, keep_prob 0.5, T = 10), the query's arithmetic f32 or bf16; evaluate "
                          "and step_envs: device events around one call, the two sides alternating in one process, "
                          "quartiles by statistics.quantiles; train_envs: wall time of whole calls of two lengths, "
                          "differenced, sides alternating",
                   results=results, verdict=verdict(results))
        if a.parent_f32:
            res["f32_evaluate_against_parent"] = against_parent(a.parent_f32, a.here_f32)
    tr.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
