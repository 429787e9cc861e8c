"""Prioritised replay draws (include/reacher_replay_priority.h) measured on the GPU, five parts, one JSON
file (default profiles/replay_prioritized.json), also printed.  A and B alternate inside one run; every
figure is a median with its quartiles (statistics.quantiles).  Nothing is asserted anywhere.

(a) ``sample_rows`` and ``sample_windows`` (T = 10), uniform against ``prioritized=True``, at B in
    {1,024, 16,384, 163,840} from a full ring of 8,192 episodes with random priorities: a host clock
    from before the call to after a device synchronise, and device events around 20 calls back to back
    in a stream that is never waited on.
(b) The uniform calls of this library against those of another build of the library (``--parent-lib``:
    the parent commit's libreacher.so), both through the same bare ctypes calls on rings of their own,
    alternating; "A/A" times this library against itself the same way, which is the run's own spread.
(c) ``update_priorities`` (rows and T = 10 windows) at the same sizes, and a push of 4,096 episodes
    into a ring without priorities, with init="const" and with init="record".
(d) ms per optimiser step of both ``train_envs`` at 4,096 envs (the LSTM in bf16) with
    replay_capacity = 8,192 and replay_windows = 16,384: replay_priority "none", "record", "refresh";
    whole driver calls of two lengths, differenced (scripts/bench_replay.py's method).
(e) For the same three settings and one seed: the evaluation return every ``--eval-every`` optimiser
    steps and the training batches' action-MSE (which under prioritised draws is the error on the
    records the draw prefers, NOT on the uniform aggregate).  On record; whether prioritising helps on
    this task is an open question and the file says what was seen.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reacherdistilation_amd import _native as nat  # noqa: E402
from reacherdistilation_amd import lstm_train, mlp_train  # noqa: E402
from reacherdistilation_amd.replay import RdReplayConfig, RdReplaySample, ReplayRing  # noqa: E402

DEV = "cuda:0"
T = 10


def stats(us):
    q = statistics.quantiles(us, n=4)
    return dict(median_us=statistics.median(us), q1_us=q[0], q3_us=q[2], min_us=min(us), max_us=max(us), reps=len(us))


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def in_stream(fn, calls=20):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def alternate(fns, reps):
    """{name: (call-to-sync stats, in-stream stats)} with the sides alternating inside every repetition"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    sync, dev = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            sync[k].append(host_timed(fn))
    for _ in range(max(5, reps // 4)):
        for k, fn in fns.items():
            dev[k].append(in_stream(fn))
    return {k: dict(call_to_sync=stats(sync[k]), in_stream=stats(dev[k])) for k in fns}


def filled_ring(episodes, B, priorities):
    ring = ReplayRing(episodes, device=DEV, seed=0, max_batch=B)
    if priorities:
        ring.enable_priorities(init="record")
    g = torch.Generator().manual_seed(1)
    for lo in range(0, episodes, 1024):
        ring.push_episodes(torch.randn(min(1024, episodes - lo), 50, 21, generator=g).to(DEV))
    return ring


def part_a(B, episodes, reps):
    ring = filled_ring(episodes, B, True)
    out = dict(B=B, ring_episodes=episodes, table_bytes=episodes * 50 * 4)
    out["sample_rows"] = alternate({"uniform": lambda: ring.sample_rows(B),
                                    "prioritized": lambda: ring.sample_rows(B, prioritized=True)}, reps)
    out["sample_windows"] = alternate({"uniform": lambda: ring.sample_windows(T, B),
                                       "prioritized": lambda: ring.sample_windows(T, B, prioritized=True)}, reps)
    for k in ("sample_rows", "sample_windows"):
        for clock in ("call_to_sync", "in_stream"):
            out[k][f"extra_us_median_{clock}"] = (out[k]["prioritized"][clock]["median_us"] -
                                                  out[k]["uniform"][clock]["median_us"])
    ring.close()
    return out


class BareRing:
    """the uniform calls of one libreacher.so through bare ctypes (no ReplayRing): what part (b) times"""

    def __init__(self, lib, episodes, B):
        P, I64 = ctypes.c_void_p, ctypes.c_int64
        lib.rd_replay_create.argtypes = [ctypes.POINTER(P), ctypes.POINTER(RdReplayConfig), P, ctypes.c_int, P]
        lib.rd_replay_push_episodes.argtypes = [P, P, I64]
        lib.rd_replay_sample_windows.argtypes = [P, ctypes.POINTER(RdReplaySample), P, P, P, P, P]
        lib.rd_replay_sample_rows.argtypes = [P, ctypes.POINTER(RdReplaySample), P, P, P]
        lib.rd_replay_destroy.argtypes = [P]
        self.lib, self.B, self.h = lib, B, P()
        self.records = torch.zeros(episodes, 50, 21, device=DEV)
        c = RdReplayConfig(capacity=episodes, max_batch=B)
        stream = nat.stream_handle(torch.device(DEV))
        assert lib.rd_replay_create(ctypes.byref(self.h), ctypes.byref(c), nat.ptr(self.records), 0, stream) == 0
        g = torch.Generator().manual_seed(1)
        for lo in range(0, episodes, 1024):
            rec = torch.randn(min(1024, episodes - lo), 50, 21, generator=g).to(DEV)
            assert lib.rd_replay_push_episodes(self.h, nat.ptr(rec), rec.shape[0]) == 0
        torch.cuda.synchronize()
        kw = dict(dtype=torch.float32, device=DEV)
        self.w = [torch.zeros(T, B, 11, **kw), torch.zeros(T, B, 4, **kw), torch.zeros(T, B, 4, **kw), torch.zeros(T, B, 1, **kw)]
        self.r = [torch.zeros(B, 16, **kw), torch.zeros(B, 4, **kw)]
        self.s = RdReplaySample(steps=T, start_mode=0, windows=B, window_base=0, recent=0, seed=0)

    def windows(self):
        assert self.lib.rd_replay_sample_windows(self.h, ctypes.byref(self.s), *(nat.ptr(v) for v in self.w), None) == 0

    def rows(self):
        assert self.lib.rd_replay_sample_rows(self.h, ctypes.byref(self.s), *(nat.ptr(v) for v in self.r), None) == 0

    def close(self):
        self.lib.rd_replay_destroy(self.h)


def part_b(B, episodes, reps, parent_path):
    here = nat.load()
    rings = {"this": BareRing(here, episodes, B), "this_again": BareRing(here, episodes, B)}
    if parent_path:
        rings["parent"] = BareRing(ctypes.CDLL(parent_path), episodes, B)
    out = dict(B=B, ring_episodes=episodes)
    out["sample_rows"] = alternate({k: r.rows for k, r in rings.items()}, reps)
    out["sample_windows"] = alternate({k: r.windows for k, r in rings.items()}, reps)
    assert torch.equal(rings["this"].w[0], rings["this_again"].w[0])
    if parent_path:   # same draw counter on every ring: the same batch, bitwise
        out["same_batch_as_parent"] = all(torch.equal(a, b) for a, b in zip(rings["this"].w + rings["this"].r,
                                                                            rings["parent"].w + rings["parent"].r))
    for r in rings.values():
        r.close()
    return out


def part_c(B, episodes, reps):
    ring = filled_ring(episodes, B, True)
    _, _, idx_r = ring.sample_rows(B, with_idx=True, prioritized=True)
    idx_r = idx_r.clone()
    *_, idx_w = ring.sample_windows(T, B, with_idx=True, prioritized=True)
    idx_w = idx_w.clone()
    s_r, s_w = torch.randn(B, 4, device=DEV), torch.randn(T, B, 4, device=DEV)
    out = dict(B=B, ring_episodes=episodes)
    out["update_priorities"] = alternate({"rows": lambda: ring.update_priorities(idx_r, s_r),
                                          "windows_T10": lambda: ring.update_priorities(idx_w, s_w)}, reps)
    ring.close()
    return out


def part_c_push(episodes, pushed, reps):
    eps = torch.randn(pushed, 50, 21, device=DEV)
    rings = {"no_priorities": ReplayRing(episodes, device=DEV, max_batch=64)}
    for init in ("const", "record"):
        rings[f"init_{init}"] = ReplayRing(episodes, device=DEV, max_batch=64)
        rings[f"init_{init}"].enable_priorities(init=init)
    out = dict(ring_episodes=episodes, pushed_episodes=pushed, copy_bytes=2 * pushed * 50 * 21 * 4)
    out["push_episodes"] = alternate({k: (lambda r=r: r.push_episodes(eps)) for k, r in rings.items()}, reps)
    for r in rings.values():
        r.close()
    return out


MODES = ("none", "record", "refresh")


def driver_kw(mod):
    return dict(dtype="bf16") if mod is lstm_train else {}


def part_d(n, windows, capacity, lengths, rounds=3):
    def wall(mod, mode, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr, _ = mod.train_envs(n, steps, replay_capacity=capacity, replay_windows=windows, replay_priority=mode,
                               device=DEV, **driver_kw(mod))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        tr.close()
        return dt

    a, b = lengths
    out = dict(n_envs=n, replay_capacity=capacity, replay_windows=windows, lengths=list(lengths), lstm_dtype="bf16")
    for name, mod in (("mlp", mlp_train), ("lstm", lstm_train)):
        for mode in MODES:
            wall(mod, mode, a)   # code objects, allocator
        ms = {mode: [] for mode in MODES}
        for _ in range(rounds):  # the three modes alternate inside every round
            for mode in MODES:
                ta, tb = wall(mod, mode, a), wall(mod, mode, b)
                ms[mode].append(1e3 * (tb - ta) / (b - a))
        out[name] = {mode: dict(ms_per_opt_step=statistics.median(v), each_round=v) for mode, v in ms.items()}
    return out


def part_e(n, windows, capacity, steps, eval_every, seed):
    out = dict(n_envs=n, replay_capacity=capacity, replay_windows=windows, opt_steps=steps, eval_every=eval_every,
               seed=seed, eval="mean return of 4,096 fresh envs, one noiseless episode, seed + 1", lstm_dtype="bf16",
               note="batch_action_mse is the error on the DRAWN batch: under prioritised draws that is the records "
                    "the draw prefers, not the uniform aggregate; the evaluation return is the comparable figure")
    for name, mod in (("mlp", mlp_train), ("lstm", lstm_train)):
        out[name] = {}
        for mode in MODES:
            tr, hist, evals = mod.train_envs(n, steps, replay_capacity=capacity, replay_windows=windows,
                                             replay_priority=mode, eval_every=eval_every, seed=seed, device=DEV,
                                             **driver_kw(mod))
            mse = [h[2] for h in hist]
            out[name][mode] = dict(eval_return=[[k, r] for k, r in evals],
                                   batch_action_mse=[[k, statistics.fmean(mse[k - eval_every:k])]
                                                     for k in range(eval_every, steps + 1, eval_every)])
            tr.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 16384, 163840])
    ap.add_argument("--episodes", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=16384)
    ap.add_argument("--lengths", type=int, nargs=2, default=[10, 50])
    ap.add_argument("--opt-steps", type=int, default=400)
    ap.add_argument("--eval-every", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--parent-lib", default="", help="another build's libreacher.so for part (b)")
    ap.add_argument("--parts", default="abcde")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_prioritized.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_replay_prio.py measures on a HIP device; none found")
    res = dict(device=torch.cuda.get_device_name(0),
               method="alternating sides in one run; host clock from call to device synchronise and device events "
                      "around 20 back-to-back calls; drivers: wall time of whole train_envs calls, two lengths "
                      "differenced; quartiles by statistics.quantiles")

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")

    if "a" in a.parts:
        res["a_uniform_vs_prioritized"] = [part_a(B, a.episodes, a.reps) for B in a.batches]
        save()
    if "b" in a.parts:
        res["b_uniform_this_vs_parent"] = dict(parent_lib=bool(a.parent_lib),
                                               sizes=[part_b(B, a.episodes, a.reps, a.parent_lib) for B in a.batches])
        save()
    if "c" in a.parts:
        res["c_updates"] = [part_c(B, a.episodes, a.reps) for B in a.batches]
        res["c_push"] = part_c_push(a.episodes, a.envs, a.reps)
        save()
    if "d" in a.parts:
        res["d_train_envs_ms_per_opt_step"] = part_d(a.envs, a.windows, 2 * a.envs, tuple(a.lengths))
        save()
    if "e" in a.parts:
        res["e_convergence"] = part_e(a.envs, a.windows, 2 * a.envs, a.opt_steps, a.eval_every, a.seed)
        save()
    print(json.dumps(res))
