"""The device replay ring (replay.ReplayRing) measured on the GPU, two parts, one JSON file (default
profiles/replay_sample_vs_torch.json), also printed.

1. ``sample_windows`` at T = 10 and B in {1,024, 16,384, 163,840} from a full ring of 8,192 episodes
   against the torch-indexing gather of DeviceDataset.training_batches (pool="ring": host RNG, the
   [2, T, B] index tensor built on the host and copied over, one advanced-indexing gather, four
   slices made contiguous) at the same shapes and from the same records.  Each call is timed with a host
   clock from before the call to after a device synchronise (what a driver that needs the batch waits
   for, host work included), alternating the two sides; the ring's calls are also timed back to back
   with device events (20 calls per measurement), the time they take inside a stream that is never
   waited on.  Algorithmic bytes of a batch: its T B 20 output floats written and as many read.  They
   are reported as a fraction of the float4-copy bandwidth measured in this run
   (scripts/micro/copy_bw.hip as libcopybw.so, read + write bytes per second, best plain variant).
2. ``lstm_train.train_envs`` at 4,096 envs (bf16) with a ring (replay_windows = 16,384) against the
   on-policy driver (one step_envs per optimiser step on 41 x 4,096 windows) at the same env count:
   wall time of whole driver calls that end in a device read, two lengths each, differenced so that
   construction drops out (median of three differences after one untimed call); in ms per optimiser
   step and per env step.  THE TWO TRAIN ON DIFFERENT BATCHES (16,384 windows drawn from the aggregate
   against the 167,936 overlapping windows the step just produced) AND ARE NOT EQUIVALENT WORK; the
   figures say what an optimiser step costs in each mode, not which learns faster.  No threshold is
   asserted anywhere.
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
from reacherdistilation_amd import lstm_train  # noqa: E402
from reacherdistilation_amd.dataset import DeviceDataset  # noqa: E402
from reacherdistilation_amd.replay import ReplayRing  # noqa: E402

DEV = "cuda:0"
T = 10


def copy_ceiling(gib=1.0, reps=20):
    """GB/s of the best plain float4 copy variant (bench.py's copy_ceiling, variants 1-6)."""
    path = os.path.join(ROOT, "scripts", "micro", "libcopybw.so")
    if not os.path.exists(path):
        raise SystemExit(f"{path} not built: run __graft_entry__.build() first (the fraction needs this run's copy)")
    lib = ctypes.CDLL(path)
    lib.copy_bw_tbs.restype = ctypes.c_double
    lib.copy_bw_tbs.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.copy_bw_name.restype = ctypes.c_char_p
    lib.copy_bw_name.argtypes = [ctypes.c_int]
    nbytes = int(gib * (1 << 30))
    res = {lib.copy_bw_name(v).decode(): 1e3 * lib.copy_bw_tbs(nbytes, v, blocks, reps)
           for v, blocks in ((1, 65536), (2, 65536), (3, 0), (4, 0), (5, 0), (6, 0))}
    best = max(res, key=res.get)
    return dict(best_gbs=res[best], best=best, variants_gbs=res, bytes=nbytes)


def stats(us):
    q = statistics.quantiles(us, n=4)
    return dict(median_us=statistics.median(us), q1_us=q[0], q3_us=q[2], min_us=min(us), max_us=max(us), reps=len(us))


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def sample_vs_torch(B, episodes, reps, copy_gbs):
    ring = ReplayRing(episodes, device=DEV, seed=0, max_batch=B)
    ds = DeviceDataset(capacity=episodes, device=DEV, seed=0, batch_size=B, steps_unrolled=T, epochs=1, pool="ring")
    g = torch.Generator().manual_seed(1)
    for lo in range(0, episodes, 1024):   # the same records on both sides
        rec = torch.randn(min(1024, episodes - lo), 50, 21, generator=g).to(DEV)
        ring.push_episodes(rec)
        ds.write_episodes(rec)
    assert ring.counters()[0] == episodes == ds.stored() and torch.equal(ring.records, ds.ring)

    def ours():
        ring.sample_windows(T, B, common_start=True)

    def theirs():
        for _ in ds.training_batches():
            pass

    for _ in range(3):
        ours()
        theirs()
    o_us, t_us, dev_us = [], [], []
    for _ in range(reps):
        t_us.append(host_timed(theirs))
        o_us.append(host_timed(ours))
    for _ in range(max(5, reps // 4)):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(20):
            ours()
        e.record()
        e.synchronize()
        dev_us.append(s.elapsed_time(e) * 1e3 / 20)
    nbytes = 2 * T * B * 20 * 4
    o, t, d = stats(o_us), stats(t_us), stats(dev_us)
    gbs = nbytes / (d["median_us"] * 1e-6) / 1e9
    ring.close()
    return dict(T=T, B=B, ring_episodes=episodes, algorithmic_bytes=nbytes, start="common (training_batches' rule)",
                sample_windows_call_to_sync=o, torch_gather_call_to_sync=t, sample_windows_in_stream=d,
                speedup_median_call_to_sync=t["median_us"] / o["median_us"],
                ring_beats_torch=o["q3_us"] < t["q1_us"],
                in_stream_gbs=gbs, in_stream_fraction_of_copy=gbs / copy_gbs,
                call_to_sync_fraction_of_copy=nbytes / (o["median_us"] * 1e-6) / 1e9 / copy_gbs)


def driver_ms(n, lengths, rounds=3, **kw):
    """ms per optimiser step of lstm_train.train_envs: wall time of two whole calls, differenced (median of
    ``rounds`` differences, after one untimed call of the same configuration)."""
    def wall(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st, _ = lstm_train.train_envs(n, steps, dtype="bf16", device=DEV, **kw)   # ends in a metrics read
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st.close()
        return dt

    a, b = lengths
    wall(a)   # code objects, allocator
    pairs = [(wall(a), wall(b)) for _ in range(rounds)]
    ms = [1e3 * (tb - ta) / (b - a) for ta, tb in pairs]
    return statistics.median(ms), dict(ms_per_opt_step_each_round=ms, wall_s=[list(p) for p in pairs])


def drivers(n, windows, capacity, lengths):
    out = dict(n_envs=n, dtype="bf16", steps_unrolled=T, lengths=list(lengths),
               note="the two modes train on different batches and are not equivalent work")
    ms, raw = driver_ms(n, lengths)
    out["on_policy"] = dict(windows_per_opt_step=n * 41, env_steps_per_opt_step=50 * n, ms_per_opt_step=ms,
                            ms_per_env_step_of_all_envs=ms / 50, raw=raw)
    for upa in (1, 4):
        ms, raw = driver_ms(n, lengths, replay_capacity=capacity, replay_windows=windows, updates_per_act=upa)
        out[f"replay_updates_per_act_{upa}"] = dict(
            windows_per_opt_step=windows, replay_capacity=capacity, env_steps_per_opt_step=50 * n / upa,
            ms_per_opt_step=ms, ms_per_env_step_of_all_envs=ms * upa / 50, raw=raw)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 16384, 163840])
    ap.add_argument("--episodes", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=16384)
    ap.add_argument("--lengths", type=int, nargs=2, default=[10, 50], help="opt_steps of the two differenced driver calls")
    ap.add_argument("--no-drivers", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_sample_vs_torch.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_replay.py measures on a HIP device; none found")
    ceil = copy_ceiling()
    res = dict(device=torch.cuda.get_device_name(0),
               method="part 1: host clock from call to device synchronise, alternating sides, and device events "
                      "around 20 back-to-back ring samples; part 2: wall time of whole train_envs calls, two lengths "
                      "differenced; quartiles by statistics.quantiles",
               copy_ceiling=ceil,
               sample_windows=[sample_vs_torch(B, a.episodes, a.reps, ceil["best_gbs"]) for B in a.batches])
    if not a.no_drivers:
        res["train_envs"] = drivers(a.envs, a.windows, 2 * a.envs, tuple(a.lengths))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
