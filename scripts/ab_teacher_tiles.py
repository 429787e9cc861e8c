"""Per-step time of the fused step (K = 1) per rdd_config.teacher_tiles mask, all masks in ONE
process: per workload one trainer per mask, timed round-robin in `rounds` passes (so clock drift
hits every mask alike); prints one JSON line per workload with each mask's per-pass figures.
  python scripts/ab_teacher_tiles.py [steps] [workload,...] [rounds]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from reacherdistilation_amd.distill import DistillConfig, DistillTrainer  # noqa: E402

WL = {"c2": dict(n_envs=4096), "c3": dict(n_envs=65536, loss="kl"), "c4": dict(n_envs=262144),
      "n131072": dict(n_envs=131072), "n32768": dict(n_envs=32768), "n49152": dict(n_envs=49152),   # 32-env groups
      "n98304": dict(n_envs=98304), "n196608": dict(n_envs=196608)}                                   # 1.5 / 3 groups per pair
MASKS = (0, 0b0010, 0b1010, 0b1110)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    names = sys.argv[2].split(",") if len(sys.argv) > 2 else ["c4", "c3", "c2"]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    dev = torch.device("cuda", 0)
    for name in names:
        trs = {m: DistillTrainer(DistillConfig(seed=0, teacher_tiles=m, **WL[name]), device=dev) for m in MASKS}
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:   # clock settle
            trs[0].step()
            torch.cuda.synchronize(dev)
        out = {"workload": name, "steps": steps, "us_per_step": {m: [] for m in MASKS}}
        for _ in range(rounds):
            for m, tr in trs.items():
                for _ in range(max(2, steps // 10)):
                    tr.step()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(steps):
                    tr.step()
                torch.cuda.synchronize(dev)
                out["us_per_step"][m].append((time.perf_counter() - t0) * 1e6 / steps)
        out["layout"] = {m: tr.last_layout(teacher_tiles=True) for m, tr in trs.items()}
        for tr in trs.values():
            tr.counter()   # raises on a timed-out hand-off
            tr.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
