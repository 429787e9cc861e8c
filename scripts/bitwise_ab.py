"""A/B of two builds on the same steps: writes the student parameters and the last gradient
after a few fused steps of several configs to an .npz (the build is chosen with RD_LIB), so
two runs can be compared bit for bit.
--lstm runs the LSTM student's case set instead: three rdl_step calls per case and loss from seeded
parameters and windows; parameters, gradient, the three metrics rows and the final state are written.
--mlp runs the reference MLP student's: three rdm_step calls from seeded rows for mse and kl, keep_prob
1.0 and 0.5, f32 and bf16, at a 16-row-block and a 64-row-block size; one rdm_forward; and, at env
counts that take either block size (one with a capped grid, so that a workgroup takes several blocks),
rdm_evaluate with records, rdm_envs_act with each act_with and rdm_step_envs.
usage: RD_LIB=libreacher_x.so python scripts/bitwise_ab.py [--lstm | --mlp] out.npz  (GPU)
       python scripts/bitwise_ab.py --compare a.npz b.npz"""
import os
import sys

import numpy as np

CASES = {   # name: DistillConfig overrides
    "c2": dict(n_envs=4096),
    "c2_g16": dict(n_envs=4096, group_envs=16),   # the plain layout at c2 (auto picks helper pairs)
    "c2_exact": dict(n_envs=4096, f32_split=False),
    "small_777": dict(n_envs=777, loss="kl"),
    "c4": dict(n_envs=262144),
    "c5": dict(n_envs=131072, act_with="student", student_dtype="bf16"),
    "ragged_5003": dict(n_envs=5003, loss="kl"),
    "grid7_kl": dict(n_envs=3000, loss="kl", grid=7),
    "grid300": dict(n_envs=300 * 4 * 64, grid=300),
    "accum3": dict(n_envs=20000, accum_steps=3),
    "c3_exact": dict(n_envs=65536, loss="kl", f32_split=False),
    "c5_exact": dict(n_envs=131072, act_with="student", student_dtype="bf16", f32_split=False),
}


def run(out):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from reacherdistilation_amd.distill import DistillConfig, DistillTrainer
    res = {}
    for name, kw in CASES.items():
        cfg = dict(loss="mse", f32_split=True, seed=3)
        cfg.update(kw)
        tr = DistillTrainer(DistillConfig(**cfg), device="cuda:0")
        for _ in range(6):
            tr.step()
        torch.cuda.synchronize()
        res[name + "_params"] = tr.student_params().cpu().numpy()
        res[name + "_grad"] = tr.grad().cpu().numpy()
        res[name + "_state"] = tr.env_state().cpu().numpy()
        tr.close()
    np.savez(out, **res)
    print("wrote", out, flush=True)


LSTM_CASES = {   # name: (T, B, StudentLstmConfig overrides, with state0): every launch sequence of student_lstm.hip
    "persist_20": (10, 20, {}, False),             # persistent cell, wide fused head with the loss, grad_finish_kernel
    "step_20": (10, 20, dict(step_recurrence=True), False),   # per-step f32 cell, fused head, one loss block
    "layers_20": (10, 20, dict(layer_head=True), False),      # persistent cell, per-layer head, dense32_grad_kernel
    "step_t3_130": (3, 130, {}, False),            # per-step cell (B > 32), two loss blocks + metrics_kernel, GEMM tail
    "head_narrow_1000": (10, 1000, {}, False),     # fused head, one tile per workgroup, four waves
    "head_tiles_4100": (10, 4100, {}, False),      # fused head, several tiles per workgroup, two-level column sums
    "bf16_20": (10, 20, dict(dtype="bf16"), False),           # bf16 cell, one weight-gradient split
    "bf16_t3_130": (3, 130, dict(dtype="bf16"), False),       # bf16 cell, several splits
    "state0_20": (10, 20, {}, True),
    "state0_step_20": (10, 20, dict(step_recurrence=True), True),
}


def run_lstm(out):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from reacherdistilation_amd.student_lstm import StudentLstmConfig, StudentLstmTrainer
    res = {}
    for name, (T, B, kw, with_state) in LSTM_CASES.items():
        rng = np.random.RandomState(11)
        ob = rng.standard_normal((T, B, 11)).astype(np.float32)
        prev = (0.5 * rng.standard_normal((T, B, 4))).astype(np.float32)
        tgt = rng.uniform(-1.0, 0.5, (T, B, 4)).astype(np.float32)
        st = (0.3 * rng.standard_normal((2, B, 200))).astype(np.float32) if with_state else None
        for loss in ("mse", "kl"):
            tr = StudentLstmTrainer(StudentLstmConfig(loss=loss, steps=T, max_windows=B, keep_prob=0.5, seed=5, **kw),
                                    device="cuda:0")
            for _ in range(3):
                tr.step(ob, prev, tgt, st)
            torch.cuda.synchronize()
            key = f"{name}_{loss}"
            res[key + "_params"] = tr.params().cpu().numpy()
            res[key + "_grad"] = tr.grad().cpu().numpy()
            res[key + "_metrics"] = tr.metrics(3)
            res[key + "_state"] = tr.final_state(B).cpu().numpy()
            tr.close()
            print("ran", key, flush=True)
    np.savez(out, **res)
    print("wrote", out, flush=True)


MLP_ROWS = {"r200": 200, "r5000": 5000}   # a 16-row-block and a 64-row-block size at grid = 64
MLP_ENVS = {   # name: (n_envs, grid, K): every block choice of the closed-loop launches
    "e83": (83, 0, 7),            # 16-env blocks, a ragged last block
    "e300_g4": (300, 4, 3),       # 64-env blocks (19 blocks of 16 > 4), a workgroup takes two blocks
    "e100_g3": (100, 3, 50),      # 64-env blocks, an episode's TimeLimit reset inside the call
}


def run_mlp(out):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from reacherdistilation_amd.distill import DistillConfig, DistillTrainer
    from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer
    teacher = DistillTrainer(DistillConfig(n_envs=64, seed=0), device="cuda:0").teacher
    res = {}
    for dtype in ("f32", "bf16"):
        for rname, n in MLP_ROWS.items():
            rng = np.random.RandomState(13)
            x = rng.uniform(-1.0, 1.0, (n, 16)).astype(np.float32)
            tgt = rng.uniform(-1.0, 0.5, (n, 4)).astype(np.float32)
            for loss in ("mse", "kl"):
                for kp in (1.0, 0.5):
                    tr = StudentMlpTrainer(StudentMlpConfig(loss=loss, keep_prob=kp, seed=5, grid=64, dtype=dtype),
                                           device="cuda:0")
                    for _ in range(3):
                        tr.step(x, tgt)
                    torch.cuda.synchronize()
                    key = f"{dtype}_{rname}_{loss}_kp{kp}"
                    res[key + "_params"] = tr.params().cpu().numpy()
                    res[key + "_grad"] = tr.grad().cpu().numpy()
                    res[key + "_metrics"] = tr.metrics(3)
                    tr.close()
                    print("ran", key, flush=True)
            tr = StudentMlpTrainer(StudentMlpConfig(grid=64, dtype=dtype), device="cuda:0")
            res[f"{dtype}_{rname}_forward"] = tr.forward(x).cpu().numpy()
            tr.close()
        for ename, (n, grid, K) in MLP_ENVS.items():
            key = f"{dtype}_{ename}"
            tr = StudentMlpTrainer(StudentMlpConfig(loss="kl", keep_prob=0.5, seed=5, dtype=dtype), device="cuda:0")
            tr.set_teacher(teacher)
            ev = tr.evaluate(n, 2, seed=9, final_dist=True, records=True, grid=grid)
            res[key + "_eval_returns"] = ev.returns.cpu().numpy()
            res[key + "_eval_final_dist"] = ev.final_dist.cpu().numpy()
            res[key + "_eval_records"] = ev.records.cpu().numpy()
            tr.attach_envs(n, seed=9, grid=grid, accum_steps=K)
            for act in ("teacher", "student"):
                r = tr.act_envs(act)
                for f in ("x", "t_pdflat", "s_pdflat", "reward"):
                    res[f"{key}_act_{act}_{f}"] = getattr(r, f).cpu().numpy()
            r = tr.step_envs("student")
            for f in ("x", "t_pdflat", "s_pdflat", "reward"):
                res[f"{key}_step_envs_{f}"] = getattr(r, f).cpu().numpy()
            st, step, episode = tr.env_state()
            res[key + "_step_envs_state"] = st.cpu().numpy()
            res[key + "_step_envs_clock"] = np.array([step, episode], np.int32)
            res[key + "_step_envs_params"] = tr.params().cpu().numpy()
            res[key + "_step_envs_grad"] = tr.grad().cpu().numpy()
            res[key + "_step_envs_metrics"] = tr.metrics(1)
            tr.close()
            print("ran", key, flush=True)
    np.savez(out, **res)
    print("wrote", out, flush=True)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = 0
    for k in A.files:
        same = np.array_equal(A[k].view(np.uint32), B[k].view(np.uint32))
        d = float(np.abs(A[k] - B[k]).max())
        print(f"{k:24s} bitwise_equal={same} max_abs_diff={d:.3g}")
        bad += not same
    print("ALL BITWISE EQUAL" if not bad else f"{bad} arrays differ")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    if sys.argv[1] == "--lstm":
        run_lstm(sys.argv[2])
    elif sys.argv[1] == "--mlp":
        run_mlp(sys.argv[2])
    else:
        run(sys.argv[1])
