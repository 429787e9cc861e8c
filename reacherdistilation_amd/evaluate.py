"""Whole-episode policy evaluation and episode collection in one fused launch (rdd_evaluate,
include/reacher_distill.h, DistillTrainer.evaluate; rdm_evaluate, include/reacher_student_mlp.h,
StudentMlpTrainer.evaluate; rdl_evaluate, include/reacher_student_lstm.h,
StudentLstmTrainer.evaluate).

  evaluate_student_lstm  the same for the reference's LSTM student (student_lstm_graph on the window
                    of the episode's last T records, the LSTM state carried from query to query),
                    the student lstm_train.py distils; its weights stream from L2
  evaluate_student_mlp  evaluate_policy for the reference's own MLP student (student_mlp_graph on
                    rows ob | prev pdflat | prev reward): the average-reward quantity the reference
                    plots per keep_prob, on the student it actually distils
  evaluate_policy   the fused counterpart of teacher.episode_returns: the 50-step returns of a
                    policy's mean action, what the reference reads offline from recorded episodes
                    (extract_reward.py, plot.py)
  collect_episodes  teacher.collect_reward's signature and result (the same dataset, bit for bit)
                    with one launch per chunk of rounds in place of 100 launches per round

All keep each env's whole episode on chip, the 2x64 nets' weights in LDS (DESIGN.md §3
"Evaluation"); the arithmetic is that of the stepwise loops they replace, so the results are
bitwise theirs (tests/test_evaluate_gpu.py, tests/test_student_*_evaluate_gpu.py).
"""
from __future__ import annotations

import numpy as np
import torch

from .config import MAX_CAPACITY, STEPS_UNROLLED
from .dataset import DeviceDataset
from .distill import DistillConfig, DistillTrainer
from .env import gym_reset_draws
from .pages import PageStore
from .policy import MlpPolicyParams, TeacherAgent
from .student_lstm import StudentLstmConfig, StudentLstmTrainer
from .student_mlp import StudentMlpConfig, StudentMlpTrainer

__all__ = ["evaluate_policy", "evaluate_student_mlp", "evaluate_student_lstm", "collect_episodes", "gym_draw_table"]

# collect_episodes: episodes (rounds x envs) per launch; their records (4,200 B each) are one tensor
CHUNK_EPISODES = 16384


def gym_draw_table(seed: int, n_envs: int, episodes: int) -> np.ndarray:
    """Reset draws [episodes, n_envs, 6] f32 of gym-seeded envs, env i seeded ``seed + i`` as
    make_mujoco_env(env_id, seed + i): BatchedReacher(n_envs, seed, reset="gym")'s table."""
    return np.stack([gym_reset_draws(seed + i, episodes) for i in range(n_envs)], axis=1).astype(np.float32)


def evaluate_policy(params: MlpPolicyParams, episodes: int, *, n_envs: int | None = None, seed: int = 0,
                    reset: str = "gym", device="cuda:0") -> np.ndarray:
    """50-step returns of ``params``' mean action over ``episodes`` episodes: ``n_envs`` envs
    (default: one env per episode, as teacher.episode_returns) run ceil(episodes / n_envs)
    consecutive episodes each, in one launch.  Returns a float32 array [episodes] in (round, env)
    order, each entry the f32 sum of the episode's step rewards in step order.
    reset "gym": env i is seeded seed + i like gym/baselines (env.gym_reset_draws);
    "philox": Philox(seed, i, round)."""
    if reset not in ("gym", "philox"):
        raise ValueError(f"unknown reset mode {reset!r}")
    episodes = int(episodes)
    n = episodes if n_envs is None else int(n_envs)
    if episodes < 1 or n < 1:
        raise ValueError("episodes >= 1 and n_envs >= 1")
    E = -(-episodes // n)
    dev = torch.device(device)
    tr = DistillTrainer(DistillConfig(n_envs=64, seed=seed), device=dev, teacher=params)
    try:
        draws = gym_draw_table(seed, n, E) if reset == "gym" else None
        ret = tr.evaluate("teacher", n, E, seed=seed, draws=draws).returns
        return ret.reshape(-1)[:episodes].cpu().numpy()
    finally:
        tr.close()


def evaluate_student_mlp(trainer_or_params, teacher: MlpPolicyParams | None, episodes: int, *,
                         n_envs: int | None = None, seed: int = 0, reset: str = "gym", device="cuda:0",
                         noise: str = "none", noise_scale: float = 1.0, noise_seed: int | None = None,
                         faults=None) -> np.ndarray:
    """evaluate_policy for the reference student: the 50-step returns of its mean action over
    ``episodes`` student-stepped episodes, in one launch (StudentMlpTrainer.evaluate).
    ``trainer_or_params`` is a StudentMlpTrainer (evaluated as it stands, on its device; ``teacher``
    replaces its teacher unless None) or a flat parameter vector [24,380] (a trainer is made on
    ``device`` and closed).  The teacher labels every observation: the student's row carries the
    teacher's previous pdflat and the previous record's reward, which is carried over resets, so an
    env's consecutive episodes (n_envs < episodes) are not independent -- as in the driver's loop.
    Returns a float32 array [episodes] in (round, env) order; ``n_envs`` (default: one env per
    episode), ``seed`` and ``reset`` as evaluate_policy.  ``noise``, ``noise_scale``, ``noise_seed``:
    StudentMlpTrainer.evaluate's -- the returns under perturbed actions ("policy": the policy sampled;
    "fixed": an isotropic sigma), noise_seed defaulting to ``seed``.  ``faults``: StudentMlpTrainer.evaluate's
    -- the returns with the student reading its observation through sensor faults, e.g.
    ("missing", 0.9)."""
    if reset not in ("gym", "philox"):
        raise ValueError(f"unknown reset mode {reset!r}")
    episodes = int(episodes)
    n = episodes if n_envs is None else int(n_envs)
    if episodes < 1 or n < 1:
        raise ValueError("episodes >= 1 and n_envs >= 1")
    E = -(-episodes // n)
    own = not isinstance(trainer_or_params, StudentMlpTrainer)
    tr = StudentMlpTrainer(StudentMlpConfig(seed=seed), device=device, params=trainer_or_params) if own \
        else trainer_or_params
    try:
        if teacher is not None:
            tr.set_teacher(teacher)
        draws = gym_draw_table(seed, n, E) if reset == "gym" else None
        ret = tr.evaluate(n, E, seed=seed, draws=draws, noise=noise, noise_scale=noise_scale,
                          noise_seed=noise_seed, faults=faults).returns
        return ret.reshape(-1)[:episodes].cpu().numpy()
    finally:
        if own:
            tr.close()


def evaluate_student_lstm(trainer_or_params, teacher: MlpPolicyParams | None, episodes: int, *,
                          n_envs: int | None = None, seed: int = 0, reset: str = "gym", device="cuda:0",
                          steps: int = STEPS_UNROLLED, dtype: str = "f32", query_dtype: str = "f32",
                          noise: str = "none", noise_scale: float = 1.0, noise_seed: int | None = None,
                          faults=None) -> np.ndarray:
    """evaluate_student_mlp for the reference's LSTM student: the 50-step returns of its mean action
    over ``episodes`` student-stepped episodes, in one rollout launch (StudentLstmTrainer.evaluate).
    ``trainer_or_params`` is a StudentLstmTrainer (evaluated as it stands, on its device; ``teacher``
    replaces its teacher unless None) or a flat parameter vector of student_lstm.n_params(steps)
    floats (a trainer of ``steps`` unrolled steps is made on ``device`` and closed).  The LSTM state
    starts at zero and is carried from query to query over the resets, as the driver carries it, so
    an env's consecutive episodes (n_envs < episodes) are not independent.  Returns a float32 array
    [episodes] in (round, env) order; ``n_envs`` (default: one env per episode), ``seed`` and
    ``reset`` as evaluate_policy.  ``dtype`` and ``query_dtype`` are StudentLstmConfig's for the trainer
    made from a parameter vector (dtype="bf16", query_dtype="bf16": the policy as deployed on the bf16
    cell); a given trainer is evaluated with its own setting.  ``noise``, ``noise_scale``, ``noise_seed``:
    StudentLstmTrainer.evaluate's, as in evaluate_student_mlp; so is ``faults``."""
    if reset not in ("gym", "philox"):
        raise ValueError(f"unknown reset mode {reset!r}")
    episodes = int(episodes)
    n = episodes if n_envs is None else int(n_envs)
    if episodes < 1 or n < 1:
        raise ValueError("episodes >= 1 and n_envs >= 1")
    E = -(-episodes // n)
    own = not isinstance(trainer_or_params, StudentLstmTrainer)
    tr = StudentLstmTrainer(StudentLstmConfig(seed=seed, steps=int(steps), dtype=dtype, query_dtype=query_dtype),
                            device=device,
                            params=trainer_or_params) if own else trainer_or_params
    try:
        if teacher is not None:
            tr.set_teacher(teacher)
        draws = gym_draw_table(seed, n, E) if reset == "gym" else None
        ret = tr.evaluate(n, E, seed=seed, draws=draws, noise=noise, noise_scale=noise_scale,
                          noise_seed=noise_seed, faults=faults).returns
        return ret.reshape(-1)[:episodes].cpu().numpy()
    finally:
        if own:
            tr.close()


def collect_episodes(episodes: int, n_envs: int = 1, *, seed: int = 0, teacher: MlpPolicyParams | None = None,
                     teacher_path: str | None = None, dataset: DeviceDataset | None = None,
                     store_dir: str | None = None, device="cuda:0", reset: str = "gym") -> DeviceDataset:
    """teacher.collect_reward with the rounds fused: record ``episodes`` teacher-stepped episodes
    (rounded up to whole rounds of ``n_envs``; the last round's surplus is dropped) into
    ``dataset`` (a new DeviceDataset when None, its pages in ``store_dir``), the same records bit
    for bit.  Round r is episode r of every env; a launch covers a chunk of rounds (at most
    CHUNK_EPISODES episodes of records at a time).  A chunk after the first replays the previous
    chunk's last round first, so that the reward carried into its first records is the stepwise
    one.  With a page store, full pages of MAX_CAPACITY episodes are dumped as collect_reward does."""
    if episodes < 0 or n_envs < 1:
        raise ValueError("episodes >= 0 and n_envs >= 1")
    if reset not in ("gym", "philox"):
        raise ValueError(f"unknown reset mode {reset!r}")
    dev = torch.device(device)
    pi = teacher if teacher is not None else TeacherAgent(restore=teacher_path is not None, path=teacher_path).pi
    if dataset is None:
        dataset = DeviceDataset(capacity=max(5000, int(episodes)), device=dev, seed=seed,
                                store=PageStore(store_dir) if store_dir else None)
    rounds = -(-int(episodes) // n_envs)
    if rounds == 0:
        return dataset
    tr = DistillTrainer(DistillConfig(n_envs=64, seed=seed), device=dev, teacher=pi)
    table = torch.from_numpy(gym_draw_table(seed, n_envs, rounds)).to(dev) if reset == "gym" else None
    per = max(1, CHUNK_EPISODES // n_envs)
    done = 0
    for r0 in range(0, rounds, per):
        r1 = min(rounds, r0 + per)
        lead = 1 if r0 else 0   # the previous round again: its last reward opens this chunk's records
        rec = tr.evaluate("teacher", n_envs, r1 - r0 + lead, seed=seed, first_episode=r0 - lead,
                          draws=table[r0 - lead:r1] if table is not None else None, records=True).records[lead:]
        for eps in rec:   # one round: [n_envs, 50, 21] in env order
            take = min(n_envs, episodes - done)
            eps = eps[:take]
            if dataset.store is None:
                dataset.write_episodes(eps)
            else:   # page by page: dump whenever the episode count reaches a multiple of MAX_CAPACITY
                e = 0
                while e < take:
                    k = min(take - e, MAX_CAPACITY - dataset.num_episodes() % MAX_CAPACITY)
                    dataset.write_episodes(eps[e:e + k])
                    e += k
                    if dataset.num_episodes() % MAX_CAPACITY == 0:
                        dataset.dump()
            done += take
    torch.cuda.current_stream(dev).synchronize()   # the records are in the dataset before the trainer goes
    tr.close()
    return dataset
