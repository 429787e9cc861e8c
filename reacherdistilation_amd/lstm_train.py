"""The reference's LSTM distillation driver, ``lstm_train.train(train, restore)`` (reference
src/distilation/lstm_train.py:18-201), re-expressed over the MI355X path: the env is the HIP
Reacher-v2 (``make_mujoco_env``), the teacher query is ``rdd_forward``, and the student is
the reference's ``student_lstm_graph`` trained by the kernels behind ``StudentLstmTrainer``
on windows from the device-resident ``DeviceDataset``.

Phases as in the reference:
  1. (:114-135) the teacher steps the env until ``num_episodes() > 2 * LSTM_BATCH_SIZE``;
  2. (:139-201) per env step: one optimiser step on each [T, B] window from
     ``training_batches()`` (zero initial LSTM state, :159), teacher relabel of the current
     observation, the student's mean action from the test window's last output with the
     previous query's final state as initial state (:166-183), record with 's', env.step
     with the student action; episode boundaries reset the env and flush the dataset.

Fixes of the reference as committed: the test window's prev_pdflat column is
the per-step series (``DeviceDataset.test_windows``), not the single element that only
broadcasts at 0 or >= T-1 records.

``train_envs`` is the batched form: many persistent lockstep envs, one
``StudentLstmTrainer.step_envs`` call per optimiser step (single GPU).
"""
from __future__ import annotations


import torch

from . import obs_faults as obf
from .config import LSTM_BATCH_SIZE, MAX_CAPACITY, STEPS_UNROLLED, TOTAL_EPISODES
from .dataset import DeviceDataset
from .distill import DistillConfig, DistillTrainer
from .driver_env import DriverEnv, episode_loss, teacher_share
from .pages import PageStore
from .policy import TeacherAgent
from .student_lstm import StudentLstmConfig, StudentLstmTrainer


def _restore(st, restore: bool, path: str | None, log):
    """lstm_train.py:102-107: fresh variables unless restoring; a missing checkpoint only
    prints, as the reference does."""
    if not restore:
        return
    if path and st.checkpoint_exists(path):
        st.load(path)
    else:
        log("attempt to restore trained data but {0} does not exist".format(path))


def train(train: bool = True, restore: bool = False, *, episodes: int = TOTAL_EPISODES, loss: str = "kl",
          lr: float = 1e-3, keep_prob: float = 1.0, seed: int = 0, device="cuda:0", teacher_path: str | None = None,
          warmup_episodes: int = 2 * LSTM_BATCH_SIZE, student_path: str | None = None, log=print,
          gym_env: bool = False, store_dir: str | None = None, pool: str = "reference", dtype: str = "f32"):
    """Returns (student trainer, dataset, per-episode summed training loss).  ``dtype``:
    StudentLstmConfig.dtype ("bf16": the cell matrix's products on the bf16 MFMAs).  ``store_dir``:
    the dataset's page directory (lstm_train.py:104-109); episodes are dumped to it every
    MAX_CAPACITY episodes (:200) and its stored pages join the training pool (dataset.py:
    164-177); ``pool="ring"`` draws windows uniformly from the device ring instead.  With
    ``student_path`` the student (params + Adam slots) is restored from it when ``restore``
    (lstm_train.py:102-107) and saved to it after every episode (:199).  Env I/O on the device
    (driver_env.DriverEnv; gym_env=True through the gym-API env), window losses read once per
    episode."""
    env = DriverEnv(seed, device, gym_api=gym_env)
    teacher = TeacherAgent(restore=teacher_path is not None, path=teacher_path)   # always restored (ref. :29)
    tq = DistillTrainer(DistillConfig(n_envs=64, seed=seed), device=device, teacher=teacher.pi)
    st = StudentLstmTrainer(StudentLstmConfig(loss=loss, lr=lr, keep_prob=keep_prob, seed=seed,
                                              steps=STEPS_UNROLLED, max_windows=LSTM_BATCH_SIZE, dtype=dtype),
                            device=device)
    dataset = DeviceDataset(device=device, seed=seed, batch_size=LSTM_BATCH_SIZE, steps_unrolled=STEPS_UNROLLED,
                            store=PageStore(store_dir) if store_dir else None, pool=pool)
    _restore(st, restore, student_path, log)
    losses = []
    if not train:
        return st, dataset, losses
    ob = env.reset()
    reward = torch.zeros(1, device=env.device)

    def teacher_query(o):
        t, _ = tq.forward(o, student=False)
        return t[0]

    log("Begin Training! First Accumulate observation with teacher")
    while dataset.num_episodes() <= warmup_episodes:
        t_pdflat = teacher_query(ob)
        dataset.write(ob=ob, reward=reward, t_pdflat=t_pdflat, stepped_with="t")
        ob, reward, new = env.step(t_pdflat)
        if new:
            dataset.flush()
    log("Accumulated sufficient data points from teacher. now train")

    state = None   # curr_state_batch: zero at the start (lstm_train.py:88-89)
    opt_steps = 0
    while True:
        for ob_b, t_b, prev_b, _prew_b in dataset.training_batches():
            st.step(ob_b, prev_b, t_b)          # zero initial state (lstm_train.py:159)
            opt_steps += 1
        t_pdflat = teacher_query(ob)
        ob_w, prev_w, _ = dataset.test_windows(ob)
        out, state = st.forward(ob_w, prev_w, state)
        s_pdflat = out[STEPS_UNROLLED - 1, LSTM_BATCH_SIZE - 1].clone()
        dataset.write(ob=ob, reward=reward, t_pdflat=t_pdflat, s_pdflat=s_pdflat, stepped_with="s")
        ob, reward, new = env.step(s_pdflat)
        if new:
            log("************** Episode {0} ****************".format(dataset.num_episodes()))
            total_loss = episode_loss(st.metrics(opt_steps)[:, 0] if opt_steps else [])
            log("recent loss: %f " % total_loss)
            losses.append(total_loss)
            opt_steps = 0
            dataset.flush()
            if dataset.store is not None and dataset.num_episodes() % MAX_CAPACITY == 0:
                dataset.dump()          # lstm_train.py:200
            if student_path:
                st.save(student_path)   # saver.save every episode (lstm_train.py:199)
            if dataset.num_episodes() >= episodes:
                break
    return st, dataset, losses


# -- the LSTM student distilled on-policy over many envs ---------------------------------------
def train_envs(n_envs: int, opt_steps: int, *, keep_prob: float = 1.0, loss: str = "kl", lr: float = 1e-3,
               accum_steps: int = 50, warmup_steps: int = 0, seed: int = 0, teacher=None, device="cuda:0",
               eval_every: int = 0, eval_envs: int = 4096, dtype: str = "f32", replay_capacity: int = 0,
               replay_windows: int = 0, updates_per_act: int = 1, replay_recent: int = 0, query_dtype: str = "f32",
               beta0: float = 0.0, beta_decay: float = 1.0, noise: str = "none", noise_scale: float = 1.0,
               replay_priority: str = "none", faults=None, eval_faults=None):
    """Batched on-policy distillation of the LSTM student (student_lstm_graph with input dropout
    ``keep_prob``): ``n_envs`` persistent lockstep envs, ``opt_steps`` optimiser steps, each one
    StudentLstmTrainer.step_envs call: ``accum_steps`` (a multiple of 50) env steps of every env in one
    launch, then the training pass and Adam on the query windows that lie inside an episode, from a
    zero initial state as lstm_train.py:159; nothing waits on the GPU between steps.  The first
    ``warmup_steps`` optimiser steps are stepped with the teacher's mean (the driver's phase 1: the
    student is not evaluated), the rest with the student's (phase 2, DAgger).
    Cost: every 50 env steps of an env hold 51 - T training windows, so a step trains on
    B = n_envs (accum_steps / 50) (51 - T) windows -- 41 x n_envs at T = 10 and accum_steps = 50 -- and
    the trainer is created with ``max_windows`` = B.  Its activations are about 2,900 floats per
    window position, 116 KB per window at T = 10: 4.8 MB per env, 1.2 GB at 256 envs, 19 GB at 4,096;
    T x B is at most 2^22 (n_envs <= 10,229 at the defaults).  A few hundred envs is the modest choice.
    ``dtype``: StudentLstmConfig.dtype; with "bf16" the training pass runs the cell matrix's products
    on the bf16 MFMAs while the envs are still stepped with the f32 master weights, unless
    ``query_dtype`` (StudentLstmConfig.query_dtype) is "bf16" too: the act phase, act_envs and the
    evaluations then run the cell the training pass trains.
    ``teacher``: an MlpPolicyParams (default: the synthetic teacher DistillTrainer defaults to).
    Returns (trainer, history), history rows (optimiser step, loss, action-MSE, mean step reward) with
    the loss of the trainer's metrics ring (the sum over the batch's T x B rows for "kl"), the
    action-MSE the mean over rows and both action dims against the teacher, the reward the mean over
    the call's env steps.  With ``eval_every`` > 0 returns (trainer, history, evals): evals rows
    (optimiser step, mean return of StudentLstmTrainer.evaluate over ``eval_envs`` fresh envs, one
    episode) after every eval_every-th step.  Single GPU.
    ``replay_capacity`` > 0 trains from a replay.ReplayRing of that many episodes instead (the aggregate
    of the reference's DAgger loop, dataset.py:166-194): each iteration is act_envs (``accum_steps`` env
    steps, no training), ring.push_steps of its (accum_steps / 50) n_envs episodes, then
    ``updates_per_act`` x { ring.sample_windows(T, ``replay_windows``, recent=``replay_recent``), step }:
    the batch no longer follows from the env count (``max_windows`` = replay_windows), and its windows
    come from old and new episodes alike, drawn on the device.  History rows stay per optimiser step
    (the reward that of the act call the step followed); an act call is stepped with the teacher while
    the optimiser step it precedes is a warm-up step.
    ``beta0``, ``beta_decay``: DAgger's mixture pi_i = beta_i pi* + (1 - beta_i) pi^_i instead of the hard
    switch at ``warmup_steps``: optimiser step k >= warmup_steps is stepped with the teacher share
    beta = beta0 beta_decay^(k - warmup_steps) (StudentLstmTrainer.set_teacher_share: a coin per env and
    step, the records' stepped_with its outcome), exactly 0 once below 2^-24; with a ring an act call
    takes the beta of the optimiser step it precedes.  The defaults (beta0 = 0) are the hard switch,
    the same launches as before.
    ``noise``, ``noise_scale``: action noise in every envs call of the run, warm-up steps included
    (StudentLstmTrainer.set_action_noise, keyed by ``seed``): "fixed" with the teacher acting
    (warmup_steps = opt_steps) is DART's noisy expert, "policy" samples whoever acts.  The evaluations
    stay noiseless.  The default "none" is the same launches as before.
    ``faults``: sensor faults on what the acting student reads in every envs call of the run
    (StudentLstmTrainer.set_obs_faults, keyed by ``seed``), as evaluate's ``faults``: ("dropout" | "missing",
    keep_prob).  The windows it trains on stay clean.  ``eval_faults``: the same for the periodic
    evaluation (StudentLstmTrainer.evaluate(faults=)).  The defaults (None) are the same launches as before.
    ``replay_priority`` (needs a ring): "record" draws the batches in proportion to the records' priorities
    (ReplayRing.enable_priorities: the student's squared action error against the teacher) instead of
    uniformly; a push writes the priorities from the record's own s_pdflat, the student as it acted, or
    the maximum priority when the teacher stepped the act call (s_pdflat is zero there and says nothing
    about the student).  "refresh" also re-scores every sampled batch with the current student (one
    forward per optimiser step, ReplayRing.update_priorities) before it trains on it.  The default
    "none" is the uniform loop, the same launches as before."""
    from .policy import synthetic_teacher
    n, steps, K, T = int(n_envs), int(opt_steps), int(accum_steps), STEPS_UNROLLED
    if steps < 1 or not 0 <= int(warmup_steps) <= steps:
        raise ValueError("opt_steps >= 1 and 0 <= warmup_steps <= opt_steps")
    if not 0.0 <= float(beta0) <= 1.0 or not 0.0 <= float(beta_decay) <= 1.0:
        raise ValueError("beta0 and beta_decay in [0, 1]")
    if n < 1 or K < 50 or K % 50:
        raise ValueError("n_envs >= 1 and accum_steps a positive multiple of 50")
    cap, Bw, upa = int(replay_capacity), int(replay_windows), int(updates_per_act)
    prio = str(replay_priority)
    if prio not in ("none", "record", "refresh") or (prio != "none" and cap <= 0):
        raise ValueError('replay_priority is "none", "record" or "refresh", and needs replay_capacity > 0')
    if cap < 0 or (cap and (Bw < 1 or upa < 1 or int(replay_recent) < 0 or n * (K // 50) > cap)):
        raise ValueError("replay_capacity >= (accum_steps / 50) n_envs, replay_windows >= 1, updates_per_act >= 1 "
                         "and replay_recent >= 0")
    st = StudentLstmTrainer(StudentLstmConfig(loss=loss, lr=lr, keep_prob=keep_prob, seed=seed, steps=T,
                                              max_windows=Bw if cap else n * (K // 50) * (51 - T),
                                              metrics_len=steps, dtype=dtype, query_dtype=query_dtype), device=device)
    st.set_teacher(teacher if teacher is not None else synthetic_teacher(DistillConfig().teacher_seed))
    st.attach_envs(n, seed=seed, accum_steps=K)
    if noise != "none":
        st.set_action_noise(noise, noise_scale)
    of = obf.parse(faults, seed)
    if of is not None:
        st.set_obs_faults(obf.MODE_NAMES[of.mode], of.keep_prob, of.seed)
    rew = torch.zeros(steps, device=st.device)
    evals = []
    ring = None
    if cap:
        from .replay import ReplayRing
        ring = st.replay = ReplayRing(cap, device=device, seed=seed, max_batch=Bw)
        if prio != "none":
            ring.enable_priorities(init="record")
    for k in range(steps):
        act_with = "teacher" if k < int(warmup_steps) else "student"
        if beta0 > 0 and act_with == "student" and (ring is None or k % upa == 0):
            st.set_teacher_share(teacher_share(k, warmup_steps, beta0, beta_decay))
        if ring is None:
            r = st.step_envs(act_with)
            rew[k] = r.reward.mean()
        else:
            if k % upa == 0:
                r = st.act_envs(act_with)
                if prio != "none":
                    ring.set_priority_init("const" if act_with == "teacher" else "record")
                ring.push_steps(r.records)
                mean_reward = r.reward.mean()
            if prio == "none":
                ob_w, prev_w, t_w, _ = ring.sample_windows(T, Bw, recent=int(replay_recent))
            else:
                ob_w, prev_w, t_w, _, idx = ring.sample_windows(T, Bw, recent=int(replay_recent), with_idx=True,
                                                                prioritized=True)
                if prio == "refresh":
                    ring.update_priorities(idx, st.forward(ob_w, prev_w)[0])
            st.step(ob_w, prev_w, t_w)
            rew[k] = mean_reward
        if eval_every and (k + 1) % int(eval_every) == 0:
            evals.append((k + 1, float(st.evaluate(int(eval_envs), 1, seed=seed + 1, faults=eval_faults).returns.mean())))
    m = st.metrics(steps)
    rew = rew.cpu().tolist()
    history = [(k + 1, float(m[k, 0]), float(m[k, 1] / (2 * m[k, 2])), rew[k]) for k in range(steps)]
    return (st, history, evals) if eval_every else (st, history)


def train_bptt(train: bool = True, restore: bool = False, *, episodes: int = TOTAL_EPISODES, loss: str = "kl",
               lr: float = 1e-3, keep_prob: float = 1.0, seed: int = 0, device="cuda:0", teacher_path: str | None = None,
               warmup_episodes: int = 2 * LSTM_BATCH_SIZE, student_path: str | None = None, log=print,
               gym_env: bool = False, store_dir: str | None = None, pool: str = "reference", dtype: str = "f32"):
    """The truncated-BPTT variant of the driver (reference backup/lstm_bbpt.py:18-208), same
    graph, loss and Adam.  After the teacher warm-up (:115-139) each round is
      * one BPTT pass (:141-158): ``dataset.bptt_batches()`` -- LSTM_BATCH_SIZE episodes, the
        40 windows that slide by one step -- one Adam step per window, the LSTM state carried
        from window to window (the step's final_state_batch becomes the next window's
        initial_state_batch; zero at the start of the pass);
      * then one whole episode stepped by the student (:160-205): teacher relabel, the test
        window's query with the carried query state, record with 's', env.step(student mean).
    Returns (student trainer, dataset, per-episode summed training loss).  Env I/O as in
    train()."""
    env = DriverEnv(seed, device, gym_api=gym_env)
    teacher = TeacherAgent(restore=teacher_path is not None, path=teacher_path)   # always restored (ref. :29)
    tq = DistillTrainer(DistillConfig(n_envs=64, seed=seed), device=device, teacher=teacher.pi)
    st = StudentLstmTrainer(StudentLstmConfig(loss=loss, lr=lr, keep_prob=keep_prob, seed=seed,
                                              steps=STEPS_UNROLLED, max_windows=LSTM_BATCH_SIZE, dtype=dtype),
                            device=device)
    dataset = DeviceDataset(device=device, seed=seed, batch_size=LSTM_BATCH_SIZE, steps_unrolled=STEPS_UNROLLED,
                            store=PageStore(store_dir) if store_dir else None, pool=pool)
    _restore(st, restore, student_path, log)
    losses = []
    if not train:
        return st, dataset, losses
    ob = env.reset()
    reward = torch.zeros(1, device=env.device)

    def teacher_query(o):
        t, _ = tq.forward(o, student=False)
        return t[0]

    log("Begin Training! First Accumulate observation with teacher")
    while dataset.num_episodes() <= warmup_episodes:
        t_pdflat = teacher_query(ob)
        dataset.write(ob=ob, reward=reward, t_pdflat=t_pdflat, stepped_with="t")
        ob, reward, new = env.step(t_pdflat)
        if new:
            dataset.flush()
    log("Accumulated sufficient data points from teacher. now train")

    query_state = None   # curr_state_batch (lstm_bbpt.py:94)
    while True:
        s = None         # zero_state_batch at the start of each pass (:142)
        opt_steps = 0
        for ob_b, t_b, prev_b, _prew_b in dataset.bptt_batches():
            st.step(ob_b, prev_b, t_b, state0=s)
            s = st.final_state(LSTM_BATCH_SIZE)
            opt_steps += 1
        total_loss = episode_loss(st.metrics(opt_steps)[:, 0] if opt_steps else [])
        new = False
        while not new:
            t_pdflat = teacher_query(ob)
            ob_w, prev_w, _ = dataset.test_windows(ob)
            out, query_state = st.forward(ob_w, prev_w, query_state)
            s_pdflat = out[STEPS_UNROLLED - 1, LSTM_BATCH_SIZE - 1].clone()
            dataset.write(ob=ob, reward=reward, t_pdflat=t_pdflat, s_pdflat=s_pdflat, stepped_with="s")
            ob, reward, new = env.step(s_pdflat)
        log("************** Episode {0} ****************".format(dataset.num_episodes()))
        log("recent loss: %f " % total_loss)
        losses.append(total_loss)
        dataset.flush()
        if dataset.store is not None and dataset.num_episodes() % MAX_CAPACITY == 0:
            dataset.dump()              # backup/lstm_bbpt.py:207
        if student_path:
            st.save(student_path)
        if dataset.num_episodes() >= episodes:
            break
    return st, dataset, losses
