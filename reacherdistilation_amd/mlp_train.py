"""The reference's MLP distillation driver, ``mlp_train.train(train, restore)`` (reference
src/distilation/mlp_train.py:18-204), re-expressed over the MI355X path: the env is the HIP
Reacher-v2 (``make_mujoco_env``), teacher queries and the student's training step are the
fused kernels behind ``DistillTrainer`` (``rdd_forward`` / ``rdd_step_obs``), and the
rollout -> distill buffer is the device-resident ``DeviceDataset``.

Phases as in the reference:
  1. (:120-139) the teacher steps the env until ``num_episodes() > 2 * MLP_BATCH_SIZE``,
     every step recorded (ob, reward of the previous step, teacher pdflat, 't');
  2. (:143-204) per env step: one optimiser step on each window from
     ``dataset.training_batches()``, teacher relabel of the current observation, the student's
     (deterministic mean) action, record with 's', env.step with the student action; episode
     boundaries reset the env and flush the dataset; stop after ``episodes`` episodes.

Students: ``student="policy"`` (default) is the 2x64 MlpPolicy taking the observation (the
fused DistillTrainer path); ``student="mlp"`` is the reference's own ``student_mlp_graph``
(student_nn.py:51-57) on rows ob | prev_pdflat | prev_rew (StudentMlpTrainer), trained on the
recorded teacher pdflat with input dropout ``keep_prob`` (reference KEEP_PROB = 0.5).

``train_envs`` is the same distillation of the reference student over many persistent lockstep envs
(StudentMlpTrainer.step_envs: no dataset, every optimiser step on the rows its envs just produced).

Fixes of the reference as committed: the committed
graph's (10,20,.) vs (1,20,.) placeholder mismatch is not reproduced -- every row of a [T, B]
window is a training row; prev_pdflat / prev_rew are the dataset's recorded fields, not the
committed np.random.rand "TODO revert" stand-ins (mlp_train.py:151-158).
"""
from __future__ import annotations

import torch

from . import _native as nat
from . import obs_faults as obf
from .config import EPISODE_STEPS, LSTM_BATCH_SIZE, MLP_BATCH_SIZE, MLP_EPISODE_BUDGET, OBSPACE_SHAPE, STEPS_UNROLLED
from .dataset import DeviceDataset
from .pages import PageStore
from .distill import DistillConfig, DistillTrainer
from .driver_env import DriverEnv, episode_loss, teacher_share
from .policy import TeacherAgent
from .student_mlp import StudentMlpConfig, StudentMlpTrainer, rows


def train(train: bool = True, restore: bool = False, *, episodes: int = MLP_EPISODE_BUDGET,
          loss: str = "kl", lr: float = 1e-4, seed: int = 0, device="cuda:0", teacher_path: str | None = None,
          warmup_episodes: int = 2 * MLP_BATCH_SIZE, student: str = "policy", keep_prob: float = 1.0,
          log=print, gym_env: bool = False, store_dir: str | None = None, pool: str = "reference",
          stop_loss: float | None = None, teacher=None, dtype: str = "f32"):
    """Returns (trainer, dataset, per-episode summed training loss); the trainer is the
    DistillTrainer (student="policy") or the StudentMlpTrainer (student="mlp").  The env I/O
    stays on the device (driver_env.DriverEnv; gym_env=True: through the gym-API env, numpy
    every step) and the window losses are read from the trainer's metrics ring once per
    episode, so nothing waits on the GPU inside an episode.  ``store_dir``: the dataset's page
    directory (mlp_train.py:105-110); episodes are dumped to it every 5 episodes (:203) and its
    stored pages join the training pool (dataset.py:164-177); ``pool="ring"`` draws windows
    uniformly from the device ring instead.  ``stop_loss``: also stop after the first DAgger
    episode whose mean window loss falls below it (convergence measurements).  ``teacher``: an
    MlpPolicyParams used instead of the restored / synthetic one (e.g. teacher.fit_teacher).
    ``dtype``: the arithmetic of the student="mlp" trainer (StudentMlpConfig.dtype: "f32", or "bf16"
    mixed precision, in which the student that acts is the student that is trained)."""
    if student not in ("policy", "mlp"):
        raise ValueError(f"unknown student {student!r}")
    env = DriverEnv(seed, device, gym_api=gym_env)
    pi = teacher if teacher is not None else \
        TeacherAgent(restore=teacher_path is not None, path=teacher_path).pi   # always restored (ref. :29)
    tr = DistillTrainer(DistillConfig(n_envs=64, seed=seed, loss=loss, lr=lr), device=device, teacher=pi)
    if student != "mlp" and dtype != "f32":
        raise ValueError('dtype selects the arithmetic of student="mlp" only')
    sm = StudentMlpTrainer(StudentMlpConfig(loss=loss, lr=lr, keep_prob=keep_prob, seed=seed, dtype=dtype),
                           device=device) if student == "mlp" else None
    dataset = DeviceDataset(device=device, seed=seed, store=PageStore(store_dir) if store_dir else None, pool=pool)
    ob = env.reset()                                  # [1, 11] on the device
    reward = torch.zeros(1, device=env.device)
    losses = []
    if not train:
        return (sm or tr), dataset, losses

    def query(o):
        t, s = tr.forward(o)
        if sm is not None:   # the reference student: row = ob | prev_pdflat | prev_rew
            prev, prew = dataset.current_prev()
            s = sm.forward(rows(o.view(OBSPACE_SHAPE), prev, prew))
        return t[0], s[0]

    log("Begin Training! First Accumulate observation with teacher")
    while dataset.num_episodes() <= warmup_episodes:
        t_pdflat, _ = query(ob)
        dataset.write(ob=ob, reward=reward, t_pdflat=t_pdflat, stepped_with="t")
        ob, reward, new = env.step(t_pdflat)
        if new:
            dataset.flush()
    log("Accumulated sufficient data points from teacher. now train")

    opt_steps = 0   # optimiser steps of the open episode (their losses are read at its end)
    while True:
        for ob_batch, t_batch, prev_batch, prew_batch in dataset.training_batches():
            if sm is not None:   # mlp_train.py:145-160 on the reference graph
                sm.step(rows(ob_batch, prev_batch, prew_batch), t_batch.reshape(-1, 4))
            else:           # the same feed: the window's recorded teacher pdflat (rows mode)
                tr.step_rows(ob_batch.reshape(-1, OBSPACE_SHAPE), t_batch.reshape(-1, 4))
            opt_steps += 1
        t_pdflat, s_pdflat = query(ob)
        dataset.write(ob=ob, reward=reward, t_pdflat=t_pdflat, s_pdflat=s_pdflat, stepped_with="s")
        ob, reward, new = env.step(s_pdflat)
        if new:
            log("************** Episode {0} ****************".format(dataset.num_episodes()))
            m = (sm.metrics(opt_steps)[:, 0] if sm is not None else tr.metrics(opt_steps)[:, 1]) if opt_steps else []
            total_loss = episode_loss(m)
            log("recent loss: %f " % total_loss)
            losses.append(total_loss)
            done = stop_loss is not None and opt_steps and total_loss / opt_steps < stop_loss
            opt_steps = 0
            dataset.flush()
            if dataset.store is not None and dataset.num_episodes() % 5 == 0:
                dataset.dump()          # mlp_train.py:203
            if dataset.num_episodes() >= episodes or done:
                break
    return (sm or tr), dataset, losses


# -- the reference student distilled on-policy over many envs ----------------------------------
def train_envs(n_envs: int, opt_steps: int, *, keep_prob: float = 1.0, loss: str = "kl", lr: float = 1e-4,
               accum_steps: int = 50, warmup_steps: int = 0, seed: int = 0, teacher=None, device="cuda:0",
               eval_every: int = 0, eval_envs: int = 4096, dtype: str = "f32", replay_capacity: int = 0,
               replay_windows: int = 0, updates_per_act: int = 1, replay_recent: int = 0, beta0: float = 0.0,
               beta_decay: float = 1.0, noise: str = "none", noise_scale: float = 1.0,
               replay_priority: str = "none", faults=None, eval_faults=None):
    """Batched on-policy distillation of the reference student (student_mlp_graph with input dropout
    ``keep_prob``): ``n_envs`` persistent lockstep envs, ``opt_steps`` optimiser steps, each on the
    ``accum_steps`` x n_envs rows of one StudentMlpTrainer.step_envs call (one env launch, the
    training launch and Adam; nothing waits on the GPU between steps).  The first ``warmup_steps``
    optimiser steps are stepped with the teacher's mean (the driver's phase 1), the rest with the
    student's (phase 2, DAgger).  The default accum_steps = 50 puts all 50 episode phases of the
    lockstep envs into every batch -- the role ``stagger`` plays in the fused rollout's config.
    ``teacher``: an MlpPolicyParams (default: the synthetic teacher DistillTrainer defaults to).
    Returns (trainer, history), history rows (optimiser step, loss, action-MSE, mean step reward) with
    the loss of the trainer's metrics ring (the sum over the batch's rows for "kl"), the action-MSE
    the mean over rows and both action dims against the teacher, the reward the mean over the
    batch's env steps.  With ``eval_every`` > 0 returns (trainer, history, evals): evals rows
    (optimiser step, mean return of StudentMlpTrainer.evaluate over ``eval_envs`` fresh envs, one
    episode) after every eval_every-th step -- the reference's average reward per keep_prob.
    ``dtype``: StudentMlpConfig.dtype ("bf16": mixed precision in the env, training and evaluation
    launches alike).
    ``replay_capacity`` > 0 trains from a replay.ReplayRing of that many episodes instead (the aggregate
    of the reference's DAgger loop): each iteration is act_envs (``accum_steps`` env steps, a multiple of
    50, no training), ring.push_rows of its (accum_steps / 50) n_envs episodes, then ``updates_per_act`` x
    { ring.sample_rows(``replay_windows`` rows, recent=``replay_recent``), step }.  History rows stay per
    optimiser step (the reward that of the act call the step followed); an act call is stepped with the
    teacher while the optimiser step it precedes is a warm-up step.
    ``beta0``, ``beta_decay``: DAgger's mixture pi_i = beta_i pi* + (1 - beta_i) pi^_i instead of the hard
    switch at ``warmup_steps``: optimiser step k >= warmup_steps is stepped with the teacher share
    beta = beta0 beta_decay^(k - warmup_steps) (StudentMlpTrainer.set_teacher_share: a coin per env and
    step), exactly 0 once below 2^-24; with a ring an act call takes the beta of the optimiser step it
    precedes, and the records' stepped_with is the per-row flag.  The defaults (beta0 = 0) are the hard
    switch, the same launches as before.
    ``noise``, ``noise_scale``: action noise in every envs call of the run, warm-up steps included
    (StudentMlpTrainer.set_action_noise, keyed by ``seed``): "fixed" with the teacher acting
    (warmup_steps = opt_steps) is DART's noisy expert, "policy" samples whoever acts.  The evaluations
    stay noiseless.  The default "none" is the same launches as before.
    ``replay_priority`` (needs a ring): "record" draws the batches in proportion to the records' priorities
    (ReplayRing.enable_priorities: the student's squared action error against the teacher) instead of
    uniformly; a push writes the priorities from the record's own s_pdflat, the student as it acted, or
    the maximum priority when the teacher stepped the act call (s_pdflat is zero there and says nothing
    about the student).  "refresh" also re-scores every sampled batch with the current student (one
    forward per optimiser step, ReplayRing.update_priorities) before it trains on it.  The default
    "none" is the uniform loop, the same launches as before.
    ``faults``: sensor faults on what the acting student reads in every envs call of the run
    (StudentMlpTrainer.set_obs_faults, keyed by ``seed``), as evaluate's ``faults``: ("dropout" | "missing",
    keep_prob).  The rows it trains on stay clean.  ``eval_faults``: the same for the periodic evaluation
    (StudentMlpTrainer.evaluate(faults=)).  The defaults (None) are the same launches as before."""
    from .policy import synthetic_teacher
    n, steps, K = int(n_envs), int(opt_steps), int(accum_steps)
    if steps < 1 or not 0 <= int(warmup_steps) <= steps:
        raise ValueError("opt_steps >= 1 and 0 <= warmup_steps <= opt_steps")
    if not 0.0 <= float(beta0) <= 1.0 or not 0.0 <= float(beta_decay) <= 1.0:
        raise ValueError("beta0 and beta_decay in [0, 1]")
    cap, Bw, upa = int(replay_capacity), int(replay_windows), int(updates_per_act)
    prio = str(replay_priority)
    if prio not in ("none", "record", "refresh") or (prio != "none" and cap <= 0):
        raise ValueError('replay_priority is "none", "record" or "refresh", and needs replay_capacity > 0')
    if cap < 0 or (cap and (Bw < 1 or upa < 1 or int(replay_recent) < 0 or K < 50 or K % 50 or n * (K // 50) > cap)):
        raise ValueError("with a replay ring: accum_steps a positive multiple of 50, replay_capacity >= "
                         "(accum_steps / 50) n_envs, replay_windows >= 1, updates_per_act >= 1, replay_recent >= 0")
    sm = StudentMlpTrainer(StudentMlpConfig(loss=loss, lr=lr, keep_prob=keep_prob, seed=seed, metrics_len=steps,
                                            dtype=dtype), device=device)
    sm.set_teacher(teacher if teacher is not None else synthetic_teacher(DistillConfig().teacher_seed))
    sm.attach_envs(n, seed=seed, accum_steps=K)
    if noise != "none":
        sm.set_action_noise(noise, noise_scale)
    of = obf.parse(faults, seed)
    if of is not None:
        sm.set_obs_faults(obf.MODE_NAMES[of.mode], of.keep_prob, of.seed)
    rew = torch.zeros(steps, device=sm.device)
    evals = []
    ring = None
    if cap:
        from .replay import ReplayRing
        ring = sm.replay = ReplayRing(cap, device=device, seed=seed, max_batch=Bw)
        if prio != "none":
            ring.enable_priorities(init="record")
    for k in range(steps):
        act_with = "teacher" if k < int(warmup_steps) else "student"
        if beta0 > 0 and act_with == "student" and (ring is None or k % upa == 0):
            sm.set_teacher_share(teacher_share(k, warmup_steps, beta0, beta_decay))
        if ring is None:
            r = sm.step_envs(act_with)
            rew[k] = r.reward.mean()
        else:
            if k % upa == 0:
                r = sm.act_envs(act_with)
                if prio != "none":
                    ring.set_priority_init("const" if act_with == "teacher" else "record")
                ring.push_rows(r, stepped_with=float(act_with == "student") if sm.stepped_with is None
                               else sm.stepped_with)
                mean_reward = r.reward.mean()
            if prio == "none":
                sm.step(*ring.sample_rows(Bw, recent=int(replay_recent)))
            else:
                x, t, idx = ring.sample_rows(Bw, recent=int(replay_recent), with_idx=True, prioritized=True)
                if prio == "refresh":
                    ring.update_priorities(idx, sm.forward(x))
                sm.step(x, t)
            rew[k] = mean_reward
        if eval_every and (k + 1) % int(eval_every) == 0:
            evals.append((k + 1, float(sm.evaluate(int(eval_envs), 1, seed=seed + 1, faults=eval_faults).returns.mean())))
    m = sm.metrics(steps)
    rew = rew.cpu().tolist()
    history = [(k + 1, float(m[k, 0]), float(m[k, 1] / (2 * m[k, 2])), rew[k]) for k in range(steps)]
    return (sm, history, evals) if eval_every else (sm, history)


# -- phase 2 on recorded teacher data (no env) ------------------------------------------------
def _windows(gen, n_eps, lens_ok, count, B=LSTM_BATCH_SIZE, T=STEPS_UNROLLED, device="cuda:0"):
    """[count, T * B] flat record indices of `count` training batches drawn as the reference's
    training_batches (dataset.py:179-194): B episodes with replacement and ONE start per batch,
    T consecutive steps from it."""
    out = torch.empty(count, T, B, dtype=torch.long)
    for k in range(count):   # batch by batch, so the sequence does not depend on how it is chunked
        eps = torch.randint(0, n_eps, (B,), generator=gen)
        start = int(torch.randint(0, EPISODE_STEPS - T + 1, (1,), generator=gen))
        out[k] = eps[None, :] * EPISODE_STEPS + start + torch.arange(T)[:, None]
    return out.reshape(count, T * B).to(device)


def fit_records(ob, t_pdflat, rew=None, *, student: str = "policy", steps: int = 250_000, loss: str = "mse",
                lr: float = 1e-4, seed: int = 0, device="cuda:0", graph_steps: int = 100, log_every: int = 0,
                trainer=None):
    """The reference's phase-2 optimiser steps (mlp_train.py:143-161) on RECORDED teacher data:
    episodes ob [E, 50, 11] with the teacher's pdflat t_pdflat [E, 50, 4] (and rewards [E, 50]
    for the reference student's prev_rew), e.g. the fixture's teacher-stepped episodes.  Each
    step is one Adam step on one training batch of 20 windows x 10 steps (200 rows, drawn as
    dataset.py:179-194 draws them, from a seeded host generator), with the recorded t_pdflat
    as the target (rows mode: no teacher network runs).  student="policy": the 2x64 MlpPolicy
    (DistillTrainer.step_rows), captured `graph_steps` steps per HIP graph with the batch
    indices drawn ahead into a device buffer; student="mlp": the reference graph
    (StudentMlpTrainer.step on rows ob | prev_pdflat | prev_rew).  Returns (trainer, history)
    with history = [(step, mean training action-MSE of the last steps)] every `log_every`."""
    ob = torch.as_tensor(ob, dtype=torch.float32)
    tp = torch.as_tensor(t_pdflat, dtype=torch.float32)
    E = ob.shape[0]
    dev = torch.device(device)
    ob_all = ob.reshape(-1, OBSPACE_SHAPE).to(dev).contiguous()
    t_all = tp.reshape(-1, 4).to(dev).contiguous()
    gen = torch.Generator().manual_seed(int(seed))
    history = []
    if student == "policy":
        tr = trainer or DistillTrainer(DistillConfig(n_envs=64, seed=seed, loss=loss, lr=lr, metrics_len=graph_steps),
                                       device=device)
        rows_per = LSTM_BATCH_SIZE * STEPS_UNROLLED
        idx_buf = torch.zeros(graph_steps, rows_per, dtype=torch.long, device=dev)
        ob_buf = torch.zeros(graph_steps, rows_per, OBSPACE_SHAPE, device=dev)
        t_buf = torch.zeros(graph_steps, rows_per, 4, device=dev)
        g = torch.cuda.CUDAGraph()
        prev = torch.cuda.current_stream(dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.graph(g):
            tr.set_stream(torch.cuda.current_stream(dev))
            torch.index_select(ob_all, 0, idx_buf.reshape(-1), out=ob_buf.reshape(-1, OBSPACE_SHAPE))
            torch.index_select(t_all, 0, idx_buf.reshape(-1), out=t_buf.reshape(-1, 4))
            for k in range(graph_steps):
                nat.check(tr._lib.rdd_step_rows(tr._h, nat.ptr(ob_buf[k]), nat.ptr(t_buf[k]), rows_per),
                          "rdd_step_rows")
        tr.set_stream(prev)
        done = 0
        while done + graph_steps <= steps:
            idx_buf.copy_(_windows(gen, E, None, graph_steps, device=dev))
            g.replay()
            done += graph_steps
            tr.steps += graph_steps
            if log_every and done % log_every < graph_steps:
                m = tr.metrics(graph_steps)
                history.append((done, float((m[:, 2] / (2 * m[:, 3])).mean())))
        if done < steps:   # the last steps % graph_steps steps eagerly: exactly `steps` Adam steps
            for i in _windows(gen, E, None, steps - done, device=dev):
                tr.step_rows(ob_all[i], t_all[i])
            done = steps
        torch.cuda.synchronize(dev)
        return tr, history
    if student != "mlp":
        raise ValueError(f"unknown student {student!r}")
    r = torch.zeros(E, EPISODE_STEPS) if rew is None else torch.as_tensor(rew, dtype=torch.float32)
    prev_t = torch.zeros_like(tp)
    prev_t[:, 1:] = tp[:, :-1]
    prev_r = torch.zeros(E, EPISODE_STEPS, 1)
    prev_r[:, 1:, 0] = r[:, :-1]
    x_all = rows(ob, prev_t, prev_r).to(dev)
    sm = trainer or StudentMlpTrainer(StudentMlpConfig(loss=loss, lr=lr, seed=seed), device=device)
    done = 0
    while done < steps:
        for i in _windows(gen, E, None, min(graph_steps, steps - done), device=dev):
            sm.step(x_all[i], t_all[i])
        done += min(graph_steps, steps - done)
        if log_every and done % log_every < graph_steps:
            m = sm.metrics(min(graph_steps, done))
            history.append((done, float((m[:, 1] / (2 * m[:, 2])).mean())))
    torch.cuda.synchronize(dev)
    return sm, history


def action_mse(trainer, ob, t_pdflat, rew=None) -> float:
    """mean over records and both action dims of (mu_student - mu_teacher)^2 on recorded
    episodes ob [E, 50, 11] / t_pdflat [E, 50, 4] (the reference LSTM student's
    0.0212 on the fixture's episodes 21-24 is this quantity)."""
    ob = torch.as_tensor(ob, dtype=torch.float32)
    tp = torch.as_tensor(t_pdflat, dtype=torch.float32)
    dev = trainer.device
    if isinstance(trainer, DistillTrainer):
        _, s = trainer.forward(ob.reshape(-1, OBSPACE_SHAPE).to(dev), teacher=False)
    else:
        E = ob.shape[0]
        r = torch.zeros(E, EPISODE_STEPS) if rew is None else torch.as_tensor(rew, dtype=torch.float32)
        prev_t = torch.zeros_like(tp)
        prev_t[:, 1:] = tp[:, :-1]
        prev_r = torch.zeros(E, EPISODE_STEPS, 1)
        prev_r[:, 1:, 0] = r[:, :-1]
        s = trainer.forward(rows(ob, prev_t, prev_r).to(dev))
    d = s[:, :2].double().cpu() - tp.reshape(-1, 4)[:, :2].double()
    return float((d ** 2).mean())
