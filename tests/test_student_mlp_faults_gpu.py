"""Sensor faults on the reference MLP student's observation in the closed loop (rdm_envs_set_obs_faults,
rdm_evaluate_faulty, rd_mask_obs; StudentMlpTrainer.set_obs_faults, evaluate(faults=)) against the
stepwise loop { rdd_forward (teacher, clean ob), rd_mask_obs, rows on the masked ob, rdm_forward,
[rd_perturb_actions], rd_step } -- tests/test_student_mlp_envs_mix_gpu's MixedStepwise with the student's
row built from obs_faults.mask_obs of the observation.  rd_mask_obs runs the device functions the fused
kernels inline and every other piece is the plain loop's, so every comparison is bitwise (torch.equal):
a difference is a reordering to find, not a tolerance to add.  keep_prob = 0.5; envs in {1, 17, 83}: one
env, a ragged 16-block, a full 64-block plus a ragged one (grid = 1) or six 16-blocks; 100 lockstep steps,
so one reset is crossed.  Default synthetic teacher, glorot students."""
import pytest
import torch

from tests import envs_mix
from tests import obs_faults as of
from tests.test_student_mlp_envs_mix_gpu import STEPS, MixedStepwise, _cat, _student, tr   # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEEP = of.KEEP
SEED, BASE, FIRST = 11, 5, 3
F_REW, F_T, F_S, F_WITH = 11, 12, 16, 20
NAMES = ("x", "t_pdflat", "s_pdflat", "reward", "stepped_with", "actions")


def _keep(sm, r):
    """x, t_pdflat, s_pdflat, reward, stepped_with, actions of the call's steps"""
    K = r.x.shape[0]
    return tuple(v.clone() for v in (r.x, r.t_pdflat, r.s_pdflat, r.reward, sm.stepped_with[:K], sm.actions[:K]))


class FaultyStepwise(MixedStepwise):
    """MixedStepwise under sensor faults: the student's forward runs on the row whose observation went
    through rd_mask_obs at (mask seed, env_base + i, episode, step); the teacher reads the clean
    observation and x is the clean row.  The acting pdflat -- the student's, or the teacher's where the
    NumPy coin fell -- goes through rd_perturb_actions (mode "none": its mean) and steps the env."""

    def __init__(self, tr, sm, n, seed, env_base, mode, keep_prob=KEEP, beta=0.0, noise="none", scale=1.0):   # noqa: F811
        super().__init__(tr, sm, n, seed, env_base, beta=beta)
        self.seed, self.mode, self.keep_prob, self.noise, self.scale = seed, mode, keep_prob, noise, scale

    def steps(self, K):
        """(x [K, n, 16], t_pdflat, s_pdflat [K, n, 4], reward, stepped_with [K, n], actions [K, n, 2])"""
        from reacherdistilation_amd.action_noise import perturb_actions
        from reacherdistilation_amd.obs_faults import mask_obs
        from reacherdistilation_amd.student_mlp import rows
        n, out = self.n, []
        for _ in range(K):
            ep, s = self.g // STEPS, self.g % STEPS
            t, _ = self.tr.forward(self.ob, teacher=True, student=False)
            pt = torch.zeros_like(self.prev_t) if s == 0 else self.prev_t
            pr = torch.zeros_like(self.prev_r) if s == 0 else self.prev_r
            x = rows(self.ob, pt, pr)
            seen = mask_obs(self.ob, mode=self.mode, keep_prob=self.keep_prob, seed=self.seed, env_base=self.base,
                            episode=ep, step=s)
            sf = self.sm.forward(rows(seen, pt, pr))
            coin = torch.from_numpy(envs_mix.teacher_coins(self.coin_seed, self.base, n, ep, s, self.beta)).to(DEV)
            acting = torch.where(coin[:, None], t, sf)
            act = perturb_actions(acting, mode=self.noise, scale=self.scale, seed=self.seed, env_base=self.base,
                                  episode=ep, step=s)
            self.prev_t, self.prev_r = t.clone(), self.reward.clone().view(n, 1)   # this record's fields
            ob, rew, _, _ = self.env.step(act)
            self.ob, self.reward = ob.clone(), rew.clone()
            self.g += 1
            out.append((x, t.clone(), sf, self.reward, (~coin).float(), act))
        return tuple(torch.stack([o[j] for o in out]) for j in range(6))


def stepwise_evaluate(tr, student, env, episodes, shadow, faults, noise, lstm):   # noqa: F811
    """The loop the faulty evaluations fuse, on ``env`` (its next reset opens the run's first episode):
    (returns [E, n], final distance [E, n], records [E, n, 50, 21], the LSTM's final state or None).
    ``faults`` = (mode, keep_prob, seed, env_base, first_episode); ``noise`` = (mode, scale, seed).  The
    MLP's row, and every record of the LSTM's window, carries the observation masked at its own (episode,
    step); the records keep the clean one."""
    from reacherdistilation_amd.action_noise import perturb_actions
    from reacherdistilation_amd.obs_faults import mask_obs
    from reacherdistilation_amd.student_mlp import rows
    fmode, keep_prob, fseed, base, first = faults
    nmode, scale, nseed = noise
    n, T = env.n, getattr(student, "T", 0)
    ob = env.reset()
    reward = torch.zeros(n, device=DEV)
    zero = torch.zeros(n, 2, device=DEV)
    rets, dists, state = [], [], None
    rec = torch.zeros(episodes, STEPS, n, 21, device=DEV)
    for e in range(episodes):
        ret = torch.zeros(n, dtype=torch.float32, device=DEV)
        obs, prevs = [], []
        for s in range(STEPS):
            t, _ = tr.forward(ob, teacher=True, student=False)
            prev_t = rec[e, s - 1, :, F_T:F_S].clone() if s else torch.zeros(n, 4, device=DEV)
            seen = mask_obs(ob, mode=fmode, keep_prob=keep_prob, seed=fseed, env_base=base, episode=first + e, step=s)
            if lstm:
                obs.append(seen.clone())
                prevs.append(prev_t)
                k = min(s + 1, T)
                ob_w, prev_w = torch.zeros(T, n, 11, device=DEV), torch.zeros(T, n, 4, device=DEV)
                ob_w[T - k:] = torch.stack(obs[-k:])
                prev_w[T - k:] = torch.stack(prevs[-k:])
                out, state = student.forward(ob_w, prev_w, state)
                sf = out[T - 1]
            else:
                prev_r = rec[e, s - 1, :, F_REW].clone().view(n, 1) if s else torch.zeros(n, 1, device=DEV)
                sf = student.forward(rows(seen, prev_t, prev_r))
            act = perturb_actions(sf, mode=nmode, scale=scale, seed=nseed, env_base=base, episode=first + e, step=s)
            r = rec[e, s]
            r[:, :F_REW] = ob
            r[:, F_REW] = reward
            r[:, F_T:F_S] = t
            r[:, F_S:F_WITH] = sf
            r[:, F_WITH] = 1.0
            if s == STEPS - 1:
                es, _, _ = env.get_state()
                shadow.set_state(es, step=0, episode=0)
                shadow.step(act)
                dists.append((-shadow.step(zero)[1]).clone())
            ob, rew, _, _ = env.step(act)
            ret = ret + rew
            reward = rew.clone()
        rets.append(ret)
    return torch.stack(rets), torch.stack(dists), rec.transpose(1, 2).contiguous(), state


def evaluate_case(tr, student, n, table, fmode, noise, lstm, fseed=None):   # noqa: F811
    """(the fused result, the stepwise reference) of one faulty evaluation over 2 episodes"""
    from reacherdistilation_amd.env import BatchedReacher
    from reacherdistilation_amd.evaluate import gym_draw_table
    kw = dict(final_dist=True, records=True, noise=noise, noise_scale=1.0, noise_seed=9,
              faults=(fmode, KEEP) if fseed is None else dict(mode=fmode, keep_prob=KEEP, seed=fseed))
    if lstm:
        kw["final_state"] = True
    key = SEED if fseed is None else fseed
    if table:   # gym draws: env_base = 0, first_episode = 0
        env = BatchedReacher(n, seed=SEED, device=DEV, reset="gym")
        res = student.evaluate(n, 2, seed=SEED, draws=gym_draw_table(SEED, n, 2), **kw)
        where = (0, 0)
    else:
        env = BatchedReacher(n, seed=SEED, device=DEV, env_base=BASE)
        for _ in range(FIRST):
            env.reset()   # each reset opens the next Philox episode
        res = student.evaluate(n, 2, seed=SEED, env_base=BASE, first_episode=FIRST, **kw)
        where = (BASE, FIRST)
    shadow = BatchedReacher(n, device=DEV)
    ref = stepwise_evaluate(tr, student, env, 2, shadow, (fmode, KEEP, key, *where), (noise, 1.0, 9), lstm)
    torch.cuda.synchronize()
    env.close()
    shadow.close()
    return res, ref


def same_evaluation(res, ref):
    ret, dist, rec, state = ref
    assert torch.equal(res.records, rec)
    assert torch.equal(res.returns, ret)
    assert torch.equal(res.final_dist, dist)
    if state is not None:
        assert torch.equal(res.state, state)


# ---------------------------------------------------------------- evaluate
# (n, dtype, mode, noise, draws table): both dtypes x both modes x noise on / off, every block shape
EVALS = [(1, "f32", "dropout", "none", False), (17, "f32", "missing", "policy", True),
         (83, "f32", "dropout", "policy", False), (83, "f32", "missing", "none", False),
         (17, "bf16", "dropout", "none", False), (83, "bf16", "missing", "policy", False),
         (1, "bf16", "dropout", "policy", True), (17, "bf16", "missing", "none", False)]


@pytest.mark.parametrize("n,dtype,mode,noise,table", EVALS)
def test_faulty_evaluation_equals_the_stepwise_loop(tr, n, dtype, mode, noise, table):   # noqa: F811
    """evaluate(faults=(mode, 0.5)) over 2 episodes: records, returns and final_dist of the stepwise loop,
    bit for bit; the records' ob is the clean one; the returns differ from the clean evaluation's."""
    sm = _student(tr, dtype=dtype)
    res, ref = evaluate_case(tr, sm, n, table, mode, noise, lstm=False, fseed=None if n != 17 else 21)
    same_evaluation(res, ref)
    kw = dict(seed=SEED, noise=noise, noise_seed=9, records=True)
    if table:
        from reacherdistilation_amd.evaluate import gym_draw_table
        kw["draws"] = gym_draw_table(SEED, n, 2)
    else:
        kw.update(env_base=BASE, first_episode=FIRST)
    clean = sm.evaluate(n, 2, **kw)
    assert not torch.equal(clean.returns, res.returns)   # the mask bites
    assert torch.equal(clean.records[0, :, 0, :F_S], res.records[0, :, 0, :F_S])   # step 0: ob, reward field, T_0
    assert not torch.equal(clean.records[0, :, 0, F_S:F_WITH], res.records[0, :, 0, F_S:F_WITH])   # S_0 read the mask
    sm.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_evaluation_end_points_and_grid(tr, dtype):   # noqa: F811
    """keep_prob = 1 under either mode is the plain (or the noisy) evaluation bit for bit: the same
    arithmetic.  n = 83 on one workgroup (64-env blocks) equals the automatic grid (16-env blocks).  The
    envs' set_obs_faults is never read by evaluate()."""
    sm = _student(tr, dtype=dtype)
    kw = dict(seed=SEED, env_base=BASE, first_episode=FIRST, final_dist=True, records=True)
    for noise in ("none", "policy"):
        plain = sm.evaluate(83, 2, noise=noise, **kw)
        for mode in ("dropout", "missing"):
            one = sm.evaluate(83, 2, noise=noise, faults=(mode, 1.0), **kw)
            assert torch.equal(one.returns, plain.returns) and torch.equal(one.final_dist, plain.final_dist)
            assert torch.equal(one.records, plain.records)
    a = sm.evaluate(83, 2, grid=1, faults=("dropout", KEEP), noise="policy", **kw)
    b = sm.evaluate(83, 2, faults=("dropout", KEEP), noise="policy", **kw)
    assert torch.equal(a.returns, b.returns) and torch.equal(a.final_dist, b.final_dist) and torch.equal(a.records, b.records)
    plain = sm.evaluate(17, 1, **kw)
    sm.set_obs_faults("missing", KEEP)
    sm.attach_envs(17, seed=SEED, accum_steps=7)
    sm.act_envs()
    again = sm.evaluate(17, 1, **kw)
    assert torch.equal(plain.returns, again.returns) and torch.equal(plain.records, again.records)
    assert sm.obs_faults() == dict(mode="missing", keep_prob=KEEP, seed=SEED)
    sm.close()


# ---------------------------------------------------------------- the envs calls
# (n, dtype, mode, beta, noise): both dtypes x both betas x noise on / off, both modes, every block shape
RUNS = [(1, "f32", "dropout", 0.0, "none"), (17, "f32", "missing", 0.5, "policy"),
        (83, "f32", "dropout", 0.5, "none"), (83, "f32", "missing", 0.0, "policy"),
        (17, "bf16", "dropout", 0.0, "policy"), (83, "bf16", "missing", 0.5, "none"),
        (1, "bf16", "missing", 0.5, "policy"), (17, "bf16", "dropout", 0.0, "none")]


@pytest.mark.parametrize("n,dtype,mode,beta,noise", RUNS)
def test_faulty_run_equals_the_stepwise_loop(tr, n, dtype, mode, beta, noise):   # noqa: F811
    """act_envs over 100 steps as one K = 100 call on the automatic grid, and as 30 + 70 on one workgroup
    (grid = 1: 64-env blocks): x (clean), both pdflats, the rewards, stepped_with and the actions are the
    stepwise loop's bit for bit, and so is the env state -- whatever the split and the grid."""
    assert (SEED, BASE, n, 2 * STEPS) in of.RUNS
    sm = _student(tr, dtype=dtype)
    loop = FaultyStepwise(tr, sm, n, SEED, BASE, mode, beta=beta, noise=noise)
    want = loop.steps(2 * STEPS)
    sm.set_obs_faults(mode, KEEP)   # before the attach: the mask takes the envs' seed when it comes
    sm.set_teacher_share(beta)
    sm.set_action_noise(noise, 1.0)
    for calls, grid in (((100,), 0), ((30, 70), 1)):
        sm.attach_envs(n, seed=SEED, env_base=BASE, accum_steps=2 * STEPS, grid=grid, flags=True, actions=True)
        assert sm.obs_faults() == dict(mode=mode, keep_prob=KEEP, seed=SEED)
        got = _cat([_keep(sm, sm.act_envs(steps=K)) for K in calls])
        for name, g, w in zip(NAMES, got, want):
            assert torch.equal(g, w), (calls, name)
        st, step, episode = loop.env.get_state()
        gs, gstep, gep = sm.env_state()
        assert torch.equal(gs, st) and (gstep, gep) == (step, episode) == (0, 2)
    if beta > 0:
        assert 0 < float(want[4].mean()) < 1   # both actors stepped
    loop.close()
    sm.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_mask_is_applied_and_only_to_what_the_student_reads(tr, dtype):   # noqa: F811
    """At keep_prob = 0.5 the trajectory differs from the clean call's for at least one env, while x and
    t_pdflat at step 0 -- the clean observation and the teacher on it -- equal the clean call's and
    s_pdflat at step 0 does not.  keep_prob = 1 under either mode is the plain call bit for bit.  With the
    teacher acting, the faults set change nothing at all."""
    n, K = 83, 2 * STEPS
    plain, faulty = _student(tr, dtype=dtype), _student(tr, dtype=dtype)
    for sm in (plain, faulty):
        sm.attach_envs(n, seed=SEED, env_base=BASE, accum_steps=K)
    rp = plain.act_envs()
    for mode in ("dropout", "missing"):
        faulty.set_obs_faults(mode, KEEP)
        faulty.reset_envs()
        rf = faulty.act_envs()
        assert torch.equal(rf.x[0], rp.x[0]) and torch.equal(rf.t_pdflat[0], rp.t_pdflat[0]), mode
        assert not torch.equal(rf.s_pdflat[0], rp.s_pdflat[0]), mode
        assert bool((rf.reward != rp.reward).any(dim=0).any()), mode
        assert not torch.equal(rf.x[1], rp.x[1]), mode
        faulty.set_obs_faults(mode, 1.0)   # the same arithmetic
        faulty.reset_envs()
        rf = faulty.act_envs()
        for name in ("x", "t_pdflat", "s_pdflat", "reward"):
            assert torch.equal(getattr(rf, name), getattr(rp, name)), (mode, name)
        assert torch.equal(faulty.env_state()[0], plain.env_state()[0])
    faulty.set_obs_faults("missing", KEEP)
    for sm in (plain, faulty):
        sm.reset_envs()
    rp, rf = plain.act_envs("teacher"), faulty.act_envs("teacher")
    for name in ("x", "t_pdflat", "s_pdflat", "reward"):
        assert torch.equal(getattr(rf, name), getattr(rp, name)), name
    assert torch.equal(faulty.env_state()[0], plain.env_state()[0])
    faulty.set_obs_faults("none")   # set back: the plain student call again
    rp, rf = plain.act_envs(), faulty.act_envs()
    for name in ("x", "t_pdflat", "s_pdflat", "reward"):
        assert torch.equal(getattr(rf, name), getattr(rp, name)), name
    plain.close()
    faulty.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_step_envs_equals_the_stepwise_loop_then_step_on_the_clean_rows(tr, dtype):   # noqa: F811
    """step_envs under faults, policy noise and beta = 0.5, (n, K, optimiser steps) = (83, 7, 8), against a
    twin stepped stepwise and trained with step on the K n CLEAN rows (its own keep_prob = 0.5 dropout):
    after every step the parameters, gradient, counter and metrics are equal bit for bit."""
    import numpy as np
    n, K, opt_steps = 83, 7, 8
    cfg = dict(loss="kl", lr=1e-3, keep_prob=0.5, seed=4, dtype=dtype)
    fused, twin = _student(tr, **cfg), _student(tr, **cfg)
    fused.attach_envs(n, seed=SEED, env_base=BASE, accum_steps=K, flags=True, actions=True)
    fused.set_teacher_share(0.5)
    fused.set_action_noise("policy", 1.0)
    fused.set_obs_faults("dropout", KEEP)
    loop = FaultyStepwise(tr, twin, n, SEED, BASE, "dropout", beta=0.5, noise="policy")
    for k in range(opt_steps):
        r = fused.step_envs()
        x, t, s, rew, flags, act = loop.steps(K)
        assert torch.equal(r.x, x) and torch.equal(r.t_pdflat, t) and torch.equal(r.s_pdflat, s), k
        assert torch.equal(r.reward, rew) and torch.equal(fused.stepped_with, flags), k
        assert torch.equal(fused.actions, act), k
        twin.step(x.reshape(-1, 16), t.reshape(-1, 4))
        assert torch.equal(fused.params(), twin.params()), k
        assert torch.equal(fused.grad(), twin.grad()), k
        assert fused.counter() == twin.counter() == k + 1
        assert np.array_equal(fused.metrics(1), twin.metrics(1)), k
    st, step, episode = loop.env.get_state()
    gs, gstep, gep = fused.env_state()
    assert torch.equal(gs, st) and (gstep, gep) == (step, episode) == (6, 1)
    loop.close()
    fused.close()
    twin.close()


def test_a_captured_call_replays_the_next_steps_mask_and_keeps_its_setting(tr):   # noqa: F811
    """act_envs under faults (n = 83, K = 7) captured and replayed twice equals two eager calls on a twin:
    the clock is the device's, so the replays draw the next steps' mask; and the faults are kernel
    arguments -- set to "none" after the capture, the replays are still the faulty calls."""
    a, b = _student(tr), _student(tr)
    for sm in (a, b):
        sm.attach_envs(83, seed=SEED, env_base=BASE, accum_steps=7)
        sm.set_obs_faults("missing", KEEP, seed=9)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(a.device)
    with torch.cuda.graph(g):
        res = a.act_envs()
    a._sync_stream()
    a.set_obs_faults("none")
    for _ in range(2):
        g.replay()
    b.act_envs()
    want = b.act_envs()
    torch.cuda.synchronize(a.device)
    for name in ("x", "t_pdflat", "s_pdflat", "reward"):
        assert torch.equal(getattr(res, name), getattr(want, name)), name
    (sa, ka, ea), (sb, kb, eb) = a.env_state(), b.env_state()
    assert torch.equal(sa, sb) and (ka, ea) == (kb, eb) == (14, 0)
    a.close()
    b.close()
