"""Sensor faults on the LSTM student's observations in the closed loop (rdl_envs_set_obs_faults,
rdl_evaluate_faulty, rd_mask_obs; StudentLstmTrainer.set_obs_faults, evaluate(faults=)) against the
stepwise loop of tests/test_student_lstm_envs_gpu.py -- the teacher's forward on the clean observation,
the window of the episode's last T records with every record's observation passed through
obs_faults.mask_obs (rd_mask_obs: the device functions the fused kernels inline) at the record's OWN
(episode, step), forward from the carried (c, h), [rd_perturb_actions], env.step.  Every comparison is
bitwise (torch.equal): a difference is a reordering to find, not a tolerance to add.  keep_prob = 0.5;
envs in {1, 17, 83}; 100 lockstep steps, so one reset is crossed; T in {3, 10}; the f32 query, and a bf16
handle with query_dtype = "bf16".  Default synthetic teacher, that suite's parameters."""
import pytest
import torch

from tests import envs_mix
from tests import obs_faults as of
from tests.test_student_lstm_envs_gpu import STEPS, Stepwise, _host_windows, _student, tr   # noqa: F401
from tests.test_student_mlp_faults_gpu import evaluate_case, same_evaluation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEEP = of.KEEP
SEED, BASE, FIRST = 11, 5, 3
F_REW, F_T, F_S, F_WITH = 11, 12, 16, 20
DTYPES = {"f32": {}, "bf16": dict(dtype="bf16", query_dtype="bf16")}


class FaultyStepwise(Stepwise):
    """Stepwise under sensor faults: the loop keeps the clean observations of the open episode and the
    global step each was recorded at; a query's window holds, for each of its records, rd_mask_obs of that
    observation at (mask seed, env_base + i, the record's episode, the record's step) -- so a record
    carries one mask at every position and in every later query that holds it.  The acting pdflat -- the
    student's, the teacher's in a "teacher" run (no query) or where the NumPy coin fell -- goes through
    rd_perturb_actions (mode "none": its mean) and steps the env.  The records keep the clean
    observation."""

    def __init__(self, tr, st, n, seed, env_base, mode, keep_prob=KEEP, beta=0.0, noise="none"):   # noqa: F811
        super().__init__(tr, st, n, seed, env_base)
        self.seed, self.base, self.mode, self.keep_prob, self.beta, self.noise, self.g = \
            seed, env_base, mode, keep_prob, beta, noise, 0
        self.at = []   # the global step of each kept observation

    def steps(self, K, act_with="student"):
        """(records [K, n, 21], reward [K, n]) of the next K steps."""
        from reacherdistilation_amd.action_noise import perturb_actions
        from reacherdistilation_amd.obs_faults import mask_obs
        n, T, recs, rews = self.n, self.st.T, [], []
        for _ in range(K):
            t, _ = self.tr.forward(self.ob, teacher=True, student=False)
            self.obs.append(self.ob.clone())
            self.at.append(self.g)
            self.prevs.append(self.prev_t.clone() if self.s else torch.zeros(n, 4, device=DEV))
            if act_with == "student":
                k = min(self.s + 1, T)
                ob_w, prev_w = torch.zeros(T, n, 11, device=DEV), torch.zeros(T, n, 4, device=DEV)
                ob_w[T - k:] = torch.stack([mask_obs(o, mode=self.mode, keep_prob=self.keep_prob, seed=self.seed,
                                                     env_base=self.base, episode=g // STEPS, step=g % STEPS)
                                            for o, g in zip(self.obs[-k:], self.at[-k:])])
                prev_w[T - k:] = torch.stack(self.prevs[-k:])
                out, self.state = self.st.forward(ob_w, prev_w, self.state)
                sf = out[T - 1].clone()
                coin = torch.from_numpy(envs_mix.teacher_coins(self.seed, self.base, n, self.g // STEPS, self.s,
                                                               self.beta)).to(DEV)
                acting, flags = torch.where(coin[:, None], t, sf), (~coin).float()
            else:
                sf, acting, flags = torch.zeros(n, 4, device=DEV), t, torch.zeros(n, device=DEV)
            r = torch.zeros(n, 21, device=DEV)
            r[:, :F_REW] = self.ob
            r[:, F_REW] = self.reward
            r[:, F_T:F_S] = t
            r[:, F_S:F_WITH] = sf
            r[:, F_WITH] = flags
            act = perturb_actions(acting, mode=self.noise if act_with == "student" else "none", scale=1.0, seed=self.seed,
                                  env_base=self.base, episode=self.g // STEPS, step=self.s)
            self.prev_t = t.clone()
            ob, rew, _, _ = self.env.step(act)
            self.ob, self.reward = ob.clone(), rew.clone()
            self.s = (self.s + 1) % STEPS
            self.g += 1
            if self.s == 0:
                self.obs, self.prevs, self.at = [], [], []
            recs.append(r)
            rews.append(self.reward)
        return torch.stack(recs), torch.stack(rews)


def _same_envs(st, loop, clock):
    es, step, episode = loop.env.get_state()
    gs, gstep, gep = st.env_state()
    assert torch.equal(gs, es) and (gstep, gep) == (step, episode) == clock
    assert torch.equal(st.query_state(), loop.query_state())


# ---------------------------------------------------------------- evaluate
# (n, T, dtype, mode, noise, draws table): both T x both queries, both modes, noise on / off
EVALS = [(1, 10, "f32", "dropout", "none", False), (17, 3, "f32", "missing", "policy", True),
         (83, 10, "f32", "missing", "policy", False), (17, 10, "bf16", "dropout", "policy", False),
         (83, 3, "bf16", "missing", "none", False), (17, 3, "f32", "dropout", "none", False)]


@pytest.mark.parametrize("n,T,dtype,mode,noise,table", EVALS)
def test_faulty_evaluation_equals_the_stepwise_loop(tr, n, T, dtype, mode, noise, table):   # noqa: F811
    """evaluate(faults=(mode, 0.5)) over 2 episodes: records, returns, final_dist and the final (c, h) of
    the stepwise loop, bit for bit; the records' ob is the clean one; the returns differ from the clean
    evaluation's while step 0's ob and T_0 do not."""
    st = _student(tr, T=T, max_windows=n, **DTYPES[dtype])
    res, ref = evaluate_case(tr, st, n, table, mode, noise, lstm=True, fseed=None if n != 17 else 21)
    same_evaluation(res, ref)
    kw = dict(seed=SEED, noise=noise, noise_seed=9, records=True)
    if table:
        from reacherdistilation_amd.evaluate import gym_draw_table
        kw["draws"] = gym_draw_table(SEED, n, 2)
    else:
        kw.update(env_base=BASE, first_episode=FIRST)
    clean = st.evaluate(n, 2, **kw)
    assert not torch.equal(clean.returns, res.returns)   # the mask bites
    assert torch.equal(clean.records[0, :, 0, :F_S], res.records[0, :, 0, :F_S])
    assert not torch.equal(clean.records[0, :, 0, F_S:F_WITH], res.records[0, :, 0, F_S:F_WITH])
    st.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_evaluation_end_points_and_grid(tr, dtype):   # noqa: F811
    """keep_prob = 1 under either mode is the plain (or the noisy) evaluation bit for bit; n = 83 on one
    workgroup, which walks the six blocks, equals the automatic grid; evaluate() never reads the envs'
    set_obs_faults."""
    st = _student(tr, T=10, max_windows=83, **DTYPES[dtype])
    kw = dict(seed=SEED, env_base=BASE, first_episode=FIRST, final_dist=True, records=True, final_state=True)

    def same(a, b):
        assert torch.equal(a.returns, b.returns) and torch.equal(a.final_dist, b.final_dist)
        assert torch.equal(a.records, b.records) and torch.equal(a.state, b.state)

    for noise in ("none", "policy"):
        plain = st.evaluate(83, 1, noise=noise, **kw)
        for mode in ("dropout", "missing"):
            same(st.evaluate(83, 1, noise=noise, faults=(mode, 1.0), **kw), plain)
    same(st.evaluate(83, 2, grid=1, faults=("dropout", KEEP), noise="policy", **kw),
         st.evaluate(83, 2, faults=("dropout", KEEP), noise="policy", **kw))
    plain = st.evaluate(17, 1, **kw)
    st.set_obs_faults("missing", KEEP)
    st.attach_envs(17, seed=SEED, accum_steps=7)
    st.act_envs(steps=7)
    same(st.evaluate(17, 1, **kw), plain)
    assert st.obs_faults() == dict(mode="missing", keep_prob=KEEP, seed=SEED)
    st.close()


# ---------------------------------------------------------------- the envs calls
# (n, T, dtype, mode, beta, noise): both T x both queries, both betas, noise on / off, both modes
RUNS = [(1, 10, "f32", "dropout", 0.5, "policy"), (17, 3, "f32", "missing", 0.0, "none"),
        (83, 10, "f32", "missing", 0.5, "none"), (17, 10, "bf16", "dropout", 0.0, "policy"),
        (83, 3, "bf16", "missing", 0.5, "policy"), (17, 3, "bf16", "dropout", 0.5, "none"),
        (17, 10, "f32", "dropout", 0.0, "none")]


@pytest.mark.parametrize("n,T,dtype,mode,beta,noise", RUNS)
def test_faulty_run_equals_the_stepwise_loop(tr, n, T, dtype, mode, beta, noise):   # noqa: F811
    """act_envs over 100 steps as one K = 100 call on the automatic grid, and as 30 + 70 on one workgroup
    (grid = 1, which walks the blocks): all 21 columns of the records (clean ob), the rewards, (c, h) and
    the env state are the stepwise loop's bit for bit.  The 30 + 70 split puts a call boundary inside an
    episode, whose first windows reach into the records of the call before, and the 70 cross the reset:
    the older records of a window keep the mask of their own (episode, step) over both.  The three window
    buffers of the K = 100 call are the host gather of the CLEAN records: ob_w is what a clean call on this
    trajectory would write."""
    assert (SEED, BASE, n, 2 * STEPS) in of.RUNS
    B = n * 2 * (51 - T)
    st = _student(tr, T=T, max_windows=B, **DTYPES[dtype])
    loop = FaultyStepwise(tr, st, n, SEED, BASE, mode, beta=beta, noise=noise)
    wrec, wrew = loop.steps(2 * STEPS)
    st.set_obs_faults(mode, KEEP)   # before the attach: the mask takes the envs' seed when it comes
    st.set_teacher_share(beta)
    st.set_action_noise(noise, 1.0)
    for calls, grid in (((100,), 0), ((30, 70), 1)):
        st.attach_envs(n, seed=SEED, env_base=BASE, accum_steps=2 * STEPS, grid=grid)
        assert st.obs_faults() == dict(mode=mode, keep_prob=KEEP, seed=SEED)
        recs, rews = [], []
        for K in calls:
            r = st.act_envs(steps=K)
            recs.append(r.records.clone())
            rews.append(r.reward.clone())
            if K == 2 * STEPS:
                ob_w, prev_w, t_w, ends = _host_windows(wrec, T)
                assert len(ends) == 2 * (51 - T)
                assert torch.equal(r.ob_w, ob_w) and torch.equal(r.prev_w, prev_w) and torch.equal(r.t_w, t_w)
        assert torch.equal(torch.cat(recs), wrec), calls
        assert torch.equal(torch.cat(rews), wrew), calls
        _same_envs(st, loop, (0, 2))
    if beta > 0:
        assert 0 < float(wrec[..., F_WITH].mean()) < 1   # both actors stepped
    loop.close()
    st.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_mask_is_applied_and_only_to_what_the_student_reads(tr, dtype):   # noqa: F811
    """At keep_prob = 0.5 the trajectory differs from the clean call's, while record 0 -- the clean
    observation, the carried reward, the teacher on it -- equals the clean call's and S_0 does not.
    keep_prob = 1 under either mode is the plain call bit for bit, windows and (c, h) included.  With the
    teacher acting, the faults set change nothing at all; set back to "none", neither do they."""
    n, T = 17, 10
    plain, faulty = (_student(tr, T=T, max_windows=n * 41, **DTYPES[dtype]) for _ in range(2))
    for st in (plain, faulty):
        st.attach_envs(n, seed=SEED, env_base=BASE, accum_steps=STEPS)

    def same(ra, rb):
        for name in ("records", "reward", "ob_w", "prev_w", "t_w"):
            assert torch.equal(getattr(ra, name), getattr(rb, name)), name
        assert torch.equal(faulty.query_state(), plain.query_state())
        assert torch.equal(faulty.env_state()[0], plain.env_state()[0])

    rp = plain.act_envs()
    for mode in ("dropout", "missing"):
        faulty.set_obs_faults(mode, KEEP)
        faulty.attach_envs(n, seed=SEED, env_base=BASE, accum_steps=STEPS)
        rf = faulty.act_envs()
        assert torch.equal(rf.records[0, :, :F_S], rp.records[0, :, :F_S]), mode
        assert not torch.equal(rf.records[0, :, F_S:F_WITH], rp.records[0, :, F_S:F_WITH]), mode
        assert bool((rf.reward != rp.reward).any(dim=0).any()), mode
        faulty.set_obs_faults(mode, 1.0)   # the same arithmetic
        faulty.attach_envs(n, seed=SEED, env_base=BASE, accum_steps=STEPS)
        same(faulty.act_envs(), rp)
    faulty.set_obs_faults("missing", KEEP)
    for st in (plain, faulty):
        st.attach_envs(n, seed=SEED, env_base=BASE, accum_steps=STEPS)
    same(faulty.act_envs("teacher"), plain.act_envs("teacher"))
    faulty.set_obs_faults("none")
    same(faulty.act_envs(), plain.act_envs())
    plain.close()
    faulty.close()


@pytest.mark.parametrize("T", [3, 10])
def test_records_of_an_earlier_call_carry_their_own_mask(tr, T):   # noqa: F811
    """7 steps with the teacher acting (no query: the ring only records), then the student under faults
    for 4 + 50 steps: its first windows hold records the teacher call wrote, each masked at the
    step it was recorded at, and the windows after the reset start from zero rows again -- the stepwise
    loop's bits.  The handle's history keeps the clean readings: with the faults switched off for 3 more
    steps mid-episode the windows read the same records unmasked, as the loop, told the same, does."""
    n = 17
    st = _student(tr, T=T, max_windows=n)
    loop = FaultyStepwise(tr, st, n, SEED, BASE, "missing")
    st.attach_envs(n, seed=SEED, env_base=BASE, accum_steps=STEPS)
    st.set_obs_faults("missing", KEEP)
    for K, actor in ((7, "teacher"), (4, "student"), (50, "student")):
        r = st.act_envs(actor, steps=K)
        wrec, wrew = loop.steps(K, act_with=actor)
        assert torch.equal(r.records, wrec) and torch.equal(r.reward, wrew), (K, actor)
    _same_envs(st, loop, (11, 1))
    st.set_obs_faults("none")
    loop.mode = "none"
    r = st.act_envs(steps=3)
    wrec, wrew = loop.steps(3)
    assert torch.equal(r.records, wrec) and torch.equal(r.reward, wrew)
    _same_envs(st, loop, (14, 1))
    loop.close()
    st.close()


def test_step_envs_equals_act_then_step(tr):   # noqa: F811
    """step_envs under faults, policy noise and beta = 0.5, n = 17, against a twin driven as act_envs, then
    step on the (clean) windows it wrote, with the training's own keep_prob = 0.5 dropout: after each of
    two optimiser steps the parameters, gradient, counter and metrics are equal bit for bit."""
    import numpy as np
    n, T = 17, 10
    B = n * 41
    cfg = dict(loss="kl", lr=1e-3, keep_prob=0.5, seed=4)
    fused, twin = _student(tr, max_windows=B, **cfg), _student(tr, max_windows=B, **cfg)
    for st in (fused, twin):
        st.attach_envs(n, seed=SEED, env_base=BASE, accum_steps=STEPS)
        st.set_teacher_share(0.5)
        st.set_action_noise("policy", 1.0)
        st.set_obs_faults("dropout", KEEP)
    for k in range(2):
        r = fused.step_envs()
        w = twin.act_envs()
        for name in ("records", "reward", "ob_w", "prev_w", "t_w"):
            assert torch.equal(getattr(r, name), getattr(w, name)), (k, name)
        twin.step(w.ob_w, w.prev_w, w.t_w)
        assert torch.equal(fused.params(), twin.params()), k
        assert torch.equal(fused.grad(), twin.grad()), k
        assert fused.counter() == twin.counter() == k + 1
        assert np.array_equal(fused.metrics(1), twin.metrics(1)), k
    assert fused.metrics(1)[0, 2] == T * B
    assert torch.equal(fused.query_state(), twin.query_state())
    fused.close()
    twin.close()


def test_a_captured_call_replays_the_next_steps_mask(tr):   # noqa: F811
    """act_envs under faults (n = 17, K = 7) captured and replayed twice equals two eager calls on a twin;
    set to "none" after the capture, the replays are still the faulty calls."""
    a, b = (_student(tr, max_windows=17 * 41) for _ in range(2))
    for st in (a, b):
        st.attach_envs(17, seed=SEED, env_base=BASE, accum_steps=7)
        st.set_obs_faults("missing", KEEP, seed=9)
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
    assert torch.equal(res.records, want.records) and torch.equal(res.reward, want.reward)
    assert torch.equal(a.query_state(), b.query_state()) and torch.equal(a.env_state()[0], b.env_state()[0])
    assert a.env_state()[1:] == (14, 0)
    a.close()
    b.close()
