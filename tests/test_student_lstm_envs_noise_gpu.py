"""Action noise in the LSTM student's persistent envs (rdl_envs_set_action_noise, rdl_envs_bind_actions;
StudentLstmTrainer.set_action_noise, actions) against the stepwise loop of
tests/test_student_lstm_envs_gpu.py -- the teacher's forward, the window of the episode's last T records,
forward from the carried (c, h), env.step -- with the acting pdflat passed through
action_noise.perturb_actions (rd_perturb_actions: the device function the fused kernels inline) before
the step.  Every comparison is bitwise (torch.equal): a difference is a reordering to find, not a
tolerance to add.  Default synthetic teacher, that suite's parameters, T = 10; with the f32 query and
with the bf16 cell's (dtype = query_dtype = "bf16")."""
import pytest
import torch

from tests import envs_mix
from tests.test_student_lstm_envs_gpu import STEPS, Stepwise, _host_windows, _student, tr   # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 10
RD_EINVAL = -100000
F_REW, F_T, F_S, F_WITH = 11, 12, 16, 20
DTYPES = {"f32": {}, "bf16": dict(dtype="bf16", query_dtype="bf16")}


class NoisyStepwise(Stepwise):
    """Stepwise under action noise: the acting pdflat -- the student's, the teacher's in a "teacher" run
    (no query, s_pdflat and stepped_with 0) or where the NumPy coin of tests/envs_mix.py fell -- goes
    through rd_perturb_actions at (noise seed, env_base + i, episode, step), and its action steps the
    env.  The record keeps the pdflats, not the action."""

    def __init__(self, tr, st, n, seed, env_base, mode, scale, beta=0.0, act_with="student"):   # noqa: F811
        super().__init__(tr, st, n, seed, env_base)
        self.seed, self.base, self.mode, self.scale, self.beta, self.act_with, self.g = \
            seed, env_base, mode, scale, beta, act_with, 0

    def steps(self, K):
        """(records [K, n, 21], reward [K, n], actions [K, n, 2]) of the next K steps."""
        from reacherdistilation_amd.action_noise import perturb_actions
        n, recs, rews, acts = self.n, [], [], []
        for _ in range(K):
            t, _ = self.tr.forward(self.ob, teacher=True, student=False)
            self.obs.append(self.ob.clone())
            self.prevs.append(self.prev_t.clone() if self.s else torch.zeros(n, 4, device=DEV))
            if self.act_with == "student":
                k = min(self.s + 1, T)
                ob_w, prev_w = torch.zeros(T, n, 11, device=DEV), torch.zeros(T, n, 4, device=DEV)
                ob_w[T - k:] = torch.stack(self.obs[-k:])
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
            act = perturb_actions(acting, mode=self.mode, scale=self.scale, seed=self.seed, env_base=self.base,
                                  episode=self.g // STEPS, step=self.s)
            self.prev_t = t.clone()
            ob, rew, _, _ = self.env.step(act)
            self.ob, self.reward = ob.clone(), rew.clone()
            self.s = (self.s + 1) % STEPS
            self.g += 1
            if self.s == 0:
                self.obs, self.prevs = [], []
            recs.append(r)
            rews.append(self.reward)
            acts.append(act)
        return torch.stack(recs), torch.stack(rews), torch.stack(acts)


# (n, dtype, mode, scale, beta, actor): both modes, both betas, both actors, both queries
RUNS = [(1, "f32", "policy", 1.0, 0.5, "student"), (17, "f32", "fixed", 0.3, 0.0, "student"),
        (35, "f32", "policy", 1.0, 0.5, "student"), (17, "bf16", "policy", 1.0, 0.5, "student"),
        (35, "bf16", "fixed", 0.3, 0.0, "student"), (17, "f32", "fixed", 0.3, 0.5, "teacher")]


@pytest.mark.parametrize("n,dtype,mode,scale,beta,actor", RUNS)
def test_noisy_run_equals_the_stepwise_loop(tr, n, dtype, mode, scale, beta, actor):   # noqa: F811
    """100 steps as two K = 50 calls and as K = 7 calls (fourteen, and a last one of 2; 35 envs then on
    one workgroup, which walks the three blocks): all 21 columns of the records, the rewards, the
    bound actions, (c, h) and the env state are the stepwise loop's bit for bit, and the three window
    buffers of the K = 50 calls are the host gather of its records."""
    seed, base = 11, 5
    st = _student(tr, max_windows=n * 41, **DTYPES[dtype])
    loop = NoisyStepwise(tr, st, n, seed, base, mode, scale, beta=beta, act_with=actor)
    wrec, wrew, wact = loop.steps(2 * STEPS)
    acting = torch.where((wrec[..., F_WITH] == 0)[..., None], wrec[..., F_T:F_S], wrec[..., F_S:F_WITH])
    assert not torch.equal(wact, acting[..., :2])
    es, step, episode = loop.env.get_state()
    st.set_action_noise(mode, scale)   # before the attach: the noise takes the envs' seed when it comes
    st.set_teacher_share(beta)
    for calls, grid in (((50, 50), 0), ((7,) * 14 + (2,), 1)):
        st.attach_envs(n, seed=seed, env_base=base, accum_steps=STEPS, grid=grid, actions=True)
        assert st.action_noise == dict(mode=mode, scale=pytest.approx(scale), seed=seed)
        recs, rews, acts = [], [], []
        for K in calls:
            r = st.act_envs(actor, steps=K)
            recs.append(r.records.clone())
            rews.append(r.reward.clone())
            acts.append(st.actions[:K].clone())
            if K == STEPS:
                ob_w, prev_w, t_w, ends = _host_windows(wrec[len(recs) * STEPS - STEPS:len(recs) * STEPS], T)
                assert len(ends) == 41
                assert torch.equal(r.ob_w, ob_w) and torch.equal(r.prev_w, prev_w) and torch.equal(r.t_w, t_w)
        assert torch.equal(torch.cat(recs), wrec), calls[0]
        assert torch.equal(torch.cat(rews), wrew), calls[0]
        assert torch.equal(torch.cat(acts), wact), calls[0]
        gs, gstep, gep = st.env_state()
        assert torch.equal(gs, es) and (gstep, gep) == (step, episode) == (0, 2)
        assert torch.equal(st.query_state(), loop.query_state())
    loop.close()
    st.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_end_points(tr, dtype):   # noqa: F811
    """scale = 0 with the actions buffer bound runs the noisy instances: a twin's plain calls of either
    actor -- records, rewards, windows, (c, h), env state -- and actions = the acting means.  Set back
    to "none" and unbound, the call is the plain one again, bit for bit."""
    n, seed, base = 17, 11, 5
    a, b = (_student(tr, max_windows=n * 41, **DTYPES[dtype]) for _ in range(2))
    a.attach_envs(n, seed=seed, env_base=base, accum_steps=STEPS, actions=True)
    b.attach_envs(n, seed=seed, env_base=base, accum_steps=STEPS)
    assert a.actions is not None and b.actions is None and a.action_noise["mode"] == "none"

    def same(ra, rb):
        for name in ("records", "reward", "ob_w", "prev_w", "t_w"):
            assert torch.equal(getattr(ra, name), getattr(rb, name)), name
        assert torch.equal(a.query_state(), b.query_state()) and torch.equal(a.env_state()[0], b.env_state()[0])

    for mode, actor in (("none", "student"), ("fixed", "teacher"), ("policy", "student")):
        a.set_action_noise(mode, 0.0)
        ra, rb = a.act_envs(actor), b.act_envs(actor)
        same(ra, rb)
        means = rb.records[..., F_S:F_S + 2] if actor == "student" else rb.records[..., F_T:F_T + 2]
        assert torch.equal(a.actions, means), (mode, actor)
    a.set_action_noise("policy", 1.0)
    assert not torch.equal(a.act_envs().reward, b.act_envs().reward)
    for st in (a, b):
        st.attach_envs(n, seed=seed, env_base=base, accum_steps=STEPS)
    a.set_action_noise("none")
    assert a._lib.rdl_envs_bind_actions(a._h, None, 0) == 0
    same(a.act_envs(), b.act_envs())
    assert bool((a.actions == 0).all())   # no longer written
    a.close()
    b.close()


def test_step_envs_equals_act_then_step(tr):   # noqa: F811
    """step_envs under policy noise at beta = 0.5, n = 17, against a twin driven as act_envs, then step
    on the windows it wrote: after each of two optimiser steps the parameters, gradient, counter and
    metrics are equal bit for bit (the training is on every in-episode window, as without noise)."""
    import numpy as np
    n, seed, base = 17, 11, 5
    B = n * 41
    cfg = dict(loss="kl", lr=1e-3, keep_prob=0.5, seed=4)
    fused, twin = _student(tr, max_windows=B, **cfg), _student(tr, max_windows=B, **cfg)
    for st in (fused, twin):
        st.attach_envs(n, seed=seed, env_base=base, accum_steps=STEPS, actions=True)
        st.set_teacher_share(0.5)
        st.set_action_noise("policy", 1.0)
    for k in range(2):
        r = fused.step_envs()
        w = twin.act_envs()
        for name in ("records", "reward", "ob_w", "prev_w", "t_w"):
            assert torch.equal(getattr(r, name), getattr(w, name)), (k, name)
        assert torch.equal(fused.actions, twin.actions), k
        twin.step(w.ob_w, w.prev_w, w.t_w)
        assert torch.equal(fused.params(), twin.params()), k
        assert torch.equal(fused.grad(), twin.grad()), k
        assert fused.counter() == twin.counter() == k + 1
        assert np.array_equal(fused.metrics(1), twin.metrics(1)), k
    assert fused.metrics(1)[0, 2] == T * B
    assert torch.equal(fused.query_state(), twin.query_state())
    assert torch.equal(fused.env_state()[0], twin.env_state()[0])
    fused.close()
    twin.close()


def test_a_captured_call_replays_the_next_steps_noise(tr):   # noqa: F811
    """act_envs under fixed noise (n = 17, K = 7) captured and replayed twice equals two eager calls on
    a twin; set to "none" after the capture, the replays are still the noisy calls."""
    a, b = (_student(tr, max_windows=17 * 41) for _ in range(2))
    for st in (a, b):
        st.attach_envs(17, seed=11, env_base=5, accum_steps=7, actions=True)
        st.set_action_noise("fixed", 0.3, seed=9)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(a.device)
    with torch.cuda.graph(g):
        res = a.act_envs()
    a._sync_stream()
    a.set_action_noise("none")
    for _ in range(2):
        g.replay()
    b.act_envs()
    first = b.actions.clone()
    want = b.act_envs()
    torch.cuda.synchronize(a.device)
    assert torch.equal(res.records, want.records) and torch.equal(res.reward, want.reward)
    assert torch.equal(a.actions, b.actions) and not torch.equal(first, b.actions)
    assert torch.equal(a.query_state(), b.query_state()) and torch.equal(a.env_state()[0], b.env_state()[0])
    assert a.env_state()[1:] == (14, 0)
    a.close()
    b.close()


def test_bind_with_too_few_rows_is_refused(tr):   # noqa: F811
    from reacherdistilation_amd import _native as nat
    n, K = 17, 50
    st = _student(tr, max_windows=n * 41)
    st.attach_envs(n, seed=11, accum_steps=K)
    lib, short = st._lib, torch.zeros(K * n - 1, 2, device=DEV)
    assert lib.rdl_envs_bind_actions(st._h, nat.ptr(short), short.shape[0]) == 0
    b = st._envs
    w = (nat.ptr(b.ob_w), nat.ptr(b.prev_w), nat.ptr(b.t_w))
    for fn, tail in (("rdl_envs_act", (*w, n * 41)), ("rdl_rollout_envs", w), ("rdl_step_envs", w)):
        assert getattr(lib, fn)(st._h, 1, K, nat.ptr(b.records), nat.ptr(b.reward), *tail) == RD_EINVAL
        msg = lib.rd_last_error().decode()
        assert fn + ":" in msg and "rows" in msg and "rdl_envs_bind_actions" in msg, msg
    assert lib.rdl_envs_act(st._h, 1, K - 1, nat.ptr(b.records), nat.ptr(b.reward), None, None, None, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(short[:(K - 1) * n].view(K - 1, n, 2), b.records[:K - 1, :, F_S:F_S + 2])   # noise off: the means
    assert lib.rdl_envs_bind_actions(st._h, nat.ptr(short), 0) == RD_EINVAL and "rows" in lib.rd_last_error().decode()
    assert lib.rdl_envs_bind_actions(st._h, None, 0) == 0   # unbound: the plain student call again
    assert lib.rdl_envs_act(st._h, 1, K, nat.ptr(b.records), nat.ptr(b.reward), *w, n * 41) == 0
    torch.cuda.synchronize()
    st.close()
