"""DAgger's beta-mixture in the LSTM student's persistent envs (rdl_envs_set_teacher_share;
StudentLstmTrainer.set_teacher_share) against the stepwise loop of tests/test_student_lstm_envs_gpu.py
-- the teacher's forward, the window of the episode's last T records, forward from the carried (c, h),
env.step -- with the action picked per env by the NumPy coin of tests/envs_mix.py, and against the two
end points it lies between.  The mixed instances run the student instance's step in its order, so
every comparison is bitwise (torch.equal): a difference is a reordering to find, not a tolerance to
add.  Default synthetic teacher, that suite's parameters, T = 10; with the f32 query and with the bf16
cell's (dtype = query_dtype = "bf16")."""
import numpy as np
import pytest
import torch

from tests import envs_mix
from tests.test_student_lstm_envs_gpu import STEPS, Stepwise, _host_windows, _student, tr   # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETA = envs_mix.BETA
T = 10
F_REW, F_T, F_S, F_WITH = 11, 12, 16, 20
DTYPES = {"f32": {}, "bf16": dict(dtype="bf16", query_dtype="bf16")}


class MixedStepwise(Stepwise):
    """Stepwise with the student always queried and the env stepped with its mean, or with the
    teacher's where the NumPy coin of (coin seed, env_base + i, episode, step) says so; the record's
    stepped_with is 1 - coin."""

    def __init__(self, tr, st, n, seed, env_base, beta=BETA):   # noqa: F811
        super().__init__(tr, st, n, seed, env_base)
        self.coin_seed, self.base, self.beta, self.g = seed, env_base, beta, 0

    def steps(self, K):
        n, recs, rews = self.n, [], []
        for _ in range(K):
            t, _ = self.tr.forward(self.ob, teacher=True, student=False)
            self.obs.append(self.ob.clone())
            self.prevs.append(self.prev_t.clone() if self.s else torch.zeros(n, 4, device=DEV))
            k = min(self.s + 1, T)
            ob_w, prev_w = torch.zeros(T, n, 11, device=DEV), torch.zeros(T, n, 4, device=DEV)
            ob_w[T - k:] = torch.stack(self.obs[-k:])
            prev_w[T - k:] = torch.stack(self.prevs[-k:])
            out, self.state = self.st.forward(ob_w, prev_w, self.state)
            sf = out[T - 1].clone()
            coin = torch.from_numpy(envs_mix.teacher_coins(self.coin_seed, self.base, n, self.g // STEPS, self.s,
                                                           self.beta)).to(DEV)
            r = torch.zeros(n, 21, device=DEV)
            r[:, :F_REW] = self.ob
            r[:, F_REW] = self.reward
            r[:, F_T:F_S] = t
            r[:, F_S:F_WITH] = sf
            r[:, F_WITH] = (~coin).float()
            act = torch.where(coin[:, None], t[:, :2], sf[:, :2]).contiguous()
            self.prev_t = t.clone()
            ob, rew, _, _ = self.env.step(act)
            self.ob, self.reward = ob.clone(), rew.clone()
            self.s = (self.s + 1) % STEPS
            self.g += 1
            if self.s == 0:
                self.obs, self.prevs = [], []
            recs.append(r)
            rews.append(self.reward)
        return torch.stack(recs), torch.stack(rews)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 17, 35])
def test_mixed_run_equals_the_stepwise_loop(tr, n, dtype):   # noqa: F811
    """100 steps at beta = 0.5 as two K = 50 calls and as K = 7 calls (fourteen, and a last one of 2;
    35 envs then on one workgroup, which walks the three blocks): all 21 columns of the records,
    stepped_with = 1 - coin among them, the rewards, (c, h) and the env state are the stepwise loop's
    bit for bit, and the three window buffers of the K = 50 calls are the host gather of its records."""
    seed, base = 11, 5
    st = _student(tr, max_windows=n * 41, **DTYPES[dtype])
    loop = MixedStepwise(tr, st, n, seed, base)
    wrec, wrew = loop.steps(2 * STEPS)
    coins = envs_mix.coin_table(seed, base, n, 2 * STEPS, BETA)
    assert torch.equal(wrec[..., F_WITH], torch.from_numpy(1.0 - coins.astype(np.float32)).to(DEV))
    assert 0 < float(wrec[..., F_WITH].mean()) < 1   # both actors stepped
    es, step, episode = loop.env.get_state()
    st.set_teacher_share(BETA)
    for calls, grid in (((50, 50), 0), ((7,) * 14 + (2,), 1)):
        st.attach_envs(n, seed=seed, env_base=base, accum_steps=STEPS, grid=grid)
        assert st.teacher_share == BETA
        recs, rews = [], []
        for K in calls:
            r = st.act_envs(steps=K)
            recs.append(r.records.clone())
            rews.append(r.reward.clone())
            if K == STEPS:
                ob_w, prev_w, t_w, ends = _host_windows(wrec[len(recs) * STEPS - STEPS:len(recs) * STEPS], T)
                assert len(ends) == 41
                assert torch.equal(r.ob_w, ob_w) and torch.equal(r.prev_w, prev_w) and torch.equal(r.t_w, t_w)
        assert torch.equal(torch.cat(recs), wrec), calls[0]
        assert torch.equal(torch.cat(rews), wrew), calls[0]
        gs, gstep, gep = st.env_state()
        assert torch.equal(gs, es) and (gstep, gep) == (step, episode) == (0, 2)
        assert torch.equal(st.query_state(), loop.query_state())
    loop.close()
    st.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_end_points(tr, dtype):   # noqa: F811
    """beta = 1: the records' ob, reward and t_pdflat columns and the env state of a twin's
    act_envs("teacher"), while s_pdflat is written, stepped_with is 0 and (c, h) has advanced.
    beta = 0 after beta = 0.5 was set: a twin's plain student run."""
    n, seed, base = 17, 11, 5
    a, b = (_student(tr, max_windows=n * 41, **DTYPES[dtype]) for _ in range(2))
    for st in (a, b):
        st.attach_envs(n, seed=seed, env_base=base, accum_steps=STEPS)
    a.set_teacher_share(1.0)
    ra, rb = a.act_envs().records, b.act_envs("teacher").records
    assert torch.equal(ra[..., :F_S], rb[..., :F_S])
    assert torch.equal(a.env_state()[0], b.env_state()[0]) and a.env_state()[1:] == b.env_state()[1:] == (0, 1)
    assert bool((ra[..., F_S:F_WITH] != 0).any()) and bool((rb[..., F_S:F_WITH] == 0).all())
    assert bool((ra[..., F_WITH] == 0).all())
    assert bool((a.query_state() != 0).any()) and bool((b.query_state() == 0).all())
    # beta = 0 again: the student instance, as if no share had ever been set
    for st in (a, b):
        st.attach_envs(n, seed=seed, env_base=base, accum_steps=STEPS)
    a.set_teacher_share(BETA)
    a.set_teacher_share(0.0)
    assert a.teacher_share == 0.0
    ra, rb = a.act_envs(), b.act_envs()
    for name in ("records", "reward", "ob_w", "prev_w", "t_w"):
        assert torch.equal(getattr(ra, name), getattr(rb, name)), name
    assert torch.equal(a.query_state(), b.query_state()) and torch.equal(a.env_state()[0], b.env_state()[0])
    assert bool((ra.records[..., F_WITH] == 1).all())
    a.close()
    b.close()


def test_step_envs_equals_act_then_step(tr):   # noqa: F811
    """step_envs at beta = 0.5, n = 17, against a twin driven as act_envs, then step on the windows it
    wrote: after each of two optimiser steps the parameters, gradient, counter and metrics are equal
    bit for bit (the training is on every in-episode window, whoever stepped its records), and the
    records' flags are the NumPy coins."""
    n, seed, base = 17, 11, 5
    B = n * 41
    cfg = dict(loss="kl", lr=1e-3, keep_prob=0.5, seed=4)
    fused, twin = _student(tr, max_windows=B, **cfg), _student(tr, max_windows=B, **cfg)
    for st in (fused, twin):
        st.attach_envs(n, seed=seed, env_base=base, accum_steps=STEPS)
        st.set_teacher_share(BETA)
    coins = envs_mix.coin_table(seed, base, n, 2 * STEPS, BETA)
    for k in range(2):
        r = fused.step_envs()
        w = twin.act_envs()
        for name in ("records", "reward", "ob_w", "prev_w", "t_w"):
            assert torch.equal(getattr(r, name), getattr(w, name)), (k, name)
        want = torch.from_numpy(1.0 - coins[k * STEPS:(k + 1) * STEPS].astype(np.float32)).to(DEV)
        assert torch.equal(r.records[..., F_WITH], want), k
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
