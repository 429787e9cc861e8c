"""DAgger's beta-mixture in the reference MLP student's persistent envs (rdm_envs_set_teacher_share,
rdm_envs_bind_stepped_with; StudentMlpTrainer.set_teacher_share, stepped_with) against the stepwise
loop -- BatchedReacher with Philox resets, DistillTrainer.forward (teacher), rows(),
StudentMlpTrainer.forward, the action picked per env by the NumPy coin of tests/envs_mix.py,
env.step -- and against the two end points it lies between.  The mixed instances call the student
instance's functions in its order, so every comparison is bitwise (torch.equal): a difference is a
reordering to find, not a tolerance to add.  Default synthetic teacher, glorot students."""
import numpy as np
import pytest
import torch

from tests import envs_mix

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 50
BETA = envs_mix.BETA
F_WITH = 20
RD_EINVAL = -100000


@pytest.fixture(scope="module")
def tr():
    """The DistillTrainer whose forward is the stepwise teacher, and whose teacher every student gets."""
    from reacherdistilation_amd.distill import DistillConfig, DistillTrainer
    t = DistillTrainer(DistillConfig(n_envs=64, seed=3), device=DEV)
    yield t
    t.close()


def _student(tr, **cfg):
    from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer
    sm = StudentMlpTrainer(StudentMlpConfig(**cfg), device=DEV)
    sm.set_teacher(tr.teacher)
    return sm


def _keep(sm, r):
    """x, t_pdflat, s_pdflat, reward, stepped_with of the call's steps"""
    K = r.x.shape[0]
    return tuple(v.clone() for v in (r.x, r.t_pdflat, r.s_pdflat, r.reward, sm.stepped_with[:K]))


def _cat(parts):
    return tuple(torch.cat([p[j] for p in parts]) for j in range(len(parts[0])))


class MixedStepwise:
    """The loop the mixed envs kernel fuses: per step the teacher's pdflat, the row ob | the previous
    record's t_pdflat | its reward field (zeros at an episode's step 0), the student's forward on it,
    and env.step with the student's mean, or the teacher's where the NumPy coin of (coin seed,
    env_base + i, episode, step) says so."""

    def __init__(self, tr, sm, n, seed, env_base, coin_seed=None, beta=BETA):
        from reacherdistilation_amd.env import BatchedReacher
        self.tr, self.sm, self.n, self.base, self.beta = tr, sm, n, env_base, beta
        self.coin_seed = seed if coin_seed is None else coin_seed
        self.env = BatchedReacher(n, seed=seed, device=DEV, env_base=env_base)
        self.ob = self.env.reset().clone()
        self.reward = torch.zeros(n, device=DEV)
        self.prev_t, self.prev_r = torch.zeros(n, 4, device=DEV), torch.zeros(n, 1, device=DEV)
        self.g = 0   # lockstep steps since the reset

    def steps(self, K):
        """(x [K, n, 16], t_pdflat, s_pdflat [K, n, 4], reward [K, n], stepped_with [K, n]) of the next K steps."""
        from reacherdistilation_amd.student_mlp import rows
        n, out = self.n, []
        for _ in range(K):
            t, _ = self.tr.forward(self.ob, teacher=True, student=False)
            first = self.g % STEPS == 0
            x = rows(self.ob, torch.zeros_like(self.prev_t) if first else self.prev_t,
                     torch.zeros_like(self.prev_r) if first else self.prev_r)
            sf = self.sm.forward(x)
            coin = torch.from_numpy(envs_mix.teacher_coins(self.coin_seed, self.base, n, self.g // STEPS,
                                                           self.g % STEPS, self.beta)).to(DEV)
            act = torch.where(coin[:, None], t[:, :2], sf[:, :2]).contiguous()
            self.prev_t, self.prev_r = t.clone(), self.reward.clone().view(n, 1)   # this record's fields
            ob, rew, _, _ = self.env.step(act)
            self.ob, self.reward = ob.clone(), rew.clone()
            self.g += 1
            out.append((x, t.clone(), sf, self.reward, (~coin).float()))
        return tuple(torch.stack([o[j] for o in out]) for j in range(5))

    def close(self):
        self.env.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 17, 83])
def test_mixed_run_equals_the_stepwise_loop(tr, n, dtype):
    """100 steps at beta = 0.5 as two K = 50 calls and as fifteen K = 7 calls (the first 100): x, both
    pdflats, the rewards and stepped_with = 1 - coin are the stepwise loop's bit for bit, and so is the
    env state after the two K = 50 calls -- whatever the split of the steps over the calls."""
    seed, base = 11, 5
    sm = _student(tr, dtype=dtype)
    loop = MixedStepwise(tr, sm, n, seed, base)
    want = loop.steps(2 * STEPS)
    coins = envs_mix.coin_table(seed, base, n, 2 * STEPS, BETA)
    assert torch.equal(want[4], torch.from_numpy(1.0 - coins.astype(np.float32)).to(DEV))
    sm.set_teacher_share(BETA)   # before the attach: the coins take the envs' seed when it comes
    assert sm.stepped_with is None and sm.teacher_share == BETA
    for K, calls in ((50, 2), (7, 15)):
        sm.attach_envs(n, seed=seed, env_base=base, accum_steps=K)
        assert sm.stepped_with.shape == (K, n) and sm.teacher_share == BETA
        got = _cat([_keep(sm, sm.act_envs()) for _ in range(calls)])
        for name, g, w in zip(("x", "t_pdflat", "s_pdflat", "reward", "stepped_with"), got, want):
            assert torch.equal(g[:2 * STEPS], w), (K, name)
        if K == 50:
            st, step, episode = loop.env.get_state()
            gs, gstep, gep = sm.env_state()
            assert torch.equal(gs, st) and (gstep, gep) == (step, episode) == (0, 2)
    flags = want[4].cpu().numpy()
    assert 0 < flags.mean() < 1   # both actors stepped
    loop.close()
    sm.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_blocks_of_64_equal_blocks_of_16(tr, dtype):
    """n = 595 at beta = 0.5: grid=1 runs 64-env blocks on one workgroup, nine full ones and a ragged
    tail of 19, the automatic grid 16-env blocks; the same bits for K = 50, the same envs afterwards,
    and the flags are the NumPy coins (a coin does not depend on the block its env is in)."""
    n, seed = 595, 7
    a, b = _student(tr, dtype=dtype), _student(tr, dtype=dtype)
    a.attach_envs(n, seed=seed, accum_steps=STEPS, grid=1)
    b.attach_envs(n, seed=seed, accum_steps=STEPS)
    a.set_teacher_share(BETA)
    b.set_teacher_share(BETA)
    ka, kb = _keep(a, a.act_envs()), _keep(b, b.act_envs())
    for u, v in zip(ka, kb):
        assert torch.equal(u, v)
    coins = envs_mix.coin_table(seed, 0, n, STEPS, BETA)
    assert torch.equal(ka[4], torch.from_numpy(1.0 - coins.astype(np.float32)).to(DEV))
    (sa, sta, ea), (sb, stb, eb) = a.env_state(), b.env_state()
    assert torch.equal(sa, sb) and (sta, ea) == (stb, eb) == (0, 1)
    a.close()
    b.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n", [17, 83])
def test_end_points(tr, n, dtype):
    """beta = 0 with the flag buffer bound runs the mixed instance: the outputs and env state of a twin
    without a buffer (the student instance), flags all 1.  beta = 1: x, t_pdflat, reward and the env
    state of a twin's act_envs("teacher"), s_pdflat = forward(x), flags all 0."""
    K, seed, base = STEPS, 11, 5
    mixed, plain = _student(tr, dtype=dtype), _student(tr, dtype=dtype)
    mixed.attach_envs(n, seed=seed, env_base=base, accum_steps=K, flags=True)
    plain.attach_envs(n, seed=seed, env_base=base, accum_steps=K)
    assert mixed.stepped_with is not None and plain.stepped_with is None and mixed.teacher_share == 0.0
    rm, rp = mixed.act_envs(), plain.act_envs()
    for u, v in zip((rm.x, rm.t_pdflat, rm.s_pdflat, rm.reward), (rp.x, rp.t_pdflat, rp.s_pdflat, rp.reward)):
        assert torch.equal(u, v)
    assert torch.equal(mixed.env_state()[0], plain.env_state()[0])
    assert bool((mixed.stepped_with == 1).all())
    # beta = 1 from the same envs on: the teacher steps every env, the student is still evaluated
    mixed.set_teacher_share(1.0)
    rm, rp = mixed.act_envs(), plain.act_envs("teacher")
    assert torch.equal(rm.x, rp.x) and torch.equal(rm.t_pdflat, rp.t_pdflat) and torch.equal(rm.reward, rp.reward)
    assert torch.equal(mixed.env_state()[0], plain.env_state()[0])
    assert torch.equal(rm.s_pdflat.reshape(-1, 4), mixed.forward(rm.x.reshape(-1, 16)))
    assert bool((rp.s_pdflat == 0).all()) and bool((rm.s_pdflat != 0).any())
    assert bool((mixed.stepped_with == 0).all())
    mixed.close()
    plain.close()


@pytest.mark.parametrize("keep_prob", [1.0, 0.5])
def test_step_envs_equals_the_stepwise_loop(tr, keep_prob):
    """step_envs at beta = 0.5, (n, K, optimiser steps) = (83, 7, 8), against a twin stepped stepwise
    and trained with step on the K n rows: after every step the parameters, gradient, counter and
    metrics are equal bit for bit (the training is on every row, whoever stepped it)."""
    n, K, opt_steps = 83, 7, 8
    cfg = dict(loss="kl", lr=1e-3, keep_prob=keep_prob, seed=4)
    fused, twin = _student(tr, **cfg), _student(tr, **cfg)
    fused.attach_envs(n, seed=11, env_base=5, accum_steps=K)
    fused.set_teacher_share(BETA)
    loop = MixedStepwise(tr, twin, n, 11, 5)
    for k in range(opt_steps):
        r = fused.step_envs()
        x, t, s, rew, flags = loop.steps(K)
        assert torch.equal(r.x, x) and torch.equal(r.t_pdflat, t) and torch.equal(r.s_pdflat, s), k
        assert torch.equal(r.reward, rew) and torch.equal(fused.stepped_with, flags), k
        twin.step(x.reshape(-1, 16), t.reshape(-1, 4))
        assert torch.equal(fused.params(), twin.params()), k
        assert torch.equal(fused.grad(), twin.grad()), k
        assert fused.counter() == twin.counter() == k + 1
        assert np.array_equal(fused.metrics(1), twin.metrics(1)), k
    assert fused.metrics(1)[0, 2] == K * n
    st, step, episode = loop.env.get_state()
    gs, gstep, gep = fused.env_state()
    assert torch.equal(gs, st) and (gstep, gep) == (step, episode) == (6, 1)
    loop.close()
    fused.close()
    twin.close()


def test_ring_takes_the_flags(tr):
    """ReplayRing.push_rows with the flag tensor after one K = 50 call at n = 17 (an explicit coin
    seed): ring column 20 is the flags, the NumPy coins', and every other column is what the scalar
    push writes."""
    from reacherdistilation_amd.replay import ReplayRing
    n, seed, base, coin_seed = 17, 11, 5, 9
    sm = _student(tr)
    sm.attach_envs(n, seed=seed, env_base=base, accum_steps=STEPS)
    sm.set_teacher_share(BETA, seed=coin_seed)
    r = sm.act_envs()
    coins = envs_mix.coin_table(coin_seed, base, n, STEPS, BETA)
    want = torch.from_numpy(1.0 - coins.astype(np.float32)).to(DEV)
    assert torch.equal(sm.stepped_with, want)
    a, b = ReplayRing(n, device=DEV, max_batch=8), ReplayRing(n, device=DEV, max_batch=8)
    a.push_rows(r, stepped_with=sm.stepped_with)
    b.push_rows(r, stepped_with=1.0)
    ra, rb = a.records, b.records   # [n, 50, 21]: episode i is env i's
    assert torch.equal(ra[..., F_WITH], want.t())
    assert torch.equal(ra[..., :F_WITH], rb[..., :F_WITH]) and bool((rb[..., F_WITH] == 1).all())
    assert a.counters()[0] == b.counters()[0] == n
    with pytest.raises(ValueError):
        a.push_rows(r, stepped_with=sm.stepped_with[:7])
    a.close()
    b.close()
    sm.close()


def test_teacher_calls_ignore_beta(tr):
    """act_envs("teacher") under beta = 0.5 is a twin's without: the same outputs and envs; the bound
    flags read 0."""
    n = 83
    a, b = _student(tr), _student(tr)
    for sm in (a, b):
        sm.attach_envs(n, seed=11, env_base=5, accum_steps=STEPS)
    a.set_teacher_share(BETA)
    ra, rb = a.act_envs("teacher"), b.act_envs("teacher")
    for u, v in zip((ra.x, ra.t_pdflat, ra.s_pdflat, ra.reward), (rb.x, rb.t_pdflat, rb.s_pdflat, rb.reward)):
        assert torch.equal(u, v)
    assert torch.equal(a.env_state()[0], b.env_state()[0])
    assert bool((a.stepped_with == 0).all()) and bool((ra.s_pdflat == 0).all())
    a.close()
    b.close()


def test_bind_with_too_few_rows_is_refused(tr):
    from reacherdistilation_amd import _native as nat
    n, K = 17, 7
    sm = _student(tr)
    sm.attach_envs(n, seed=11, accum_steps=K)
    lib, short = sm._lib, torch.zeros(K * n - 1, device=DEV)
    assert lib.rdm_envs_bind_stepped_with(sm._h, nat.ptr(short), short.numel()) == 0
    b = sm._envs
    args = (sm._h, 1, K, nat.ptr(b.x), nat.ptr(b.t_pdflat), nat.ptr(b.s_pdflat), nat.ptr(b.reward))
    for fn in ("rdm_envs_act", "rdm_rollout_envs", "rdm_step_envs"):
        assert getattr(lib, fn)(*args) == RD_EINVAL
        msg = lib.rd_last_error().decode()
        assert fn + ":" in msg and "rows" in msg, msg
    assert lib.rdm_envs_act(sm._h, 1, K - 1, *args[3:]) == 0   # (K - 1) n rows fit
    torch.cuda.synchronize()
    assert bool((short[:(K - 1) * n] == 1).all())
    assert lib.rdm_envs_bind_stepped_with(sm._h, nat.ptr(short), 0) == RD_EINVAL and "rows" in lib.rd_last_error().decode()
    assert lib.rdm_envs_bind_stepped_with(sm._h, None, 0) == 0   # unbound: the plain student call again
    assert lib.rdm_envs_act(*args) == 0
    torch.cuda.synchronize()
    sm.close()
