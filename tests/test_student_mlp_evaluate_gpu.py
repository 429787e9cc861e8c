"""Whole-episode evaluation of the reference MLP student in one launch (rdm_evaluate /
StudentMlpTrainer.evaluate) against the stepwise loop it replaces: BatchedReacher stepped with
StudentMlpTrainer.forward's means on rows assembled from DistillTrainer.forward's teacher output.
The fused kernel calls the same device functions in the same order, so every comparison with
the stepwise path is bitwise (torch.equal): a difference is a reordering to find, not a tolerance
to add.  All tests use the default synthetic teacher and a glorot student."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import policy_np as pn
from oracle import refnet_np as rn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 50
F_REW, F_T, F_S, F_WITH = 11, 12, 16, 20


@pytest.fixture(scope="module")
def pair():
    """(DistillTrainer for the teacher's stepwise forward, StudentMlpTrainer with that teacher set),
    shared by the tests: forward and evaluate leave both unchanged."""
    from reacherdistilation_amd.distill import DistillConfig, DistillTrainer
    from reacherdistilation_amd.student_mlp import StudentMlpTrainer
    tr = DistillTrainer(DistillConfig(n_envs=64, seed=3), device=DEV)
    sm = StudentMlpTrainer(device=DEV)
    sm.set_teacher(tr.teacher)
    yield tr, sm
    sm.close()
    tr.close()


def _stepwise(tr, sm, env, episodes, shadow):
    """The loop rdm_evaluate fuses, on ``env`` (its next reset opens episode 0 of the run):
    returns [E, n], final distance [E, n], records [E, n, 50, 21].  Row s = ob | record s-1's
    teacher pdflat | record s-1's reward field (zeros at s = 0); the reward variable runs on over
    the resets, as the driver's does.  The final distance is read from ``shadow`` as
    tests/test_evaluate_gpu.py::_stepwise reads it."""
    from reacherdistilation_amd.student_mlp import rows
    n = env.n
    ob = env.reset()
    reward = torch.zeros(n, device=DEV)
    zero = torch.zeros(n, 2, device=DEV)
    rets, dists = [], []
    rec = torch.zeros(episodes, STEPS, n, 21, device=DEV)
    for e in range(episodes):
        ret = torch.zeros(n, dtype=torch.float32, device=DEV)
        prev_t, prev_r = torch.zeros(n, 4, device=DEV), torch.zeros(n, 1, device=DEV)
        for s in range(STEPS):
            t, _ = tr.forward(ob, teacher=True, student=False)
            sf = sm.forward(rows(ob, prev_t, prev_r))
            act = sf[:, :2].contiguous()
            r = rec[e, s]
            r[:, :F_REW] = ob
            r[:, F_REW] = reward
            r[:, F_T:F_S] = t
            r[:, F_S:F_WITH] = sf
            r[:, F_WITH] = 1.0
            prev_t, prev_r = t.clone(), reward.clone().view(n, 1)   # this record's fields: the next row's
            if s == STEPS - 1:
                st, _, _ = env.get_state()
                shadow.set_state(st, step=0, episode=0)
                shadow.step(act)
                dists.append((-shadow.step(zero)[1]).clone())
            ob, rew, _, _ = env.step(act)
            ret = ret + rew
            reward = rew.clone()
        rets.append(ret)
    return torch.stack(rets), torch.stack(dists), rec.transpose(1, 2).contiguous()


_CASES = {}


def _gym_case(pair, n, episodes=2, seed=7):
    """The stepwise reference of one (n, episodes, seed), computed once and shared."""
    from reacherdistilation_amd.env import BatchedReacher
    from reacherdistilation_amd.evaluate import gym_draw_table
    key = (n, episodes, seed)
    if key not in _CASES:
        env, shadow = BatchedReacher(n, seed=seed, device=DEV, reset="gym"), BatchedReacher(n, device=DEV)
        ref = _stepwise(*pair, env, episodes, shadow)
        env.close()
        shadow.close()
        _CASES[key] = (ref, gym_draw_table(seed, n, episodes))
    return _CASES[key]


@pytest.mark.parametrize("n", [1, 17, 83])
def test_fused_equals_stepwise_bitwise(pair, n):
    """Gym draw table (env i seeded seed + i), E = 2: returns, final distances and every record
    equal the stepwise run's, bit for bit."""
    sm = pair[1]
    (ret, dist, rec), draws = _gym_case(pair, n)
    res = sm.evaluate(n, 2, draws=draws, final_dist=True, records=True)
    torch.cuda.synchronize()
    assert res.returns.shape == (2, n) and res.final_dist.shape == (2, n) and res.records.shape == (2, n, STEPS, 21)
    assert torch.equal(res.records, rec)
    assert torch.equal(res.returns, ret)
    assert torch.equal(res.final_dist, dist)
    assert bool(torch.isfinite(res.returns).all()) and bool((res.returns < 0).all()) and bool((res.final_dist >= 0).all())
    assert bool((res.records[..., F_WITH] == 1).all())
    # the optional outputs do not change the returns
    assert torch.equal(sm.evaluate(n, 2, draws=draws).returns, ret)


def test_the_drivers_own_loop(pair):
    """mlp_train.train's phase-2 loop with no optimiser step (DriverEnv, DeviceDataset.write /
    current_prev / flush, query as the driver's): its three student-stepped episodes are
    rdm_evaluate's records of one env over three episodes, bit for bit -- the row assembly and the
    reward carried over the resets, pinned to the dataset's code."""
    from reacherdistilation_amd.config import OBSPACE_SHAPE
    from reacherdistilation_amd.dataset import DeviceDataset
    from reacherdistilation_amd.driver_env import DriverEnv
    from reacherdistilation_amd.evaluate import gym_draw_table
    from reacherdistilation_amd.student_mlp import rows
    tr, sm = pair
    seed, E = 5, 3
    env = DriverEnv(seed, DEV)
    dataset = DeviceDataset(capacity=8, device=DEV, seed=seed)
    ob = env.reset()
    reward = torch.zeros(1, device=DEV)

    def query(o):   # mlp_train.py's, student="mlp"
        t, s = tr.forward(o)
        prev, prew = dataset.current_prev()
        s = sm.forward(rows(o.view(OBSPACE_SHAPE), prev, prew))
        return t[0], s[0]

    while dataset.num_episodes() < E:
        t_pdflat, s_pdflat = query(ob)
        dataset.write(ob=ob, reward=reward, t_pdflat=t_pdflat, s_pdflat=s_pdflat, stepped_with="s")
        ob, reward, new = env.step(s_pdflat)
        if new:
            dataset.flush()
    res = sm.evaluate(1, E, draws=gym_draw_table(seed, 1, E), records=True)
    torch.cuda.synchronize()
    assert dataset.lens[:E] == [STEPS] * E
    assert torch.equal(dataset.ring[:E], res.records.view(E, STEPS, 21))
    assert float(res.records[0, 0, 0, F_REW]) == 0.0 and float(res.records[1, 0, 0, F_REW]) != 0.0
    # and the records go into a dataset as whole episodes
    other = DeviceDataset(capacity=8, device=DEV, seed=seed)
    assert other.write_episodes(res.records.view(E, STEPS, 21)) == E
    assert torch.equal(other.ring[:E], dataset.ring[:E])


def test_blocks_of_64_equal_blocks_of_16_and_the_stepwise_run(pair):
    """n = 595 on one workgroup (grid=1) runs as 64-env blocks -- nine full ones and a ragged tail
    of 19 -- and on the automatic grid as 16-env blocks: the same bits, and the stepwise run's."""
    sm, n = pair[1], 595
    (ret, dist, rec), draws = _gym_case(pair, n, episodes=1)
    a = sm.evaluate(n, 1, draws=draws, final_dist=True, records=True, grid=1)
    b = sm.evaluate(n, 1, draws=draws, final_dist=True, records=True)
    torch.cuda.synchronize()
    for x, y in ((a.returns, b.returns), (a.final_dist, b.final_dist), (a.records, b.records)):
        assert torch.equal(x, y)
    assert torch.equal(a.returns, ret) and torch.equal(a.final_dist, dist) and torch.equal(a.records, rec)


@pytest.mark.parametrize("first_episode", [0, 3])
def test_philox_resets(pair, first_episode):
    """draws=None: episode e resets from Philox(seed, env_base + i, first_episode + e), as
    BatchedReacher's Philox mode does."""
    from reacherdistilation_amd.env import BatchedReacher
    tr, sm = pair
    n, seed, base = 83, 11, 5
    env, shadow = BatchedReacher(n, seed=seed, device=DEV, env_base=base), BatchedReacher(n, device=DEV)
    for _ in range(first_episode):
        env.reset()   # each reset opens the next Philox episode
    ret, dist, rec = _stepwise(tr, sm, env, 2, shadow)
    res = sm.evaluate(n, 2, seed=seed, env_base=base, first_episode=first_episode, final_dist=True, records=True)
    torch.cuda.synchronize()
    assert torch.equal(res.returns, ret) and torch.equal(res.final_dist, dist) and torch.equal(res.records, rec)
    env.close()
    shadow.close()


def test_records_against_the_oracles(pair):
    """Independent of the product's forwards: n = 17, E = 2.  Every row is rebuilt on the host from
    the returned records (ob_s | record s-1's t_pdflat | record s-1's reward, zeros at s = 0); the
    student's pdflat is oracle.refnet_np.forward of it at tests/test_student_mlp_gpu.py's forward
    tolerance, the teacher's is oracle.policy_np's at tests/test_distill_gpu.py's."""
    tr, sm = pair
    n, E = 17, 2
    _, draws = _gym_case(pair, n)
    rec = sm.evaluate(n, E, draws=draws, records=True).records.cpu().numpy()
    x = np.zeros((E, n, STEPS, 16), np.float32)
    x[..., :11] = rec[..., :F_REW]
    x[:, :, 1:, 11:15] = rec[:, :, :-1, F_T:F_S]
    x[:, :, 1:, 15] = rec[:, :, :-1, F_REW]
    want = rn.forward(sm.params().cpu().numpy(), x.reshape(-1, 16))["pdflat"]
    np.testing.assert_allclose(rec[..., F_S:F_WITH].reshape(-1, 4), want, atol=2e-5, rtol=1e-4)
    p = tr.teacher
    ob = rec[..., :F_REW].reshape(-1, 11).astype(np.float64)
    ft = pn.forward(p.flat.astype(np.float64), p.ob_mean.astype(np.float64), p.ob_std.astype(np.float64), ob)
    np.testing.assert_allclose(rec[..., F_T:F_T + 2].reshape(-1, 2), ft["mean"], atol=2e-5, rtol=1e-5)
    assert np.all(rec[..., F_T + 2:F_S] == p.flat[pn.P_LS:].astype(np.float32))
    # the reward carried over the reset reaches episode 1's first record (and, through it, row 1)
    assert np.all(rec[0, :, 0, F_REW] == 0.0) and np.any(rec[1, :, 0, F_REW] != 0.0)
    assert np.all(x[1, :, 1, 15] == rec[1, :, 0, F_REW])


def _batch(n, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1, 1, (n, 16)).astype(np.float32)
    t = np.concatenate([rs.uniform(-.5, .5, (n, 2)), rs.uniform(-1.0, -0.2, (n, 2))], 1).astype(np.float32)
    return torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)


def test_evaluate_has_no_side_effects(pair):
    """Params, Adam counter and gradient buffer are unchanged by an evaluation, and a training step
    after an evaluation equals the same step taken without it."""
    from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer
    x, t = _batch(200)
    a, b = (StudentMlpTrainer(StudentMlpConfig(lr=1e-3), device=DEV) for _ in range(2))
    b.set_teacher(pair[0].teacher)
    for tr in (a, b):
        tr.step(x, t)
        tr.rollout(x, t)
    p0, g0, c0 = b.params().clone(), b.grad().clone(), b.counter()
    b.evaluate(83, 2, seed=1, final_dist=True, records=True)
    b.evaluate(595, 1, seed=1, grid=1)
    torch.cuda.synchronize()
    assert torch.equal(b.params(), p0) and torch.equal(b.grad(), g0) and b.counter() == c0 == 1
    for tr in (a, b):
        tr.step(x, t)
    torch.cuda.synchronize()
    assert torch.equal(a.params(), b.params()) and torch.equal(a.grad(), b.grad())
    assert a.counter() == b.counter() == 2 and np.array_equal(a.metrics(2), b.metrics(2))
    assert not torch.equal(b.params(), p0)
    a.close()
    b.close()


def test_a_captured_evaluation_replays_the_eager_result(pair):
    from reacherdistilation_amd.evaluate import gym_draw_table
    sm, n = pair[1], 83
    draws = torch.from_numpy(gym_draw_table(7, n, 2)).to(DEV)
    kw = dict(draws=draws, final_dist=True, records=True)
    eager = sm.evaluate(n, 2, **kw)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(sm.device)
    with torch.cuda.graph(g):
        res = sm.evaluate(n, 2, **kw)
    sm._sync_stream()
    for _ in range(2):
        for t in (res.returns, res.final_dist, res.records):
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize(sm.device)
        assert torch.equal(res.returns, eager.returns) and torch.equal(res.final_dist, eager.final_dist)
        assert torch.equal(res.records, eager.records)


def test_bad_arguments_raise(pair):
    from reacherdistilation_amd import _native as nat
    from reacherdistilation_amd.student_mlp import RdmEvalConfig, StudentMlpTrainer
    sm = pair[1]
    with pytest.raises(ValueError):
        sm.evaluate(0, 1)
    with pytest.raises(ValueError):
        sm.evaluate(4, 0)
    with pytest.raises(ValueError):
        sm.evaluate(4, 1, draws=np.zeros((1, 3, 6), np.float32))
    fresh = StudentMlpTrainer(device=DEV)
    with pytest.raises(RuntimeError):
        fresh.evaluate(4, 1)
    out = torch.zeros(4, device=DEV)   # the C ABI's own answer with no teacher set
    cfg = RdmEvalConfig(n_envs=4, episodes=1)
    assert fresh._lib.rdm_evaluate(fresh._h, ctypes.byref(cfg), nat.ptr(out), None, None) == -100000
    assert "rdm_evaluate" in fresh._lib.rd_last_error().decode() and "teacher" in fresh._lib.rd_last_error().decode()
    fresh.close()


def test_evaluate_student_mlp_is_the_fused_returns(pair):
    """One env per episode, gym seeds seed + i: the returns of StudentMlpTrainer.evaluate, from a
    trainer or from its parameters; n_envs < episodes runs rounds."""
    from reacherdistilation_amd import evaluate
    tr, sm = pair
    (ret, _, _), _ = _gym_case(pair, 17, episodes=2, seed=7)
    one = evaluate.evaluate_student_mlp(sm, tr.teacher, 17, seed=7)
    assert one.shape == (17,) and one.dtype == np.float32 and np.array_equal(one, ret[0].cpu().numpy())
    rounds = evaluate.evaluate_student_mlp(sm.params().cpu().numpy(), tr.teacher, 30, n_envs=17, seed=7, device=DEV)
    assert rounds.shape == (30,) and np.array_equal(rounds, ret.reshape(-1)[:30].cpu().numpy())
    ph = evaluate.evaluate_student_mlp(sm, None, 6, n_envs=3, seed=4, reset="philox")
    assert ph.shape == (6,) and np.isfinite(ph).all()
