"""Whole-episode evaluation in one launch (rdd_evaluate / DistillTrainer.evaluate,
reacherdistilation_amd.evaluate) against the stepwise loops it replaces: BatchedReacher stepped
with DistillTrainer.forward's means.  The fused kernel calls the same device functions in the
same order, so every comparison is bitwise (torch.equal): a difference is a reordering to find,
not a tolerance to add."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 50
F_REW, F_T, F_S, F_WITH = 11, 12, 16, 20


@pytest.fixture(scope="module")
def trainers():
    """One small trainer per student dtype (default teacher and student), shared by the tests: evaluate
    and forward leave a trainer unchanged."""
    from reacherdistilation_amd.distill import DistillConfig, DistillTrainer
    trs = {dt: DistillTrainer(DistillConfig(n_envs=64, seed=3, student_dtype=dt), device=DEV) for dt in ("f32", "bf16")}
    yield trs
    for tr in trs.values():
        tr.close()


def _stepwise(tr, policy, env, episodes, shadow):
    """The loop rdd_evaluate fuses, on ``env`` (its next reset opens episode 0 of the run):
    returns [E, n], final distance [E, n], records [E, n, 50, 21] (both pdflats when the student
    steps, the teacher's alone otherwise).  The final distance of an episode is read from
    ``shadow``: the env's state before the episode's last step, stepped there without the reset,
    then stepped with a zero action, whose reward is exactly -|fingertip - target|."""
    n = env.n
    student = policy == "student"
    ob = env.reset()
    reward = torch.zeros(n, device=DEV)
    zero = torch.zeros(n, 2, device=DEV)
    rets, dists = [], []
    rec = torch.zeros(episodes, STEPS, n, 21, device=DEV)
    for e in range(episodes):
        ret = torch.zeros(n, dtype=torch.float32, device=DEV)
        for s in range(STEPS):
            t, sf = tr.forward(ob, teacher=True, student=student)
            act = (sf if student else t)[:, :2].contiguous()
            r = rec[e, s]
            r[:, :F_REW] = ob
            r[:, F_REW] = reward
            r[:, F_T:F_S] = t
            if student:
                r[:, F_S:F_WITH] = sf
                r[:, F_WITH] = 1.0
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


def _gym_case(tr, policy, n, episodes=2, seed=7):
    from reacherdistilation_amd.env import BatchedReacher
    from reacherdistilation_amd.evaluate import gym_draw_table
    env, shadow = BatchedReacher(n, seed=seed, device=DEV, reset="gym"), BatchedReacher(n, device=DEV)
    ref = _stepwise(tr, policy, env, episodes, shadow)
    env.close()
    shadow.close()
    return ref, gym_draw_table(seed, n, episodes)


@pytest.mark.parametrize("n", [1, 17, 83])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("policy", ["teacher", "student"])
def test_fused_equals_stepwise_bitwise(trainers, policy, dtype, n):
    """Gym draw table (env i seeded seed + i), E = 2: returns, final distances and each episode's
    first observation equal the stepwise run's, bit for bit."""
    tr = trainers[dtype]
    (ret, dist, rec), draws = _gym_case(tr, policy, n)
    res = tr.evaluate(policy, n, 2, draws=draws, final_dist=True, records=True)
    torch.cuda.synchronize()
    assert res.returns.shape == (2, n) and res.final_dist.shape == (2, n) and res.records.shape == (2, n, STEPS, 21)
    assert torch.equal(res.returns, ret)
    assert torch.equal(res.final_dist, dist)
    assert torch.equal(res.records[:, :, 0, :F_REW], rec[:, :, 0, :F_REW])
    assert bool(torch.isfinite(res.returns).all()) and bool((res.returns < 0).all()) and bool((res.final_dist >= 0).all())
    # the optional outputs do not change the returns
    assert torch.equal(tr.evaluate(policy, n, 2, draws=draws).returns, ret)


@pytest.mark.parametrize("dtype,policy", [("f32", "teacher"), ("bf16", "student")])
def test_groups_of_64_equal_groups_of_16_and_the_stepwise_run(trainers, dtype, policy):
    """n = 595 on one workgroup (grid=1) runs as 64-env groups -- nine full ones, then a full
    16-env tile and a 3-env partial tile -- and on the automatic grid as 16-env groups: the same
    bits, and the stepwise run's."""
    tr, n = trainers[dtype], 595
    (ret, dist, rec), draws = _gym_case(tr, policy, n, episodes=1)
    a = tr.evaluate(policy, n, 1, draws=draws, final_dist=True, records=True, grid=1)
    b = tr.evaluate(policy, n, 1, draws=draws, final_dist=True, records=True)
    torch.cuda.synchronize()
    for x, y in ((a.returns, b.returns), (a.final_dist, b.final_dist), (a.records, b.records)):
        assert torch.equal(x, y)
    assert torch.equal(a.returns, ret) and torch.equal(a.final_dist, dist) and torch.equal(a.records, rec)


@pytest.mark.parametrize("first_episode", [0, 3])
def test_philox_resets(trainers, first_episode):
    """draws=None: episode e resets from Philox(seed, env_base + i, first_episode + e), as
    BatchedReacher's Philox mode does."""
    from reacherdistilation_amd.env import BatchedReacher
    tr, n, seed, base = trainers["f32"], 83, 11, 5
    env, shadow = BatchedReacher(n, seed=seed, device=DEV, env_base=base), BatchedReacher(n, device=DEV)
    for _ in range(first_episode):
        env.reset()   # each reset opens the next Philox episode
    ret, dist, rec = _stepwise(tr, "teacher", env, 2, shadow)
    res = tr.evaluate("teacher", n, 2, seed=seed, env_base=base, first_episode=first_episode, final_dist=True,
                      records=True)
    torch.cuda.synchronize()
    assert torch.equal(res.returns, ret) and torch.equal(res.final_dist, dist)
    assert torch.equal(res.records[:, :, 0, :F_REW], rec[:, :, 0, :F_REW])
    env.close()
    shadow.close()


def test_envs_are_isolated_and_the_layout_does_not_matter(trainers):
    tr = trainers["bf16"]
    kw = dict(seed=9, first_episode=1, final_dist=True, records=True)
    a = tr.evaluate("student", 83, 2, env_base=0, **kw)
    b = tr.evaluate("student", 19, 2, env_base=64, **kw)       # envs 64..82 on their own
    c = tr.evaluate("student", 83, 2, env_base=0, grid=1, **kw)
    d = tr.evaluate("student", 83, 2, env_base=0, **kw)
    torch.cuda.synchronize()
    assert torch.equal(a.returns[:, 64:], b.returns) and torch.equal(a.final_dist[:, 64:], b.final_dist)
    assert torch.equal(a.records[:, 64:], b.records)
    for other in (c, d):
        assert torch.equal(a.returns, other.returns) and torch.equal(a.final_dist, other.final_dist)
        assert torch.equal(a.records, other.records)
    # seed=None is the trainer's seed (3)
    assert torch.equal(tr.evaluate("student", 19, 1).returns, tr.evaluate("student", 19, 1, seed=3).returns)
    assert not torch.equal(tr.evaluate("student", 19, 1).returns, tr.evaluate("student", 19, 1, seed=4).returns)


@pytest.mark.parametrize("episodes,n_envs", [(5, 3), (4, 1)])
def test_collect_episodes_equals_collect_reward(episodes, n_envs):
    """The fused collector leaves the dataset teacher.collect_reward leaves ((4, 1): lstm_train's
    warm-up), reward column carried over the resets included."""
    from reacherdistilation_amd import evaluate, teacher
    a = evaluate.collect_episodes(episodes, n_envs, seed=0, device=DEV)
    b = teacher.collect_reward(episodes, n_envs, seed=0, device=DEV)
    torch.cuda.synchronize()
    assert a.num_episodes() == b.num_episodes() == episodes and a.lens[:episodes] == b.lens[:episodes]
    assert torch.equal(a.ring[:episodes], b.ring[:episodes])
    assert float(a.ring[0, 0, F_REW]) == 0.0 and float(a.ring[n_envs, 0, F_REW]) != 0.0   # carried over the reset


def test_collect_episodes_in_chunks_and_through_the_page_store(tmp_path, monkeypatch):
    """One round per launch (each later chunk replays the round before it for the carried reward)
    and page-by-page dumps: the same ring and the same pages as collect_reward."""
    from reacherdistilation_amd import evaluate, teacher
    from reacherdistilation_amd.config import MAX_CAPACITY
    from reacherdistilation_amd.pages import read_page
    monkeypatch.setattr(evaluate, "CHUNK_EPISODES", 3)
    a = evaluate.collect_episodes(8, 3, seed=2, device=DEV, reset="philox")
    b = teacher.collect_reward(8, 3, seed=2, device=DEV, reset="philox")
    assert a.num_episodes() == b.num_episodes() == 8 and torch.equal(a.ring[:8], b.ring[:8])
    monkeypatch.setattr(evaluate, "CHUNK_EPISODES", 16384)
    k = MAX_CAPACITY + 3
    pa, pb = tmp_path / "a", tmp_path / "b"
    a = evaluate.collect_episodes(k, 8, seed=1, device=DEV, store_dir=str(pa))
    b = teacher.collect_reward(k, 8, seed=1, device=DEV, store_dir=str(pb))
    assert torch.equal(a.ring[:k], b.ring[:k])
    fa, fb = a.store.sorted_pages(), b.store.sorted_pages()
    assert len(fa) == len(fb) == 1 and read_page(fa[0]) == read_page(fb[0])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_student_stepped_records(trainers, dtype):
    """n = 17, E = 2, the student stepping: every record equals the stepwise loop's -- both
    pdflats, stepped_with = 1, the reward carried over the reset at (e = 1, s = 0)."""
    tr = trainers[dtype]
    (ret, dist, rec), draws = _gym_case(tr, "student", 17)
    res = tr.evaluate("student", 17, 2, draws=draws, records=True)
    torch.cuda.synchronize()
    assert torch.equal(res.records, rec)
    r = res.records
    assert bool((r[..., F_WITH] == 1).all()) and bool((r[0, :, 0, F_REW] == 0).all())
    assert bool((r[1, :, 0, F_REW] != 0).all()) and bool((r[..., F_S:F_S + 2] != r[..., F_T:F_T + 2]).any())
    # records' rewards are the returns' terms, shifted by one step
    assert torch.equal(r[0, :, 1:, F_REW], rec[0, :, 1:, F_REW])


def test_teacher_stepped_records_leave_the_student_fields_zero(trainers):
    tr = trainers["bf16"]
    (ret, dist, rec), draws = _gym_case(tr, "teacher", 17)
    res = tr.evaluate("teacher", 17, 2, draws=draws, records=True)
    torch.cuda.synchronize()
    assert torch.equal(res.records, rec)
    assert float(res.records[..., F_S:].abs().sum()) == 0.0


def test_evaluate_has_no_side_effects():
    """Two identical trainers take 3 steps; one of them evaluates both policies between the
    steps: env state, student parameters, counters and metrics end bitwise equal."""
    from reacherdistilation_amd.distill import DistillConfig, DistillTrainer
    cfg = dict(n_envs=64, seed=5, act_with="student", loss="kl", lr=1e-3, metrics_len=16)
    a, b = (DistillTrainer(DistillConfig(**cfg), device=DEV) for _ in range(2))
    for _ in range(3):
        a.step()
        b.step()
        for policy in ("teacher", "student"):
            b.evaluate(policy, 83, 2, final_dist=True, records=True)
    torch.cuda.synchronize()
    assert torch.equal(a.env_state(), b.env_state())
    assert torch.equal(a.student_params(), b.student_params())
    assert torch.equal(a.grad(), b.grad())
    assert a.counters() == b.counters() == (3, 3)
    assert np.array_equal(a.metrics(3), b.metrics(3))
    a.close()
    b.close()


def _graph_nodes(graph: int) -> int:
    """Nodes of a captured HIP graph (hipGraphGetNodes of the runtime torch loaded)."""
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    hip = ctypes.CDLL(path)
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphGetNodes.restype = ctypes.c_int
    cnt = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(ctypes.c_void_p(graph), None, ctypes.byref(cnt)) == 0
    return cnt.value


def test_one_launch_captures_into_a_single_node_graph(trainers):
    """Captured on a side stream the way DistillTrainer.capture does, and replayed twice: the
    eager result both times, from a graph of one kernel node (no workspace, no copies)."""
    from reacherdistilation_amd.evaluate import gym_draw_table
    tr, n = trainers["f32"], 83
    draws = torch.from_numpy(gym_draw_table(7, n, 2)).to(DEV)
    kw = dict(draws=draws, final_dist=True, records=True)
    eager = tr.evaluate("teacher", n, 2, **kw)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    prev = torch.cuda.current_stream(tr.device)
    torch.cuda.synchronize(tr.device)
    try:
        with torch.cuda.graph(g):
            tr.set_stream(torch.cuda.current_stream(tr.device))
            res = tr.evaluate("teacher", n, 2, **kw)
    finally:
        tr.set_stream(prev)
    assert _graph_nodes(g.raw_cuda_graph()) == 1
    for _ in range(2):
        for t in (res.returns, res.final_dist, res.records):
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize(tr.device)
        assert torch.equal(res.returns, eager.returns) and torch.equal(res.final_dist, eager.final_dist)
        assert torch.equal(res.records, eager.records)


def test_evaluate_policy_is_the_fused_episode_returns():
    """One env per episode, gym seeds seed + i: the episodes of teacher.episode_returns (which sums
    the same f32 rewards in f64: equal to f32 rounding), and n_envs < episodes runs rounds."""
    from reacherdistilation_amd import evaluate, teacher
    from reacherdistilation_amd.policy import synthetic_teacher
    pi = synthetic_teacher(1)
    fused = evaluate.evaluate_policy(pi, 19, seed=4, device=DEV)
    ref = teacher.episode_returns(pi, 19, seed=4, device=DEV)
    assert fused.shape == (19,) and fused.dtype == np.float32
    np.testing.assert_allclose(fused, ref, rtol=0, atol=50 * 2.0 ** -24 * np.abs(ref).max())
    rounds = evaluate.evaluate_policy(pi, 5, n_envs=3, seed=4, device=DEV)
    assert rounds.shape == (5,) and np.array_equal(rounds[:3], fused[:3])
    ph = evaluate.evaluate_policy(pi, 6, n_envs=3, seed=4, reset="philox", device=DEV)
    assert ph.shape == (6,) and np.isfinite(ph).all() and not np.array_equal(ph[:3], fused[:3])
