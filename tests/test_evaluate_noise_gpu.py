"""Evaluation under action noise (rdm_ / rdl_evaluate_noisy; evaluate(noise=...) of both students)
against the stepwise loops of tests/test_student_mlp_evaluate_gpu.py and
tests/test_student_lstm_evaluate_gpu.py with the student's pdflat passed through
action_noise.perturb_actions (rd_perturb_actions: the device function the fused kernels inline) before
env.step.  Bitwise (torch.equal): returns, final distances, every record, and the LSTM's final state.
Two episodes, n in {1, 17}, gym draw tables and Philox resets (first_episode = 3: the noise's episode
index is first_episode + e either way); and evaluate() without the keyword does not read the envs'
noise setting."""
import pytest
import torch

from tests.test_student_lstm_evaluate_gpu import rig   # noqa: F401
from tests.test_student_mlp_evaluate_gpu import pair   # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 50
F_REW, F_T, F_S, F_WITH = 11, 12, 16, 20
SEED, BASE, FIRST = 11, 5, 3
NOISES = [("policy", 1.0, 9), ("fixed", 0.3, None)]   # (mode, scale, noise seed; None: evaluate's seed)


def _stepwise(tr, student, env, episodes, shadow, noise, lstm):
    """The loop the noisy evaluations fuse, on ``env`` (its next reset opens the run's first episode):
    (returns [E, n], final distance [E, n], records [E, n, 50, 21], the LSTM's final state or None).
    ``noise`` = (mode, scale, seed, env_base, first_episode)."""
    from reacherdistilation_amd.action_noise import perturb_actions
    from reacherdistilation_amd.student_mlp import rows
    mode, scale, nseed, base, first = noise
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
            if lstm:
                obs.append(ob.clone())
                prevs.append(prev_t)
                k = min(s + 1, T)
                ob_w, prev_w = torch.zeros(T, n, 11, device=DEV), torch.zeros(T, n, 4, device=DEV)
                ob_w[T - k:] = torch.stack(obs[-k:])
                prev_w[T - k:] = torch.stack(prevs[-k:])
                out, state = student.forward(ob_w, prev_w, state)
                sf = out[T - 1]
            else:
                prev_r = rec[e, s - 1, :, F_REW].clone().view(n, 1) if s else torch.zeros(n, 1, device=DEV)
                sf = student.forward(rows(ob, prev_t, prev_r))   # the previous record's reward field
            act = perturb_actions(sf, mode=mode, scale=scale, seed=nseed, env_base=base, episode=first + e, step=s)
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


def _case(tr, student, n, table, mode, scale, nseed, lstm):
    """(the fused result, the stepwise reference) of one noisy evaluation"""
    from reacherdistilation_amd.env import BatchedReacher
    from reacherdistilation_amd.evaluate import gym_draw_table
    kw = dict(final_dist=True, records=True, noise=mode, noise_scale=scale, noise_seed=nseed)
    if lstm:
        kw["final_state"] = True
    key = SEED if nseed is None else nseed
    if table:   # gym draws: env_base = 0, first_episode = 0
        env = BatchedReacher(n, seed=SEED, device=DEV, reset="gym")
        res = student.evaluate(n, 2, seed=SEED, draws=gym_draw_table(SEED, n, 2), **kw)
        noise = (mode, scale, key, 0, 0)
    else:
        env = BatchedReacher(n, seed=SEED, device=DEV, env_base=BASE)
        for _ in range(FIRST):
            env.reset()   # each reset opens the next Philox episode
        res = student.evaluate(n, 2, seed=SEED, env_base=BASE, first_episode=FIRST, **kw)
        noise = (mode, scale, key, BASE, FIRST)
    shadow = BatchedReacher(n, device=DEV)
    ref = _stepwise(tr, student, env, 2, shadow, noise, lstm)
    torch.cuda.synchronize()
    env.close()
    shadow.close()
    return res, ref


def _same(res, ref):
    ret, dist, rec, state = ref
    assert torch.equal(res.records, rec)
    assert torch.equal(res.returns, ret)
    assert torch.equal(res.final_dist, dist)
    if state is not None:
        assert torch.equal(res.state, state)


@pytest.mark.parametrize("table", [True, False], ids=["table", "philox"])
@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("mode,scale,nseed", NOISES)
def test_mlp_noisy_evaluation_equals_the_stepwise_loop(pair, n, table, mode, scale, nseed):   # noqa: F811
    tr, sm = pair
    res, ref = _case(tr, sm, n, table, mode, scale, nseed, lstm=False)
    _same(res, ref)
    kw = dict(seed=SEED) if table else dict(seed=SEED, env_base=BASE, first_episode=FIRST)
    if table:
        from reacherdistilation_amd.evaluate import gym_draw_table
        kw["draws"] = gym_draw_table(SEED, n, 2)
    assert not torch.equal(sm.evaluate(n, 2, **kw).returns, res.returns)   # the noise bites


@pytest.mark.parametrize("table", [True, False], ids=["table", "philox"])
@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("mode,scale,nseed", NOISES)
def test_lstm_noisy_evaluation_equals_the_stepwise_loop(rig, n, table, mode, scale, nseed):   # noqa: F811
    tr, make = rig
    res, ref = _case(tr, make(10, n), n, table, mode, scale, nseed, lstm=True)
    _same(res, ref)


def test_lstm_noisy_evaluation_on_the_bf16_query(rig):   # noqa: F811
    """dtype = query_dtype = "bf16": the bf16 cell's noisy instance against the same loop on that trainer."""
    from reacherdistilation_amd.student_lstm import StudentLstmConfig, StudentLstmTrainer
    from tests.test_student_lstm_evaluate_gpu import _params
    tr, _ = rig
    st = StudentLstmTrainer(StudentLstmConfig(steps=10, max_windows=17, dtype="bf16", query_dtype="bf16"), device=DEV,
                            params=_params(T=10))
    st.set_teacher(tr.teacher)
    res, ref = _case(tr, st, 17, False, "policy", 1.0, 9, lstm=True)
    _same(res, ref)
    st.close()


def test_mlp_noisy_evaluation_in_bf16_and_64_env_blocks(pair):   # noqa: F811
    """The bf16 layers' noisy instance against the loop on that trainer (n = 17), and n = 83 on one
    workgroup (64-env blocks) against the automatic grid (16-env blocks): the same bits."""
    from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer
    tr, sm = pair
    bf = StudentMlpTrainer(StudentMlpConfig(dtype="bf16"), device=DEV)
    bf.set_teacher(tr.teacher)
    res, ref = _case(tr, bf, 17, False, "policy", 1.0, 9, lstm=False)
    _same(res, ref)
    kw = dict(seed=SEED, env_base=BASE, final_dist=True, records=True, noise="fixed", noise_scale=0.3)
    for t in (sm, bf):
        a, b = t.evaluate(83, 2, grid=1, **kw), t.evaluate(83, 2, **kw)
        assert torch.equal(a.returns, b.returns) and torch.equal(a.final_dist, b.final_dist)
        assert torch.equal(a.records, b.records)
    bf.close()


def test_evaluate_without_the_keyword_ignores_the_envs_noise(pair, rig):   # noqa: F811
    """A trainer whose envs act under noise still evaluates noiselessly: evaluate() equals a fresh
    twin's, for both students; and the native call refuses RD_NOISE_NONE."""
    import ctypes

    from reacherdistilation_amd import _native as nat
    from reacherdistilation_amd.student_mlp import RdmEvalConfig, StudentMlpTrainer
    tr, sm = pair
    twin = StudentMlpTrainer(device=DEV)
    twin.set_teacher(tr.teacher)
    twin.attach_envs(17, seed=SEED, accum_steps=7)
    twin.set_action_noise("fixed", 0.5)
    twin.act_envs()
    kw = dict(seed=SEED, env_base=BASE, final_dist=True, records=True)
    a, b = twin.evaluate(17, 2, **kw), sm.evaluate(17, 2, **kw)
    assert torch.equal(a.returns, b.returns) and torch.equal(a.records, b.records)
    assert twin.action_noise["mode"] == "fixed"
    c = RdmEvalConfig(n_envs=17, env_base=0, seed=0, episodes=1, first_episode=0, grid=0, draws=None)
    nz = nat.RdActionNoise(mode=0, scale=1.0, seed=0)
    out = torch.zeros(17, device=DEV)
    assert twin._lib.rdm_evaluate_noisy(twin._h, ctypes.byref(c), ctypes.byref(nz), nat.ptr(out), None, None) == -100000
    assert "RD_NOISE_NONE" in twin._lib.rd_last_error().decode()
    twin.close()
    st = rig[1](10, 17)
    st.attach_envs(17, seed=SEED, accum_steps=7)
    before = st.evaluate(17, 1, **kw)
    st.set_action_noise("policy", 1.0)
    st.act_envs(steps=7)
    after = st.evaluate(17, 1, **kw)
    assert torch.equal(before.returns, after.returns) and torch.equal(before.records, after.records)
    st.set_action_noise("none")
