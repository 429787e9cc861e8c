"""Batched on-policy distillation of the LSTM student over persistent envs (rdl_envs_act /
rdl_rollout_envs / rdl_step_envs; StudentLstmTrainer.attach_envs, act_envs, rollout_envs, step_envs)
against the paths it fuses: rdl_evaluate's records, and the stepwise loop of BatchedReacher (Philox
resets), DistillTrainer.forward (teacher), the window of the episode's last T records,
StudentLstmTrainer.forward from the carried state, and step on host-gathered windows.  The envs kernel
runs the stepwise forward's arithmetic in its order, so every comparison is bitwise (torch.equal): a
difference is a reordering to find, not a tolerance to add.  All tests use the default synthetic
teacher and tests/test_student_lstm_gpu.py's parameters (non-zero biases); T = 10 unless said."""
import numpy as np
import pytest
import torch

from oracle import lstm_np as ln

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 50
F_REW, F_T, F_S, F_WITH = 11, 12, 16, 20
RD_EINVAL = -100000


def _params(seed=6, T=10):
    """tests/test_student_lstm_gpu.py::_params: glorot kernels, biases uniform in [-0.1, 0.1]."""
    p = ln.init(seed, T)
    rs = np.random.RandomState(seed + 1)
    for k, (o, s) in ln.layout(T)[0].items():
        if len(s) == 1:
            p[o:o + s[0]] = rs.uniform(-.1, .1, s[0]).astype(np.float32)
    return p


@pytest.fixture(scope="module")
def tr():
    """The DistillTrainer whose forward is the stepwise teacher, and whose teacher every student gets."""
    from reacherdistilation_amd.distill import DistillConfig, DistillTrainer
    t = DistillTrainer(DistillConfig(n_envs=64, seed=3), device=DEV)
    yield t
    t.close()


def _student(tr, T=10, max_windows=64, teacher=True, **cfg):
    from reacherdistilation_amd.student_lstm import StudentLstmConfig, StudentLstmTrainer
    st = StudentLstmTrainer(StudentLstmConfig(steps=T, max_windows=max_windows, **cfg), device=DEV, params=_params(T=T))
    if teacher:
        st.set_teacher(tr.teacher)
    return st


class Stepwise:
    """The loop the envs kernel fuses, on a BatchedReacher with Philox resets: per step the teacher's
    pdflat, the window of the open episode's last T records (ob | the previous record's t_pdflat, 0 at
    its step 0; zero rows before it), position T-1 of the student's forward on it from the carried
    state, and env.step with the actor's mean.  The reward variable and the state run on over the
    resets, as the driver's do."""

    def __init__(self, tr, st, n, seed, env_base):
        from reacherdistilation_amd.env import BatchedReacher
        self.tr, self.st, self.n = tr, st, n
        self.env = BatchedReacher(n, seed=seed, device=DEV, env_base=env_base)
        self.ob = self.env.reset().clone()
        self.reward = torch.zeros(n, device=DEV)
        self.prev_t = torch.zeros(n, 4, device=DEV)
        self.obs, self.prevs = [], []
        self.state = None
        self.s = 0

    def steps(self, K, act_with="student"):
        """(records [K, n, 21], reward [K, n]) of the next K steps."""
        n, T, recs, rews = self.n, self.st.T, [], []
        for _ in range(K):
            t, _ = self.tr.forward(self.ob, teacher=True, student=False)
            self.obs.append(self.ob.clone())
            self.prevs.append(self.prev_t.clone() if self.s else torch.zeros(n, 4, device=DEV))
            if act_with == "student":
                k = min(self.s + 1, T)
                ob_w, prev_w = torch.zeros(T, n, 11, device=DEV), torch.zeros(T, n, 4, device=DEV)
                ob_w[T - k:] = torch.stack(self.obs[-k:])
                prev_w[T - k:] = torch.stack(self.prevs[-k:])
                out, self.state = self.st.forward(ob_w, prev_w, self.state)
                sf = out[T - 1].clone()
            else:
                sf = torch.zeros(n, 4, device=DEV)
            r = torch.zeros(n, 21, device=DEV)
            r[:, :F_REW] = self.ob
            r[:, F_REW] = self.reward
            r[:, F_T:F_S] = t
            r[:, F_S:F_WITH] = sf
            r[:, F_WITH] = 1.0 if act_with == "student" else 0.0
            act = (sf if act_with == "student" else t)[:, :2].contiguous()
            self.prev_t = t.clone()
            ob, rew, _, _ = self.env.step(act)
            self.ob, self.reward = ob.clone(), rew.clone()
            self.s = (self.s + 1) % STEPS
            if self.s == 0:
                self.obs, self.prevs = [], []
            recs.append(r)
            rews.append(self.reward)
        return torch.stack(recs), torch.stack(rews)

    def query_state(self):
        return self.state if self.state is not None else torch.zeros(2, self.n, 200, device=DEV)

    def close(self):
        self.env.close()


def _same_envs(st, loop):
    es, step, episode = loop.env.get_state()
    gs, gstep, gep = st.env_state()
    assert torch.equal(gs, es) and (gstep, gep) == (step, episode)
    assert torch.equal(st.query_state(), loop.query_state())


def _run_calls(st, calls, act="student"):
    recs, rews = [], []
    for K in calls:
        r = st.act_envs(act, steps=K)
        assert r.records.shape == (K, st.n_envs, 21) and r.reward.shape == (K, st.n_envs)
        recs.append(r.records.clone())
        rews.append(r.reward.clone())
    return torch.cat(recs), torch.cat(rews)


@pytest.mark.parametrize("n,grid", [(1, 0), (17, 0), (33, 1)])
def test_act_equals_the_stepwise_loop_bitwise(tr, n, grid):
    """57 steps as calls of 3, 50 and 4 -- the second crosses the episode's reset, the windows of the
    second and third reach into records of the call before -- for a ragged block (1), a full block and
    a ragged one (17), and three blocks walked by one workgroup, which reloads the carried state per
    block (33, grid = 1): records, rewards, env state, clock and (c, h) of the stepwise loop."""
    st = _student(tr, max_windows=n)
    st.attach_envs(n, seed=11, env_base=5, grid=grid, accum_steps=STEPS)
    loop = Stepwise(tr, st, n, 11, 5)
    rec, rew = _run_calls(st, (3, 50, 4))
    wrec, wrew = loop.steps(57)
    assert torch.equal(rec, wrec)
    assert torch.equal(rew, wrew)
    _same_envs(st, loop)
    assert st.env_state()[1:] == (7, 1)
    assert bool((rec[..., F_WITH] == 1).all()) and bool((rec[..., F_S:F_WITH] != 0).any())
    assert bool((rec[0, :, F_REW] == 0).all()) and bool((rec[STEPS, :, F_REW] != 0).all())   # carried over the reset
    loop.close()
    st.close()


def test_act_equals_evaluate(tr):
    """From a fresh attach, 100 student steps are evaluate(n, 2, seed=..., records=True,
    final_state=True): every record and the final (c, h), bit for bit -- and with them the oracle
    bound of tests/test_student_lstm_evaluate_gpu.py."""
    n, seed, base = 17, 11, 5
    st = _student(tr, max_windows=n)
    res = st.evaluate(n, 2, seed=seed, env_base=base, records=True, final_state=True)
    want = res.records.transpose(1, 2).reshape(2 * STEPS, n, 21)   # [E, n, 50, 21] -> [100, n, 21]
    st.attach_envs(n, seed=seed, env_base=base, accum_steps=STEPS)
    rec, rew = _run_calls(st, (50, 50))
    assert torch.equal(rec, want)
    assert torch.equal(st.query_state(), res.state)
    for e in range(2):
        ret = torch.zeros(n, device=DEV)
        for s in range(STEPS):
            ret = ret + rew[e * STEPS + s]
        assert torch.equal(ret, res.returns[e])
    assert st.env_state()[1:] == (0, 2)
    st.close()


@pytest.mark.parametrize("T", [3, 1])
def test_other_unroll_lengths(tr, T):
    n = 17
    st = _student(tr, T=T, max_windows=n)
    st.attach_envs(n, seed=2, accum_steps=STEPS)
    loop = Stepwise(tr, st, n, 2, 0)
    rec, rew = _run_calls(st, (3, 50, 4))
    wrec, wrew = loop.steps(57)
    assert torch.equal(rec, wrec) and torch.equal(rew, wrew)
    _same_envs(st, loop)
    loop.close()
    st.close()


def test_teacher_stepped_warm_up_then_the_student(tr):
    """act_with="teacher" (the drivers' warm-up): s_pdflat and stepped_with 0, (c, h) as it was -- after
    a student call, so that it is not zero -- and the records of the stepwise teacher-stepped loop; the
    student call after it goes on from the same envs and history."""
    n = 17
    st = _student(tr, max_windows=n)
    st.attach_envs(n, seed=11, env_base=5, accum_steps=STEPS)
    loop = Stepwise(tr, st, n, 11, 5)
    for act, K in (("student", 4), ("teacher", 7), ("student", 45)):
        q0 = st.query_state().clone()
        rec, rew = _run_calls(st, (K,), act)
        wrec, wrew = loop.steps(K, act)
        assert torch.equal(rec, wrec) and torch.equal(rew, wrew), act
        if act == "teacher":
            assert bool((rec[..., F_S:F_WITH] == 0).all()) and bool((rec[..., F_WITH] == 0).all())
            assert bool((rec[..., F_T:F_T + 2] != 0).any())
            assert torch.equal(st.query_state(), q0) and bool((q0 != 0).any())
        _same_envs(st, loop)
    assert st.env_state()[1:] == (6, 1)
    loop.close()
    st.close()


def test_parameters_replaced_mid_episode(tr):
    """act_envs(5), set_params(other), act_envs(5): the second call's windows hold records of the
    first, whose x rows (prev . Wp + bp) must be formed with the NEW Wp, bp, as the stepwise loop forms
    every window's at every query.  Reusing x rows carried from the first call fails this."""
    n = 17
    st = _student(tr, max_windows=n)
    p0, p1 = _params(), _params(seed=9)
    assert not np.array_equal(p0[:160], p1[:160])   # Wp, bp differ
    st.attach_envs(n, seed=11, env_base=5, accum_steps=STEPS)
    a = _run_calls(st, (5,))
    st.set_params(p1)
    b = _run_calls(st, (5,))
    q = st.query_state().clone()
    st.set_params(p0)
    loop = Stepwise(tr, st, n, 11, 5)
    wa = loop.steps(5)
    st.set_params(p1)
    wb = loop.steps(5)
    for u, v in zip(a + b, wa + wb):
        assert torch.equal(u, v)
    assert torch.equal(q, loop.query_state())
    loop.close()
    st.close()


def _host_windows(rec, T, first_step=0):
    """The training windows of the step-major records rec [G, n, 21] of consecutive lockstep steps
    (rec[0] at episode step first_step): for every step whose episode step s >= T-1, in step order
    then env order, the records s-T+1 .. s.  Returns (ob_w, prev_w, t_w, global step of each window's
    last record)."""
    G, n = rec.shape[:2]
    prev = torch.zeros(G, n, 4, device=rec.device)
    prev[1:] = rec[:-1, :, F_T:F_S]
    for g in range(G):
        if (first_step + g) % STEPS == 0:
            prev[g] = 0
    ends = [g for g in range(G) if (first_step + g) % STEPS >= T - 1 and g - T + 1 >= 0]
    idx = torch.tensor([[g - T + 1 + p for g in ends] for p in range(T)], device=rec.device)   # [T, W]
    ob_w = rec[idx][..., :F_REW].reshape(T, len(ends) * n, 11)
    prev_w = prev[idx].reshape(T, len(ends) * n, 4)
    t_w = rec[idx][..., F_T:F_S].reshape(T, len(ends) * n, 4)
    return ob_w, prev_w, t_w, ends


def test_windows_equal_the_host_gather(tr):
    """The windows of a 50-step call against windows gathered on the host from the concatenated
    records of all calls so far: with the clock at phase 0 (steps 9 .. 49 qualify) and at phase 23
    after act_envs(23) (steps 23 .. 49 of this episode, then 9 .. 22 of the next: the first nine
    windows reach into the 23 records of the call before).  B = n 41, ordered by step then env."""
    n, T = 17, 10
    st = _student(tr, max_windows=n)
    st.attach_envs(n, seed=11, env_base=5, accum_steps=STEPS)
    r = st.act_envs()
    assert r.ob_w.shape == (T, n * 41, 11) and r.prev_w.shape == r.t_w.shape == (T, n * 41, 4)
    all_rec = [r.records.clone()]
    ob_w, prev_w, t_w, ends = _host_windows(all_rec[0], T)
    assert ends == list(range(9, 50))
    assert torch.equal(r.ob_w, ob_w) and torch.equal(r.prev_w, prev_w) and torch.equal(r.t_w, t_w)
    assert bool((r.prev_w[0, :n] == 0).all()) and bool((r.prev_w[0, n:] != 0).any())   # step 9's window starts at record 0
    short = st.act_envs(steps=23)
    assert short.ob_w is None and short.prev_w is None and short.t_w is None
    all_rec.append(short.records.clone())
    r = st.act_envs()
    all_rec.append(r.records.clone())
    rec = torch.cat(all_rec)
    ob_w, prev_w, t_w, ends = _host_windows(rec, T)
    keep = [k for k, g in enumerate(ends) if g >= 73]   # the windows that end in the last call
    assert [ends[k] - 73 for k in keep] == list(range(0, 27)) + list(range(36, 50))
    cols = torch.tensor([k * n + i for k in keep for i in range(n)], device=DEV)
    assert r.ob_w.shape == (T, n * 41, 11)
    assert torch.equal(r.ob_w, ob_w[:, cols]) and torch.equal(r.prev_w, prev_w[:, cols])
    assert torch.equal(r.t_w, t_w[:, cols])
    assert st.env_state()[1:] == (23, 2)
    st.close()


@pytest.mark.parametrize("loss", ["kl", "mse"])
@pytest.mark.parametrize("keep_prob", [1.0, 0.5])
def test_step_envs_equals_act_then_step(tr, keep_prob, loss):
    """step_envs against a twin driven as act_envs, then step(ob_w, prev_w, t_w) on the windows it
    returned: after each of two optimiser steps (the second acts with the updated parameters, and its
    first windows reach into the first call's records) parameters, gradient, metrics, counter and
    final_state are equal bit for bit, and so are the buffers and the envs."""
    n, T = 17, 10
    B = n * 41
    cfg = dict(loss=loss, lr=1e-3, keep_prob=keep_prob, seed=4)
    fused, twin = _student(tr, max_windows=B, **cfg), _student(tr, max_windows=B, **cfg)
    for st in (fused, twin):
        st.attach_envs(n, seed=11, env_base=5, accum_steps=STEPS)
        st.act_envs(steps=23)   # phase 23: windows across the reset and into the earlier call
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
        assert torch.equal(fused.final_state(B), twin.final_state(B)), k
    assert fused.metrics(1)[0, 2] == T * B and np.isfinite(fused.metrics(2)).all()
    assert not torch.equal(fused.params(), torch.from_numpy(_params()).to(DEV))
    (sa, ka, ea), (sb, kb, eb) = fused.env_state(), twin.env_state()
    assert torch.equal(sa, sb) and (ka, ea) == (kb, eb) == (23, 2)
    assert torch.equal(fused.query_state(), twin.query_state())
    # rollout_envs: the same gradient, nothing applied
    p, c = fused.params().clone(), fused.counter()
    r = fused.rollout_envs()
    w = twin.act_envs()
    twin.rollout(w.ob_w, w.prev_w, w.t_w)
    assert torch.equal(r.ob_w, w.ob_w) and torch.equal(fused.grad(), twin.grad())
    assert torch.equal(fused.params(), p) and fused.counter() == c
    fused.close()
    twin.close()


def _batch(T, B, seed=0):
    rs = np.random.RandomState(seed)
    ob = rs.uniform(-1, 1, (T, B, 11)).astype(np.float32)
    prev = rs.uniform(-.5, .5, (T, B, 4)).astype(np.float32)
    t = np.concatenate([rs.uniform(-.5, .5, (T, B, 2)), rs.uniform(-1.0, -0.2, (T, B, 2))], 2).astype(np.float32)
    return tuple(torch.from_numpy(v).to(DEV) for v in (ob, prev, t))


def test_act_envs_has_no_side_effects(tr):
    """Params, Adam slots, gradient, counter and metrics are unchanged by act_envs (student, teacher,
    short and window-writing calls); reset_envs() and the same calls reproduce the first run's
    buffers; and a training step afterwards equals the same step on a trainer that never attached envs."""
    T, B = 10, 20
    ob, prev, t = _batch(T, B)
    a = _student(tr, max_windows=B, teacher=False, lr=1e-3)
    b = _student(tr, max_windows=B, lr=1e-3)
    for st in (a, b):
        st.step(ob, prev, t)
        st.rollout(ob, prev, t)
    b.attach_envs(17, seed=1, accum_steps=STEPS)
    p0, g0, c0, m0 = b.params().clone(), b.grad().clone(), b.counter(), b.metrics(1)
    s0 = [v.clone() for v in b._slots()]
    keep = lambda r: [v.clone() for v in (r.records, r.reward, r.ob_w, r.prev_w, r.t_w) if v is not None]
    run = lambda: [keep(b.act_envs()), keep(b.act_envs("teacher", steps=7)), keep(b.act_envs(steps=3))]
    first = run()
    assert torch.equal(b.params(), p0) and torch.equal(b.grad(), g0) and b.counter() == c0 == 1
    assert np.array_equal(b.metrics(1), m0)
    for u, v in zip(b._slots(), s0):
        assert torch.equal(u, v)
    assert len(first[0]) == 5 and len(first[1]) == 2 and b.env_state()[1:] == (10, 1)
    b.reset_envs()
    assert bool((b.query_state() == 0).all()) and b.env_state()[1:] == (0, 0)
    for u, v in zip(first, run()):
        for p, q in zip(u, v):
            assert torch.equal(p, q)
    for st in (a, b):
        st.step(ob, prev, t)
    assert torch.equal(a.params(), b.params()) and torch.equal(a.grad(), b.grad())
    assert a.counter() == b.counter() == 2 and np.array_equal(a.metrics(2), b.metrics(2))
    assert torch.equal(a.final_state(B), b.final_state(B))
    a.close()
    b.close()


def test_a_captured_step_replays_the_next_steps(tr):
    """step_envs captured and replayed twice: the clock is the device's, so the replays are two
    consecutive optimiser steps -- parameters, gradient, buffers, envs and (c, h) of two eager calls on
    a twin, bit for bit."""
    n = 17
    B = n * 41
    cfg = dict(loss="kl", lr=1e-3, keep_prob=0.5, seed=4)
    a, b = _student(tr, max_windows=B, **cfg), _student(tr, max_windows=B, **cfg)
    for st in (a, b):
        st.attach_envs(n, seed=11, env_base=5, accum_steps=STEPS)
        st.act_envs(steps=23)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(a.device)
    with torch.cuda.graph(g):
        res = a.step_envs()
    a._sync_stream()
    for _ in range(2):
        g.replay()
    for _ in range(2):
        want = b.step_envs()
    torch.cuda.synchronize(a.device)
    for name in ("records", "reward", "ob_w", "prev_w", "t_w"):
        assert torch.equal(getattr(res, name), getattr(want, name)), name
    assert torch.equal(a.params(), b.params()) and torch.equal(a.grad(), b.grad())
    assert a.counter() == b.counter() == 2 and np.array_equal(a.metrics(2), b.metrics(2))
    (sa, ka, ea), (sb, kb, eb) = a.env_state(), b.env_state()
    assert torch.equal(sa, sb) and (ka, ea) == (kb, eb) == (23, 2)
    assert torch.equal(a.query_state(), b.query_state())
    a.close()
    b.close()


def test_bad_arguments_raise(tr):
    from reacherdistilation_amd import _native as nat
    fresh = _student(tr, max_windows=20, teacher=False)
    lib = fresh._lib
    msg = lambda: lib.rd_last_error().decode()
    rec = torch.zeros(50, 4, 21, device=DEV)
    w = [torch.zeros(10, 4 * 41, d, device=DEV) for d in (11, 4, 4)]
    for call in (fresh.act_envs, fresh.rollout_envs, fresh.step_envs, fresh.reset_envs, fresh.env_state,
                 fresh.query_state):
        with pytest.raises(RuntimeError):   # no envs attached
            call()
    assert lib.rdl_envs_act(fresh._h, 1, 1, nat.ptr(rec), None, None, None, None, 0) == RD_EINVAL
    assert "rdl_envs_act" in msg() and "no envs attached" in msg()
    assert lib.rdl_step_envs(fresh._h, 1, 50, nat.ptr(rec), None, *(nat.ptr(x) for x in w)) == RD_EINVAL
    assert "rdl_step_envs" in msg() and "no envs attached" in msg()
    with pytest.raises(ValueError):
        fresh.attach_envs(0)
    with pytest.raises(ValueError):
        fresh.attach_envs(4, accum_steps=0)
    fresh.attach_envs(4, accum_steps=STEPS)
    with pytest.raises(RuntimeError):   # no teacher
        fresh.act_envs()
    for name in ("rdl_rollout_envs", "rdl_step_envs"):   # the C ABI's own answer
        assert getattr(lib, name)(fresh._h, 1, 50, nat.ptr(rec), None, *(nat.ptr(x) for x in w)) == RD_EINVAL
        assert name in msg() and "teacher" in msg()
    assert lib.rdl_envs_act(fresh._h, 1, 1, nat.ptr(rec), None, None, None, None, 0) == RD_EINVAL
    assert "rdl_envs_act" in msg() and "teacher" in msg()
    fresh.set_teacher(tr.teacher)
    with pytest.raises(ValueError):
        fresh.act_envs(steps=0)
    with pytest.raises(ValueError):
        fresh.act_envs(steps=51)   # more than the buffers hold
    with pytest.raises(ValueError):
        fresh.act_envs("expert")
    assert lib.rdl_envs_act(fresh._h, 2, 1, nat.ptr(rec), None, None, None, None, 0) == RD_EINVAL
    assert "rdl_envs_act" in msg() and "act_with" in msg()
    for call in (fresh.step_envs, fresh.rollout_envs):
        with pytest.raises(nat.NativeError, match="multiple"):   # steps = 49
            call(steps=49)
        with pytest.raises(nat.NativeError, match="max_windows"):   # B = 4 x 41 = 164 > 20
            call()
    assert fresh.act_envs(steps=49).records.shape == (49, 4, 21) and fresh.counter() == 0
    fresh.close()
    long = _student(tr, T=17, max_windows=20)   # T > RDL_EVAL_MAX_STEPS
    long.attach_envs(4, accum_steps=STEPS)
    for call in (long.act_envs, long.step_envs):
        with pytest.raises(nat.NativeError, match="16"):
            call()
    torch.cuda.synchronize()
    long.close()


def test_train_envs_smoke():
    """16 envs, 4 optimiser steps of 50 env steps, the first one teacher-stepped: four finite history
    rows whose losses are the trainer's metrics ring, on 16 x 41 windows each.  No falling loss is
    asserted (the MLP driver's curve was not monotone at smoke settings); a longer curve is in
    profiles/student_lstm_envs_fused_vs_stepwise.json."""
    from reacherdistilation_amd import lstm_train
    st, history = lstm_train.train_envs(16, 4, keep_prob=0.5, warmup_steps=1)
    h = np.asarray(history, np.float64)
    print("train_envs history (step, loss, action-MSE, mean step reward):")
    for row in history:
        print("  %3d %.6f %.6f %.6f" % row)
    assert h.shape == (4, 4) and np.isfinite(h).all()
    assert np.array_equal(h[:, 0], np.arange(1, 5)) and st.counter() == 4
    m = st.metrics(4)
    assert np.array_equal(h[:, 1], m[:, 0]) and np.all(m[:, 2] == 10 * 16 * 41)
    assert np.array_equal(h[:, 2], m[:, 1] / (2 * m[:, 2])) and np.all(h[:, 3] < 0)
    assert st.env_state()[1:] == (0, 4)
    st.close()
