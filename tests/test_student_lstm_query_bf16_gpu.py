"""The LSTM student's closed-loop query on its bf16 cell (rdl_set_query_dtype's RDL_DTYPE_BF16,
StudentLstmConfig.query_dtype = "bf16"; csrc/student_lstm_query_bf16.h): rdl_evaluate, rdl_envs_act and
the act phase of rdl_step_envs against the stepwise loop run with the SAME bf16 handle, whose forward is
the bf16 window pass.  A query step is that pass's arithmetic operation for operation, so every
comparison with the stepwise path is bitwise (torch.equal): a difference is a reordering to find, not a
tolerance to add.  Independent of the product's forwards, the records are compared with the emulation
chain of tests/lstm_query_bf16.py (rounded operands, f64 sums) in the bf16 forward test's form.
All tests use the default synthetic teacher and tests/test_student_lstm_gpu.py's parameters.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import policy_np as pn
from tests import lstm_query_bf16 as lq
from tests.test_student_lstm_envs_gpu import STEPS, Stepwise, _run_calls, _same_envs, _student, tr   # noqa: F401
from tests.test_student_lstm_evaluate_gpu import _oracle_chain, _stepwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F_REW, F_T, F_S, F_WITH = 11, 12, 16, 20
ALL = dict(final_dist=True, records=True, final_state=True)
BF = dict(dtype="bf16", query_dtype="bf16")
RD_EINVAL = -100000


@pytest.fixture(scope="module")
def make(tr):   # noqa: F811
    """make(T, B): a cached bf16 trainer of T unrolled steps and max_windows B with the bf16 query and
    the teacher set.  forward and evaluate leave the parameters unchanged, so the tests share them; a
    test that switches the query dtype switches it back."""
    made = {}

    def get(T, B):
        if (T, B) not in made:
            made[T, B] = _student(tr, T=T, max_windows=B, **BF)
        return made[T, B]

    yield get
    for st in made.values():
        st.close()


_CASES = {}


def _case(tr, make, n, T=10, episodes=2, seed=7, with_state=False):   # noqa: F811
    """The stepwise reference of one case, computed once and shared: (reference, draw table, state0)."""
    from reacherdistilation_amd.env import BatchedReacher
    from reacherdistilation_amd.evaluate import gym_draw_table
    key = (n, T, episodes, seed, with_state)
    if key not in _CASES:
        state0 = None
        if with_state:
            state0 = torch.from_numpy(np.random.RandomState(5).uniform(-.5, .5, (2, n, 200)).astype(np.float32)).to(DEV)
        env, shadow = BatchedReacher(n, seed=seed, device=DEV, reset="gym"), BatchedReacher(n, device=DEV)
        ref = _stepwise(tr, make(T, n), env, episodes, shadow, state0)
        env.close()
        shadow.close()
        _CASES[key] = (ref, gym_draw_table(seed, n, episodes), state0)
    return _CASES[key]


def _same(res, ref):
    ret, dist, rec, state = ref
    assert torch.equal(res.records, rec)
    assert torch.equal(res.returns, ret)
    assert torch.equal(res.final_dist, dist)
    assert torch.equal(res.state, state)


# ---------------------------------------------------------------- 1. fused equals stepwise
@pytest.mark.parametrize("n,grid,with_state", [(1, 0, False), (17, 0, False), (33, 0, False), (33, 1, False),
                                               (17, 0, True)])
def test_fused_equals_stepwise_bitwise(tr, make, n, grid, with_state):   # noqa: F811
    """Gym draw table, E = 2, T = 10: returns, final distances, every record and the final state equal
    the stepwise run's with the same bf16 handle, bit for bit -- a ragged block (1), a full and a ragged
    one (17), three blocks on three workgroups and on one, which walks them in turn and reloads the
    state (33, grid = 1), and a given state0."""
    st = make(10, n)
    assert st.query_dtype == "bf16"
    ref, draws, state0 = _case(tr, make, n, with_state=with_state)
    res = st.evaluate(n, 2, draws=draws, state0=state0, grid=grid, **ALL)
    torch.cuda.synchronize()
    _same(res, ref)
    assert bool(torch.isfinite(res.returns).all()) and bool((res.records[..., F_WITH] == 1).all())


@pytest.mark.parametrize("T", [3, 1])
def test_other_unroll_lengths(tr, make, T):   # noqa: F811
    n = 17
    st = make(T, n)
    ref, draws, _ = _case(tr, make, n, T=T)
    res = st.evaluate(n, 2, draws=draws, **ALL)
    torch.cuda.synchronize()
    _same(res, ref)


# ---------------------------------------------------------------- 2. the bf16 path ran
def test_the_setting_selects_the_arithmetic(tr, make):   # noqa: F811
    """On one handle: the records' s_pdflat under the bf16 query differ from those under the f32 query
    in at least half of the elements (the share the bf16 forward test demands against the f64 oracle);
    query_dtype reports the setting; and back on "f32" the handle returns the bits of an f32 handle
    with the same parameters (test_student_lstm_bf16_gpu.py::test_queries_stay_f32_on_the_master)."""
    n = 17
    st = make(10, n)
    _, draws, _ = _case(tr, make, n)
    b = st.evaluate(n, 2, draws=draws, **ALL)
    try:
        st.set_query_dtype("f32")
        assert st.query_dtype == "f32" and st._lib.rdl_query_dtype(st._h) == 0
        f = st.evaluate(n, 2, draws=draws, **ALL)
    finally:
        st.set_query_dtype("bf16")
    assert st.query_dtype == "bf16" and st._lib.rdl_query_dtype(st._h) == 1
    again = st.evaluate(n, 2, draws=draws, **ALL)
    share = float((b.records[..., F_S:F_WITH] != f.records[..., F_S:F_WITH]).float().mean())
    print(f"s_pdflat elements that differ between the bf16 and the f32 query: {share:.3f}")
    assert share >= 0.5, share
    assert torch.equal(again.records, b.records) and torch.equal(again.state, b.state)
    hf = _student(tr, max_windows=n)
    want = hf.evaluate(n, 2, draws=draws, **ALL)
    for name in ("returns", "final_dist", "records", "state"):
        assert torch.equal(getattr(f, name), getattr(want, name)), name
    hf.close()


# ---------------------------------------------------------------- 3. independent of the product's forwards
def test_records_against_the_emulation_chain(tr, make):   # noqa: F811
    """n = 17, E = 2, T = 10.  Every window is rebuilt on the host from the returned records,
    tests.lstm_bf16.forward (rounded operands, f64 sums) runs the 100 queries with the state chained in
    the emulation, and position T-1's pdflat is compared with the records' s_pdflat in the bf16 forward
    test's form: median |got - emulation| <= 5e-5, max |got - emulation| <= max |emulation chain - f64
    oracle chain|.  The stepwise loop with the same handle is the reference for whether that cap can be
    relied on over a chain; its two quantities are printed first.  Measured on an MI355X, the stepwise
    loop: median 1.425e-07, max 2.299e-04 against the cap 1.649e-03 (0.14 of it; the fused launch's
    records are the same bits), so the cap is kept as it is.  (A single forward's max is ~4e-5: over
    the chain a rounding that flips near a tie stays in the carried state; the host-side stand-in with
    f32 sums shows the same, 1.4e-4 against 7.3e-4.)
    The teacher's fields are checked as in test_records_against_the_oracles."""
    n, E, T = 17, 2, 10
    st = make(T, n)
    ref, draws, _ = _case(tr, make, n)
    rec = st.evaluate(n, E, draws=draws, records=True).records.cpu().numpy()
    params = st.params().cpu().numpy()
    quantities = {}
    for name, r in (("stepwise loop", ref[2].cpu().numpy()), ("fused", rec)):
        emu, ora = lq.emulation_chain(r, params, T), _oracle_chain(r, params, T)
        quantities[name] = lq.bounds(r[..., F_S:F_WITH], emu, ora)
        print("%s: median |got - emulation| %.3e  max %.3e  cap max |emulation - oracle| %.3e" % (name, *quantities[name]))
    med, mx, cap = quantities["fused"]
    assert med <= 5e-5, med
    assert mx <= cap, (mx, cap)
    p = tr.teacher
    ob = rec[..., :F_REW].reshape(-1, 11).astype(np.float64)
    ft = pn.forward(p.flat.astype(np.float64), p.ob_mean.astype(np.float64), p.ob_std.astype(np.float64), ob)
    np.testing.assert_allclose(rec[..., F_T:F_T + 2].reshape(-1, 2), ft["mean"], atol=2e-5, rtol=1e-5)
    assert np.all(rec[..., F_T + 2:F_S] == p.flat[pn.P_LS:].astype(np.float32))
    assert np.all(rec[0, :, 0, F_REW] == 0.0) and np.any(rec[1, :, 0, F_REW] != 0.0)


# ---------------------------------------------------------------- 4. the persistent envs
@pytest.mark.parametrize("n,grid", [(17, 0), (33, 1)])
def test_act_equals_evaluate(tr, n, grid):   # noqa: F811
    """From a fresh attach, 100 student steps are evaluate(n, 2) with Philox resets of the same seed and
    env_base: every record and the final (c, h), bit for bit."""
    seed, base = 11, 5
    st = _student(tr, max_windows=n, **BF)
    res = st.evaluate(n, 2, seed=seed, env_base=base, records=True, final_state=True)
    want = res.records.transpose(1, 2).reshape(2 * STEPS, n, 21)
    st.attach_envs(n, seed=seed, env_base=base, grid=grid, accum_steps=STEPS)
    rec, rew = _run_calls(st, (50, 50))
    assert torch.equal(rec, want)
    assert torch.equal(st.query_state(), res.state)
    assert bool((rec[..., F_S:F_WITH] != 0).any()) and st.env_state()[1:] == (0, 2)
    # and the f32 query on the same handle acts otherwise
    st.set_query_dtype("f32")
    st.reset_envs()
    assert not torch.equal(_run_calls(st, (50,))[0], want[:50])
    st.close()


def test_teacher_stepped_warm_up_then_the_student(tr):   # noqa: F811
    """50 teacher-stepped steps (no cell, (c, h) untouched), then the student on the history they left:
    bitwise the stepwise loop with the same bf16 handle."""
    n = 17
    st = _student(tr, max_windows=n, **BF)
    st.attach_envs(n, seed=11, env_base=5, accum_steps=STEPS)
    loop = Stepwise(tr, st, n, 11, 5)
    for act, K in (("teacher", 50), ("student", 27)):
        rec, rew = _run_calls(st, (K,), act)
        wrec, wrew = loop.steps(K, act)
        assert torch.equal(rec, wrec) and torch.equal(rew, wrew), act
        _same_envs(st, loop)
    assert bool((rec[..., F_S:F_WITH] != 0).any()) and st.env_state()[1:] == (27, 1)
    loop.close()
    st.close()


# ---------------------------------------------------------------- 5. step_envs
@pytest.mark.parametrize("loss", ["mse", "kl"])
@pytest.mark.parametrize("keep_prob", [1.0, 0.5])
def test_step_envs_equals_act_then_step(tr, keep_prob, loss):   # noqa: F811
    """step_envs("student") against a twin driven as act_envs, then step on the windows it returned:
    parameters, gradient, metrics, counter, final_state, records and windows equal bit for bit over two
    optimiser steps."""
    n, T = 17, 10
    B = n * 41
    cfg = dict(loss=loss, lr=1e-3, keep_prob=keep_prob, seed=4, **BF)
    fused, twin = _student(tr, max_windows=B, **cfg), _student(tr, max_windows=B, **cfg)
    for st in (fused, twin):
        st.attach_envs(n, seed=11, env_base=5, accum_steps=STEPS)
        st.act_envs(steps=23)
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
    assert torch.equal(fused.query_state(), twin.query_state())
    for st in (fused, twin):
        st.close()


def test_the_second_step_envs_queries_with_the_re_formed_image(tr):   # noqa: F811
    """The bf16 query reads the handle's forward image, which every Adam step re-forms: the second
    step_envs' records differ from those of a handle that acted without stepping, and equal the stepwise
    loop whose forwards run on the stepped parameters."""
    n = 17
    B = n * 41
    cfg = dict(loss="kl", lr=1e-3, keep_prob=0.5, seed=4, **BF)
    fused, idle, ref = (_student(tr, max_windows=B, **cfg) for _ in range(3))
    for st in (fused, idle):
        st.attach_envs(n, seed=11, env_base=5, accum_steps=STEPS)
        st.act_envs(steps=23)
    first = fused.step_envs().records.clone()
    assert torch.equal(idle.act_envs().records, first)   # the first act phase: the same parameters still
    p1 = fused.params().clone()
    second = fused.step_envs().records.clone()
    assert not torch.equal(idle.act_envs().records, second)
    loop = Stepwise(tr, ref, n, 11, 5)
    wrec, _ = loop.steps(23 + STEPS)
    assert torch.equal(wrec[23:], first)
    ref.set_params(p1)
    wrec, _ = loop.steps(STEPS)
    assert torch.equal(wrec, second)
    loop.close()
    for st in (fused, idle, ref):
        st.close()


# ---------------------------------------------------------------- 6. no side effects
def test_the_bf16_query_has_no_side_effects(tr):   # noqa: F811
    """evaluate and act_envs under the bf16 query leave the parameters, the Adam slots and counter, the
    gradient, the metrics and final_state as they were, and a following step equals a twin's that never
    queried."""
    from tests.test_student_lstm_envs_gpu import _batch
    T, B = 10, 20
    ob, prev, t = _batch(T, B)
    a = _student(tr, max_windows=B, teacher=False, lr=1e-3, **BF)
    b = _student(tr, max_windows=B, lr=1e-3, **BF)
    for st in (a, b):
        st.step(ob, prev, t)
        st.rollout(ob, prev, t)
    b.attach_envs(17, seed=1, accum_steps=STEPS)
    p0, g0, c0, m0, f0 = b.params().clone(), b.grad().clone(), b.counter(), b.metrics(1), b.final_state(B).clone()
    s0 = [v.clone() for v in b._slots()]
    b.evaluate(17, 2, seed=1, **ALL)
    b.evaluate(35, 1, seed=1, grid=1)
    b.act_envs()
    b.act_envs("teacher", steps=7)
    b.act_envs(steps=3)
    torch.cuda.synchronize()
    assert torch.equal(b.params(), p0) and torch.equal(b.grad(), g0) and b.counter() == c0 == 1
    assert np.array_equal(b.metrics(1), m0) and torch.equal(b.final_state(B), f0)
    for u, v in zip(b._slots(), s0):
        assert torch.equal(u, v)
    for st in (a, b):
        st.step(ob, prev, t)
    assert torch.equal(a.params(), b.params()) and torch.equal(a.grad(), b.grad())
    assert a.counter() == b.counter() == 2 and np.array_equal(a.metrics(2), b.metrics(2))
    assert torch.equal(a.final_state(B), b.final_state(B))
    a.close()
    b.close()


# ---------------------------------------------------------------- 7. graph capture
def test_a_captured_evaluation_replays_the_eager_result(tr, make):   # noqa: F811
    """Captured under the bf16 query, replayed after the setting went back to f32: a captured call
    keeps the kernel it was captured with."""
    n = 17
    st = make(10, n)
    ref, draws, _ = _case(tr, make, n)
    draws = torch.from_numpy(draws).to(DEV)
    eager = st.evaluate(n, 2, draws=draws, **ALL)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(st.device)
    with torch.cuda.graph(g):
        res = st.evaluate(n, 2, draws=draws, **ALL)
    st._sync_stream()
    try:
        for k in range(2):
            for t in (res.returns, res.final_dist, res.records, res.state):
                t.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize(st.device)
            assert torch.equal(res.returns, eager.returns) and torch.equal(res.final_dist, eager.final_dist)
            assert torch.equal(res.records, eager.records) and torch.equal(res.state, eager.state)
            st.set_query_dtype("f32")
    finally:
        st.set_query_dtype("bf16")
    _same(eager, ref)


# ---------------------------------------------------------------- 8. bad arguments
def test_bad_arguments_raise(tr):   # noqa: F811
    f32 = _student(tr, max_windows=4, teacher=False)
    lib = f32._lib
    msg = lambda: lib.rd_last_error().decode()
    assert f32.query_dtype == "f32"
    with pytest.raises(ValueError, match="query_dtype"):
        f32.set_query_dtype("bf16")
    assert f32.query_dtype == "f32"
    assert lib.rdl_set_query_dtype(f32._h, 1) == RD_EINVAL   # the C ABI's own answer
    assert "rdl_set_query_dtype" in msg() and "dtype" in msg() and f32.query_dtype == "f32"
    f32.set_query_dtype("f32")
    bf = _student(tr, max_windows=4, teacher=False, dtype="bf16")
    assert bf.query_dtype == "f32"   # an opt-in
    bf.set_query_dtype("bf16")
    for bad in ("fp16", "", None, 1):
        with pytest.raises(ValueError, match="query_dtype"):
            bf.set_query_dtype(bad)
    for bad in (2, -1):
        assert lib.rdl_set_query_dtype(bf._h, bad) == RD_EINVAL
        assert "rdl_set_query_dtype" in msg() and "dtype" in msg()
    assert bf.query_dtype == "bf16"
    assert lib.rdl_set_query_dtype(None, 0) == RD_EINVAL and "rdl_set_query_dtype" in msg() and "null" in msg()
    assert lib.rdl_set_query_dtype(ctypes.c_void_p(), 1) == RD_EINVAL and lib.rdl_query_dtype(None) == -1
    f32.close()
    bf.close()
