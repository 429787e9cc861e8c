"""GPU checks of the LSTM student's bf16 mode (rdl_create_dtype's RDL_DTYPE_BF16, StudentLstmConfig(dtype=
"bf16"); csrc/student_lstm_bf16.h) against the emulation tests/lstm_bf16.py (the header's "Arithmetic"
with f64 sums) and the f64 oracle oracle/lstm_np.py -- neither is the code under test.

Bounds.  The device differs from the emulation by f32 sums, by expf / tanhf, and by the bf16 roundings
those flip (an operand within an f32 ulp of a bf16 tie rounds the other way: one flip moves a product by
2^-9 of it).  Forward, per tensor and shape: median |got - emulation| <= 5e-5 (the f32 test's absolute
tolerance; a CPU stand-in with f32 sums gives 4e-8); max |got - emulation| <= max |emulation - oracle|,
i.e. a flipped rounding is bounded by the effect of rounding every operand (stand-in: 4.4e-5 against
3.6e-4 .. 6.9e-4 for pdflat); at least half of pdflat outside the f32 test's 5e-5 + 1e-4 |ref| against
the f64 oracle (bf16 is what runs; the emulation alone gives 0.68-0.75); over all shapes together at
most 1 % of pdflat outside that tolerance against the emulation (stand-in: 0 of 18,228).  Gradient: the
f32 test's bounds against the emulation (relative L2 < 5e-4, per element <= 1e-3 max|g| + 1e-6), and
rel(got, emulation) <= 0.25 rel(emulation, oracle), both computed here (stand-in ratios 0.0001 ..
0.028; an f32 gradient has ratio ~1 and fails by construction), and tests/student_parity.py's per-entry
bound against the emulation, with its bf16 tolerances and the scale M on the emulation's rounded operands
(asserted from 2,000 windows on, here (4, 2000); below, one rounding flip exceeds its cap, so only the exact
zeros are asserted and the figure is printed: that module's "Tolerances").
"""
import functools

import numpy as np
import pytest
import torch

from oracle import lstm_np as ln
from oracle import policy_np as pn
from tests import lstm_bf16 as lb
from tests import student_parity as sp
from tests.test_student_lstm_envs_gpu import STEPS, _student, tr   # noqa: F401  (tr: the teacher's fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RDL_KERNELS_STEP_RECURRENCE, RDL_KERNELS_LAYER_HEAD = 1, 2


def _trainer(T=10, B=20, loss="kl", params=None, dtype="bf16", **kw):
    from reacherdistilation_amd.student_lstm import StudentLstmConfig, StudentLstmTrainer
    return StudentLstmTrainer(StudentLstmConfig(loss=loss, steps=T, max_windows=B, dtype=dtype, **kw), device=DEV,
                              params=lb.params(T=T) if params is None else params)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _grad_check(g, want, M, label, rows, bf16=True):
    """tests/test_student_lstm_gpu.py's gradient bounds."""
    g = np.asarray(g, np.float64)
    rel = lb.rel_l2(g, want)
    print(f"rel L2 {rel:.3e}  max err {np.abs(g - want).max():.3e}  max |g| {np.abs(want).max():.3e}")
    assert rel < 5e-4, rel
    assert np.abs(g - want).max() <= 1e-3 * np.abs(want).max() + 1e-6
    sp.check_grad(g, dict(g64=want, M=M), label, rows, bf16)
    return rel


# ---------------------------------------------------------------- forward
FWD_CASES = [(10, 1, False), (10, 20, True), (10, 65, False), (3, 130, True), (10, 330, False), (1, 7, True)]


@functools.lru_cache(maxsize=None)
def _forward_case(T, B, with_state):
    """(device, emulation, oracle), each (pdflat, c, h), computed once per shape."""
    ob, prev, _ = lb.batch(T, B, B)
    st = lb.state(B) if with_state else None
    tr_ = _trainer(T, B)
    y, fin = tr_.forward(_t(ob), _t(prev), None if st is None else _t(st))
    p = tr_.params().cpu().numpy()
    got = (y.cpu().numpy().astype(np.float64), fin[0].cpu().numpy().astype(np.float64),
           fin[1].cpu().numpy().astype(np.float64))
    tr_.close()
    emu, ora = lb.forward(p, ob, prev, st), ln.forward(p, ob, prev, st)
    return got, (emu["pdflat"], *emu["state"]), (ora["pdflat"], *ora["state"])


@pytest.mark.parametrize("T,B,with_state", FWD_CASES)
def test_forward_matches_the_emulation(T, B, with_state):
    got, emu, ora = _forward_case(T, B, with_state)
    for name, g, e, o in zip(("pdflat", "c", "h"), got, emu, ora):
        err, cap = np.abs(g - e), np.abs(e - o).max()
        print(f"{name}: median {np.median(err):.3e}  max {err.max():.3e}  cap max|emu - oracle| {cap:.3e}")
        assert np.median(err) <= 5e-5, (name, np.median(err))
        assert err.max() <= cap, (name, err.max(), cap)
    share = lb.outside(got[0], ora[0])
    print(f"pdflat outside the f32 tolerance against the f64 oracle: {share:.3f}")
    assert share >= 0.5, share


def test_forward_outputs_of_all_shapes_stay_inside_the_f32_tolerance_of_the_emulation():
    out = n = 0
    for case in FWD_CASES:
        got, emu, _ = _forward_case(*case)
        out += int(np.sum(np.abs(got[0] - emu[0]) > 5e-5 + 1e-4 * np.abs(emu[0])))
        n += got[0].size
    print(f"{out} of {n} pdflat outputs outside 5e-5 + 1e-4 |ref| against the emulation")
    assert n == 18228 and out <= 0.01 * n, (out, n)


# ---------------------------------------------------------------- gradient
def _gradient_case(T, B, loss, with_state=False, keep_prob=1.0, seed=0, **kw):
    ob, prev, t = lb.batch(T, B, 3 + B)
    st = lb.state(B, 2) if with_state else None
    tr_ = _trainer(T, B, loss, keep_prob=keep_prob, seed=seed, **kw)
    p = tr_.params().cpu().numpy()
    g = tr_.rollout(_t(ob), _t(prev), _t(t), None if st is None else _t(st)).cpu().numpy()
    tr_.apply()
    m = tr_.metrics(1)[0]
    tr_.close()
    ge, L, sq, fw = lb.step_gradient(p, ob, prev, t, loss, st, keep_prob=keep_prob, seed=seed)
    go, _, _, _ = lb.step_gradient(p, ob, prev, t, loss, st, keep_prob=keep_prob, seed=seed, rounded=False)
    M = sp.lstm_scale(p, fw, ln.loss_and_dout(fw["pdflat"], t, loss, T * B)[1], rounded=True)
    what = " ".join(sorted(kw) + ["from a state"] * with_state + ["dropout"] * (keep_prob < 1))
    rel = _grad_check(g, ge, M, f"lstm bf16 {loss} ({T},{B}) {what or 'default'}", B)
    cap = lb.rel_l2(ge, go)
    print(f"rel(got, emulation) {rel:.3e}  rel(emulation, oracle) {cap:.3e}  ratio {rel / cap:.4f}")
    assert rel <= 0.25 * cap, (rel, cap)
    print(f"loss {m[0]:.6e} / {L:.6e}  sq {m[1]:.6e} / {sq:.6e}  rows {m[2]}")
    assert abs(m[0] - L) <= 2e-4 * abs(L) and abs(m[1] - sq) <= 2e-4 * sq and m[2] == T * B


@pytest.mark.parametrize("loss", ["mse", "kl"])
@pytest.mark.parametrize("T,B", [(10, 1), (10, 20), (10, 65), (4, 330), (4, 2000), (1, 7)])
def test_gradient_and_metrics_match_the_emulation(loss, T, B):
    _gradient_case(T, B, loss)


# The per-step shapes of tests/test_student_lstm_gpu.py's PATH_CASES (a bf16 handle takes no other path): the
# weight gradient's 64-row chunks (bf_wg_chunk) end in 54, 10 and 18 rows, none a multiple of the MFMA's 32-row
# k step; (10, 53): the fused head's last tile holds 5 windows
@pytest.mark.parametrize("loss", ["mse", "kl"])
@pytest.mark.parametrize("layer_head", [False, True])
@pytest.mark.parametrize("T,B", [(10, 31), (10, 33), (10, 53)])
def test_gradient_at_the_per_step_edges(loss, layer_head, T, B):
    _gradient_case(T, B, loss, **({"layer_head": True} if layer_head else {}))


def test_gradient_from_a_given_initial_state():
    _gradient_case(5, 40, "kl", with_state=True)


def test_gradient_with_input_dropout():
    _gradient_case(10, 50, "mse", keep_prob=0.5, seed=77)


# ---------------------------------------------------------------- Adam and the images
def test_adam_steps_and_the_images_follow_the_master():
    T, B = 10, 20
    tr_ = _trainer(T, B, "kl")
    ob, prev, t = lb.batch(T, B, 8)
    opt = pn.AdamTF1(ln.P_LSTM, lr=1e-3)
    p = tr_.params().cpu().numpy().copy()
    for k in range(3):
        tr_.step(_t(ob), _t(prev), _t(t))
        g = tr_.grad().cpu().numpy()          # the device's own gradient: isolates Adam from rounding flips
        want = opt.step(p, g)
        got = tr_.params().cpu().numpy()
        tol = 1e-6 + 1e-4 * np.abs(want - p).max()
        print(f"step {k}: max |params - AdamTF1| {np.abs(got - want).max():.3e}  tol {tol:.3e}")
        assert np.abs(got - want).max() <= tol
        p = got.copy()
    assert tr_.counter() == 3
    # the images are those of the master after the last step: a fresh handle built from it agrees bitwise
    y, fin = tr_.forward(_t(ob), _t(prev))
    fresh = _trainer(T, B, "kl", params=tr_.params())
    y2, fin2 = fresh.forward(_t(ob), _t(prev))
    assert torch.equal(y, y2) and torch.equal(fin, fin2)
    f32 = _trainer(T, B, "kl", params=tr_.params(), dtype="f32")
    y3, _ = f32.forward(_t(ob), _t(prev))
    assert not torch.equal(y, y3)
    for x in (tr_, fresh, f32):
        x.close()


def test_checkpoints_cross_the_dtypes(tmp_path):
    """The checkpoint is the f32 master plus slots: a bf16 trainer loads an f32 trainer's and the reverse,
    and load re-forms the images."""
    T, B = 10, 20
    ob, prev, t = lb.batch(T, B, 51)
    a = _trainer(T, B, "kl", dtype="f32")
    a.step(_t(ob), _t(prev), _t(t))
    path = str(tmp_path / "lstm.safetensors")
    a.save(path)
    b = _trainer(T, B, "kl", params=ln.init(99))
    b.load(path)
    assert torch.equal(a.params(), b.params())
    assert all(torch.equal(x, y) for x, y in zip(a._slots(), b._slots()))
    fresh = _trainer(T, B, "kl", params=a.params())
    assert torch.equal(b.forward(_t(ob), _t(prev))[0], fresh.forward(_t(ob), _t(prev))[0])
    b.step(_t(ob), _t(prev), _t(t))
    b.save(path)
    a.load(path)
    assert torch.equal(a.params(), b.params())
    for x in (a, b, fresh):
        x.close()


# ---------------------------------------------------------------- determinism
def test_two_rollouts_are_bitwise_equal():
    T, B = 4, 2000
    ob, prev, t = lb.batch(T, B, 2)
    g1 = _trainer(T, B).rollout(_t(ob), _t(prev), _t(t)).clone()
    g2 = _trainer(T, B).rollout(_t(ob), _t(prev), _t(t)).clone()
    assert torch.equal(g1, g2)


def test_sharded_windows_sum_to_the_full_batch():
    T, B = 10, 60
    ob, prev, t = lb.batch(T, B, 9)
    from reacherdistilation_amd.student_lstm import StudentLstmConfig, StudentLstmTrainer

    def make(bmax, row_base):
        return StudentLstmTrainer(StudentLstmConfig(loss="mse", steps=T, max_windows=bmax, keep_prob=0.8, seed=3,
                                                    dtype="bf16"), device=DEV, params=lb.params(), row_base=row_base)
    full, a, b = make(B, 0), make(25, 0), make(35, 25)
    gf = full.rollout(_t(ob), _t(prev), _t(t)).clone()
    ga = a.rollout(_t(ob[:, :25]), _t(prev[:, :25]), _t(t[:, :25]), windows_global=B).clone()
    gb = b.rollout(_t(ob[:, 25:]), _t(prev[:, 25:]), _t(t[:, 25:]), windows_global=B).clone()
    M = sp.lstm_reference(lb.params(), ob, prev, t, "mse", rounded=True, keep_prob=0.8, seed=3)["M"]
    _grad_check((ga + gb).cpu().numpy(), gf.cpu().numpy().astype(np.float64), M, "lstm bf16 sharded 25 + 35 vs 60", B,
                bf16=False)   # two device gradients of the same arithmetic: the f32 bounds
    for x in (full, a, b):
        x.close()


# ---------------------------------------------------------------- paths
def _outputs(tr_, ob, prev, t, st=None):
    y, fin = tr_.forward(_t(ob), _t(prev), None if st is None else _t(st))
    g = tr_.rollout(_t(ob), _t(prev), _t(t), None if st is None else _t(st)).clone()
    return y, fin, g, tr_.final_state(ob.shape[1])


@pytest.mark.parametrize("T,B", [(10, 20), (3, 32)])
def test_step_recurrence_bit_changes_nothing(T, B):
    """At most 32 windows an f32 handle would take the persistent kernels; a bf16 handle never does."""
    ob, prev, t = lb.batch(T, B, 11 + B)
    st = lb.state(B, 4)
    a, b = _trainer(T, B), _trainer(T, B, step_recurrence=True)
    for x, y in zip(_outputs(a, ob, prev, t, st), _outputs(b, ob, prev, t, st)):
        assert torch.equal(x, y)
    a.close()
    b.close()


@pytest.mark.parametrize("T,B", [(10, 20), (3, 130)])
def test_layer_head_path(T, B):
    """The head is f32 on either path: same activations and dh (so the final state and the cell's
    gradient are bitwise equal), head weight gradients within the fused-versus-layer test's 1e-5 of
    their largest entry."""
    ob, prev, t = lb.batch(T, B, 21 + B)
    a, b = _trainer(T, B, "mse"), _trainer(T, B, "mse", layer_head=True)
    assert a.fused_head and not b.fused_head
    (ya, fa, ga, sa), (yb, fb, gb, sb) = _outputs(a, ob, prev, t), _outputs(b, ob, prev, t)
    assert torch.equal(ya, yb) and torch.equal(fa, fb) and torch.equal(sa, sb)
    ga, gb = ga.cpu().numpy(), gb.cpu().numpy()
    w1 = ln.CELL_PARAMS
    assert np.array_equal(ga[:w1], gb[:w1])
    assert np.abs(ga[w1:] - gb[w1:]).max() <= 1e-5 * np.abs(gb[w1:]).max()
    a.close()
    b.close()


# ---------------------------------------------------------------- contracts
@pytest.mark.parametrize("n", [17, 33])
def test_queries_stay_f32_on_the_master(tr, n):   # noqa: F811
    """evaluate and act_envs on a bf16 handle are bitwise an f32 handle's with the same parameters."""
    hb, hf = _student(tr, max_windows=n * 41, dtype="bf16"), _student(tr, max_windows=n * 41)
    eb = hb.evaluate(n, 1, seed=5, final_dist=True, records=True, final_state=True)
    ef = hf.evaluate(n, 1, seed=5, final_dist=True, records=True, final_state=True)
    for name in ("returns", "final_dist", "records", "state"):
        assert torch.equal(getattr(eb, name), getattr(ef, name)), name
    for st in (hb, hf):
        st.attach_envs(n, seed=11, env_base=5, accum_steps=STEPS)
    for K in (23, 50):
        rb, rf = hb.act_envs(steps=K), hf.act_envs(steps=K)
        for name in ("records", "reward") + (("ob_w", "prev_w", "t_w") if K == 50 else ()):
            assert torch.equal(getattr(rb, name), getattr(rf, name)), (K, name)
    assert torch.equal(hb.query_state(), hf.query_state())
    hb.close()
    hf.close()


@pytest.mark.parametrize("n", [17, 33])
def test_step_envs_equals_act_then_a_bf16_step(tr, n):   # noqa: F811
    T, B = 10, n * 41
    cfg = dict(loss="kl", lr=1e-3, keep_prob=0.5, seed=4, dtype="bf16")
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
    # the training pass was the bf16 one: an f32 handle from the same start takes another step
    f32 = _student(tr, max_windows=B, **dict(cfg, dtype="f32"))
    f32.attach_envs(n, seed=11, env_base=5, accum_steps=STEPS)
    f32.act_envs(steps=23)
    f32.step_envs()
    f32.step_envs()
    assert not torch.equal(f32.params(), fused.params())
    for st in (fused, twin, f32):
        st.close()


def test_graph_step_equals_eager():
    T, B = 10, 20
    ob, prev, t = lb.batch(T, B, 21)
    eager, graphed = _trainer(T, B, keep_prob=0.5, seed=4), _trainer(T, B, keep_prob=0.5, seed=4)
    step = graphed.graph_step(B)
    for _ in range(3):
        eager.step(_t(ob), _t(prev), _t(t))
        step(_t(ob).to(DEV), _t(prev).to(DEV), _t(t).to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(eager.params(), graphed.params())
    assert eager.counter() == graphed.counter() == 3
    np.testing.assert_array_equal(eager.metrics(3), graphed.metrics(3))
    y, _ = eager.forward(_t(ob), _t(prev))     # the replays re-formed the images too
    y2, _ = graphed.forward(_t(ob), _t(prev))
    assert torch.equal(y, y2)
    eager.close()
    graphed.close()


def test_an_unknown_dtype_raises():
    import ctypes

    from reacherdistilation_amd import _native as nat
    from reacherdistilation_amd.student_lstm import RdlConfig, StudentLstmConfig
    with pytest.raises(ValueError, match="dtype"):
        _trainer(dtype="fp16")
    with pytest.raises(ValueError, match="dtype"):
        StudentLstmConfig(dtype=2)
    c = RdlConfig(loss=1, lr=1e-3, beta1=.9, beta2=.999, eps=1e-8, steps=10, max_windows=20, metrics_len=0,
                  keep_prob=1.0, seed=0, row_base=0, kernels=0)
    h = ctypes.c_void_p()
    assert nat.load().rdl_create_dtype(ctypes.byref(h), ctypes.byref(c), 2, 0, None) == -100000 and not h.value
