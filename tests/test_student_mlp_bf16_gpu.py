"""The reference MLP student in bf16 mixed precision (StudentMlpConfig(dtype="bf16"),
rdm_create_dtype's RDM_DTYPE_BF16) against tests/refnet_bf16.py, the layer-wise emulation of the
arithmetic include/reacher_student_mlp.h states (layers 1-3 round their matrix operands to bf16,
everything else f32; f64 sums in the emulation), and against the paths the handle fuses.

Shapes: the default grid takes n <= 16 grid / 2 rows to the 16-row instance (n = 1, 17, 20, 200);
grid=2 takes everything above 16 rows to the 64-row instance (n = 17: one ragged block; 64: a full
one; 65: two workgroups, one row in the second; 330: three blocks per workgroup, a ragged last).

Forward against the emulation: the kernel's f32 sums and tanh move an activation by ~5e-8, which
flips the bf16 rounding of a few operands further down (about one row in 200 has a flipped operand),
so most outputs agree to f32 accuracy and the outputs of such a row differ by a bf16 ulp's worth.
Per shape: a median <= 2e-5 (measured 5e-8 .. 1.1e-7); >= 90 % of the same outputs outside the f32
test's tolerance 2e-5 + 1e-4 |ref| against the f64 oracle (measured 94 .. 100 %): the bf16 arithmetic
is the one running; and the largest single error within MAX_ERR_BOUND, 4x the largest measured on an
MI355X over these shapes (MAX_ERR_MEASURED = 6.5e-4, at grid=2 n=65; 1.1e-3 at n = 4,099).
The share of outputs outside that tolerance against the emulation is capped at 1 % over the outputs
of all shapes together (measured 16 of 2,776 = 0.58 %; 0.88 % at n = 4,099).  Per shape it is 0, 0,
0.75 %, 0, 0, 1.15 %, 0.53 %: a flipped row puts 3-4 of its outputs outside, so at 65 rows and fewer
(<= 260 outputs) a 1 % cap on the one shape would allow no flip at all, and grid=2 n=65 has one such
row (3 of 260 outputs).
Gradient: relative L2 < 2e-4 against the emulation (the f32 test's bound; measured 4e-8 without a
flip, up to 4.8e-5 with), > 1e-3 against the f64 oracle's gradient (measured 2.4e-3 .. 4.4e-3), and
tests/student_parity.py's per-entry bound against the emulation, with its bf16 tolerances and the scale
M on the emulation's rounded operands (asserted from 2,000 rows on, which no shape here reaches; below,
one rounding flip exceeds its cap, so only the exact zeros are asserted and the figure is printed: that
module's "Tolerances").
The bitwise contracts (evaluate, act_envs, step_envs against the stepwise loop)
are those of tests/test_student_mlp_evaluate_gpu.py and tests/test_student_mlp_envs_gpu.py, whose
helpers are imported unchanged.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import policy_np as pn
from oracle import refnet_np as rn
from tests import refnet_bf16 as rb
from tests import student_parity as sp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 50
RD_EINVAL = -100000
MAX_ERR_MEASURED = 6.5017e-4   # largest |forward - emulation| over FWD_SHAPES on an MI355X (grid=2, n=65)
MAX_ERR_BOUND = 4 * MAX_ERR_MEASURED
FWD_SHAPES = [(0, 1), (0, 17), (0, 200), (2, 17), (2, 64), (2, 65), (2, 330)]   # (grid, n)
GRAD_SHAPES = [(0, 1), (0, 20), (0, 200), (2, 65), (2, 330)]


def _trainer(loss="kl", params=None, dtype="bf16", **kw):
    from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer
    return StudentMlpTrainer(StudentMlpConfig(loss=loss, dtype=dtype, **kw), device=DEV,
                             params=rb.params() if params is None else params)


_REF = {}


def _forward_ref(n):
    """(rows, emulation's pdflat, f64 oracle's pdflat) of one n, computed once and shared."""
    if n not in _REF:
        x, _ = rb.batch(n, n)
        p = rb.params()
        _REF[n] = (x, rb.forward(p, x)["pdflat"], rn.forward(p, x)["pdflat"])
    return _REF[n]


_GOT = {}


def _forward_got(grid, n):
    """The kernel's pdflat of one shape (f64), run once and shared."""
    if (grid, n) not in _GOT:
        tr = _trainer(grid=grid)
        _GOT[grid, n] = tr.forward(torch.from_numpy(_forward_ref(n)[0])).cpu().numpy().astype(np.float64)
        tr.close()
    return _GOT[grid, n]


@pytest.mark.parametrize("grid,n", FWD_SHAPES)
def test_forward_matches_the_emulation(grid, n):
    _, want, oracle = _forward_ref(n)
    got = _forward_got(grid, n)
    err = np.abs(got - want)
    print("forward grid=%d n=%d: median %.3e max %.3e outside %.4f vs oracle outside %.4f"
          % (grid, n, np.median(err), err.max(), rb.outside(got, want), rb.outside(got, oracle)))
    assert got.shape == (n, 4) and np.all(np.isfinite(got))
    assert np.median(err) <= 2e-5
    assert rb.outside(got, oracle) >= 0.9
    assert err.max() <= MAX_ERR_BOUND


def test_forward_share_outside_the_f32_tolerance():
    """At most 1 % of the outputs of all shapes lie outside 2e-5 + 1e-4 |ref| of the emulation."""
    got = np.concatenate([_forward_got(grid, n) for grid, n in FWD_SHAPES])
    want = np.concatenate([_forward_ref(n)[1] for _, n in FWD_SHAPES])
    print("forward, all shapes: %d outputs, outside %.4f" % (got.size, rb.outside(got, want)))
    assert rb.outside(got, want) <= 0.01


def _grad_check(g, want, M, label, rows, bf16=True):   # tests/test_student_mlp_gpu.py's bounds
    rel = rb.rel_l2(g, want)
    assert rel < 2e-4, rel
    assert np.abs(np.asarray(g, np.float64) - want).max() <= 1e-4 * np.abs(want).max() + 1e-6
    sp.check_grad(g, dict(g64=want, M=M), label, rows, bf16)
    return rel


def _check_step(tr, x, t, loss, n, label="", **drop):
    p = tr.params().cpu().numpy()
    g = tr.rollout(torch.from_numpy(x), torch.from_numpy(t)).cpu().numpy()
    want, lval, sq = rb.step_gradient(p, x, t, loss, **drop)
    oracle, _, _ = rb.step_gradient(p, x, t, loss, rounded=(), **drop)
    rel = rb.rel_l2(g, want)
    print("gradient %s n=%d: rel L2 %.3e vs emulation, %.3e vs oracle" % (loss, n, rel, rb.rel_l2(g, oracle)))
    M = sp.mlp_reference(p, x, t, loss, rounded=rb.BF_LAYERS, **drop)["M"]
    _grad_check(g, want, M, f"mlp bf16 {loss} n={n}{label}", n)
    assert rb.rel_l2(g, oracle) > 1e-3
    tr.apply()
    m = tr.metrics(1)[0]
    assert abs(m[0] - lval) <= 1e-4 * abs(lval) + 1e-6 and abs(m[1] - sq) <= 1e-4 * sq + 1e-6 and m[2] == n


@pytest.mark.parametrize("loss", ["mse", "kl"])
@pytest.mark.parametrize("grid,n", GRAD_SHAPES)
def test_gradient_and_metrics_match_the_emulation(loss, grid, n):
    tr = _trainer(loss, grid=grid)
    x, t = rb.batch(n, 7 + n)
    _check_step(tr, x, t, loss, n, f" grid={grid}")
    tr.close()


# tests/test_student_mlp_gpu.py's EDGE_SHAPES, with the paths they reach (the BF = true instances of the
# same two kernels)
@pytest.mark.parametrize("loss", ["mse", "kl"])
@pytest.mark.parametrize("grid", [0, 2])
@pytest.mark.parametrize("n", [15, 16, 17, 63, 64, 65, 129])
def test_gradient_at_the_block_edges(loss, grid, n):
    tr = _trainer(loss, grid=grid)
    # at most 20 rows: a batch without a forward operand on a bf16 tie (student_parity.mlp_bf16_seed)
    x, t = rb.batch(n, sp.mlp_bf16_seed(n, 7 + n) if n <= sp.TIE_MAX_ROWS else 7 + n)
    _check_step(tr, x, t, loss, n, f" grid={grid}")
    tr.close()


def test_dropout_matches_the_emulations_mask():
    tr = _trainer("kl", keep_prob=0.5, seed=99)
    x, t = rb.batch(200, 5)
    _check_step(tr, x, t, "kl", 200, " dropout", keep_prob=0.5, seed=99, step=0)
    tr.close()


ADAM_ROWS = 20


def test_three_adam_steps_match_the_emulation():
    """TF1 Adam's first updates are lr g / (|g| + eps'): sign-like in g, so an element whose gradient
    is smaller than the gradient's own error takes a step of the wrong sign.  A bf16 rounding flip
    moves the gradient by ~3e-5 of its norm (above), which is enough for a few of the 24,380 elements
    (300 rows: 2 of them, off by 2 lr); without a flip the gradient agrees to 5e-8.  The batch is
    therefore kept to ADAM_ROWS rows (two 16-row blocks, one ragged): Adam's arithmetic does not
    depend on the batch, and the bf16 image it re-forms is checked below on the full 300 rows."""
    tr = _trainer("kl", lr=1e-3)
    x, t = rb.batch(300, 3)
    xa, ta = x[:ADAM_ROWS], t[:ADAM_ROWS]
    p = tr.params().cpu().numpy().copy()
    opt = pn.AdamTF1(rn.P_REF, lr=1e-3)
    for k in range(3):
        g, _, _ = rb.step_gradient(p.astype(np.float64), xa, ta, "kl")
        before = p.copy()
        p = opt.step(p, g)
        tr.step(torch.from_numpy(xa), torch.from_numpy(ta))
        got = tr.params().cpu().numpy()
        tol = 1e-6 + 1e-4 * np.abs(p - before).max()
        print("adam step %d: rel L2 of the gradient %.3e, max |dp| %.3e (tol %.3e), %d outside"
              % (k, rb.rel_l2(tr.grad().cpu().numpy(), g), np.abs(got - p).max(), tol, int((np.abs(got - p) > tol).sum())))
        np.testing.assert_allclose(got, p, atol=tol)
        p = got.copy()   # continue from the device's parameters (isolates each step)
    assert tr.counter() == 3
    # the bf16 weights followed Adam: a fresh trainer packs the same image from the parameters
    xs = torch.from_numpy(x)
    fresh, f32 = _trainer(params=tr.params()), _trainer(params=tr.params(), dtype="f32")
    out = tr.forward(xs)
    assert torch.equal(out, fresh.forward(xs))
    assert not torch.equal(out, f32.forward(xs))
    for a in (tr, fresh, f32):
        a.close()


def test_sharded_rows_sum_to_the_full_batch():
    from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer
    x, t = rb.batch(1000, 9)
    cfg = StudentMlpConfig(loss="mse", keep_prob=0.7, seed=5, dtype="bf16")
    full = StudentMlpTrainer(cfg, device=DEV, params=rb.params()).rollout(torch.from_numpy(x), torch.from_numpy(t))
    a = StudentMlpTrainer(cfg, device=DEV, params=rb.params(), row_base=0)
    b = StudentMlpTrainer(cfg, device=DEV, params=rb.params(), row_base=600)
    ga = a.rollout(torch.from_numpy(x[:600]), torch.from_numpy(t[:600]), n_global=1000).clone()
    gb = b.rollout(torch.from_numpy(x[600:]), torch.from_numpy(t[600:]), n_global=1000).clone()
    M = sp.mlp_reference(rb.params(), x, t, "mse", rounded=rb.BF_LAYERS, keep_prob=0.7, seed=5)["M"]
    _grad_check((ga + gb).cpu().numpy(), full.cpu().numpy().astype(np.float64), M, "mlp bf16 sharded 600 + 400 vs 1000", 1000,
                bf16=False)   # two device gradients of the same arithmetic: the f32 bounds


# -- the bitwise contracts, in bf16 ---------------------------------------------------------------
ENVS = [(17, 0), (65, 2)]   # (envs, grid): 16-env blocks; 64-env blocks on two workgroups


@pytest.fixture(scope="module")
def tr():
    """The DistillTrainer whose forward is the stepwise teacher, and whose teacher every student gets."""
    from reacherdistilation_amd.distill import DistillConfig, DistillTrainer
    t = DistillTrainer(DistillConfig(n_envs=64, seed=3), device=DEV)
    yield t
    t.close()


def _student(tr, **cfg):
    sm = _trainer(params=None, **cfg)
    sm.set_teacher(tr.teacher)
    return sm


@pytest.mark.parametrize("n,grid", ENVS)
def test_evaluate_equals_the_stepwise_loop(tr, n, grid):
    from reacherdistilation_amd.env import BatchedReacher
    from reacherdistilation_amd.evaluate import gym_draw_table
    from tests.test_student_mlp_evaluate_gpu import _stepwise
    sm = _student(tr)
    env, shadow = BatchedReacher(n, seed=7, device=DEV, reset="gym"), BatchedReacher(n, device=DEV)
    ret, dist, rec = _stepwise(tr, sm, env, 1, shadow)
    res = sm.evaluate(n, 1, draws=gym_draw_table(7, n, 1), final_dist=True, records=True, grid=grid)
    torch.cuda.synchronize()
    assert torch.equal(res.records, rec) and torch.equal(res.returns, ret) and torch.equal(res.final_dist, dist)
    assert bool(torch.isfinite(res.returns).all())
    # the student that acts is the bf16 one: the f32 student's records differ
    f32 = _student(tr, dtype="f32")
    assert not torch.equal(f32.evaluate(n, 1, draws=gym_draw_table(7, n, 1), records=True, grid=grid).records, rec)
    for a in (env, shadow, sm, f32):
        a.close()


@pytest.mark.parametrize("n,grid", ENVS)
def test_act_envs_equals_the_stepwise_loop(tr, n, grid):
    from tests.test_student_mlp_envs_gpu import Stepwise, _cat, _keep
    sm = _student(tr)
    sm.attach_envs(n, seed=11, env_base=5, accum_steps=STEPS, grid=grid)
    loop = Stepwise(tr, sm, n, 11, 5)
    got = _cat([_keep(sm.act_envs(steps=k)) for k in (3, 50, 4)])
    want = loop.steps(57)
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    assert bool((got[2] != 0).any()) and bool(torch.isfinite(got[0]).all())
    st, step, episode = loop.env.get_state()
    gs, gstep, gep = sm.env_state()
    assert torch.equal(gs, st) and (gstep, gep) == (step, episode) == (7, 1)
    loop.close()
    sm.close()


@pytest.mark.parametrize("n,grid", ENVS)
def test_step_envs_equals_act_then_step_on_a_twin(tr, n, grid):
    cfg = dict(loss="kl", lr=1e-3, keep_prob=0.5, seed=4)
    fused, twin = _student(tr, **cfg), _student(tr, **cfg)
    for sm in (fused, twin):
        sm.attach_envs(n, seed=11, env_base=5, accum_steps=STEPS, grid=grid)
    for k in range(2):
        r = fused.step_envs()
        w = twin.act_envs()
        for u, v in zip((r.x, r.t_pdflat, r.s_pdflat, r.reward), (w.x, w.t_pdflat, w.s_pdflat, w.reward)):
            assert torch.equal(u, v)
        twin.step(w.x.reshape(-1, 16), w.t_pdflat.reshape(-1, 4))
        assert torch.equal(fused.params(), twin.params()) and torch.equal(fused.grad(), twin.grad()), k
        assert fused.counter() == twin.counter() == k + 1
        assert np.array_equal(fused.metrics(1), twin.metrics(1)), k
    assert fused.metrics(1)[0, 2] == STEPS * n
    fused.close()
    twin.close()


def test_learns_a_fixed_teacher():
    """test_student_mlp_gpu.py's criterion and settings in bf16: KL to a fixed target policy falls by
    > 10x in 300 Adam steps (lr 1e-3)."""
    from tests.test_student_mlp_gpu import _batch, _params
    teacher = rn.init(77)
    x, _ = _batch(2000, 2)
    t = rn.forward(teacher, x)["pdflat"].astype(np.float32)
    tr = _trainer("kl", lr=1e-3, params=_params())
    xs, ts = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    for _ in range(300):
        tr.step(xs, ts)
    m = tr.metrics(300)
    print("KL curve (every 50th step):", " ".join("%.4g" % v for v in m[::50, 0]), "last %.4g" % m[-1, 0])
    assert np.all(np.isfinite(m[:, 0])) and m[-1, 0] < 0.1 * m[0, 0], (m[0, 0], m[-1, 0])
    tr.close()


def test_train_envs_passes_the_dtype_on():
    """mlp_train.train_envs(dtype="bf16") trains the bf16 student: its history is that of the same
    step_envs calls on a bf16 trainer, bit for bit, and not the f32 driver's."""
    from reacherdistilation_amd import mlp_train
    kw = dict(keep_prob=0.5, lr=1e-3, accum_steps=5, seed=3)
    sm, history = mlp_train.train_envs(17, 3, dtype="bf16", **kw)
    assert sm.cfg.dtype == "bf16" and sm.counter() == 3 and np.isfinite(np.asarray(history)).all()
    twin = _trainer("kl", lr=1e-3, keep_prob=0.5, seed=3, metrics_len=3, params=sm_init())
    twin.set_teacher(sm.teacher)
    twin.attach_envs(17, seed=3, accum_steps=5)
    for _ in range(3):
        twin.step_envs()
    assert torch.equal(twin.params(), sm.params()) and np.array_equal(twin.metrics(3), sm.metrics(3))
    f32, _ = mlp_train.train_envs(17, 3, **kw)
    assert f32.cfg.dtype == "f32" and not torch.equal(f32.params(), sm.params())
    for a in (sm, twin, f32):
        a.close()


def sm_init():
    from reacherdistilation_amd.student_mlp import StudentMlpConfig, glorot_init
    return glorot_init(StudentMlpConfig().init_seed)   # the driver's trainer starts from the default init


def test_an_unknown_dtype_is_refused_by_the_library():
    from reacherdistilation_amd import _native as nat
    from reacherdistilation_amd.student_mlp import StudentMlpConfig
    lib = nat.load()
    c, _ = StudentMlpConfig().native()
    h = ctypes.c_void_p()
    for bad in (2, -1):
        assert lib.rdm_create_dtype(ctypes.byref(h), ctypes.byref(c), bad, 0, None) == RD_EINVAL and not h.value
        assert "dtype" in lib.rd_last_error().decode()
    # rdm_create itself is the f32 student: the bits of rdm_create_dtype(.., RDM_DTYPE_F32, ..), not bf16's
    assert lib.rdm_create(ctypes.byref(h), ctypes.byref(c), 0, None) == 0 and h.value
    x = torch.from_numpy(rb.batch(17, 1)[0]).to(DEV)
    p = torch.from_numpy(rb.params()).to(DEV)
    out = torch.empty(17, 4, device=DEV)
    assert lib.rdm_set_params(h, nat.ptr(p)) == 0 and lib.rdm_forward(h, nat.ptr(x), 17, nat.ptr(out)) == 0
    torch.cuda.synchronize()
    f32, bf = _trainer(dtype="f32"), _trainer()
    assert torch.equal(out, f32.forward(x)) and not torch.equal(out, bf.forward(x))
    assert lib.rdm_destroy(h) == 0
    f32.close()
    bf.close()
