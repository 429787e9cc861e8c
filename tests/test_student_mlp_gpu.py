"""GPU parity of the reference student (csrc/student_mlp.hip) against oracle/refnet_np.py.

Tolerances: the kernel computes in f32 (exact f32 products, f32 sums in MFMA order) against
the f64 oracle.  Forward: |err| <= 2e-5 + 1e-4 |ref|.  Gradient: relative L2 error < 2e-4,
per-element |err| <= 1e-4 max|g| + 1e-6, and tests/student_parity.py's per-entry bound (each
entry against the sum over the rows of |the row's contribution|).  Adam step: parameters
within 1e-6 + 1e-4 |update| of the oracle's TF1 Adam fed the oracle gradient.
"""
import numpy as np
import pytest
import torch

from oracle import policy_np as pn
from oracle import refnet_np as rn
from tests import student_parity as sp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _batch(n, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1, 1, (n, 16)).astype(np.float32)
    t = np.concatenate([rs.uniform(-.5, .5, (n, 2)), rs.uniform(-1.0, -0.2, (n, 2))], 1).astype(np.float32)
    return x, t


def _params(seed=4):
    p = rn.init(seed)
    rs = np.random.RandomState(seed + 100)
    for (_, bo, _, b) in rn.LAYOUT:
        p[bo:bo + b] = rs.uniform(-.1, .1, b).astype(np.float32)
    return p


def _trainer(loss="kl", params=None, **kw):
    from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer
    return StudentMlpTrainer(StudentMlpConfig(loss=loss, **kw), device=DEV,
                             params=_params() if params is None else params)


def _grad_check(g, want, M, label, rows):
    """want: the oracle's gradient (or, sharded, the full batch's from the GPU); M: the per-entry
    scale of the full batch (student_parity.mlp_scale)."""
    g = np.asarray(g, np.float64)
    rel = np.linalg.norm(g - want) / np.linalg.norm(want)
    assert rel < 2e-4, rel
    assert np.abs(g - want).max() <= 1e-4 * np.abs(want).max() + 1e-6
    sp.check_grad(g, dict(g64=want, M=M), label, rows)
    return rel


@pytest.mark.parametrize("n", [1, 17, 64, 65, 200, 1000, 4099])
def test_forward_matches_oracle(n):
    tr = _trainer()
    x, _ = _batch(n, n)
    got = tr.forward(torch.from_numpy(x)).cpu().numpy()
    want = rn.forward(tr.params().cpu().numpy(), x)["pdflat"]
    np.testing.assert_allclose(got, want, atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("loss", ["mse", "kl"])
@pytest.mark.parametrize("n", [1, 20, 200, 1000, 20000])
def test_gradient_and_metrics_match_oracle(loss, n):
    tr = _trainer(loss)
    x, t = _batch(n, 7 + n)
    p = tr.params().cpu().numpy()
    g = tr.rollout(torch.from_numpy(x), torch.from_numpy(t)).cpu().numpy()
    fw = rn.forward(p, x)
    lval, d, sq = rn.loss_and_dout(fw["pdflat"], t, loss, n)
    _grad_check(g, rn.backward(p, fw, d), sp.mlp_scale(p, fw, d), f"mlp f32 {loss} n={n}", n)
    tr.apply()
    m = tr.metrics(1)[0]
    assert abs(m[0] - lval) <= 1e-4 * abs(lval) + 1e-6 and abs(m[1] - sq) <= 1e-4 * sq + 1e-6 and m[2] == n


# launch_train's choice (csrc/student_mlp.hip use_small_rows): 16-row blocks while ceil(n / 16) <= grid / 2,
# else 64-row blocks, one workgroup per block up to `grid` workgroups (grid 0: the CU count, so 16-row
# blocks at every n here).  The path each shape reaches:
EDGE_SHAPES = [
    (15, 0), (16, 0), (17, 0),      # 16-row kernel: one ragged block; one full; two, one row in the second
    (63, 0), (64, 0), (65, 0),      # 16-row kernel: four blocks, the last ragged; four full; five, one row in the last
    (129, 0),                       # 16-row kernel: nine workgroups, one row in the last
    (15, 2), (16, 2),               # grid / 2 = 1 block: still the 16-row kernel, on one workgroup
    (17, 2), (63, 2), (64, 2),      # 64-row kernel, one workgroup: a ragged block (17, 63 rows) and a full one
    (65, 2),                        # 64-row kernel, two workgroups, one row in the second
    (129, 2),                       # 64-row kernel, three blocks on two workgroups: one loops over two, the last has one row
]


@pytest.mark.parametrize("loss", ["mse", "kl"])
@pytest.mark.parametrize("n,grid", EDGE_SHAPES)
def test_gradient_at_the_block_edges(loss, n, grid):
    tr = _trainer(loss, grid=grid)
    x, t = _batch(n, 7 + n)
    p = tr.params().cpu().numpy()
    g = tr.rollout(torch.from_numpy(x), torch.from_numpy(t)).cpu().numpy()
    fw = rn.forward(p, x)
    _, d, _ = rn.loss_and_dout(fw["pdflat"], t, loss, n)
    _grad_check(g, rn.backward(p, fw, d), sp.mlp_scale(p, fw, d), f"mlp f32 {loss} n={n} grid={grid}", n)
    tr.close()


@pytest.mark.parametrize("loss", ["mse", "kl"])
@pytest.mark.parametrize("grid", [2, 0])
def test_each_row_contribution_isolated(loss, grid):
    """64 rows: one 64-row block on one workgroup (grid=2: every lane of a wave owns one row) or four
    16-row blocks (the default grid).  g(batch) - g(batch with row r replaced by a fixed row z) is
    c(x_r) - c(z), compared per entry with the oracle's for every r under student_parity's
    isolation bound (tests/test_student_parity_mutation.py: a row's lost lanes-48-63 share of one
    dW is thousands of times that bound)."""
    n = 64
    tr = _trainer(loss, grid=grid)
    x, t = _batch(n, 31)
    zx, zt = sp.ISO_MLP_Z
    p = tr.params().cpu().numpy()

    def grad_of(xs, ts):
        return tr.rollout(torch.from_numpy(xs), torch.from_numpy(ts)).cpu().numpy().astype(np.float64)

    ref = sp.mlp_reference(p, x, t, loss)
    refz = sp.mlp_reference(p, zx[None], zt[None], loss, n_global=n)
    g_all = grad_of(x, t)
    sp.check_grad(g_all, ref, f"mlp f32 isolation {loss} grid={grid} batch", n)
    worst = (0.0, 0, 0)
    for r in range(n):
        xe, te = x.copy(), t.copy()
        xe[r], te[r] = zx, zt
        d_gpu = g_all - grad_of(xe, te)
        Mx = sp.scale(ref["products"], rn.P_REF, [r])
        d64 = sp.row_contribution(ref["products"], rn.P_REF, [r]) - refz["g64"]
        bound = sp.isolation_bound(Mx, refz["M"], ref["M"], ref["M"] - Mx + refz["M"])
        ratio, k = sp.isolation_ratio(d_gpu, d64, bound)
        worst = max(worst, (ratio, r, k))
        assert ratio <= 1.0, (r, sp.block_of(sp.mlp_layout()[0], k), ratio)
    print(f"student_parity isolation mlp f32 {loss} grid={grid}: worst error / bound {worst[0]:.3f} "
          f"(row {worst[1]}, {sp.block_of(sp.mlp_layout()[0], worst[2])})")
    tr.close()


def test_adam_step_matches_oracle():
    tr = _trainer("kl", lr=1e-3)
    x, t = _batch(300, 3)
    p = tr.params().cpu().numpy().copy()
    opt = pn.AdamTF1(rn.P_REF, lr=1e-3)
    for k in range(3):
        fw = rn.forward(p.astype(np.float64), x)
        _, d, _ = rn.loss_and_dout(fw["pdflat"], t, "kl", 300)
        g = rn.backward(p.astype(np.float64), fw, d)
        before = p.copy()
        p = opt.step(p, g)
        tr.step(torch.from_numpy(x), torch.from_numpy(t))
        got = tr.params().cpu().numpy()
        np.testing.assert_allclose(got, p, atol=1e-6 + 1e-4 * np.abs(p - before).max())
        p = got.copy()   # continue from the device's parameters (isolates each step)
    assert tr.counter() == 3


def test_dropout_matches_oracle_mask():
    tr = _trainer("mse", keep_prob=0.5, seed=99)
    x, t = _batch(500, 5)
    p = tr.params().cpu().numpy()
    for step in range(2):   # the mask is keyed by the optimiser step
        g = tr.rollout(torch.from_numpy(x), torch.from_numpy(t)).cpu().numpy()
        xd = rn.dropout(x, 0.5, seed=99, step=step)
        fw = rn.forward(p, xd)
        _, d, _ = rn.loss_and_dout(fw["pdflat"], t, "mse", 500)
        _grad_check(g, rn.backward(p, fw, d), sp.mlp_scale(p, fw, d), f"mlp f32 dropout mse n=500 step {step}", 500)
        tr.apply()
        p = tr.params().cpu().numpy()


def test_sharded_rows_sum_to_the_full_batch():
    """Two trainers with contiguous halves (row_base) == one trainer on all rows (the
    multi-GPU contract: all_reduce(SUM) of the shard gradients)."""
    from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer
    x, t = _batch(1000, 9)
    cfg = StudentMlpConfig(loss="mse", keep_prob=0.7, seed=5)
    full = StudentMlpTrainer(cfg, device=DEV, params=_params()).rollout(torch.from_numpy(x), torch.from_numpy(t))
    a = StudentMlpTrainer(cfg, device=DEV, params=_params(), row_base=0)
    b = StudentMlpTrainer(cfg, device=DEV, params=_params(), row_base=600)
    ga = a.rollout(torch.from_numpy(x[:600]), torch.from_numpy(t[:600]), n_global=1000).clone()
    gb = b.rollout(torch.from_numpy(x[600:]), torch.from_numpy(t[600:]), n_global=1000).clone()
    fw = rn.forward(_params(), rn.dropout(x, 0.7, seed=5, step=0))
    M = sp.mlp_scale(_params(), fw, rn.loss_and_dout(fw["pdflat"], t, "mse", 1000)[1])
    _grad_check((ga + gb).cpu().numpy(), full.cpu().numpy().astype(np.float64), M, "mlp f32 sharded 600 + 400 vs 1000", 1000)


def test_deterministic():
    x, t = _batch(5000, 1)
    g1 = _trainer().rollout(torch.from_numpy(x), torch.from_numpy(t)).clone()
    g2 = _trainer().rollout(torch.from_numpy(x), torch.from_numpy(t)).clone()
    assert torch.equal(g1, g2)


def test_learns_a_fixed_teacher():
    """KL to a fixed target policy falls by > 10x in 300 Adam steps (lr 1e-3)."""
    teacher = rn.init(77)
    x, _ = _batch(2000, 2)
    t = rn.forward(teacher, x)["pdflat"].astype(np.float32)
    tr = _trainer("kl", lr=1e-3)
    xs, ts = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    for _ in range(300):
        tr.step(xs, ts)
    m = tr.metrics(300)
    assert np.all(np.isfinite(m[:, 0])) and m[-1, 0] < 0.1 * m[0, 0], (m[0, 0], m[-1, 0])


def test_bad_arguments_raise():
    from reacherdistilation_amd._native import NativeError
    tr = _trainer()
    with pytest.raises(ValueError):
        tr.forward(torch.zeros(0, 16))
    with pytest.raises(ValueError):
        tr.rollout(torch.zeros(4, 16), torch.zeros(3, 4))
    mis = torch.zeros(65, device=DEV)[1:].view(4, 16)   # 4-byte offset: not 16-B aligned
    with pytest.raises(NativeError):
        tr.rollout(mis, torch.zeros(4, 4, device=DEV))


def test_graph_step_equals_eager():
    x, t = _batch(200, 13)
    eager, graphed = _trainer("kl", keep_prob=0.5, seed=3), _trainer("kl", keep_prob=0.5, seed=3)
    step = graphed.graph_step(200)
    for _ in range(3):
        eager.step(torch.from_numpy(x), torch.from_numpy(t))
        step(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(eager.params(), graphed.params())
    np.testing.assert_array_equal(eager.metrics(3), graphed.metrics(3))
