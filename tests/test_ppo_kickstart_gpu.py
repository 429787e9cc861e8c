"""GPU tests of the PPO trainer's kickstarting (include/reacher_ppo.h, csrc/ppo.hip): the teacher's
labels on the actor batch, the kickstart instance's minibatch gradient against the oracle
(oracle/ppo_np.py + the KL part of tests/ppo_kickstart.py) under tests/ppo_parity.py's tolerances,
the lambda schedule and its metric, the seeded observation filter, the refusals, and that lambda = 0
is the computation of a trainer that never saw a teacher.

Shapes are the smallest that still exercise a ragged 16-row teacher tile, a ragged 32-row minibatch
tile, a dropped minibatch tail, a multi-epoch shuffle and a grid-stride loop.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ppo_np as pp
from tests import ppo_kickstart as ks
from tests import ppo_parity as par

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COEF = 0.7
LAM = float(np.float32(COEF))


def _trainer(**kw):
    from reacherdistilation_amd.ppo import PPOConfig, PPOTrainer
    cfg = dict(n_envs=256, horizon=64, seed=11, optim_batchsize=0, optim_epochs=1, max_timesteps=10 ** 6)
    cfg.update(kw)
    return PPOTrainer(PPOConfig(**cfg), device=DEV)


def _teacher_params():
    from reacherdistilation_amd.policy import MlpPolicyParams
    return MlpPolicyParams(*ks.teacher())


def _kickstarted(coef=COEF, decay=0, **kw):
    tr = _trainer(**kw)
    tr.set_teacher(_teacher_params())
    tr.set_distill(coef, decay)
    return tr


def _np(x):
    return x.cpu().numpy().astype(np.float64)


def _params(tr):
    return torch.cat([tr.policy(), tr.value()]).cpu()


def _actor_batch(tr):
    """rollout(), then the oracle's view of the batch (as tests/test_ppo_clip_gpu.py) plus the
    teacher's f64 pdflat on the raw observations."""
    pol0 = tr.policy().cpu().numpy()
    tr.rollout()
    b = {k: _np(v) for k, v in tr.batch().items()}
    mean1, std1 = (_np(x) for x in tr.obfilter())
    ob = b["ob"].reshape(-1, 11)
    z = pp.obz(ob, mean1, std1)
    a = b["ac"].reshape(-1, 2)
    fp = pp.pol_forward(pol0, z)
    return dict(ob=ob, z=z, a=a, lpo=pp.logp(fp["mean"], fp["logstd"], a), atarg=pp.standardize(b["adv"].reshape(-1)),
                ret=b["ret"].reshape(-1), tflat=ks.teacher_pdflat(*ks.teacher(), ob))


def _reference(pol, vf, b, rows, eps, lam=LAM):
    return ks.reference(pol, vf, b["z"][rows], b["a"][rows], b["lpo"][rows], b["atarg"][rows], b["ret"][rows], eps,
                        b["tflat"][rows], lam)


@pytest.fixture(scope="module")
def distill_teacher():
    """A DistillTrainer holding the tests' teacher: rdd_forward is the labels' reference."""
    from reacherdistilation_amd.distill import DistillConfig, DistillTrainer
    tr = DistillTrainer(DistillConfig(n_envs=64), device=DEV, teacher=_teacher_params())
    yield tr
    tr.close()


# ---------------------------------------------------------------- 1. labels
@pytest.mark.parametrize("n,T", [(50, 3), (96, 1), (300, 7), (1040, 17)])
def test_labels_are_bitwise_rdd_forwards_teacher_output(n, T, distill_teacher):
    """50 x 3 = 150 rows (a ragged 16-row tile), 96 x 1 (6 whole tiles, reset rows only), 300 x 7 = 2,100
    (ragged, 33 workgroups), 1040 x 17 = 17,680 rows = 1,105 tiles over the label kernel's 256
    workgroups x 4 waves (its grid-stride loop).  The teacher's filter sends input 6 past the +-5
    clip on some rows and not on others."""
    tr = _trainer(n_envs=n, horizon=T)
    tp = _teacher_params()
    tr.set_teacher(tp)
    tr.rollout()
    ob = tr.batch()["ob"]
    z6 = (_np(ob).reshape(-1, 11)[:, 6] - float(tp.ob_mean[6])) / float(tp.ob_std[6])
    assert (np.abs(z6) > 5).any() and (np.abs(z6) < 5).any()
    want, _ = distill_teacher.forward(ob.reshape(-1, 11), teacher=True, student=False)
    got = tr.teacher_labels()
    assert got.shape == (T, n, 4)
    assert torch.equal(got.reshape(-1, 4), want)
    np.testing.assert_allclose(_np(got).reshape(-1, 4), ks.teacher_pdflat(*ks.teacher(), _np(ob).reshape(-1, 11)),
                               atol=1e-4, rtol=1e-4)               # a sanity bound (the check is the bitwise one): this teacher
    assert torch.equal(got[..., 2:].reshape(-1, 2).cpu(), torch.tensor(ks.TEACHER_LOGSTD).expand(n * T, 2))


# ---------------------------------------------------------------- 2. the gradient
@pytest.mark.parametrize("it", [0, 1])
@pytest.mark.parametrize("n,T,mb,E", [(96, 1, 64, 1), (300, 7, 1000, 2), (50, 3, 50, 3)])
def test_kickstart_gradient_matches_oracle(n, T, mb, E, it):
    """test_shuffled_minibatch_gradient_matches_oracle's cases with a teacher and lambda = 0.7:
    optim_stepsize 1e-12 keeps the parameters, grad() is the gradient of the last minibatch of the
    last epoch, held to oracle PPO + lambda x KL by ppo_parity.check_grad.  Control: the reference
    with lambda = 0 fails the same check.  The KL metric is the mean over the last epoch's minibatches."""
    seed = 11
    tr = _kickstarted(n_envs=n, horizon=T, optim_batchsize=mb, optim_epochs=E, optim_stepsize=1e-12)
    S, nmb = n * T, (n * T) // mb
    if it:
        tr.iterate()
    pol, vf = tr.policy().cpu().numpy(), tr.value().cpu().numpy()
    assert tuple(pol[-2:]) != ks.TEACHER_LOGSTD                      # the teacher's log-std is not the learner's
    b = _actor_batch(tr)
    eps = 0.2 * (1.0 - it * S / 10 ** 6)
    assert tr.distill_coef() == np.float32(COEF)
    tr.optimize()
    np.testing.assert_allclose(tr.policy().cpu().numpy(), pol, rtol=0, atol=1e-10)
    g = _np(tr.grad())
    perm = pp.shuffles(seed, it, S, E)
    last = [_reference(pol, vf, b, perm[E - 1][j * mb:(j + 1) * mb], eps) for j in range(nmb)]
    r = last[-1]
    label = f"kickstart {n}x{T} mb {mb} epochs {E} it {it}"
    par.check_grad(g, r, label)
    r0 = _reference(pol, vf, b, perm[E - 1][(nmb - 1) * mb:nmb * mb], eps, lam=0.0)
    ok0, rep0 = par.grad_ok(g[:pp.P_POL], r0["gpol"], r0["M_pol"], r0["extra_pol"])
    assert not ok0, rep0
    kl, lam = tr.distill_metrics(1)[0]
    want_kl = np.mean([x["kl"] for x in last])
    print(f"ppo_kickstart {label}: KL {kl:.7f} / {want_kl:.7f}")
    assert lam == np.float32(COEF)
    assert abs(kl - want_kl) <= 1e-4 * want_kl + 1e-6, (kl, want_kl)
    m = tr.metrics(1)[0]                                             # the PPO metrics are still PPO's
    pol_surr, vf_loss = np.mean([x["pol_surr"] for x in last]), np.mean([x["vf_loss"] for x in last])
    assert abs(m[2] - pol_surr) < 1e-4 and abs(m[3] - vf_loss) <= 1e-4 * vf_loss + 1e-5, (m, pol_surr, vf_loss)


# ---------------------------------------------------------------- 3. clipped rows
def test_clipped_rows_still_receive_the_kl_term():
    """test_second_epoch_gradient_after_a_real_step's setup, kickstarted: two epochs of the full
    256 x 64 batch at stepsize 1e-2, the second epoch's gradient at the parameters a kickstarted
    1-epoch twin reads after its step.  Rows are outside the clip range on both sides and some are
    dead; the reference's KL part covers all rows.  Control: a reference whose KL part skips the
    dead rows fails the check."""
    kw = dict(optim_batchsize=0, optim_stepsize=1e-2)
    tr = _kickstarted(optim_epochs=2, **kw)
    b = _actor_batch(tr)
    tr1 = _kickstarted(optim_epochs=1, **kw)
    tr1.rollout()
    tr1.optimize()
    pol1, vf1 = tr1.policy().cpu().numpy(), tr1.value().cpu().numpy()
    rows = np.arange(tr.S)
    r = _reference(pol1, vf1, b, rows, 0.2)
    print("ppo_kickstart clipped: above", int(r["above"].sum()), "below", int(r["below"].sum()), "dead",
          int(r["dead"].sum()), "either", int(r["either"].sum()))
    assert min(r["above"].sum(), r["below"].sum()) >= 50, (r["above"].sum(), r["below"].sum())
    assert r["dead"].sum() >= 50
    tr.optimize()
    g = _np(tr.grad())
    par.check_grad(g, r, "kickstart second epoch 256x64")
    live_only = r["gpol_ppo"] + ks.kl_grad(pol1, b["z"], b["tflat"], LAM, keep=r["live"].astype(np.float64))
    ok, rep = par.grad_ok(g[:pp.P_POL], live_only, r["M_pol"], r["extra_pol"])
    assert not ok, rep


# ---------------------------------------------------------------- 4. lambda = 0
def _three_iterations(tr):
    for _ in range(3):
        tr.iterate()
    return tr.policy().cpu(), tr.value().cpu(), torch.from_numpy(tr.metrics(3))


def test_lambda_zero_is_the_plain_trainers_computation():
    """96 x 4, minibatches of 64 (tail dropped), two epochs, three iterations: with a teacher set and
    coef 0 (the default, and set explicitly) policy, value and metrics are bitwise those of a
    trainer that never saw a teacher; the distillation metrics are zeros; the labels are there."""
    kw = dict(n_envs=96, horizon=4, optim_batchsize=64, optim_epochs=2, optim_stepsize=3e-3)
    want = _three_iterations(_trainer(**kw))
    for explicit in (False, True):
        tr = _trainer(**kw)
        tr.set_teacher(_teacher_params())
        if explicit:
            tr.set_distill(0.0, 1000)
        assert tr.distill_coef() == 0.0
        got = _three_iterations(tr)
        for x, w in zip(got, want):
            assert torch.equal(x, w)
        np.testing.assert_array_equal(tr.distill_metrics(3), np.zeros((3, 2)))
        assert tr.teacher_labels().shape == (4, 96, 4)
    plain = _trainer(**kw)
    plain.iterate()
    np.testing.assert_array_equal(plain.distill_metrics(1), np.zeros((1, 2)))   # no teacher at all


# ---------------------------------------------------------------- 5. schedule and metric
def test_schedule_and_metric():
    """decay_timesteps = 4 S: lambda = coef x (1, 3/4, 1/2, 1/4, 0), formed in double and rounded to
    float.  Iteration 0 (one epoch, the full batch): the KL metric is the oracle's mean KL at the
    rollout's parameters.  The fifth iteration runs with lambda = 0: its parameters are bitwise
    those of a twin (the same four kickstarted iterations, so the same state) whose coefficient is
    set to 0 before it -- and coef 0 is the plain trainer's computation (the test above)."""
    n, T = 64, 50
    S = n * T
    kw = dict(n_envs=n, horizon=T, optim_stepsize=3e-3)
    tr, twin = _kickstarted(decay=4 * S, **kw), _kickstarted(decay=4 * S, **kw)
    want_lam = [np.float32(np.float64(np.float32(COEF)) * f) for f in (1.0, 0.75, 0.5, 0.25, 0.0)]
    for k in range(4):
        assert tr.distill_coef() == want_lam[k]
        pol = tr.policy().cpu().numpy()
        b = _actor_batch(tr)
        tr.optimize()
        twin.iterate()
        if k == 0:
            kl = tr.distill_metrics(1)[0, 0]
            want = ks.kl_heads(pol, b["z"], b["tflat"], 1.0)[0]
            print(f"ppo_kickstart schedule: KL {kl:.7f} / {want:.7f}")
            assert abs(kl - want) <= 1e-4 * want + 1e-6, (kl, want)
    assert torch.equal(_params(tr), _params(twin))
    assert tr.distill_coef() == 0.0
    twin.set_distill(0.0)
    tr.rollout()
    before = _params(tr)
    tr.optimize()
    twin.iterate()
    assert not torch.equal(before, _params(tr))                      # lrmult is 1 - 4 S / 10^6: PPO still steps
    assert torch.equal(_params(tr), _params(twin))
    d = tr.distill_metrics(5)
    np.testing.assert_array_equal(d[:, 1].astype(np.float32), np.array(want_lam, np.float32))
    assert np.all(np.isfinite(d)) and np.all(d[:4, 0] > 0) and d[4, 0] == 0.0
    np.testing.assert_array_equal(tr.metrics(5), twin.metrics(5))


# ---------------------------------------------------------------- 6. set_obfilter
def _filter():
    """Entries as a Reacher filter has them: |mean| below std except where the std is floored;
    std[4] and std[10] are under the 0.1 floor (sqrt of the variance floor 1e-2).  rms_finalize forms
    the variance in f32 as sumsq / count - mean^2, whose rounding error relative to std^2 is
    2^-24 (1 + mean^2 / std^2): one ulp of std holds while mean^2 <= std^2, which these entries keep."""
    mean = np.float32([0.3, -0.25, 0.1, -0.2, 0.02, -0.01, 0.4, -0.7, 0.05, -0.03, 0.0])
    std = np.float32([0.6, 0.55, 0.7, 0.65, 0.05, 0.12, 2.5, 3.5, 0.2, 0.21, 0.01])
    return mean, std


def _ulps(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want).astype(np.float32))


def test_set_obfilter_seeds_the_running_statistics():
    from reacherdistilation_amd import _native as nat
    n, T, count = 100, 30, 5000.0
    tr = _trainer(n_envs=n, horizon=T)
    mean, std = _filter()
    tr.set_obfilter(mean, std, count)
    m, s = (x.cpu().numpy() for x in tr.obfilter())
    want_s = np.maximum(std, np.float32(0.1))
    print("ppo_kickstart obfilter ulps: mean", _ulps(m, mean).max(), "std", _ulps(s, want_s).max())
    assert np.all(_ulps(m, mean)[mean != 0] <= 1) and np.all(m[mean == 0] == 0)
    assert np.all(_ulps(s, want_s) <= 1)
    vf = tr.value().cpu().numpy()
    tr.rollout()
    b = {k: _np(v) for k, v in tr.batch().items()}
    ob = b["ob"].reshape(-1, 11)
    want_v = pp.vf_forward(vf, pp.obz(ob, m.astype(np.float64), s.astype(np.float64)))["v"]
    print("ppo_kickstart obfilter vpred err:", np.abs(b["vpred"].reshape(-1) - want_v).max())
    np.testing.assert_allclose(b["vpred"].reshape(-1), want_v, atol=1e-5, rtol=0)
    plain = pp.vf_forward(vf, pp.obz(ob, np.zeros(11), np.ones(11)))["v"]
    assert np.abs(plain - want_v).max() > 1e-2                       # the seeded filter is what the rollout used
    rms = pp.RunningMeanStd()
    m64, s64 = mean.astype(np.float64), std.astype(np.float64)
    rms.sum, rms.sumsq, rms.count = m64 * count, (s64 ** 2 + m64 ** 2) * count, count
    rms.update(ob)
    m1, s1 = (_np(x) for x in tr.obfilter())
    np.testing.assert_allclose(m1, rms.mean, rtol=1e-5, atol=1e-6)   # test_ppo_batch_gpu's filter bounds
    np.testing.assert_allclose(s1, rms.std, rtol=1e-4, atol=1e-6)
    assert np.abs(m1 - mean).max() > 1e-3                            # and the batch moved it
    tr._sync_stream()
    nat.check(tr._lib.rdp_reset(tr._h), "rdp_reset")
    m0, s0 = tr.obfilter()
    assert torch.equal(m0.cpu(), torch.zeros(11)) and torch.equal(s0.cpu(), torch.ones(11))


# ---------------------------------------------------------------- 7. refusals
def test_refusals_name_their_field_and_leave_the_parameters():
    from reacherdistilation_amd import _native as nat
    tr = _trainer(n_envs=32, horizon=4)
    lib, h = tr._lib, tr._h
    before = _params(tr)
    tp = _teacher_params()
    f, mu, sd = tp.device_tensors(tr.device)
    P = nat.ptr
    null = ctypes.c_void_p()

    def refused(call, match):
        with pytest.raises(RuntimeError, match=match):
            nat.check(call(), "call")

    refused(lambda: lib.rdp_set_teacher(null, P(f), P(mu), P(sd)), "rdp_set_teacher: null handle")
    refused(lambda: lib.rdp_set_teacher(h, null, P(mu), P(sd)), "rdp_set_teacher: null params")
    refused(lambda: lib.rdp_set_teacher(h, P(f), null, P(sd)), "rdp_set_teacher: null ob_mean")
    refused(lambda: lib.rdp_set_teacher(h, P(f), P(mu), null), "rdp_set_teacher: null ob_std")
    refused(lambda: lib.rdp_set_distill(null, 1.0, 0), "rdp_set_distill: null handle")
    for bad in (float("nan"), float("inf"), -0.5):
        refused(lambda: lib.rdp_set_distill(h, bad, 0), "rdp_set_distill: coef")
    refused(lambda: lib.rdp_set_distill(h, 1.0, -1), "rdp_set_distill: decay_timesteps")
    assert lib.rdp_distill_coef(null) == -1.0 and tr.distill_coef() == 0.0
    out = torch.empty(tr.S, 4, device=DEV)
    refused(lambda: lib.rdp_get_teacher_labels(null, P(out)), "rdp_get_teacher_labels: null handle")
    refused(lambda: lib.rdp_get_teacher_labels(h, null), "rdp_get_teacher_labels: null t_pdflat")
    refused(lambda: lib.rdp_get_teacher_labels(h, P(out)), "rdp_get_teacher_labels: no teacher")
    dm = np.zeros((4, 2))
    dmp = dm.ctypes.data_as(ctypes.c_void_p)
    refused(lambda: lib.rdp_read_distill_metrics(null, 1, dmp), "rdp_read_distill_metrics: null handle")
    refused(lambda: lib.rdp_read_distill_metrics(h, 0, null), "rdp_read_distill_metrics: null out")
    refused(lambda: lib.rdp_read_distill_metrics(h, -1, dmp), "rdp_read_distill_metrics: count")
    refused(lambda: lib.rdp_read_distill_metrics(h, 1, dmp), "rdp_read_distill_metrics: only 0 iterations")
    mean, std = (torch.from_numpy(x).to(DEV) for x in _filter())
    refused(lambda: lib.rdp_set_obfilter(null, P(mean), P(std), 1.0), "rdp_set_obfilter: null handle")
    refused(lambda: lib.rdp_set_obfilter(h, null, P(std), 1.0), "rdp_set_obfilter: null mean")
    refused(lambda: lib.rdp_set_obfilter(h, P(mean), null, 1.0), "rdp_set_obfilter: null std")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: lib.rdp_set_obfilter(h, P(mean), P(std), bad), "rdp_set_obfilter: count")
    for bad in (0.0, -0.2):
        std_bad = std.clone()
        std_bad[3] = bad
        refused(lambda: lib.rdp_set_obfilter(h, P(mean), P(std_bad), 1.0), r"rdp_set_obfilter: std\[3\]")
    m0, s0 = tr.obfilter()                                           # a refused seed left the filter alone
    assert torch.equal(m0.cpu(), torch.zeros(11)) and torch.equal(s0.cpu(), torch.ones(11))
    # lambda > 0 without labels: no teacher; a teacher set after the rollout; after a reset
    tr.set_distill(COEF)
    refused(lambda: lib.rdp_iterate(h), "rdp_iterate: distill coef 0.7 > 0 but no teacher")
    tr.rollout()
    refused(lambda: lib.rdp_optimize(h), "rdp_optimize: distill coef 0.7 > 0 but the current batch has no teacher labels")
    tr.set_teacher(tp)
    refused(lambda: lib.rdp_get_teacher_labels(h, P(out)), "rdp_get_teacher_labels: no rollout since")
    refused(lambda: lib.rdp_optimize(h), "rdp_optimize: .*no teacher labels")
    assert tr.iterations() == 0
    assert torch.equal(_params(tr), before)
    tr.iterate()                                                     # with both in place it runs
    assert tr.iterations() == 1 and tr.distill_metrics(1)[0, 1] == np.float32(COEF)
    assert not torch.equal(_params(tr), before)
    nat.check(lib.rdp_reset(h), "rdp_reset")                         # keeps teacher and setting, drops the labels
    assert tr.distill_coef() == np.float32(COEF)
    refused(lambda: lib.rdp_optimize(h), "rdp_optimize: .*no teacher labels")
    refused(lambda: lib.rdp_read_distill_metrics(h, 1, dmp), "only 0 iterations")
    tr.iterate()
    assert tr.distill_metrics(1)[0, 1] == np.float32(COEF)


# ---------------------------------------------------------------- 8. it distils
def test_it_distils():
    """256 envs x 50 under the committed PPO teacher, coef 10, constant: 20 iterations, every metric
    finite, the last iteration's KL below the first's (profiles/ppo_kickstart.json has the curve)."""
    from reacherdistilation_amd.ppo import PPOConfig, PPOTrainer
    from reacherdistilation_amd.teacher import ppo_teacher
    tr = PPOTrainer(PPOConfig(n_envs=256, horizon=50, seed=3), device=DEV)
    tr.set_teacher(ppo_teacher())
    tr.set_distill(10.0)
    for _ in range(20):
        tr.iterate()
    d, m = tr.distill_metrics(20), tr.metrics(20)
    print("ppo_kickstart distils: KL", " ".join(f"{x:.4f}" for x in d[:, 0]))
    assert np.all(np.isfinite(d)) and np.all(np.isfinite(m))
    np.testing.assert_array_equal(d[:, 1], np.full(20, 10.0))
    assert d[-1, 0] < d[0, 0], (d[0, 0], d[-1, 0])
