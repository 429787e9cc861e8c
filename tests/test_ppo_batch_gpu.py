"""GPU parity of the PPO teacher trainer (csrc/ppo.hip) beyond its first full batch, against
oracle/ppo_np.py, the C oracle's env (oracle/ref_c.py) and policy_np.AdamTF1.

  * three iterations of rollouts: episode clocks, reset draws, env transitions, actions,
    value predictions, the bootstrap value, GAE, the filter and the metrics row, with env
    ids that cross 2^32, a seed with a high word, two logstd values and two GAE blocks;
  * shuffled minibatches: the gradient of the last minibatch of the last epoch is the
    oracle's over the rows that oracle.ppo_np.shuffles names (and not over other rows), by the
    relative L2 norm of [pol | vf] and by tests/ppo_parity.py's bound on each net;
  * the Adam step (epsilon 1e-5, lr = stepsize * lrmult, beta powers carried across
    iterations), the schedule clamp and the constant schedule;
  * the clipped epoch's pol_surr, vf_loss and clipfrac;
  * rdp_reset, the metrics ring and rdp_create's argument checks.

Tolerances are the project's own for each quantity (tests/test_ppo_gpu.py, test_env_gpu.py,
test_student_mlp_gpu.py); the one measured quantity, the number of env steps next to the
joint limit that land on the other side of it, is bounded by the f32 C oracle's own count.
"""
import numpy as np
import pytest
import torch

from oracle import policy_np as pn
from oracle import ppo_np as pp
from oracle import ref_c
from oracle.refnet_np import M32, philox4x32_10
from tests import ppo_parity as par

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EP = 50                                    # TimeLimit(50)
P_ALL = pp.P_POL + pp.P_VF


def _trainer(env_base=0, **kw):
    from reacherdistilation_amd.ppo import PPOConfig, PPOTrainer
    cfg = dict(n_envs=256, horizon=64, seed=11, optim_batchsize=0, optim_epochs=1, max_timesteps=10 ** 6)
    cfg.update(kw)
    return PPOTrainer(PPOConfig(**cfg), device=DEV, env_base=env_base)


def _np(x):
    return x.cpu().numpy().astype(np.float64)


def _batch(tr):
    return {k: _np(v) for k, v in tr.batch().items()}


def _params(tr):
    return torch.cat([tr.policy(), tr.value()]).cpu()


def _normals(seed, env_base, n, it, T):
    """Box-Muller normals of Philox counter {gid lo, gid hi, it, t}, key {seed lo, seed hi ^ 0xA5A5A5A5}."""
    gid = np.uint64(env_base) + np.arange(n, dtype=np.uint64)
    out = np.zeros((T, n, 2))
    for t in range(T):
        w = philox4x32_10([gid & M32, gid >> np.uint64(32), np.full(n, it, np.uint64), np.full(n, t, np.uint64)],
                          seed & 0xFFFFFFFF, (seed >> 32) ^ 0xA5A5A5A5)
        u1 = ((w[0] >> np.uint32(8)).astype(np.float64) + 1) / 16777216.0
        u2 = (w[1] >> np.uint32(8)).astype(np.float64) / 16777216.0
        rad = np.sqrt(-2 * np.log(u1))
        out[t, :, 0] = rad * np.cos(2 * np.pi * u2)
        out[t, :, 1] = rad * np.sin(2 * np.pi * u2)
    return out


def _state_of(ob, dtype=np.float64):
    """Env state [8, m] (q0 q1 v0 v1 tx ty dx dy) of observations [m, 11], as
    test_env_gpu.test_single_env_gym_api_fixture rebuilds it."""
    return np.ascontiguousarray(np.stack([np.arctan2(ob[:, 2], ob[:, 0]), np.arctan2(ob[:, 3], ob[:, 1]),
                                          ob[:, 6], ob[:, 7], ob[:, 4], ob[:, 5], ob[:, 8], ob[:, 9]]), dtype)


def check_actor_batches(recs, n, T, seed, env_base, gamma, lam):
    """recs[k]: pol, vf, mean, std read before rollout k; its batch b; the filter (mean1, std1)
    after it.  Pure numpy, so that it can be run against a CPU restatement of the rollout."""
    K = len(recs)
    g_of = lambda k, t: T * k + t                                    # env step since the trainer's reset
    ids = [env_base + e for e in range(n)]
    rms = pp.RunningMeanStd()
    for k, r in enumerate(recs):
        b = r["b"]
        # episode clocks and reset draws
        new = np.array([[float(g_of(k, t) % EP == 0)] * n for t in range(T)])
        np.testing.assert_array_equal(b["new"], new)
        for t in range(T):
            if g_of(k, t) % EP == 0:
                _, want = ref_c.reset(ref_c.philox_draws(seed, ids, g_of(k, t) // EP))
                np.testing.assert_allclose(b["ob"][t], want, atol=1e-6, rtol=0)
        # value predictions and actions under the filter and parameters read before the rollout
        z = pp.obz(b["ob"].reshape(T * n, 11), r["mean"], r["std"])
        np.testing.assert_allclose(b["vpred"].reshape(-1), pp.vf_forward(r["vf"], z)["v"], atol=2e-5, rtol=1e-4)
        fp = pp.pol_forward(r["pol"], z)
        assert fp["logstd"][0] != fp["logstd"][1]
        want_ac = fp["mean"] + np.exp(fp["logstd"]) * _normals(seed, env_base, n, k, T).reshape(T * n, 2)
        np.testing.assert_allclose(b["ac"].reshape(T * n, 2), want_ac, atol=1e-5, rtol=1e-4)
        if k + 1 < K:                                                # old value net and filter, next segment's first ob
            zn = pp.obz(recs[k + 1]["b"]["ob"][0], r["mean"], r["std"])
            assert g_of(k + 1, 0) % EP != 0
            np.testing.assert_allclose(b["nextvpred"], pp.vf_forward(r["vf"], zn)["v"], atol=2e-5, rtol=1e-4)
        adv, ret = pp.gae(b["rew"], b["vpred"], b["new"], b["nextvpred"], gamma, lam)
        np.testing.assert_allclose(b["adv"], adv, atol=1e-4 * np.abs(adv).max())
        np.testing.assert_allclose(b["ret"], ret, atol=1e-4 * np.abs(ret).max())
        rms.update(b["ob"].reshape(T * n, 11))
        np.testing.assert_allclose(r["mean1"], rms.mean, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(r["std1"], rms.std, rtol=1e-4, atol=1e-6)
    # env dynamics: ob[g + 1] is the step of ob[g] under ac[g], across the iterations' seams
    ob = np.concatenate([r["b"]["ob"] for r in recs])                # [K T, n, 11]
    ac = np.concatenate([r["b"]["ac"] for r in recs]).reshape(-1, 2)
    rew = np.concatenate([r["b"]["rew"] for r in recs]).reshape(-1)
    new = np.concatenate([r["b"]["new"] for r in recs])
    st64 = _state_of(ob.reshape(-1, 11))
    # The joint limit is a spring, and at these noise levels the elbow overshoots it past pi,
    # where arctan2 names the angle on the wrong side of the limit (the C oracle, rolled out on
    # the CPU and read back this way, missed 61 rows of 56,400).  The angle moves far less than
    # pi a step, so unwrapping each episode's sequence from its reset (|q1| < 0.1) recovers it.
    q1 = st64[1].reshape(K * T, n)
    for g0 in range(0, K * T, EP):
        q1[g0:g0 + EP] = np.unwrap(q1[g0:g0 + EP], axis=0)
    assert np.abs(np.diff(q1, axis=0))[new[1:] == 0].max() < 1.5
    st32 = st64.astype(np.float32)
    q1_before = st64[1].copy()
    want, want_rew = ref_c.step(st64, ac, np.float64)
    near = (np.abs(q1_before) > 2.8) | (np.abs(st64[1]) > 2.8)        # the f64 oracle alone decides
    np.testing.assert_allclose(rew, want_rew, atol=1e-5, rtol=0)
    pair = np.concatenate([new[1:] == 0, np.zeros((1, n), bool)]).reshape(-1)   # rows whose successor is recorded
    assert pair.sum() == (K * T - 1 - ((np.arange(1, K * T) % EP) == 0).sum()) * n
    nxt = np.concatenate([ob[1:], ob[:1]]).reshape(-1, 11)
    miss = ~np.isclose(nxt, want, atol=2e-4, rtol=1e-4).all(axis=1)
    ob32, _ = ref_c.step(st32, ac, np.float32)
    miss32 = ~np.isclose(ob32.astype(np.float64), want, atol=2e-4, rtol=1e-4).all(axis=1)
    strict = pair & ~near
    counts = dict(rows=int(pair.sum()), strict=int(strict.sum()), near=int((pair & near).sum()),
                  kernel_miss_near=int((miss & pair & near).sum()), c_f32_miss_near=int((miss32 & pair & near).sum()))
    print("transitions:", counts)
    assert not (miss & strict).any(), (np.flatnonzero(miss & strict)[:10], counts)
    assert counts["strict"] >= 0.75 * counts["rows"], counts
    assert counts["kernel_miss_near"] <= 2 * counts["c_f32_miss_near"] + 3, counts
    return counts


def episode_returns_mean(rew_all, k, T):
    """Mean over the episodes that ended in iteration k of the sum of their 50 recorded rewards."""
    ends = [g for g in range(T * k, T * (k + 1)) if (g + 1) % EP == 0]
    if not ends:
        return 0, 0.0
    sums = np.stack([rew_all[g - EP + 1:g + 1].sum(0) for g in ends])
    return len(ends), sums.mean()


def test_three_iterations_match_the_oracle():
    """n = 300 (10 rollout workgroups, the last with 12 envs; 2 GAE blocks, the second with 44
    lanes), T = 64, env ids from 2^32 - 100, seed (7 << 32) | 11, logstd (-1, -0.5), gamma 0.9,
    lam 0.8: the new flags fall at t = 0, 50 / 36 / 22.
    Measured: 47,412 of the 56,400 compared transitions (84 %) are away from the joint limit
    and none of them fails; of the 8,988 next to it the kernel misses 0 and the f32 C oracle
    0 (bound: twice the oracle's count + 3).  A CPU dry run of the checker with the f32 C
    oracle as the rollout gave 47,505 / 8,895 / 0 / 0."""
    n, T, K = 300, 64, 3
    seed, env_base = (7 << 32) | 11, 2 ** 32 - 100
    tr = _trainer(env_base=env_base, n_envs=n, horizon=T, seed=seed, gamma=0.9, lam=0.8)
    S = n * T
    pol = tr.policy().cpu().numpy()
    pol[-2:] = (-1.0, -0.5)
    tr.set_policy(pol)
    recs = []
    for k in range(K):
        r = dict(pol=tr.policy().cpu().numpy(), vf=tr.value().cpu().numpy())
        r["mean"], r["std"] = (_np(x) for x in tr.obfilter())
        tr.rollout()
        r["b"] = _batch(tr)
        r["mean1"], r["std1"] = (_np(x) for x in tr.obfilter())
        tr.optimize()
        r["pol_after"] = tr.policy().cpu().numpy().astype(np.float64)
        r["m"] = tr.metrics(1)[0]
        recs.append(r)
    np.testing.assert_array_equal(recs[0]["pol"][-2:], np.float32([-1.0, -0.5]))
    check_actor_batches(recs, n, T, seed, env_base, 0.9, 0.8)
    rew_all = np.concatenate([r["b"]["rew"] for r in recs])
    for k, r in enumerate(recs):
        m = dict(zip(("ep_ret_mean", "episodes", "pol_surr", "vf_loss", "entropy", "clipfrac", "lrmult", "timesteps"),
                     r["m"]))
        eps, ret_mean = episode_returns_mean(rew_all, k, T)
        assert eps == 1                                              # global steps 49, 99, 149
        assert m["episodes"] == n * eps
        assert m["ep_ret_mean"] == pytest.approx(ret_mean, rel=1e-5)
        assert abs(m["entropy"] - (r["pol_after"][-2:].sum() + 1 + np.log(2 * np.pi))) <= 1e-6
        assert m["timesteps"] == (k + 1) * S
        assert m["lrmult"] == pytest.approx(1 - k * S / 10 ** 6, rel=1e-6)


def test_bootstrap_value_is_zero_where_the_next_observation_starts_an_episode():
    """T = 25: the segment after iteration 0 continues an episode (nextvpred != 0), the one
    after iteration 1 starts one (nextvpred == 0 exactly, and the next batch opens with new)."""
    n, T = 33, 25
    tr = _trainer(n_envs=n, horizon=T)
    tr.iterate()
    nv = tr.batch()["nextvpred"].cpu().numpy()
    assert np.all(nv != 0)
    tr.iterate()
    b = tr.batch()
    np.testing.assert_array_equal(b["nextvpred"].cpu().numpy(), np.zeros(n, np.float32))
    assert b["new"].cpu().numpy().sum() == 0 and nv.shape == (n,)
    tr.rollout()
    new = tr.batch()["new"].cpu().numpy()
    np.testing.assert_array_equal(new[0], np.ones(n, np.float32))
    assert new[1:].sum() == 0


@pytest.mark.parametrize("it", [0, 1])
@pytest.mark.parametrize("n,T,mb,E", [(96, 1, 64, 1), (300, 7, 1000, 2), (50, 3, 50, 3)])
def test_shuffled_minibatch_gradient_matches_oracle(n, T, mb, E, it):
    """optim_stepsize 1e-12 keeps the parameters at the rollout's values through every step, so
    each minibatch sees ratio 1 and grad() after optimize() is the gradient over the rows of the
    last minibatch of the last epoch: 64 of 96 rows (tail of 32 dropped); the second 1,000 of
    2,100 rows of epoch 1 (tail 100, ragged last tile); 50-row minibatches (not a multiple of
    the 32-row tile), the third of epoch 2.  it = 1: the shuffles of the second iteration."""
    seed = 11
    tr = _trainer(n_envs=n, horizon=T, optim_batchsize=mb, optim_epochs=E, optim_stepsize=1e-12)
    S, nmb = n * T, (n * T) // mb
    if it:
        tr.iterate()
    pol, vf = tr.policy().cpu().numpy(), tr.value().cpu().numpy()
    tr.rollout()
    b = _batch(tr)
    mean1, std1 = (_np(x) for x in tr.obfilter())
    z = pp.obz(b["ob"].reshape(-1, 11), mean1, std1)
    a = b["ac"].reshape(-1, 2)
    fp = pp.pol_forward(pol, z)
    lpo = pp.logp(fp["mean"], fp["logstd"], a)
    atarg = pp.standardize(b["adv"].reshape(-1))
    ret = b["ret"].reshape(-1)
    eps = 0.2 * (1.0 - it * S / 10 ** 6)
    tr.optimize()
    np.testing.assert_allclose(tr.policy().cpu().numpy(), pol, rtol=0, atol=1e-10)
    g = _np(tr.grad())
    perm = pp.shuffles(seed, it, S, E)

    def oracle(rows):
        return pp.loss_and_grads(pol, vf, z[rows], a[rows], lpo[rows], atarg[rows], ret[rows], eps)

    def rel(r):
        want = np.concatenate([r["gpol"], r["gvf"]])
        return np.linalg.norm(g - want) / np.linalg.norm(want)

    last = [oracle(perm[E - 1][j * mb:(j + 1) * mb]) for j in range(nmb)]
    assert rel(last[-1]) < 1e-3, rel(last[-1])
    rows = perm[E - 1][(nmb - 1) * mb:nmb * mb]                      # each net at its own scale
    par.check_grad(g, par.reference(pol, vf, z[rows], a[rows], lpo[rows], atarg[rows], ret[rows], eps),
                   f"shuffled {n}x{T} mb {mb} epochs {E} it {it}")
    identity = np.arange((nmb - 1) * mb, nmb * mb)                   # the same slice without the shuffle
    assert not rel(oracle(identity)) < 1e-3, rel(oracle(identity))
    m = tr.metrics(1)[0]
    pol_surr, vf_loss = np.mean([r["pol_surr"] for r in last]), np.mean([r["vf_loss"] for r in last])
    assert abs(m[2] - pol_surr) < 1e-4 and abs(m[3] - vf_loss) <= 1e-4 * vf_loss + 1e-5, (m, pol_surr, vf_loss)


def _adam_ok(after, want, before):
    return np.all(np.abs(after - want) <= 1e-6 + 1e-4 * np.abs(want - before))


def test_adam_step_and_linear_schedule_match_the_oracle():
    """Four iterations over max_timesteps = 4 S: lrmult 1, 3/4, 1/2, 1/4.  One AdamTF1(eps 1e-5)
    stepped with the device gradient and lr = 3e-3 lrmult reproduces the parameters (1e-6 +
    1e-4 |update| per element); with eps 1e-8 it does not.  The fifth iteration has lrmult 0."""
    n, T = 64, 50
    S = n * T
    tr = _trainer(n_envs=n, horizon=T, optim_stepsize=3e-3, max_timesteps=4 * S)
    opt = pp.adam(P_ALL)
    for k in range(4):
        tr.rollout()
        before = _params(tr).numpy()
        tr.optimize()
        after = _params(tr).numpy()
        g = tr.grad().cpu().numpy()
        lrmult = 1 - k / 4
        assert tr.metrics(1)[0][6] == lrmult
        if k == 0:
            wrong = pn.AdamTF1(P_ALL, lr=np.float32(3e-3), eps=1e-8).step(before.copy(), g)
            assert not _adam_ok(after, wrong, before)
        opt.lr = np.float32(3e-3) * np.float32(lrmult)
        want = opt.step(before.copy(), g)
        assert np.abs(want - before).max() > 1e-4
        assert _adam_ok(after, want, before), np.abs(after - want).max()
    tr.rollout()
    before = _params(tr)
    tr.optimize()
    assert torch.equal(before, _params(tr))
    m = tr.metrics(5)
    assert np.all(np.isfinite(m)) and m[4, 6] == 0.0
    np.testing.assert_array_equal(m[:, 6], [1.0, 0.75, 0.5, 0.25, 0.0])
    np.testing.assert_array_equal(m[:, 7], S * np.arange(1, 6))


def test_constant_schedule_keeps_lrmult_at_one():
    n, T = 64, 50
    tr = _trainer(n_envs=n, horizon=T, optim_stepsize=3e-3, max_timesteps=4 * n * T, schedule="constant")
    for _ in range(4):
        tr.iterate()
    tr.rollout()
    before = _params(tr)
    tr.optimize()
    assert not torch.equal(before, _params(tr))                      # past max_timesteps and still stepping
    m = tr.metrics(5)
    np.testing.assert_array_equal(m[:, 6], np.ones(5))
    assert np.all(np.isfinite(m))


@pytest.mark.parametrize("stepsize", [3e-3, 1e-2])
def test_clipped_epoch_metrics_match_oracle(stepsize):
    """The second epoch over the same full batch (parameters before it from a 1-epoch twin):
    pol_surr and vf_loss of the clipped surrogate, and clipfrac = mean(|ratio - 1| > eps) up to
    the rows whose |ratio - 1| is within 1e-5 of eps, which f32 may classify either way.
    After a step of 3e-3 (test_clipped_branch_gradient_matches_oracle's) one row of 16,384 is
    outside the clip range; after one of 1e-2 rows leave it on both sides."""
    kw = dict(optim_batchsize=0, optim_stepsize=stepsize)
    tr = _trainer(optim_epochs=2, **kw)
    tr.rollout()
    pol0 = tr.policy().cpu().numpy()
    b = _batch(tr)
    mean1, std1 = (_np(x) for x in tr.obfilter())
    z = pp.obz(b["ob"].reshape(-1, 11), mean1, std1)
    a = b["ac"].reshape(-1, 2)
    fp0 = pp.pol_forward(pol0, z)
    lpo = pp.logp(fp0["mean"], fp0["logstd"], a)
    atarg = pp.standardize(b["adv"].reshape(-1))
    tr1 = _trainer(optim_epochs=1, **kw)
    tr1.rollout()
    tr1.optimize()
    pol1, vf1 = tr1.policy().cpu().numpy(), tr1.value().cpu().numpy()
    tr.optimize()
    eps = 0.2                                                        # iteration 0: lrmult 1
    r = pp.loss_and_grads(pol1, vf1, z, a, lpo, atarg, b["ret"].reshape(-1), eps)
    m = tr.metrics(1)[0]
    assert abs(m[2] - r["pol_surr"]) < 1e-4 and abs(m[3] - r["vf_loss"]) <= 1e-4 * r["vf_loss"] + 1e-5
    dev = np.abs(r["ratio"] - 1)
    clipfrac = (dev > eps).mean()
    either = (np.abs(dev - eps) < 1e-5).sum()
    print("clipfrac:", stepsize, m[5], clipfrac, "pol_surr", m[2], r["pol_surr"], "vf_loss", m[3], r["vf_loss"], "above", (r["ratio"] > 1 + eps).sum(), "below", (r["ratio"] < 1 - eps).sum(),
          "either way", either)
    assert clipfrac > 0 and m[5] > 0
    if stepsize > 3e-3:
        assert min((r["ratio"] > 1 + eps).sum(), (r["ratio"] < 1 - eps).sum()) >= 50
    assert abs(m[5] - clipfrac) <= either / tr.S, (m[5], clipfrac, either)


def _two_iterations(tr):
    for _ in range(2):
        tr.iterate()
    b = tr.batch()
    return [tr.policy().cpu(), tr.value().cpu(), torch.from_numpy(tr.metrics(2))] + [b[k].cpu() for k in sorted(b)]


def test_reset_returns_to_the_initial_state():
    """rdp_reset after two iterations (shuffled minibatches, two epochs), the initial policy
    and value set again: the next two iterations are bitwise a fresh trainer's."""
    from reacherdistilation_amd import _native as nat
    kw = dict(n_envs=100, horizon=30, optim_batchsize=1000, optim_epochs=2)
    want = _two_iterations(_trainer(**kw))
    tr = _trainer(**kw)
    pol0, vf0 = tr.policy(), tr.value()
    first = _two_iterations(tr)
    assert not torch.equal(tr.policy(), pol0)
    tr._sync_stream()
    nat.check(tr._lib.rdp_reset(tr._h), "rdp_reset")
    assert tr.iterations() == 0
    tr.set_policy(pol0)
    tr.set_value(vf0)
    mean, std = tr.obfilter()
    assert torch.equal(mean.cpu(), torch.zeros(11)) and torch.equal(std.cpu(), torch.ones(11))
    got = _two_iterations(tr)
    for x, y, w in zip(got, first, want):
        assert torch.equal(x, w) and torch.equal(y, w)


def test_metrics_ring_wraps():
    n, T = 40, 10
    tr = _trainer(n_envs=n, horizon=T, metrics_len=2)
    for _ in range(3):
        tr.iterate()
    m = tr.metrics(2)
    np.testing.assert_array_equal(m[:, 7], [2 * n * T, 3 * n * T])
    np.testing.assert_allclose(m[:, 6], [1 - n * T / 10 ** 6, 1 - 2 * n * T / 10 ** 6], rtol=1e-6)
    np.testing.assert_array_equal(tr.metrics(1)[0], m[1])
    with pytest.raises(RuntimeError):
        tr.metrics(3)


@pytest.mark.parametrize("kw", [dict(entcoeff=0.01), dict(n_envs=8, horizon=4, optim_batchsize=33),
                                dict(horizon=0), dict(n_envs=4097, horizon=4096), dict(env_base=-1)],
                         ids=["entcoeff", "batchsize_gt_S", "horizon_0", "S_gt_2p24", "env_base_lt_0"])
def test_create_refuses_bad_config(kw):
    with pytest.raises(RuntimeError, match="rdp_create"):
        _trainer(**kw)
    _trainer(n_envs=8, horizon=4, optim_batchsize=32).close()        # the largest batch size it accepts
