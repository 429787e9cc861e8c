"""CPU checks of the PPO oracle (oracle/ppo_np.py): the clipped-surrogate + value loss
gradient by finite differences (ratios inside and outside the clip range), GAE against its
definition, RunningMeanStd's moments.  Parity of PPO itself is UNPINNED by the reference
(baselines/TF absent, no reference test): these pin the restatement to the formulas."""
import json
import os

import numpy as np
import pytest

from oracle import policy_np as pn
from oracle import ppo_np as pp


def _nets(seed=0):
    rs = np.random.RandomState(seed)
    pol = np.concatenate([pn.normc(rs, (11, 64), 1.0).ravel(), rs.uniform(-.1, .1, 64),
                          pn.normc(rs, (64, 64), 1.0).ravel(), rs.uniform(-.1, .1, 64),
                          pn.normc(rs, (64, 2), 0.5).ravel(), rs.uniform(-.1, .1, 2), [-0.3, 0.2]])
    vf = np.concatenate([pn.normc(rs, (11, 64), 1.0).ravel(), rs.uniform(-.1, .1, 64),
                         pn.normc(rs, (64, 64), 1.0).ravel(), rs.uniform(-.1, .1, 64),
                         pn.normc(rs, (64, 1), 1.0).ravel(), [0.05]])
    assert pol.size == pp.P_POL and vf.size == pp.P_VF
    return pol, vf


def _batch(n, pol, seed=1, spread=0.6):
    rs = np.random.RandomState(seed)
    z = rs.uniform(-2, 2, (n, 11))
    fp = pp.pol_forward(pol, z)
    a = fp["mean"] + np.exp(fp["logstd"]) * rs.randn(n, 2)
    # old log-probs spread so that ratios fall inside and outside [1 - e, 1 + e]
    logp_old = pp.logp(fp["mean"], fp["logstd"], a) + rs.uniform(-spread, spread, n)
    return z, a, logp_old, rs.randn(n), rs.randn(n)


@pytest.mark.parametrize("seed", [0, 1])
def test_gradient_matches_finite_differences(seed):
    pol, vf = _nets(seed)
    z, a, lpo, atarg, ret = _batch(40, pol, seed + 5)
    r = pp.loss_and_grads(pol, vf, z, a, lpo, atarg, ret, 0.2)
    inside = (r["ratio"] > 0.8) & (r["ratio"] < 1.2)
    assert 0 < inside.sum() < 40        # both branches exercised
    g = np.concatenate([r["gpol"], r["gvf"]])
    x = np.concatenate([pol, vf])
    rs = np.random.RandomState(3)
    idx = list(rs.choice(x.size, 40, replace=False)) + [pp.P_POL - 1, pp.P_POL - 2, pp.P_POL - 3, x.size - 1]
    h = 1e-6
    for k in idx:
        xp, xm = x.copy(), x.copy()
        xp[k] += h
        xm[k] -= h
        fp_ = pp.total_loss(xp[:pp.P_POL], xp[pp.P_POL:], z, a, lpo, atarg, ret, 0.2)
        fm_ = pp.total_loss(xm[:pp.P_POL], xm[pp.P_POL:], z, a, lpo, atarg, ret, 0.2)
        num = (fp_ - fm_) / (2 * h)
        assert abs(num - g[k]) <= 1e-6 + 1e-5 * abs(num), (k, num, g[k])


@pytest.mark.parametrize("seed", [0, 1])
def test_grad_scale_bounds_the_gradient_and_row_contributions_sum_to_it(seed):
    """grad_scale's M is the backward on absolute values: M >= |g| entrywise, for both nets and
    with dead rows in the batch; row_contributions over all rows is the gradient itself, over a
    subset it is the gradient of the batch with the other rows' head derivatives zeroed."""
    pol, vf = _nets(seed)
    n = 40
    args = _batch(n, pol, seed + 5) + (0.2,)
    r = pp.loss_and_grads(pol, vf, *args)
    M_pol, M_vf, live = pp.grad_scale(pol, vf, *args)
    assert 0 < live.sum() < n
    outside = np.abs(r["ratio"] - 1) > 0.2
    assert (live & outside).any() and not (~live & ~outside).any()      # dead rows are outside the range
    assert (M_pol >= np.abs(r["gpol"])).all() and (M_vf >= np.abs(r["gvf"])).all()
    assert (M_pol > 0).all() and (M_vf > 0).all()
    cp, cv = pp.row_contributions(pol, vf, *args, rows=np.arange(n))
    assert np.abs(cp - r["gpol"]).max() <= 1e-12 * np.abs(r["gpol"]).max()
    assert np.abs(cv - r["gvf"]).max() <= 1e-12 * np.abs(r["gvf"]).max()
    sp, sv = np.zeros(pp.P_POL), np.zeros(pp.P_VF)
    for i in range(n):
        p, v = pp.row_contributions(pol, vf, *args, rows=[i])
        assert (p == 0).all() == (not live[i]) and (v != 0).any()        # a dead row feeds the value net only
        sp += p
        sv += v
    assert np.abs(sp - r["gpol"]).max() <= 1e-12 * np.abs(r["gpol"]).max()
    assert np.abs(sv - r["gvf"]).max() <= 1e-12 * np.abs(r["gvf"]).max()
    # as_live: the contribution a dead row would have, the clip ignored
    dead = int(np.flatnonzero(~live)[0])
    p, _ = pp.row_contributions(pol, vf, *args, rows=[dead], as_live=True)
    assert (p != 0).any()
    z, a, lpo, atarg, ret = args[:5]
    free = pp.loss_and_grads(pol, vf, z, a, lpo, atarg, ret, 1e9)        # a range nothing leaves
    q, _ = pp.row_contributions(pol, vf, z, a, lpo, atarg, ret, 1e9, rows=[dead])
    assert np.array_equal(p, q) and free["ratio"][dead] == r["ratio"][dead]


def test_grad_scale_is_zero_exactly_where_only_dead_rows_feed():
    """Observation column 3 is non-zero on dead rows only: row 3 of dW1 is fed by dead rows alone,
    so M and the gradient are exactly 0 there (policy net), while the value net, which has no dead
    rows, keeps M > 0; every other entry of M_pol stays positive."""
    pol, vf = _nets(2)
    z, a, lpo, atarg, ret = _batch(40, pol, 9)
    live = pp.grad_scale(pol, vf, z, a, lpo, atarg, ret, 0.2)[2]
    assert 0 < live.sum() < 40
    z[live, 3] = 0.0
    fp = pp.pol_forward(pol, z)                          # keep every row's ratio: logp_old moves with logp
    z0, _, lpo0, _, _ = _batch(40, pol, 9)
    fp0 = pp.pol_forward(pol, z0)
    lpo = lpo0 + pp.logp(fp["mean"], fp["logstd"], a) - pp.logp(fp0["mean"], fp0["logstd"], a)
    r = pp.loss_and_grads(pol, vf, z, a, lpo, atarg, ret, 0.2)
    M_pol, M_vf, live1 = pp.grad_scale(pol, vf, z, a, lpo, atarg, ret, 0.2)
    np.testing.assert_array_equal(live1, live)
    row3 = np.zeros(pp.P_POL, bool)
    row3[3 * 64:4 * 64] = True
    assert (M_pol[row3] == 0).all() and (r["gpol"][row3] == 0).all()
    assert (M_pol[~row3] > 0).all()
    assert (M_vf[3 * 64:4 * 64] > 0).all()


def test_gae_matches_definition():
    rs = np.random.RandomState(2)
    T, N = 7, 3
    rew, v = rs.randn(T, N), rs.randn(T, N)
    new = np.zeros((T, N))
    new[3, 0] = 1
    new[0, :] = 1
    nv = rs.randn(N)
    adv, ret = pp.gae(rew, v, new, nv, 0.9, 0.8)
    for n in range(N):
        for t in range(T):
            # sum over l of (gamma lam)^l delta_{t+l} until the episode ends
            acc, coef = 0.0, 1.0
            for u in range(t, T):
                nxt_new = new[u + 1, n] if u + 1 < T else 0.0
                vnext = v[u + 1, n] if u + 1 < T else nv[n]
                delta = rew[u, n] + 0.9 * vnext * (1 - nxt_new) - v[u, n]
                acc += coef * delta
                if nxt_new:
                    break
                coef *= 0.9 * 0.8
            assert abs(adv[t, n] - acc) < 1e-12
    np.testing.assert_allclose(ret, adv + v)


def test_running_mean_std():
    rms = pp.RunningMeanStd()
    rs = np.random.RandomState(0)
    x = rs.randn(1000, 11) * 3 + 1
    rms.update(x[:400])
    rms.update(x[400:])
    c = 1000 + 1e-2
    np.testing.assert_allclose(rms.mean, x.sum(0) / c)
    np.testing.assert_allclose(rms.std, np.sqrt((1e-2 + (x ** 2).sum(0)) / c - (x.sum(0) / c) ** 2))


def test_mt19937_64_check_value():
    """The C++ standard's own check ([rand.predef]): the 10,000th consecutive invocation of a
    default-constructed mt19937_64 (seed 5489) produces 9981545732273789042."""
    g = pp.mt19937_64(5489)
    for _ in range(9999):
        next(g)
    assert next(g) == 9981545732273789042


def test_shuffles_match_the_host_program():
    """tests/golden/ppo_shuffles.json holds the output of a stand-alone host C++ program
    (libstdc++): for each (seed, iteration, S, epochs) it constructs
    ``std::mt19937_64 rng(seed * 0x9E3779B97F4A7C15ull + iteration + 1)`` in uint64_t
    arithmetic and, per epoch, fills ``p[i] = i`` and runs ``for (i = S - 1; i > 0; --i)
    { j = rng() % (uint64_t)(i + 1); swap(p[i], p[j]); }`` without reseeding between epochs,
    printing each epoch's ``p``: the loop of the trainer's draw_perms.  The cases have a seed
    with a non-zero high word, a seed whose product wraps, iteration > 0, and more than 312
    draws (the generator's state is regenerated)."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "ppo_shuffles.json")) as f:
        cases = json.load(f)
    assert len(cases) == 3
    for c in cases:
        got = pp.shuffles(c["seed"], c["iteration"], c["S"], c["epochs"])
        np.testing.assert_array_equal(got, np.array(c["perm"]))
        for row in got:
            np.testing.assert_array_equal(np.sort(row), np.arange(c["S"]))
    a = pp.shuffles(11, 0, 10, 2)
    assert not np.array_equal(a, pp.shuffles(11, 1, 10, 2))       # the iteration enters the seed
    assert not np.array_equal(a[0], a[1])                         # the generator runs on across epochs


def test_ppo_adam_is_adamtf1_with_eps_1e_5():
    """pp.adam: policy_np.AdamTF1 (pinned to the reference's graph) with MpiAdam's epsilon and
    a per-step lr; one step against the formula in f64, and the beta powers carry."""
    opt = pp.adam(5)
    assert isinstance(opt, pn.AdamTF1) and opt.eps == np.float32(1e-5)
    g = np.array([1e-6, -1e-4, 1e-2, -1.0, 0.0], np.float32)
    x = np.ones(5, np.float32)
    opt.lr = np.float32(3e-3 * 0.75)
    opt.step(x, g)
    g64 = g.astype(np.float64)
    want = 1.0 - 3e-3 * 0.75 * np.sqrt(1 - 0.999) / (1 - 0.9) * (0.1 * g64) / (np.sqrt(0.001 * g64 * g64) + 1e-5)
    np.testing.assert_allclose(x, want, rtol=0, atol=2e-7)
    assert opt.b1p == np.float32(np.float32(0.9) * np.float32(0.9)) and opt.t == 1
    y = np.ones(5, np.float32)
    ref = pn.AdamTF1(5, lr=3e-3 * 0.75)                            # eps 1e-8 moves the small gradients further
    ref.step(y, g)
    assert abs(y[0] - x[0]) > 1e-4
