"""GPU parity of minibatch_kernel's clipped surrogate (csrc/ppo.hip) with ratios on every side of
the clip range, against oracle/ppo_np.py under tests/ppo_parity.py's per-net bound.

rollout() freezes the old log-probabilities (logp_old_kernel); set_policy / set_value then move
the nets by ppo_parity.perturbed (W3, b3, logstd and the value net) and optimize() runs with
optim_stepsize 1e-12, which leaves the parameters where they were put.  grad() is then the
gradient at the moved policy against the rollout policy's log-probabilities: about 12 % of the
rows are dead, each quadrant (ratio above / below the range x advantage sign) holds about 5 %,
and pol_surr is about 0.02 instead of 0.  Every case first asserts from the oracle's own ratios
that it is not vacuous (large cases: every quadrant holds at least 2 % of the rows; cases under
100 rows: a dead row and a live row outside the range); on the GPU's batches every case meets its
condition with the perturbation as it stands (ppo_parity.perturbed's factor 1).
"""
import numpy as np
import pytest

from oracle import ppo_np as pp
from tests import ppo_parity as par

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _trainer(**kw):
    from reacherdistilation_amd.ppo import PPOConfig, PPOTrainer
    cfg = dict(n_envs=256, horizon=64, seed=11, optim_batchsize=0, optim_epochs=1, max_timesteps=10 ** 6)
    cfg.update(kw)
    return PPOTrainer(PPOConfig(**cfg), device=DEV)


def _np(x):
    return x.cpu().numpy().astype(np.float64)


def _actor_batch(tr):
    """rollout(), then the oracle's view of the batch: z under the post-rollout filter, actions,
    the rollout policy's log-probabilities, standardized advantages, returns."""
    pol0 = tr.policy().cpu().numpy()
    tr.rollout()
    b = {k: _np(v) for k, v in tr.batch().items()}
    mean1, std1 = (_np(x) for x in tr.obfilter())
    z = pp.obz(b["ob"].reshape(-1, 11), mean1, std1)
    a = b["ac"].reshape(-1, 2)
    fp = pp.pol_forward(pol0, z)
    return dict(z=z, a=a, lpo=pp.logp(fp["mean"], fp["logstd"], a), atarg=pp.standardize(b["adv"].reshape(-1)),
                ret=b["ret"].reshape(-1))


def _reference(pol, vf, b, rows, eps):
    return par.reference(pol, vf, b["z"][rows], b["a"][rows], b["lpo"][rows], b["atarg"][rows], b["ret"][rows], eps)


def _assert_not_vacuous(r, atarg, label):
    q = par.quadrants(r, atarg)
    outside_live = int((r["live"] & (r["above"] | r["below"])).sum())
    print(f"ppo_clip {label}: quadrants {q} dead {int(r['dead'].sum())} live outside {outside_live} "
          f"pol_surr {r['pol_surr']:.4f}")
    if r["rows"] >= 100:
        assert min(q.values()) >= 0.02, (label, q)
    assert r["dead"].any() and outside_live >= 1, label


def _run(n, T, mb=0, lrmult=1.0):
    label = f"{n}x{T}" + (f" mb {mb}" if mb else "") + (f" lrmult {lrmult}" if lrmult != 1 else "")
    S = n * T
    kw = dict(max_timesteps=2 * S) if lrmult != 1 else {}
    tr = _trainer(n_envs=n, horizon=T, optim_batchsize=mb, optim_stepsize=1e-12, **kw)
    it = 0
    if lrmult != 1:
        tr.iterate()                                     # timesteps S of 2 S: lrmult 0.5 from here on
        it = 1
    eps = 0.2 * lrmult
    b = _actor_batch(tr)
    pol1, vf1 = par.perturbed(tr.policy().cpu().numpy(), tr.value().cpu().numpy())
    tr.set_policy(pol1)
    tr.set_value(vf1)
    mbs = mb or S
    nmb = S // mbs
    perm = pp.shuffles(11, it, S, 1)[0] if mb else np.arange(S)
    refs = [_reference(pol1, vf1, b, perm[j * mbs:(j + 1) * mbs], eps) for j in range(nmb)]
    last = refs[-1]
    _assert_not_vacuous(last, b["atarg"][perm[(nmb - 1) * mbs:nmb * mbs]], label)
    assert all((r["ratio"] != 1).all() for r in refs)   # a wrong old log-probability shows on any row
    if lrmult != 1:                                      # eps = 0.2 would kill other rows
        stale = pp.grad_scale(pol1, vf1, b["z"], b["a"], b["lpo"], b["atarg"], b["ret"], 0.2)[2]
        assert not np.array_equal(~stale, last["dead"]) and last["dead"].sum() > (~stale).sum()
    tr.optimize()
    np.testing.assert_allclose(tr.policy().cpu().numpy(), pol1, rtol=0, atol=1e-10)
    par.check_grad(_np(tr.grad()), last, "clip " + label)
    m = tr.metrics(1)[0]
    pol_surr, vf_loss = np.mean([r["pol_surr"] for r in refs]), np.mean([r["vf_loss"] for r in refs])
    clipfrac = np.mean([(r["above"] | r["below"]).mean() for r in refs])
    either = sum(int(r["either"].sum()) for r in refs)
    print(f"ppo_clip {label}: pol_surr {m[2]:.6f} / {pol_surr:.6f} vf_loss {m[3]:.5f} / {vf_loss:.5f} "
          f"clipfrac {m[5]:.5f} / {clipfrac:.5f} either way {either}")
    assert m[6] == pytest.approx(lrmult, rel=1e-6)
    assert abs(m[2] - pol_surr) <= 1e-5 + 1e-4 * abs(pol_surr), (m[2], pol_surr)
    assert abs(m[3] - vf_loss) <= 1e-4 * vf_loss + 1e-5, (m[3], vf_loss)
    # 2^-23: the kernel counts in units of the f32 1 / mb and the metrics row is f32
    assert clipfrac > 0 and abs(m[5] - clipfrac) <= either / (nmb * mbs) + 2.0 ** -23, (m[5], clipfrac, either)
    return last


@pytest.mark.parametrize("n,T", [(33, 1), (3, 7), (1, 50), (64, 8), (255, 63), (1040, 32)])
def test_clipped_surrogate_gradient_full_batch(n, T):
    """33 x 1: a full 32-row tile and a tile with one row.  3 x 7, 1 x 50: 21 and 50 rows in a
    padded tile.  64 x 8: 16 whole tiles.  255 x 63: 503 tiles over 256 workgroups, the last one
    ragged.  1040 x 32: 1,040 tiles, more than logp_old_kernel's 1,024 workgroups: the ratios
    differ from 1 on every row, so a wrong old log-probability on the looped tiles shows."""
    _run(n, T)


@pytest.mark.parametrize("n,T,mb", [(50, 3, 50), (300, 7, 1000)])
def test_clipped_surrogate_gradient_shuffled_minibatches(n, T, mb):
    """Minibatches of 50 and 1,000 rows, no multiple of the 32-row tile: the gradient of the
    epoch's last minibatch over the rows ppo_np.shuffles names; the metrics over all of them."""
    _run(n, T, mb=mb)


def test_clip_range_follows_lrmult():
    """After one iteration of max_timesteps = 2 S, lrmult = 0.5 and clip_eps = 0.1: more rows are
    dead than eps = 0.2 would leave."""
    _run(64, 8, lrmult=0.5)


def test_second_epoch_gradient_after_a_real_step():
    """optim_epochs 2, optim_stepsize 1e-2 on the full batch: the second epoch's gradient at the
    parameters a 1-epoch twin reads after its step, with rows outside the range on both sides
    (test_clipped_epoch_metrics_match_oracle's condition: at least 50 on each)."""
    kw = dict(optim_batchsize=0, optim_stepsize=1e-2)
    tr = _trainer(optim_epochs=2, **kw)
    b = _actor_batch(tr)
    tr1 = _trainer(optim_epochs=1, **kw)
    tr1.rollout()
    tr1.optimize()
    pol1, vf1 = tr1.policy().cpu().numpy(), tr1.value().cpu().numpy()
    r = _reference(pol1, vf1, b, np.arange(tr.S), 0.2)
    assert min(r["above"].sum(), r["below"].sum()) >= 50, (r["above"].sum(), r["below"].sum())
    assert r["dead"].any()
    tr.optimize()
    par.check_grad(_np(tr.grad()), r, "second epoch 256x64")
