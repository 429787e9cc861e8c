"""Shared oracle side of the kickstart tests (csrc/ppo.hip's kickstart instance: PPO's minibatch
loss + lambda x the minibatch-mean KL(pi || teacher)), from what oracle/ already exports (test
infrastructure: imports oracle/, never the product path).

The KL is the project's kl_loss direction, the learner first (policy_np.loss_and_dmean(..., "kl")),
per row  sum_c [ lt_c - ls_c + (exp(2 ls_c) + (mu_c - mut_c)^2) / (2 exp(2 lt_c)) - 1/2 ].  Its head
derivatives, with the minibatch's 1/mb and lambda folded in,
    dmean_c = (lambda/mb) (mu_c - mut_c) / sigmat_c^2,   dlogstd_c = (lambda/mb) (sigma_c^2/sigmat_c^2 - 1),
go through ppo_np._net_backward like the surrogate's, on every row (the clip does not touch them).
The per-entry scale M_e of tests/ppo_parity.py is extended the same way: the same backward on
absolute values, added to ppo_np.grad_scale's.
"""
import numpy as np

from oracle import policy_np as pn
from oracle import ppo_np as pp
from tests import ppo_parity as par

TEACHER_LOGSTD = (-0.7, -0.3)


def teacher(seed=3, clip_entry=6, clip_std=0.02):
    """A teacher that is not the learner: ppo_parity.perturbed(baselines_nets(seed)) weights (W3 of
    normc(0.01) + U(-.02, .02), b3 moved), log-std TEACHER_LOGSTD, and a filter of its own: means in
    U(-.3, .3), stds in U(.5, 2) except entry `clip_entry` (a joint velocity: under 0.005 at a
    reset, of order 1 later in a rollout) with mean 0.1 and std `clip_std`, which puts that input
    on both sides of the +-5 clip among the reset rows and past it on most later rows."""
    pol, vf = par.baselines_nets(seed)
    pol, _ = par.perturbed(pol, vf)
    pol[slice(*par.block("logstd"))] = TEACHER_LOGSTD
    rs = np.random.RandomState(seed + 100)
    mean = rs.uniform(-.3, .3, pp.OBD).astype(np.float32)
    std = rs.uniform(.5, 2.0, pp.OBD).astype(np.float32)
    mean[clip_entry], std[clip_entry] = 0.1, clip_std   # a reset's |velocity| < 0.005: z within -5 +- 0.25
    return pol.astype(np.float32), mean, std


def teacher_pdflat(tpol, tmean, tstd, ob):
    """[n, 4] = the teacher's mean | logstd on raw observations, in f64 (policy_np.forward)."""
    f = pn.forward(np.asarray(tpol, np.float64), np.asarray(tmean, np.float64), np.asarray(tstd, np.float64),
                   np.asarray(ob, np.float64))
    return np.concatenate([f["mean"], np.broadcast_to(f["logstd"], f["mean"].shape)], 1)


def kl_heads(pol, z, tflat, lam):
    """(mean KL over the rows, dmean [n, 2], per-row dlogstd [n, 2], forward dict) of
    lam x mean_rows KL(pi || teacher) at the learner `pol` on filtered inputs z."""
    fp = pp.pol_forward(pol, z)
    n = z.shape[0]
    mt, lt = tflat[:, :2], tflat[:, 2:]
    ls = fp["logstd"]
    vs, vt = np.exp(2 * ls), np.exp(2 * lt)
    diff = fp["mean"] - mt
    kl = (lt - ls + (vs + diff ** 2) / (2 * vt) - 0.5).sum(1)
    return kl.mean(), lam / n * diff / vt, lam / n * (vs / vt - 1.0), fp


def kl_grad(pol, z, tflat, lam, absolute=False, keep=None):
    """Gradient of lam x mean KL w.r.t. the policy vector [5060] (absolute: every factor replaced
    by its absolute value, the scale of an f32 sum over the rows, as ppo_np.grad_scale).  keep: a
    row mask for the tests' controls -- the rows outside it lose their KL term, the divisor stays."""
    _, dmean, dls, fp = kl_heads(pol, z, tflat, lam)
    if keep is not None:
        dmean, dls = dmean * keep[:, None], dls * keep[:, None]
    f = np.abs if absolute else (lambda v: v)
    _, _, W2, _, W3, _, _ = pp.unpack_pol(pol)
    return np.concatenate(pp._net_backward(f(W2), f(W3), f(fp["h1"]), f(fp["h2"]), f(z), f(dmean)) + [f(dls).sum(0)])


def reference(pol, vf, z, a, logp_old, atarg, ret, eps, tflat, lam):
    """ppo_parity.reference of the minibatch with lam x the KL part added to gpol and to M_pol; the
    value net's side is untouched.  r["kl"]: the minibatch-mean KL."""
    r = par.reference(pol, vf, z, a, logp_old, atarg, ret, eps)
    r["gpol_ppo"] = r["gpol"]
    r["gpol"] = r["gpol"] + kl_grad(pol, z, tflat, lam)
    r["M_pol"] = r["M_pol"] + kl_grad(pol, z, tflat, lam, absolute=True)
    r["kl"] = kl_heads(pol, z, tflat, lam)[0]
    return r
