"""ORACLE (test infrastructure only) -- numpy restatement of the reference teacher's PPO
training (reference teacher.py:23-37: baselines ppo1 ``pposgd_simple.learn`` with
MlpPolicy(hid_size=64, num_hid_layers=2), timesteps_per_actorbatch 2048, clip 0.2,
entcoeff 0, optim_epochs 10, optim_stepsize 3e-4, optim_batchsize 64, gamma 0.99,
lam 0.95, schedule 'linear').

baselines (commit 3900f2a, not in /root/reference; restated from its published algorithm):
  * MlpPolicy: obfilter = RunningMeanStd(sum, sumsq, count; count starts at 1e-2; std =
    sqrt(max(sumsq/count - mean^2, 1e-2))); obz = clip((ob - mean)/std, -5, 5); value net
    vf: 2 x 64 tanh + dense 1; policy pol: 2 x 64 tanh + dense 2 (mean) + free logstd[2].
  * add_vtarg_and_adv: GAE(lambda) with `new` flags (first step of an episode) and the
    bootstrap value of the observation after the segment (0 if it starts an episode).
  * loss: ratio = exp(logp - logp_old); pol_surr = -mean(min(ratio A, clip(ratio, 1 - e,
    1 + e) A)), e = clip_param * lrmult; vf_loss = mean((V - ret)^2); A standardized over
    the actor batch; entcoeff 0.  TF gradient conventions: min() passes to its first
    argument on ties; clip passes inside the closed interval.
  * MpiAdam (epsilon 1e-5, learn()'s adam_epsilon default): the TF1 form (a = lr sqrt(1 -
    b2^t) / (1 - b1^t), eps outside the sqrt) on the
    concatenated trainable vector [pol | vf] with stepsize optim_stepsize * lrmult,
    lrmult = max(1 - timesteps_so_far / max_timesteps, 0).
Parameter vectors here: pol = the 5,060-float MlpPolicy layout of policy_np (W1 b1 W2 b2
W3 b3 logstd); vf = V1[11][64] c1 V2[64][64] c2 V3[64][1] c3 (4,993 floats).

Parity status: UNPINNED beyond the formulas (TensorFlow/baselines absent; no reference test
covers PPO); checked by finite differences in tests/test_ppo_oracle.py.  The minibatch
shuffles (mt19937_64, shuffles) are the trainer's own, not baselines': pinned to the C++
standard's check value and to a libstdc++ table (tests/golden/ppo_shuffles.json).
"""
from __future__ import annotations

import numpy as np

OBD, HID = 11, 64
P_POL = OBD * HID + HID + HID * HID + HID + HID * 2 + 2 + 2     # 5060
P_VF = OBD * HID + HID + HID * HID + HID + HID + 1              # 4993
LOG2PI = np.log(2 * np.pi)


def unpack_pol(p):
    p = np.asarray(p, np.float64)
    o = 0
    out = []
    for shp in ((OBD, HID), (HID,), (HID, HID), (HID,), (HID, 2), (2,), (2,)):
        n = int(np.prod(shp))
        out.append(p[o:o + n].reshape(shp))
        o += n
    return out


def unpack_vf(p):
    p = np.asarray(p, np.float64)
    o = 0
    out = []
    for shp in ((OBD, HID), (HID,), (HID, HID), (HID,), (HID, 1), (1,)):
        n = int(np.prod(shp))
        out.append(p[o:o + n].reshape(shp))
        o += n
    return out


class RunningMeanStd:
    """baselines.common.mpi_running_mean_std.RunningMeanStd (float64 sums)."""

    def __init__(self, shape=(OBD,), epsilon=1e-2):
        self.sum = np.zeros(shape)
        self.sumsq = np.full(shape, epsilon)
        self.count = epsilon

    @property
    def mean(self):
        return self.sum / self.count

    @property
    def std(self):
        return np.sqrt(np.maximum(self.sumsq / self.count - np.square(self.mean), 1e-2))

    def update(self, x):
        x = np.asarray(x, np.float64).reshape(-1, self.sum.shape[0])
        self.sum += x.sum(0)
        self.sumsq += np.square(x).sum(0)
        self.count += x.shape[0]


def obz(ob, mean, std):
    return np.clip((np.asarray(ob, np.float64) - mean) / std, -5.0, 5.0)


def pol_forward(p, z):
    W1, b1, W2, b2, W3, b3, ls = unpack_pol(p)
    h1 = np.tanh(z @ W1 + b1)
    h2 = np.tanh(h1 @ W2 + b2)
    return dict(h1=h1, h2=h2, mean=h2 @ W3 + b3, logstd=ls)


def vf_forward(p, z):
    V1, c1, V2, c2, V3, c3 = unpack_vf(p)
    g1 = np.tanh(z @ V1 + c1)
    g2 = np.tanh(g1 @ V2 + c2)
    return dict(g1=g1, g2=g2, v=(g2 @ V3 + c3)[:, 0])


def logp(mean, logstd, a):
    std = np.exp(logstd)
    return -0.5 * (((a - mean) / std) ** 2).sum(1) - logstd.sum() - 0.5 * 2 * LOG2PI


def gae(rew, vpred, new, nextvpred, gamma=0.99, lam=0.95):
    """rew, vpred, new: [T, N]; nextvpred: [N] (already 0 where the next ob starts an
    episode).  Returns (adv, tdlamret) [T, N]."""
    T = rew.shape[0]
    new_ext = np.concatenate([new, np.zeros((1,) + new.shape[1:])], 0)
    v_ext = np.concatenate([vpred, nextvpred[None]], 0)
    adv = np.zeros_like(rew, dtype=np.float64)
    last = np.zeros(rew.shape[1:])
    for t in range(T - 1, -1, -1):
        nonterm = 1.0 - new_ext[t + 1]
        delta = rew[t] + gamma * v_ext[t + 1] * nonterm - vpred[t]
        last = delta + gamma * lam * nonterm * last
        adv[t] = last
    return adv, adv + vpred


def standardize(adv):
    return (adv - adv.mean()) / adv.std()


def _rows(pol, vf, z, a, logp_old, atarg, ret, clip_eps):
    """Per-row terms of the minibatch loss: forwards, ratio, the min / clip branch masks (TF's
    conventions) and the head derivatives dlp = d loss / d logp, dv = d loss / d v, both with
    the divisor n."""
    n = z.shape[0]
    fp, fv = pol_forward(pol, z), vf_forward(vf, z)
    lp = logp(fp["mean"], fp["logstd"], a)
    ratio = np.exp(lp - logp_old)
    s1 = ratio * atarg
    rc = np.clip(ratio, 1.0 - clip_eps, 1.0 + clip_eps)
    s2 = rc * atarg
    # d(-min)/dratio with TF's conventions
    take1 = s1 <= s2
    inside = (ratio >= 1.0 - clip_eps) & (ratio <= 1.0 + clip_eps)
    dr = np.where(take1, -atarg, np.where(inside, -atarg, 0.0)) / n
    std = np.exp(fp["logstd"])
    return dict(fp=fp, fv=fv, ratio=ratio, s1=s1, s2=s2, live=take1 | inside, dlp=dr * ratio,
                x=(a - fp["mean"]) / std, std=std, dv=2.0 * (fv["v"] - ret)[:, None] / n)


def _net_backward(W2, W3, h1, h2, z, dtop):
    """Weight / bias gradients of a 2 x 64 tanh net with a dense head from d loss / d head
    output dtop [n, k], in layout order W1 b1 W2 b2 W3 b3."""
    g3 = h2.T @ dtop
    gb3 = dtop.sum(0)
    d2 = (dtop @ W3.T) * (1 - h2 ** 2)
    g2 = h1.T @ d2
    gb2 = d2.sum(0)
    d1 = (d2 @ W2.T) * (1 - h1 ** 2)
    g1 = z.T @ d1
    gb1 = d1.sum(0)
    return [g1.ravel(), gb1, g2.ravel(), gb2, g3.ravel(), gb3]


def _grads(pol, vf, z, t, rows=slice(None), absolute=False, dlp=None):
    """(gpol, gvf) from the per-row terms t of _rows over `rows`; absolute: every factor replaced
    by its absolute value (1 - h^2 is unchanged by it); dlp: overrides t["dlp"]."""
    f = np.abs if absolute else (lambda v: v)
    dlp = (t["dlp"] if dlp is None else dlp)[rows]
    x = t["x"][rows]
    dmean = f(dlp)[:, None] * f(x) / t["std"]
    dls = (f(dlp)[:, None] * f(x ** 2 - 1.0)).sum(0)
    _, _, W2, _, W3, _, _ = unpack_pol(pol)
    fp, fv = t["fp"], t["fv"]
    gpol = np.concatenate(_net_backward(f(W2), f(W3), f(fp["h1"][rows]), f(fp["h2"][rows]), f(z[rows]), dmean) + [dls])
    _, _, V2, _, V3, _ = unpack_vf(vf)
    gvf = np.concatenate(_net_backward(f(V2), f(V3), f(fv["g1"][rows]), f(fv["g2"][rows]), f(z[rows]), f(t["dv"][rows])))
    return gpol, gvf


def loss_and_grads(pol, vf, z, a, logp_old, atarg, ret, clip_eps):
    """Minibatch loss terms and the gradient of pol_surr + vf_loss w.r.t. [pol | vf]."""
    t = _rows(pol, vf, z, a, logp_old, atarg, ret, clip_eps)
    pol_surr = -np.minimum(t["s1"], t["s2"]).mean()
    vf_loss = np.square(t["fv"]["v"] - ret).mean()
    gpol, gvf = _grads(pol, vf, z, t)
    ent = (t["fp"]["logstd"] + 0.5 * np.log(2 * np.pi * np.e)).sum()
    kl = None
    return dict(pol_surr=pol_surr, vf_loss=vf_loss, ent=ent, gpol=gpol, gvf=gvf, ratio=t["ratio"], kl=kl)


def grad_scale(pol, vf, z, a, logp_old, atarg, ret, clip_eps):
    """(M_pol, M_vf, live): M_e = sum over rows of |that row's contribution to gradient entry e|
    (an upper bound of it: loss_and_grads' backward with every factor replaced by its absolute
    value; the rows whose surrogate gradient is zero stay zero; the log-std entries are
    sum |dlp| |x^2 - 1|), the natural scale of an f32 sum over the rows.  live: the rows the
    policy gradient takes, take1 | inside."""
    t = _rows(pol, vf, z, a, logp_old, atarg, ret, clip_eps)
    M_pol, M_vf = _grads(pol, vf, z, t, absolute=True)
    return M_pol, M_vf, t["live"]


def row_contributions(pol, vf, z, a, logp_old, atarg, ret, clip_eps, rows, as_live=False):
    """(gpol, gvf) restricted to `rows` of the minibatch, the divisor n kept: over all rows it is
    loss_and_grads' gradient.  as_live: the rows' policy contribution as if none were dead."""
    t = _rows(pol, vf, z, a, logp_old, atarg, ret, clip_eps)
    dlp = -atarg / z.shape[0] * t["ratio"] if as_live else None
    return _grads(pol, vf, z, t, rows=np.asarray(rows, np.int64), dlp=dlp)


def mt19937_64(seed):
    """std::mt19937_64 (Matsumoto & Nishimura's 64-bit Mersenne Twister with the standard
    constants) as a generator of its outputs."""
    M64 = (1 << 64) - 1
    NN, MM, UM, LM = 312, 156, 0xFFFFFFFF80000000, 0x7FFFFFFF
    mt = [seed & M64]
    for i in range(1, NN):
        mt.append((6364136223846793005 * (mt[-1] ^ (mt[-1] >> 62)) + i) & M64)
    while True:
        for i in range(NN):
            x = (mt[i] & UM) | (mt[(i + 1) % NN] & LM)
            mt[i] = mt[(i + MM) % NN] ^ (x >> 1) ^ (0xB5026F5AA96619E9 if x & 1 else 0)
        for x in mt:
            x ^= (x >> 29) & 0x5555555555555555
            x ^= (x << 17) & 0x71D67FFFEDA60000
            x ^= (x << 37) & 0xFFF7EEE000000000
            yield x ^ (x >> 43)


def shuffles(seed, iteration, S, epochs):
    """The trainer's minibatch shuffles of one iteration, [epochs, S]: one mt19937_64 seeded
    with seed * 0x9E3779B97F4A7C15 + iteration + 1 (mod 2^64) runs on across the epochs; each
    epoch is a Fisher-Yates shuffle of the identity from the top (j = rng() % (i + 1))."""
    rng = mt19937_64((seed * 0x9E3779B97F4A7C15 + iteration + 1) & ((1 << 64) - 1))
    out = np.zeros((epochs, S), np.int64)
    for e in range(epochs):
        p = list(range(S))
        for i in range(S - 1, 0, -1):
            j = next(rng) % (i + 1)
            p[i], p[j] = p[j], p[i]
        out[e] = p
    return out


def adam(n):
    """MpiAdam as learn() builds it: policy_np.AdamTF1 with epsilon 1e-5 over [pol | vf]; the
    caller sets ``lr = optim_stepsize * lrmult`` (a float32) before each step."""
    from oracle.policy_np import AdamTF1
    return AdamTF1(n, eps=1e-5)


def total_loss(pol, vf, z, a, logp_old, atarg, ret, clip_eps):
    r = loss_and_grads(pol, vf, z, a, logp_old, atarg, ret, clip_eps)
    return r["pol_surr"] + r["vf_loss"]
