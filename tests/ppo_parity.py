"""Shared parity check of the PPO trainer's minibatch gradient (csrc/ppo.hip) against
oracle/ppo_np.py (test infrastructure: imports oracle/, never the product path).

The trainer's gradient is [pol | vf], and with returns of order -30 the value net's part is a
few hundred times the policy's: a relative L2 norm of the concatenation cannot see the policy
gradient (a policy gradient 5 % too large moves it by 2e-4).  So each net is held to its own
scale, as tests/parity.py holds the distillation gradient:

* global:    |g - g64| <= TOL_GLOBAL x max|g64 of that net|;
* per entry: |g - g64|_e <= TOL_ENTRY x M_e + extra_e, with M_e = sum over the minibatch's rows
  of |that row's contribution to entry e| (ppo_np.grad_scale: the natural scale of an f32 sum, so
  a bias, a log-std or a dW2 row owned by one lane group is held to its own magnitude);
* where M_e + extra_e = 0 the entry is exactly 0.

extra_e covers the rows that f32 may put on either side of the clip range: those with
| |ratio - 1| - eps | < EITHER_WAY (tests/test_ppo_batch_gpu.py sets the same rows aside for
clipfrac).  Such a row's whole policy contribution may be present or absent, so extra_e is the sum
over them of |their contribution, taken as live, to e|.  Every test asserts that they are at most
MAX_EITHER_SHARE of the minibatch, so extra cannot hide a lost tile.

Tolerances: tests/parity.py's, measured there for the same 2 x 64 nets on the exact f32 MFMA.
The rule: every GPU case is run once and its worst errors written to
profiles/ppo_parity_errors.txt; a tolerance stays while the worst measured error is at most a
quarter of it, else it becomes 4 x the worst measured error rounded up to one significant figure
(the margin covers other seeds and shapes), and never more than TOL_CAP: beyond it the check
no longer rejects one lost row of 33,280, so a need for more means the kernel is wrong.  (The
weakest mutations of tests/test_ppo_parity_mutation.py measure less than the cap: four output
rows of one tile's dV2 6e-5 at 33,280 rows, the policy part of one lost row 8e-5 at 16,065; they
are judged with the tolerances in force, so raising TOL_ENTRY past them shows there.)
Measured on MI355X (profiles/ppo_parity_errors.txt, 23 cases of 21 .. 33,280 rows, ratios at 1
and across the clip range): global <= 2.1e-7 (policy) / 1.4e-7 (value), per entry <= 7.9e-7 (policy,
W3 at 33 rows) / 3.3e-7 (value): under a quarter of both tolerances, which therefore stay.
"""
import numpy as np

from oracle import policy_np as pn
from oracle import ppo_np as pp

TOL_GLOBAL = 1e-5          # x max|g64| of the net
TOL_ENTRY = 2e-5           # x M_e
TOL_CAP = 1e-4             # no tolerance above it: one lost row of 33,280 measures 1.4e-4
EITHER_WAY = 1e-5          # | |ratio - 1| - eps | below it: f32 may classify the row either way
MAX_EITHER_SHARE = 5e-4    # of the minibatch's rows


def _blocks(names, sizes):
    out, o = [], 0
    for name, n in zip(names, sizes):
        out.append((name, o, o + n))
        o += n
    return tuple(out)


_H, _O = pp.HID, pp.OBD
BLOCKS_POL = _blocks(("W1", "b1", "W2", "b2", "W3", "b3", "logstd"), (_O * _H, _H, _H * _H, _H, _H * 2, 2, 2))
BLOCKS_VF = _blocks(("V1", "c1", "V2", "c2", "V3", "c3"), (_O * _H, _H, _H * _H, _H, _H, 1))
assert BLOCKS_POL[-1][2] == pp.P_POL and BLOCKS_VF[-1][2] == pp.P_VF


def block(name):
    """(first, end) of a named block within its own net's vector."""
    return next((a, b) for n, a, b in BLOCKS_POL + BLOCKS_VF if n == name)


def grad_report(g_net, g64_net, M_net, extra=0):
    """Errors of one net's kernel gradient against the oracle's: global (x max|g64|), per entry
    (x M_e after extra_e is taken off; entries with M_e + extra_e = 0 must be exactly 0), and
    the worst entry's block."""
    g = np.asarray(g_net, np.float64)
    blocks = {pp.P_POL: BLOCKS_POL, pp.P_VF: BLOCKS_VF}[g.size]
    extra = np.broadcast_to(np.asarray(extra, np.float64), g.shape)
    d = np.abs(g - g64_net)
    glob = float(d.max() / max(np.abs(g64_net).max(), 1e-300))
    zero = M_net == 0
    ent = np.where(zero, np.where(d > extra, np.inf, 0.0), np.maximum(d - extra, 0.0) / np.where(zero, 1.0, M_net))
    k = int(np.argmax(ent))
    blk = next(name for name, a, b in blocks if a <= k < b)
    return {"global": glob, "entry": float(ent[k]), "worst_entry": k, "block": blk}


def grad_ok(g_net, g64_net, M_net, extra=0, tol_entry=None, tol_global=None):
    r = grad_report(g_net, g64_net, M_net, extra)
    te = TOL_ENTRY if tol_entry is None else tol_entry
    tg = TOL_GLOBAL if tol_global is None else tol_global
    return r["global"] <= tg and r["entry"] <= te, r


def concat_rel(gpol, gvf, want_pol, want_vf):
    """The relative L2 error of [gpol | gvf]: what the trainer's gradient tests compared alone."""
    g, want = np.concatenate([gpol, gvf]), np.concatenate([want_pol, want_vf])
    return float(np.linalg.norm(g - want) / np.linalg.norm(want))


def reference(pol, vf, z, a, logp_old, atarg, ret, eps):
    """The oracle's side of one minibatch: loss_and_grads' dict plus M_pol, M_vf, live, the
    masks of the rows outside the clip range (above / below), dead, and `either` (rows f32 may
    classify either way) with extra_pol, their |contribution as live rows| summed."""
    args = (pol, vf, z, a, logp_old, atarg, ret, eps)
    r = pp.loss_and_grads(*args)
    r["M_pol"], r["M_vf"], r["live"] = pp.grad_scale(*args)
    ratio = r["ratio"]
    r["above"], r["below"] = ratio > 1 + eps, ratio < 1 - eps
    r["dead"] = ~r["live"]
    r["either"] = np.abs(np.abs(ratio - 1) - eps) < EITHER_WAY
    r["extra_pol"] = np.zeros(pp.P_POL)
    for i in np.flatnonzero(r["either"]):
        r["extra_pol"] += np.abs(pp.row_contributions(*args, rows=[i], as_live=True)[0])
    r["rows"], r["eps"] = z.shape[0], eps
    return r


def quadrants(r, atarg):
    """Share of the rows in each quadrant: ratio above / below the clip range x advantage sign.
    (above, A > 0) and (below, A < 0) are the dead rows; the other two are live outside it."""
    pos = atarg > 0
    return {"above+": float((r["above"] & pos).mean()), "above-": float((r["above"] & ~pos).mean()),
            "below+": float((r["below"] & pos).mean()), "below-": float((r["below"] & ~pos).mean())}


def check_grad(g, r, label):
    """Assert both nets of a kernel gradient g = [pol | vf] against reference() r, after printing
    the figures (profiles/ppo_parity_errors.txt is made of these lines)."""
    g = np.asarray(g, np.float64)
    n_either = int(r["either"].sum())
    assert n_either <= MAX_EITHER_SHARE * r["rows"], (label, n_either, r["rows"])
    okp, rp = grad_ok(g[:pp.P_POL], r["gpol"], r["M_pol"], r["extra_pol"])
    okv, rv = grad_ok(g[pp.P_POL:], r["gvf"], r["M_vf"])
    print(f"ppo_parity {label}: rows {r['rows']} dead {int(r['dead'].sum())} either {n_either} | "
          f"pol global {rp['global']:.2e} entry {rp['entry']:.2e} ({rp['block']}) | "
          f"vf global {rv['global']:.2e} entry {rv['entry']:.2e} ({rv['block']})")
    assert okp, (label, "policy", rp)
    assert okv, (label, "value", rv)
    return rp, rv


# ---------------------------------------------------------------- the clip tests' perturbation
def perturbed(pol, vf, factor=1.0, seed=5):
    """The clip tests' step off the rollout policy, from a fixed RandomState: W3 += U(-.02, .02),
    b3 += (0.12, -0.10), logstd += (0.05, -0.05), value net += U(-.01, .01), all times `factor`;
    float32 in, float32 out (what set_policy / set_value are given)."""
    rs = np.random.RandomState(seed)
    p, v = np.array(pol, np.float64), np.array(vf, np.float64)
    w3 = block("W3")
    p[w3[0]:w3[1]] += factor * rs.uniform(-.02, .02, w3[1] - w3[0])
    p[slice(*block("b3"))] += factor * np.array([0.12, -0.10])
    p[slice(*block("logstd"))] += factor * np.array([0.05, -0.05])
    v += factor * rs.uniform(-.01, .01, v.size)
    return p.astype(np.float32), v.astype(np.float32)


# ---------------------------------------------------------------- a synthetic actor batch (host tests)
def baselines_nets(seed=0):
    """MlpPolicy's initialisation: normc(1.0) hidden kernels, normc(0.01) mean head, normc(1.0)
    value head, zero biases and log-std."""
    rs = np.random.RandomState(seed)
    z = np.zeros
    pol = np.concatenate([pn.normc(rs, (_O, _H), 1.0).ravel(), z(_H), pn.normc(rs, (_H, _H), 1.0).ravel(), z(_H),
                          pn.normc(rs, (_H, 2), 0.01).ravel(), z(2), z(2)])
    vf = np.concatenate([pn.normc(rs, (_O, _H), 1.0).ravel(), z(_H), pn.normc(rs, (_H, _H), 1.0).ravel(), z(_H),
                         pn.normc(rs, (_H, 1), 1.0).ravel(), z(1)])
    return pol.astype(np.float32), vf.astype(np.float32)


def synthetic_batch(n, T, seed=0):
    """An actor batch of n envs x T steps without a GPU: baselines-initialised nets, z clipped
    standard normal, actions drawn from the policy, rewards -U(0.05, 0.3) - |a|^2 pushed through
    ppo_np.gae (episodes of 50 steps) and standardize.  logp_old is the rollout policy's own."""
    pol, vf = baselines_nets(seed)
    rs = np.random.RandomState(seed + 1)
    S = n * T
    z = np.clip(rs.standard_normal((S, _O)), -5, 5)
    fp = pp.pol_forward(pol, z)
    a = (fp["mean"] + np.exp(fp["logstd"]) * rs.standard_normal((S, 2))).astype(np.float32).astype(np.float64)
    rew = -rs.uniform(0.05, 0.3, S) - (a ** 2).sum(1)
    new = np.zeros((T, n))
    new[::50] = 1
    vpred = pp.vf_forward(vf, z)["v"]
    nextv = pp.vf_forward(vf, np.clip(rs.standard_normal((n, _O)), -5, 5))["v"]
    adv, ret = pp.gae(rew.reshape(T, n), vpred.reshape(T, n), new, nextv)
    return dict(pol=pol, vf=vf, z=z, a=a, lpo=pp.logp(fp["mean"], fp["logstd"], a),
                atarg=pp.standardize(adv.reshape(-1)), ret=ret.reshape(-1))
