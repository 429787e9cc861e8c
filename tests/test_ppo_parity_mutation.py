"""CPU mutation test of the PPO gradient check (tests/ppo_parity.py): the per-net bound rejects
each way minibatch_kernel's clipped surrogate can be subtly wrong, and the relative L2 norm of
[gpol | gvf] that the trainer's gradient tests compared alone does not.

The batches are ppo_parity.synthetic_batch at the GPU tests' row counts, moved off the rollout
policy by ppo_parity.perturbed, so about 12 % of the rows are dead and every quadrant (ratio above
/ below the range x advantage sign) is populated.  The "kernel result" is the oracle's own
gradient carried through f32, a stand-in for a correct kernel at f32 rounding.  Mutations:
  * gpol x 1.01; dlogstd x 0.98;
  * the clip ignored (every row live);
  * the min ignored (every row outside the range dead);
  * one live row lost (16,065 and 33,280 rows: one row is 3e-5 of the batch);
  * one 32-row tile losing output rows 12-15 of every 16 x 16 block of its dW2 (a lost SrcC
    load in an MFMA's last row group), in either net;
  * clip_eps left at 0.2 when lrmult = 0.5.
"""
import numpy as np
import pytest

from oracle import ppo_np as pp
from tests import ppo_parity as par

SHAPES = [(33, 1), (255, 63), (256, 64), (1040, 32)]           # 33, 16,065, 16,384, 33,280 rows
_CACHE = {}


def _case(n, T, eps=0.2):
    """(batch, perturbed nets' reference r, the oracle's arguments); computed once per shape."""
    if (n, T, eps) not in _CACHE:
        b = par.synthetic_batch(n, T)
        pol1, vf1 = par.perturbed(b["pol"], b["vf"])
        args = (pol1, vf1, b["z"], b["a"], b["lpo"], b["atarg"], b["ret"], eps)
        _CACHE[(n, T, eps)] = (b, par.reference(*args), args)
    return _CACHE[(n, T, eps)]


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _new_ok(r, gpol, gvf):
    """ppo_parity's verdict on a "kernel" gradient (gpol, gvf), carried through f32."""
    okp, rp = par.grad_ok(_f32(gpol), r["gpol"], r["M_pol"], r["extra_pol"])
    okv, rv = par.grad_ok(_f32(gvf), r["gvf"], r["M_vf"])
    return okp and okv, (rp, rv)


def _old_ok(r, gpol, gvf, tol=1e-3):
    return par.concat_rel(_f32(gpol), _f32(gvf), r["gpol"], r["gvf"]) < tol


@pytest.mark.parametrize("n,T", SHAPES)
def test_clean_gradient_passes_and_each_mutation_is_rejected(n, T):
    b, r, args = _case(n, T)
    S = n * T
    assert r["either"].sum() <= par.MAX_EITHER_SHARE * S
    q = par.quadrants(r, b["atarg"])
    if S >= 100:
        assert min(q.values()) >= 0.02, q
    assert r["dead"].any() and (r["live"] & (r["above"] | r["below"])).any()
    ok, rep = _new_ok(r, r["gpol"], r["gvf"])
    assert ok, rep
    assert max(rep[0]["entry"], rep[1]["entry"]) < 1e-6 and _old_ok(r, r["gpol"], r["gvf"])
    worst = {}

    def rejected(what, gpol, gvf=None):
        ok, rep = _new_ok(r, gpol, r["gvf"] if gvf is None else gvf)
        assert not ok, (what, rep)
        worst[what] = max(rep[0]["entry"], rep[1]["entry"])

    # the policy gradient 1 % too large; the log-std gradient 2 % too small
    rejected("gpol x 1.01", 1.01 * r["gpol"])
    ls = r["gpol"].copy()
    ls[slice(*par.block("logstd"))] *= 0.98
    rejected("dlogstd x 0.98", ls)
    # the clip ignored: every row live
    free, _ = pp.row_contributions(*args, rows=np.arange(S), as_live=True)
    rejected("clip ignored", free)
    # the min ignored: every row outside the range dead, also those the min keeps live
    kept = np.flatnonzero(r["live"] & (r["above"] | r["below"]))
    rejected("min ignored", r["gpol"] - pp.row_contributions(*args, rows=kept)[0])
    # one 32-row tile (the last whole one) loses output rows 12-15 of its dW2 blocks, per net
    t0 = (S // 32 - 1) * 32
    cp, cv = pp.row_contributions(*args, rows=np.arange(t0, t0 + 32))
    lost = np.zeros(64 * 64, bool)
    lost.reshape(64, 64)[np.arange(64) % 16 >= 12] = True
    for net, c, name in ((0, cp, "W2"), (1, cv, "V2")):
        a0, a1 = par.block(name)
        d = np.zeros_like(c)
        d[a0:a1] = np.where(lost, c[a0:a1], 0.0)
        rejected("tile rows 12-15 of d" + name, r["gpol"] - (d if net == 0 else 0), r["gvf"] - (d if net == 1 else 0))
    # one live row lost.  A row's share of the gradient goes with its advantage and its value
    # error, and a row with neither is invisible to any check, so the rows are the first, middle
    # and last of those with |A| >= 1 (A is standardised: one standard deviation) and a value
    # error of at least its RMS.  Measured over 60 random live rows of 33,280: median per-entry
    # error 7e-5, 10 % of them under 1.3e-5; over rows with |A| >= 1: at least 4e-5.
    verr = np.abs(pp.vf_forward(args[1], b["z"])["v"] - b["ret"])
    cand = np.flatnonzero(r["live"] & (np.abs(b["atarg"]) >= 1) & (verr >= np.sqrt(np.mean(verr ** 2))))
    for i in (cand[0], cand[len(cand) // 2], cand[-1]):
        cp, cv = pp.row_contributions(*args, rows=[i])
        rejected(f"row {i} lost", r["gpol"] - cp, r["gvf"] - cv)
        rejected(f"row {i} lost, policy", r["gpol"] - cp)
        rejected(f"row {i} lost, value", r["gpol"], r["gvf"] - cv)
        if S >= 16000:                                   # the concatenated norm sees none of them
            assert _old_ok(r, r["gpol"] - cp, r["gvf"] - cv)
    print(f"rows {S}: per-entry error of the clean result {max(rep[0]['entry'], rep[1]['entry']):.1e}, of the mutations",
          {k: f"{v:.1e}" for k, v in worst.items()})
    if S >= 16000:
        assert _old_ok(r, 1.01 * r["gpol"], r["gvf"]) and _old_ok(r, ls, r["gvf"])
        assert _old_ok(r, 1.05 * r["gpol"], r["gvf"])    # even 5 % passes the old check


@pytest.mark.parametrize("n,T", [(64, 8), (256, 64)])
def test_clip_eps_left_at_its_initial_value_is_rejected(n, T):
    """lrmult = 0.5: clip_eps = 0.1.  A kernel that kept 0.2 classifies other rows dead."""
    b, r, args = _case(n, T, eps=0.1)
    stale = pp.loss_and_grads(*args[:-1], 0.2)
    assert not np.array_equal(pp.grad_scale(*args[:-1], 0.2)[2], r["live"])
    assert _new_ok(r, r["gpol"], r["gvf"])[0]
    ok, rep = _new_ok(r, stale["gpol"], stale["gvf"])
    assert not ok and rep[0]["entry"] > par.TOL_CAP, rep


def test_one_row_outside_the_range_hides_an_ignored_clip_from_the_concatenated_norm():
    """The existing clipped-branch test's situation: one row of 16,384 outside the range and dead
    (the others at ratio 1).  "Clip ignored" passes its 2e-3 on the concatenated norm; the
    per-net bound rejects it."""
    b = par.synthetic_batch(256, 64)
    lpo = b["lpo"].copy()
    i = int(np.flatnonzero(b["atarg"] > 0.5)[0])
    lpo[i] -= np.log(1.3)                                 # ratio 1.3 with a positive advantage: dead
    args = (b["pol"], b["vf"], b["z"], b["a"], lpo, b["atarg"], b["ret"], 0.2)
    r = par.reference(*args)
    assert r["dead"].sum() == 1 and r["dead"][i] and (r["above"] | r["below"]).sum() == 1
    free, _ = pp.row_contributions(*args, rows=np.arange(lpo.size), as_live=True)
    assert _new_ok(r, r["gpol"], r["gvf"])[0]
    assert _old_ok(r, free, r["gvf"], tol=2e-3)
    ok, rep = _new_ok(r, free, r["gvf"])
    assert not ok, rep


def test_value_net_dominates_the_concatenated_norm():
    """Why the concatenated norm is blind: at the headline shape the value net's gradient is two
    orders of magnitude above the policy's, so the whole policy backward lost is a relative error
    of a few 1e-3."""
    _, r, _ = _case(256, 64)
    ratio = np.linalg.norm(r["gvf"]) / np.linalg.norm(r["gpol"])
    assert ratio > 100, ratio
    assert par.concat_rel(0 * r["gpol"], r["gvf"], r["gpol"], r["gvf"]) < 1e-2
    assert not _new_ok(r, 0 * r["gpol"], r["gvf"])[0]
