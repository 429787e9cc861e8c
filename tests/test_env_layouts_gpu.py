"""The env mode of the fused rollout kernel -- rdd_rollout (K = 1) and the K-step launch
rdd_rollout_accum / rdd_step_accum (rollout_kernel<.., KS = true>: the step loop, gradient partials
carried in registers over the K env steps, register-resident env state, the 1 / (K n) MSE
normalisation) -- against the f64 oracle in every layout launch_rollout can pick: the helper-pair
kernel (K = 1, f32 student), plain 16-, 32- and 64-env groups, ragged last groups, pairs that own one
group (state resident in registers under K > 1) beside pairs that own two (state re-read).
DistillConfig(grid=2) leaves 8 pairs, so every layout is reached below 1,100 envs
(tests/env_batch.py has the table and each size's residency), and DistillTrainer.last_layout()
confirms the layout each case names.

Coverage split: the K = 1 math in every layout on caller batches is tests/test_caller_batch_gpu.py's;
the env stepping against the physics oracle is tests/test_distill_gpu.py's; the K-step launch and the
env-mode gradients with non-trivial nets (tests/caller_batch.py nets(): biases, two different
observation filters, a non-zero student log-std) are pinned here.

Method: a twin trainer of the same config takes the same K env steps as staged K = 1 launches and
its env state is read before each; those f32 states give the observation rows of every sub-step, on
which the oracle gradient is summed (tests/env_batch.py oracle_sum).  The twin supplies inputs only:
no tolerance comes from it, but the env states after the launch must equal its states bitwise.
Tolerances are the project's (tests/parity.py): per entry 2e-5 x M_e and 1e-5 x max|g| for the f32
student, 1e-4 x M_e and 1e-4 x max|g| for the bf16 student, whose cases first assert that their
inputs leave room for flipped bf16 roundings (env_batch.bf16_room <= 0.5 of both bounds, a condition
on the inputs: its fix is the next state seed).  Every gradient check prints its measured errors
(pytest -s; profiles/env_layout_parity.txt keeps one run's).  tests/test_parity_mutation.py shows on
the CPU that these checks reject a dropped sub-step, a stale resident state, a wrong normalisation,
a swapped observation filter and a wrong log-std gradient.
"""
import numpy as np
import pytest
import torch

from oracle import policy_np as pn
from tests import caller_batch as cb
from tests import env_batch as eb
from tests import parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INSTANCES = [("f32", False), ("f32", True), ("bf16", False), ("bf16", True)]   # student dtype, f32_split
STUDENT_NS = (17, 257, 513, 1000)   # the sizes at which the student acts too (DAgger)


def _trainer(n, K, seed=3, **kw):
    from reacherdistilation_amd.distill import DistillConfig, DistillTrainer
    teacher, student = cb.nets()
    kw.setdefault("grid", cb.GRID)
    kw.setdefault("stagger", False)
    return DistillTrainer(DistillConfig(n_envs=n, seed=seed, accum_steps=K, **kw), device=DEV, teacher=teacher,
                          student=student)


def _pair(n, K, states=None, **kw):
    """The trainer under test and its twin, both at `states` (else their Philox reset)."""
    tr, tw = _trainer(n, K, **kw), _trainer(n, K, **kw)
    if states is not None:
        for t in (tr, tw):
            t.set_env_state(torch.from_numpy(np.array(states)))   # a copy: the shared states are read-only
    return tr, tw


def _staged(tw, K):
    """K env steps of the twin as staged K = 1 launches; its f32 env states before each."""
    sts = []
    for k in range(K):
        sts.append(tw.env_state().cpu().numpy())
        tw.launch(tw.STAGE_ROLLOUT)
        tw.launch(tw.STAGE_REDUCE_ACCUM if k else tw.STAGE_REDUCE)
    return sts


def _tols(bf16):
    return (parity.TOL_ENTRY_BF16, 1e-4) if bf16 else (parity.TOL_ENTRY, parity.TOL_GLOBAL)


def _check_launch(tag, tr, tw, K, loss, layout):
    """One launch of K env steps on tr (the K-step kernel, or rdd_rollout at K = 1) against the
    oracle on the twin's states; returns those states."""
    bf16 = tr.cfg.student_dtype == "bf16"
    c0 = tr.counters()
    sts = _staged(tw, K)
    tr.rollout_accum() if K > 1 else tr.rollout()
    g = tr.grad().cpu().numpy()
    assert tr.last_layout() == tuple(layout) + ("env",), tr.last_layout()
    assert tr.counters() == tw.counters() == (c0[0] + K, 0)
    assert torch.equal(tr.env_state(), tw.env_state()), "env states differ from the staged twin's"
    g64, M, _, _ = eb.oracle_sum(sts, loss, bf16)
    room = ""
    if bf16:   # a condition on the inputs, before the comparison
        r_ent, r_glob = eb.bf16_room(sts, loss, (g64, M))
        room = f" room {r_ent:.3f} / {r_glob:.3f}"
        assert r_ent <= eb.ROOM and r_glob <= eb.ROOM, ("the inputs leave no room: take the next seed", r_ent, r_glob)
    te, tg = _tols(bf16)
    ok, rep = parity.grad_ok(g, g64, M, te, tg)
    print(f"env {tag} n={tr.n_local} K={K} {loss} act={tr.cfg.act_with} {tr.cfg.student_dtype} "
          f"split={tr.cfg.f32_split} layout={tr.last_layout()[:3]}: global {rep['global']:.2e} "
          f"({rep['global'] / tg:.3f} of the bound) entry {rep['entry']:.2e} ({rep['entry'] / te:.3f}) "
          f"in {rep['block']}{room}")
    assert ok, rep
    return sts


def _gradient_cases():
    for sdt, split in INSTANCES:
        for n in (eb.NS if sdt == "f32" else eb.BF16_NS):
            for K in eb.KS:
                for loss in ("mse", "kl"):
                    for act in ("teacher", "student") if n in STUDENT_NS else ("teacher",):
                        yield pytest.param(n, K, loss, sdt, split, act,
                                           id=f"n{n}-K{K}-{loss}-{sdt}-{'split' if split else 'exact'}-{act}")


@pytest.mark.parametrize("n,K,loss,sdt,split,act", list(_gradient_cases()))
def test_env_gradient_matches_oracle_in_every_layout(n, K, loss, sdt, split, act):
    """rdd_rollout (K = 1) and rdd_rollout_accum (K = 3) from CPU-drawn states at every size of the
    layout table: the layout, the gradient against the oracle summed over the sub-steps, the env
    states bitwise against the staged twin, the counters."""
    tr, tw = _pair(n, K, eb.states(n, K), loss=loss, act_with=act, f32_split=split, student_dtype=sdt)
    layout = eb.table_layout(n, K, sdt == "bf16")
    assert layout == eb.expected_layout(n, K, sdt == "bf16")
    _check_launch("table", tr, tw, K, loss, layout)
    tr.close()
    tw.close()


def _fixed_cases():
    for n, gs in sorted(eb.FIXED_GROUPS):
        for sdt, split in INSTANCES:
            if sdt == "f32" or n in eb.BF16_NS:   # the bf16 student runs where its state seed is chosen for
                for loss in ("mse", "kl"):
                    yield pytest.param(n, gs, loss, sdt, split,
                                       id=f"n{n}-gs{gs}-{loss}-{sdt}-{'split' if split else 'exact'}")


@pytest.mark.parametrize("n,gs,loss,sdt,split", list(_fixed_cases()))
def test_ragged_group_on_a_resident_pair(n, gs, loss, sdt, split):
    """K = 3 with a fixed group size: a ragged 64-env group (36 envs) and a ragged 32-env group
    (11 envs) on pairs that own one group, so idle lanes sit beside register-resident envs (the
    bf16 student at 203 only)."""
    K = 3
    layout = eb.FIXED_GROUPS[n, gs]
    assert layout == eb.expected_layout(n, K, sdt == "bf16", gs)
    own = eb.owners(n, gs, layout[1])
    assert all(len(v) <= 1 for v in own.values()) and n % gs           # every pair resident, the last group ragged
    tr, tw = _pair(n, K, eb.states(n), loss=loss, f32_split=split, student_dtype=sdt, group_envs=gs)
    _check_launch(f"fixed gs={gs}", tr, tw, K, loss, layout)
    tr.close()
    tw.close()


def _episode_cases():
    for n in (64, 257, 513, 1000):
        for sdt, split in INSTANCES:
            if sdt == "f32" or n == 1000:
                for loss in ("mse", "kl"):
                    yield pytest.param(n, loss, sdt, split, id=f"n{n}-{loss}-{sdt}-{'split' if split else 'exact'}")


@pytest.mark.parametrize("n,loss,sdt,split", list(_episode_cases()))
def test_episode_end_inside_the_launch(oracle_c, n, loss, sdt, split):
    """K = 7, lockstep episodes: seven launches take the clock to 49; the eighth covers clocks
    49 .. 55, so every env resets at its first sub-step and runs six more from its Philox draw.
    Its gradient against the oracle, its states bitwise against the twin, and the states after
    sub-step 0 bitwise the oracle's draws of episode 1."""
    K, seed = eb.EPISODE_K, eb.EPISODE_SEED
    tr, tw = _pair(n, K, seed=seed, loss=loss, f32_split=split, student_dtype=sdt)
    for _ in range(7):
        tr.rollout_accum()
    for _ in range(49):
        tw.launch(tw.STAGE_ROLLOUT)
        tw.launch(tw.STAGE_REDUCE)
    assert tr.counters() == tw.counters() == (49, 0)
    assert torch.equal(tr.env_state(), tw.env_state())
    sts = _check_launch("episode end", tr, tw, K, loss, eb.table_layout(n, K))
    fresh = oracle_c.philox_reset(n, 0, seed, 1)
    assert np.array_equal(sts[1][:6], fresh[:6])
    assert not np.array_equal(sts[0][:6], oracle_c.philox_reset(n, 0, seed, 0)[:6])
    tr.close()
    tw.close()


@pytest.mark.parametrize("loss", ["mse", "kl"])
@pytest.mark.parametrize("sdt,split", INSTANCES)
def test_part_of_a_group_resets_mid_launch(oracle_c, loss, sdt, split):
    """K = 7, staggered episodes, 1,000 envs in 64-env groups: the third launch covers clocks
    14 .. 20, in which the envs of stagger offsets 31, 30 and 29 (ids 992 .. 999, 960 .. 991 and
    928 .. 959: parts of the last two groups) reset at clocks 18, 19 and 20, between sub-steps.
    Measured: per entry 0.86 - 0.89 of the f32 bound in both f32 instances, at dW1[7, 17].  At these
    clocks the synthetic teacher has every arm spinning (both velocity inputs past the filter's clip
    in every env) and hidden unit 17 is near saturation in most (median 1 - h^2 = 7e-4), where the
    kernels' f32 tanh, exact to an ulp or two of 1, resolves 1 - h^2 to ~1e-4: the oracle with nothing
    but that tanh formed in f32 on the CPU (tests/caller_batch.py tanh_f32) is 0.888 of the bound away
    at the same entry.  The figure belongs to the inputs and the tanh, not to a summation order."""
    n, K, seed = 1000, eb.EPISODE_K, eb.STAGGER_SEED
    tr, tw = _pair(n, K, seed=seed, stagger=True, loss=loss, f32_split=split, student_dtype=sdt)
    for _ in range(2):
        tr.rollout_accum()
    for _ in range(2 * K):
        tw.launch(tw.STAGE_ROLLOUT)
        tw.launch(tw.STAGE_REDUCE)
    assert torch.equal(tr.env_state(), tw.env_state())
    sts = _check_launch("partial reset", tr, tw, K, loss, eb.table_layout(n, K))
    sts.append(tw.env_state().cpu().numpy())
    fresh = oracle_c.philox_reset(n, 0, seed, 1)
    want = {18: (992, 1000), 19: (960, 992), 20: (928, 960)}
    for k in range(K):
        hit = (sts[k + 1][:6] == fresh[:6]).all(0)
        lo, hi = want.get(14 + k, (0, 0))
        assert np.array_equal(np.flatnonzero(hit), np.arange(lo, hi)), (14 + k, np.flatnonzero(hit))
        assert np.array_equal(hit, eb.reset_clock(n, 14 + k, True)[0])
    tr.close()
    tw.close()


@pytest.mark.parametrize("gs", [64, 16])
@pytest.mark.parametrize("sdt,split", [("f32", False), ("f32", True), ("bf16", True)])
def test_each_env_contribution_isolated_over_two_steps(gs, sdt, split):
    """tests/test_distill_gpu.py::test_each_env_contribution_isolated under the K-step launch
    (K = 2, 64 envs, KL): every lane of a 64-env group, and of 16-env groups, owns one env; the
    env is replaced by a fixed env z at sub-step 0 (its later state is the twin's, like every
    env's), and g(batch) - g(batch with env e replaced), both over the two env steps, is held per
    entry to the oracle's within 1e-5 x (M(x_e) + M(z)) + 5e-6 x M(batch) (bf16 student:
    1e-4 x (M(x_e) + M(z)) + 2e-5 x M(batch), under env_batch.isolation_room on the same states),
    M summed over the two sub-steps."""
    n, K, loss = eb.ISO_N, eb.ISO_K, eb.ISO_LOSS
    bf16 = sdt == "bf16"
    st, z = eb.draw_states(n, eb.ISO_SEEDS[sdt, gs]), eb.null_state()
    tr, tw = _pair(n, K, loss=loss, f32_split=split, student_dtype=sdt, group_envs=gs)
    layout = eb.expected_layout(n, K, bf16, gs) + ("env",)

    def run(states):
        for t in (tr, tw):
            t.set_env_state(torch.from_numpy(np.ascontiguousarray(states)))
        sts = _staged(tw, K)
        tr.rollout_accum()
        assert tr.last_layout() == layout, tr.last_layout()
        assert torch.equal(tr.env_state(), tw.env_state())
        return tr.grad().cpu().numpy().astype(np.float64), sts

    g_all, sts_all = run(st)
    ref = eb.oracle_sum(sts_all, loss, bf16)
    ok, rep = parity.grad_ok(g_all, ref[0], ref[1], *_tols(bf16))
    assert ok, rep
    em_all = eb.bf16_emulated_grad(sts_all, loss) if bf16 else None
    worst = room = 0.0
    for e in range(n):
        se = st.copy()
        se[:, e] = z
        g_e, sts_e = run(se)
        keep = np.arange(n) != e
        assert all(np.array_equal(x[:, keep], y[:, keep]) for x, y in zip(sts_all, sts_e))
        if bf16:   # a condition on the inputs, before the comparison
            room = max(room, eb.isolation_room(sts_all, sts_e, e, ref, em_all))
            assert room <= eb.ROOM, ("the inputs leave no room: take the next seed", e, room)
        r, k = eb.isolation_ratio(g_all - g_e, sts_all, sts_e, e, bf16, ref)
        worst = max(worst, r)
        assert r <= 1.0, (e, k, r)
    print(f"per-env K={K} n={n} gs={gs} {sdt} split={split} {loss}: worst error / bound {worst:.3f}"
          + (f" room {room:.3f}" if bf16 else ""))
    tr.close()
    tw.close()


@pytest.mark.parametrize("n", [203, 1000])
@pytest.mark.parametrize("loss", ["mse", "kl"])
def test_step_accum_end_to_end(n, loss):
    """rdd_step_accum (f32 split, K = 3): counters (K, 1); the metrics slot [sum reward, loss,
    sum (mu_s - mu_t)^2, K n] with the oracle's loss and squared error (rel 1e-3); the gradient; the
    TF1 Adam step of the oracle gradient where |g| > 1e-3 max|g| (atol 1e-6)."""
    K, lr = 3, 1e-3
    tr, tw = _pair(n, K, eb.states(n), loss=loss, lr=lr)
    p0 = tr.student_params().cpu().numpy()
    sts = _staged(tw, K)
    tr.step_accum()
    assert tr.last_layout() == eb.table_layout(n, K) + ("env",), tr.last_layout()
    assert tr.counters() == (K, 1) and tr.steps == K
    assert torch.equal(tr.env_state(), tw.env_state())
    g64, M, L, sq = eb.oracle_sum(sts, loss, sp=p0)
    ok, rep = parity.grad_ok(tr.grad().cpu().numpy(), g64, M)
    assert ok, rep
    m = tr.metrics(1)[0]
    assert m[3] == K * n and m[0] < 0.0
    assert m[1] == pytest.approx(L, rel=1e-3) and m[2] == pytest.approx(sq, rel=1e-3)
    ref = p0.copy()
    pn.AdamTF1(pn.P_TOT, lr=lr).step(ref, g64.astype(np.float32))
    p1 = tr.student_params().cpu().numpy()
    strong = np.abs(g64) > 1e-3 * np.abs(g64).max()
    print(f"step_accum n={n} {loss}: loss {m[1]:.6g} vs {L:.6g}, sq {m[2]:.6g} vs {sq:.6g}, {rep}, "
          f"max Adam dev {np.abs(p1 - ref)[strong].max():.2e}")
    np.testing.assert_allclose(p1[strong], ref[strong], atol=1e-6, rtol=0)
    assert np.abs(p1 - p0).max() > 0.5 * lr
    tr.close()
    tw.close()
