"""rdd_config.teacher_tiles (include/reacher_distill.h): the f32-split student's K = 1 teacher-mode
kernel with the teacher forward of some of a group's 16-env tiles run by the pair's consumer wave
(rollout_kernel's TCM: 0b0010, 0b1010, 0b1110; 0 = all on the producer).

A tile is masked only where a group has at least two tiles, so the cases fix the group size (64, and
32 at one size) on one workgroup (grid = 1: four pairs):
  n = 32   two tiles                         n = 64   four tiles
  n = 33   the third tile has one row        n = 81   a second, ragged group (17 envs) on pair 1
  n = 50   the last, ragged tile is tile 3, a consumer-side teacher tile under 0b1010 and 0b1110
  n = 273  pair 0 owns groups 0 and 4 (the second with 17 envs): the hand-off counters of the
           teacher tiles carry over from one group to the next
  n = 48 at 32-env groups: two tiles, the second ragged, in the second group

Per mask and for 0: (a) the gradient per entry and globally, and the env state per component,
against the f64 oracle at tests/parity.py's bounds (MSE and KL, either actor; the observation-batch
mode at n = 50); (b) the mask against teacher_tiles = 0 in one process, bitwise: states, metrics,
gradient and parameters over three steps (mlp_forward_split_t and mlp_forward_pair_split are the same
arithmetic per net; measured on MI355X: bitwise equal in every case); (c) 60 steps without a
hand-off timeout; (d) a fresh process twice, equal digests (tests/_det_child.py's harness); and that
last_layout(teacher_tiles=True) reports the mask that ran.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import caller_batch as cb
from tests import env_batch as eb
from tests import parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
MASKS = (0, 0b0010, 0b1010, 0b1110)
SIZES = ((32, 64), (33, 64), (50, 64), (64, 64), (81, 64), (273, 64), (48, 32))   # n, envs per group
ALL_COMBOS = (50, 273)   # the sizes at which every (loss, actor) pair runs
OBS_N = 50


def _trainer(n, gs, mask, **kw):
    from reacherdistilation_amd.distill import DistillConfig, DistillTrainer
    teacher, student = cb.nets()
    kw.setdefault("seed", 3)
    return DistillTrainer(DistillConfig(n_envs=n, grid=1, stagger=False, group_envs=gs, teacher_tiles=mask, **kw),
                          device=DEV, teacher=teacher, student=student)


@functools.lru_cache(maxsize=None)
def _states(n):
    st = eb.draw_states(n, n)   # limit-free (|q1| <= 2.5)
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def _reference(n, loss):
    """The oracle of one rollout from _states(n): (g64, M, teacher mean, student mean); computed once."""
    teacher, student = cb.nets()
    g64, M, (fs, ft, _, _) = parity.oracle_grad(student.flat, teacher, student, eb.obs_from_state(_states(n)), loss, n)
    return g64, M, ft["mean"].astype(np.float32), fs["mean"].astype(np.float32)


def _cases():
    for mask in MASKS:
        for n, gs in SIZES:
            combos = [("mse", "teacher"), ("kl", "student")]
            if n in ALL_COMBOS:
                combos += [("kl", "teacher"), ("mse", "student")]
            for loss, act in combos:
                yield pytest.param(mask, n, gs, loss, act, id=f"m{mask}-n{n}-gs{gs}-{loss}-{act}")


@pytest.mark.parametrize("mask,n,gs,loss,act", list(_cases()))
def test_rollout_matches_oracle(oracle_c, mask, n, gs, loss, act):
    tr = _trainer(n, gs, mask, loss=loss, act_with=act)
    st0 = _states(n)
    tr.set_env_state(torch.from_numpy(np.array(st0)))
    tr.rollout()
    g = tr.grad().cpu().numpy()
    st1 = tr.env_state().cpu().numpy()
    assert tr.counter() == 1   # raises on a timed-out hand-off
    assert tr.last_layout(teacher_tiles=True) == (gs, 1, False, "env", mask), tr.last_layout(teacher_tiles=True)
    g64, M, mt, ms = _reference(n, loss)
    ok, rep = parity.grad_ok(g, g64, M)
    ref = np.ascontiguousarray(st0.astype(np.float64))
    oracle_c.step(ref, ms if act == "student" else mt, np.float64)
    sok, worst = parity.state_ok(st1, ref, np.zeros(n, bool))
    print(f"teacher_tiles={mask} n={n} gs={gs} {loss} act={act}: global {rep['global']:.2e} entry {rep['entry']:.2e} "
          f"in {rep['block']}; state {worst}")
    assert ok, rep
    assert sok, worst
    tr.close()


@pytest.mark.parametrize("loss", ["mse", "kl"])
@pytest.mark.parametrize("mask", MASKS)
def test_obs_mode_matches_oracle(mask, loss):
    n = OBS_N
    ob, _ = cb.batch(n)
    tr = _trainer(64, 64, mask, loss=loss)
    tr.rollout_obs(torch.from_numpy(np.array(ob)).to(DEV))
    g = tr.grad().cpu().numpy()
    tr.counter()
    assert tr.last_layout(teacher_tiles=True) == (64, 1, False, "obs", mask)
    g64, M, _, _ = cb.reference("obs", n, loss)
    ok, rep = parity.grad_ok(g, g64, M)
    print(f"teacher_tiles={mask} obs n={n} {loss}: {rep}")
    assert ok, rep
    tr.close()


@pytest.mark.parametrize("n,gs", [(50, 64), (64, 64), (273, 64), (48, 32)])
@pytest.mark.parametrize("loss,act", [("mse", "teacher"), ("kl", "student")])
@pytest.mark.parametrize("mask", MASKS[1:])
def test_mask_is_bitwise_the_producer_side_teacher(mask, loss, act, n, gs):
    """Three fused steps with the mask and with teacher_tiles = 0 from the same states: env states,
    metrics rows, gradient and student parameters bitwise equal after each."""
    a, b = (_trainer(n, gs, m, loss=loss, act_with=act, lr=1e-3) for m in (mask, 0))
    for t in (a, b):
        t.set_env_state(torch.from_numpy(np.array(_states(n))))
    for k in range(3):
        a.step()
        b.step()
        assert a.last_layout(teacher_tiles=True)[4] == mask and b.last_layout(teacher_tiles=True)[4] == 0
        assert torch.equal(a.env_state(), b.env_state()), k
        assert torch.equal(a.grad(), b.grad()), k
        assert torch.equal(a.student_params(), b.student_params()), k
    assert a.counters() == b.counters() == (3, 3)
    assert np.array_equal(a.metrics(3), b.metrics(3))
    a.close()
    b.close()


@pytest.mark.parametrize("mask", MASKS[1:])
def test_sixty_steps_without_a_handoff_timeout(mask):
    tr = _trainer(64, 64, mask)
    for _ in range(60):
        tr.step()
    assert tr.counters() == (60, 60)   # reads ctl: raises if ctl[8] was set
    assert np.isfinite(tr.grad().cpu().numpy()).all()
    tr.close()


def test_bf16_student_keeps_its_mask():
    """The bf16 student's kernel is built with 0b1010 only: the field does not reach it."""
    for mask in (0, 0b1110):
        tr = _trainer(64, 64, mask, student_dtype="bf16", act_with="student")
        tr.rollout()
        tr.counter()
        assert tr.last_layout(teacher_tiles=True) == (64, 1, False, "env", 0b1010)
        tr.close()


def test_exact_and_kstep_launches_take_no_mask():
    tr = _trainer(64, 64, 0b1110, f32_split=False)
    tr.rollout()
    assert tr.last_layout(teacher_tiles=True)[4] == 0
    tr.close()
    tr = _trainer(64, 64, 0b1110, accum_steps=3)
    tr.rollout_accum()
    tr.counter()
    assert tr.last_layout(teacher_tiles=True)[4] == 0
    tr.close()


def _child():
    r = subprocess.run([sys.executable, os.path.join(HERE, "_teacher_tiles_child.py")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_first_launch_of_a_process_is_reproducible():
    a, b = _child(), _child()
    assert sorted(a) == sorted(f"tt{m}_n4160" for m in MASKS[1:])
    bad = {n: (a[n], b[n]) for n in a if len(set(a[n] + b[n])) != 1}
    assert not bad, bad
    assert len({a[n][0] for n in a}) == 1, a   # and the masks agree with each other
