"""Prioritised draws from the device replay ring (include/reacher_replay_priority.h,
reacherdistilation_amd/replay.py) against their model (tests/replay_prio_model.py): the weighted draw
over every scan-tile boundary and fill state, the shared draw counter, what the four pushes write, the
maximum-over-writers update and its skipped indices, the calls under graph replay, and the
``replay_priority`` modes of the two train_envs drivers.  The score is four float32 operations with
one rounding each and everything else is integer, so every comparison is bitwise; there is no
tolerance anywhere."""
import ctypes
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.replay_model import REC, STEPS
from tests.replay_prio_model import ERR, INIT_CONST, INIT_RECORD, SQERR, PrioRingModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RD_EINVAL = -100000
SEED = 0x0123_4567_89AB_CDEF   # both key words non-zero
BASE = 2 ** 33 + 5             # a window base past 32 bits
MEASURES = {SQERR: "sqerr", ERR: "err"}
INITS = {INIT_CONST: "const", INIT_RECORD: "record"}


def _tile():
    from reacherdistilation_amd.replay import PRIO_SCAN_TILE
    return PRIO_SCAN_TILE


def _pair(capacity, max_batch=4096, table=None, **cfg):
    """a ring with priorities enabled and its model, same config"""
    from reacherdistilation_amd.replay import ReplayRing
    c = dict(measure=SQERR, shift=16, q_min=1, q_init=2 ** 24, init=INIT_CONST)
    c.update(cfg)
    ring = ReplayRing(capacity, device=DEV, seed=SEED, max_batch=max_batch)
    ring.enable_priorities(measure=MEASURES[c["measure"]], shift=c["shift"], q_min=c["q_min"], q_init=c["q_init"],
                           init=INITS[c["init"]], table=table)
    return ring, PrioRingModel(capacity, SEED, **c)


def _episodes(E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(E, STEPS, REC, generator=g).to(DEV)


def _push(ring, model, eps):
    ring.push_episodes(eps)
    model.push_episodes(eps.cpu().numpy())


def _table(ring):
    """the device table as the uint32 it is"""
    return ring.priorities.cpu().numpy().view(np.uint32)


def _set_table(ring, model, q):
    q = np.ascontiguousarray(q, np.uint32)
    ring.priorities.copy_(torch.from_numpy(q.view(np.int32)))
    model.q[:] = q


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (what, k)


def _fill_state(ring, model, fill):
    """partly filled, exactly full, or wrapped twice (more than 2 x capacity episodes pushed)"""
    cap = model.capacity
    pushes = {"part": [max(1, (2 * cap) // 3)], "full": [cap], "wrapped": [cap, cap, max(1, cap // 3)]}[fill]
    for k, E in enumerate(pushes):
        _push(ring, model, _episodes(E, 100 + k))
    assert ring.counters() == (sum(pushes), 0) and model.pushed == sum(pushes)


def _check_draws(ring, model, Bs=(1, 255, 257, 4096), recents=(0, 3), Ts=(1, 10, 50)):
    for T, recent, B in itertools.product(Ts, recents, Bs):
        got = ring.sample_windows(T, B, recent=recent, window_base=BASE, with_idx=True, prioritized=True, with_prob=True)
        _same(got, model.sample_windows_prio(T, B, recent, BASE), ("windows", T, recent, B))
        if T == 1:
            got = ring.sample_rows(B, recent=recent, window_base=BASE, with_idx=True, prioritized=True, with_prob=True)
            _same(got, model.sample_rows_prio(B, recent, BASE), ("rows", recent, B))
    assert ring.counters() == (model.pushed, model.draws)


# -- the draw -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["part", "full", "wrapped"])
@pytest.mark.parametrize("cap", ["5", "12", "300", "tile-1", "tile+1", "2tile+3"])
def test_prioritised_draw_equals_the_model(cap, fill):
    """idx, prob and every gathered tensor, at capacities on both sides of one and two scan tiles; at
    300 every entry is 2^24, so the T = 1 total (300 x 50 x 2^24 at full) passes 2^32 and a 32-bit sum
    anywhere would show; elsewhere random entries that include 1 and 2^24."""
    t = _tile()
    capacity = {"5": 5, "12": 12, "300": 300, "tile-1": t - 1, "tile+1": t + 1, "2tile+3": 2 * t + 3}[cap]
    ring, model = _pair(capacity)
    _fill_state(ring, model, fill)
    if capacity == 300:
        ring.fill_priorities(2 ** 24)
        model.fill(2 ** 24)
        assert model.stored() * 50 * 2 ** 24 > 2 ** 32
    else:
        q = np.random.RandomState(capacity).randint(1, 2 ** 24 + 1, (capacity, STEPS))
        q[0, :3], q[-1, -3:] = (1, 2 ** 24, 1), (2 ** 24, 1, 2 ** 24)
        _set_table(ring, model, q)
    small = capacity > 2 * t                         # the two-tile ring: fewer batch sizes, same paths
    _check_draws(ring, model, Bs=(257, 4096) if small else (1, 255, 257, 4096))
    assert np.array_equal(_table(ring), model.q)     # a draw writes nothing to the table
    ring.close()


def test_every_read_clamps_raw_entries():
    """0 and 2^31 written straight into ring.priorities read as 1 and 2^24"""
    ring, model = _pair(12)
    _fill_state(ring, model, "wrapped")
    q = np.random.RandomState(1).randint(1, 2 ** 20, (12, STEPS)).astype(np.uint32)
    q[::2, ::3], q[1::2, 1::4], q[5] = 0, 2 ** 31, 2 ** 32 - 1
    _set_table(ring, model, q)
    assert (_table(ring) == 0).any() and (_table(ring) == 2 ** 31).any()
    _check_draws(ring, model, Bs=(257,))
    q[:] = 0                                         # all zero: the uniform law, prob = 1 / (12 x 41) exactly
    _set_table(ring, model, q)
    *_, prob = ring.sample_windows(10, 64, prioritized=True, with_prob=True)
    assert bool((prob == np.float32(1.0 / (12 * 41))).all())
    ring.close()


# -- the counter ----------------------------------------------------------------------------------
def test_one_draw_counter_for_both_kinds_of_sample():
    from reacherdistilation_amd.replay import ReplayRing
    ring, model = _pair(12)
    plain = ReplayRing(12, device=DEV, seed=SEED, max_batch=4096)
    eps = _episodes(7, 3)
    _push(ring, model, eps)
    plain.push_episodes(eps)
    ring.sample_rows(64, prioritized=True)
    assert ring.counters() == (7, 1)
    ring.sample_windows(10, 64, prioritized=True)
    assert ring.counters() == (7, 2)
    for _ in range(2):
        plain.sample_rows(64)
    # draw index 2 on both: a uniform sample on a ring with priorities is the ring's without them
    a = ring.sample_rows(64, window_base=BASE, with_idx=True)
    b = plain.sample_rows(64, window_base=BASE, with_idx=True)
    _same(a, [v.cpu().numpy() for v in b], "uniform rows")
    a = ring.sample_windows(10, 64, common_start=True, with_idx=True)
    b = plain.sample_windows(10, 64, common_start=True, with_idx=True)
    _same(a, [v.cpu().numpy() for v in b], "uniform windows")
    assert ring.counters() == plain.counters() == (7, 4)
    model.draws = 4
    _same(ring.sample_rows(64, with_idx=True, prioritized=True, with_prob=True), model.sample_rows_prio(64), "d = 4")
    ring.close()
    plain.close()


def test_checks_that_read_an_enabled_handle():
    from reacherdistilation_amd import _native as nat
    from reacherdistilation_amd._native import NativeError
    from reacherdistilation_amd.replay import RdReplayPrioConfig, RdReplaySample, ReplayRing
    ring, _ = _pair(12, max_batch=64)
    with pytest.raises(NativeError) as e:            # nothing was ever pushed
        ring.sample_rows(8, prioritized=True)
    assert f"rc={RD_EINVAL}" in str(e.value) and "never been pushed" in str(e.value)
    with pytest.raises(NativeError) as e:
        ring.sample_windows(10, 8, prioritized=True)
    assert f"rc={RD_EINVAL}" in str(e.value) and "never been pushed" in str(e.value)
    ring.push_episodes(_episodes(2, 1))
    # windows > max_batch and a second enable, natively (the Python layer refuses both first)
    x, t = torch.zeros(65, 16, device=DEV), torch.zeros(65, 4, device=DEV)
    s = RdReplaySample(steps=1, start_mode=0, windows=65, window_base=0, recent=0, seed=1)
    assert ring._lib.rd_replay_prio_sample_rows(ring._h, ctypes.byref(s), nat.ptr(x), nat.ptr(t), None, None) == RD_EINVAL
    assert "max_batch" in ring._lib.rd_last_error().decode()
    idx, sp = torch.zeros(65, 2, dtype=torch.int32, device=DEV), torch.zeros(65, 4, device=DEV)
    assert ring._lib.rd_replay_prio_update_rows(ring._h, nat.ptr(idx), nat.ptr(sp), 65) == RD_EINVAL
    assert "max_batch" in ring._lib.rd_last_error().decode()
    c = RdReplayPrioConfig(measure=0, shift=16, q_min=1, q_init=5, init_mode=0, reserved=0)
    assert ring._lib.rd_replay_prio_enable(ring._h, ctypes.byref(c), nat.ptr(ring.priorities)) == RD_EINVAL
    assert "already enabled" in ring._lib.rd_last_error().decode()
    assert ring._lib.rd_replay_prio_enabled(ring._h) == 1
    assert ring._lib.rd_replay_prio_table(ring._h) == ring.priorities.data_ptr()
    assert ring.counters() == (2, 0) and bool((ring.priorities == 2 ** 24).all())   # the refused calls did nothing
    with pytest.raises(ValueError):
        ring.enable_priorities()
    with pytest.raises(ValueError):
        ring.sample_windows(10, 8, common_start=True, prioritized=True)
    ring.close()
    off = ReplayRing(12, device=DEV, seed=SEED, max_batch=64)   # priorities never enabled
    off.push_episodes(_episodes(2, 1))
    for call in (lambda: off.sample_rows(8, prioritized=True), lambda: off.fill_priorities(3),
                 lambda: off.update_priorities(idx[:8], sp[:8]), lambda: off.set_priority_init("record")):
        with pytest.raises(ValueError):
            call()
    assert off._lib.rd_replay_prio_enabled(off._h) == 0 and off._lib.rd_replay_prio_table(off._h) is None
    s.windows = 8
    assert off._lib.rd_replay_prio_sample_rows(off._h, ctypes.byref(s), nat.ptr(x), nat.ptr(t), None, None) == RD_EINVAL
    assert "not enabled" in off._lib.rd_last_error().decode()
    off.close()


# -- pushes ---------------------------------------------------------------------------------------
def _spiked(shape, seed):
    """random outputs with NaN, +-inf and 1e6 among them: the !(v < 2^24) branch runs"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(*shape, generator=g)
    flat = v.view(-1)
    for k, bad in enumerate((float("nan"), float("inf"), float("-inf"), 1e6, -1e6)):
        flat[7 + 13 * k::97] = bad
    return v.to(DEV)


@pytest.mark.parametrize("shift", [0, 16, 24])
@pytest.mark.parametrize("measure", [SQERR, ERR])
def test_every_push_writes_its_slots_priorities(measure, shift):
    """init="record" through push_steps, push_episodes, push_rows and its flags form, with wrap; then
    init="const"; set_priority_init takes effect at the next push."""
    cap, n = 12, 5
    ring, model = _pair(cap, measure=measure, shift=shift, q_min=3, q_init=77, init=INIT_RECORD)
    assert bool((ring.priorities == 77).all())

    def check(what):
        assert np.array_equal(_bits(ring.records), _bits(model.ring)), what
        assert np.array_equal(_table(ring), model.q), what
        assert ring.counters()[0] == model.pushed, what

    def rows(seed):
        return SimpleNamespace(x=_spiked((50, n, 16), seed), t_pdflat=_spiked((50, n, 4), seed + 1),
                               s_pdflat=_spiked((50, n, 4), seed + 2), reward=torch.randn(50, n, device=DEV))

    carry = np.zeros(n, np.float32)
    for rnd, init in enumerate((INIT_RECORD, INIT_CONST, INIT_RECORD)):   # 3 x 17 episodes through 12 slots
        ring.set_priority_init(INITS[init])
        model.init = init
        rec = _spiked((100, 1, REC), 10 * rnd)               # push_steps: 2 episodes of one env
        ring.push_steps(rec)
        model.push_steps(rec.cpu().numpy())
        check(("steps", rnd))
        eps = _spiked((n, STEPS, REC), 10 * rnd + 1)
        ring.push_episodes(eps)
        model.push_episodes(eps.cpu().numpy())
        check(("episodes", rnd))
        for flags in (None, (torch.rand(50, n, device=DEV) < 0.5).float()):
            r = rows(10 * rnd + (2 if flags is None else 5))
            ring.push_rows(r, stepped_with=flags)
            c = [v.cpu().numpy() for v in (r.x, r.t_pdflat, r.s_pdflat, r.reward)]
            if flags is None:
                model.push_rows(*c, carry, 1.0)
            else:                                            # the model's push_rows has one flag: set them after
                model.push_rows(*c, carry, 0.0)
                for i in range(n):
                    model.ring[(model.pushed - n + i) % cap, :, 20] = flags[:, i].cpu().numpy()
            carry = c[3][-1].copy()
            check(("rows", rnd, flags is not None))
            if init == INIT_CONST:
                assert (_table(ring) == 77).any()
    assert model.pushed == 3 * (2 + 3 * n) > 2 * cap
    got = _table(ring)                                       # the last 12 episodes: all scored from their records
    assert (got == 2 ** 24).any() and got.min() >= 3 and len(np.unique(got)) > 2
    ring.close()


# -- updates --------------------------------------------------------------------------------------
CANARY = 0x5A5A5A5A


def _canaried(cap):
    big = torch.full((cap + 4, STEPS), CANARY, dtype=torch.int32, device=DEV)
    return big, big[2:-2]


@pytest.mark.parametrize("measure", [SQERR, ERR])
def test_updates_take_the_maximum_and_skip_what_lies_outside(measure):
    cap = 12
    big, table = _canaried(cap)
    ring, model = _pair(cap, table=table, measure=measure, shift=16, q_min=2, q_init=50)
    assert ring.priorities.data_ptr() == table.data_ptr() and bool((table == 50).all())
    _fill_state(ring, model, "wrapped")
    # rows: record (2, 7) named by three writers with different outputs; bad entries of every kind
    idx = torch.tensor([[2, 7], [2, 7], [2, 7], [-1, 0], [cap, 0], [3, -1], [4, 50], [5, 49], [0, 0], [11, 49],
                        [2 ** 31 - 1, 3], [-2 ** 31, 0], [7, 2 ** 31 - 1]], dtype=torch.int32, device=DEV)
    s = _spiked((len(idx), 4), 4)
    s[:3, :2] = ring.records[2, 7, 12:14] + torch.tensor([[0.5, 0.0], [2.0, 0.0], [1.0, 0.0]], device=DEV)
    ring.update_priorities(idx, s)
    before = model.q.copy()
    model.update(idx.cpu().numpy(), s.cpu().numpy())
    assert np.array_equal(_table(ring), model.q)
    assert sorted(np.argwhere(model.q != before).tolist()) == [[0, 0], [2, 7], [5, 49], [11, 49]]
    three = [model.q[2, 7]]
    for b in range(3):                                       # each writer alone
        model.update(idx[b:b + 1].cpu().numpy(), s[b:b + 1].cpu().numpy())
        three.append(model.q[2, 7])
    assert three[0] == three[2] == max(three[1:]) and len(set(three[1:])) == 3
    # a real batch: sampled rows scored with arbitrary outputs, duplicates included
    x, t, idx = ring.sample_rows(4096, with_idx=True, prioritized=True)
    s = _spiked((4096, 4), 5)
    ring.update_priorities(idx, s)
    model.sample_rows_prio(4096)
    model.update(idx.cpu().numpy(), s.cpu().numpy())
    assert np.array_equal(_table(ring), model.q)
    assert len({tuple(r) for r in idx.cpu().tolist()}) < 4096
    # windows (T = 10): start 45 is skipped, overlapping windows share records
    idx = torch.tensor([[6, 45], [6, 0], [6, 5], [cap, 0], [-1, 3], [1, 41], [1, 40], [9, -1]], dtype=torch.int32, device=DEV)
    s = _spiked((10, len(idx), 4), 6)
    before = model.q.copy()
    ring.update_priorities(idx, s)
    model.update(idx.cpu().numpy(), s.cpu().numpy())
    assert np.array_equal(_table(ring), model.q)
    changed = {tuple(a) for a in np.argwhere(model.q != before).tolist()}
    assert changed and changed <= {(6, r) for r in range(15)} | {(1, r) for r in range(40, 50)}
    _, _, _, _, idx = ring.sample_windows(10, 257, with_idx=True, prioritized=True)
    s = _spiked((10, 257, 4), 7)
    ring.update_priorities(idx, s)
    model.sample_windows_prio(10, 257)
    model.update(idx.cpu().numpy(), s.cpu().numpy())
    assert np.array_equal(_table(ring), model.q)
    # nothing was ever written outside the table
    assert bool((big[:2] == CANARY).all()) and bool((big[-2:] == CANARY).all())
    ring.reset()                                             # the counters go, the table stays
    assert ring.counters() == (0, 0) and np.array_equal(_table(ring), model.q)
    ring.close()


# -- capture --------------------------------------------------------------------------------------
def test_push_sample_and_update_replay_from_one_graph():
    """One torch.cuda.graph holds a push, a prioritised sample and an update on one stream (a linear
    chain); each replay is the model's NEXT push, NEXT draw and the update of what it drew."""
    cap, T, B = 12, 10, 257
    ring, model = _pair(cap, shift=16, q_min=1, q_init=2 ** 20, init=INIT_RECORD)
    model.init = INIT_RECORD
    _push(ring, model, _episodes(7, 50))
    got = ring.sample_windows(T, B, with_idx=True, prioritized=True, with_prob=True)   # the buffers exist before
    _same(got, model.sample_windows_prio(T, B), "eager")
    static_eps = torch.zeros(4, STEPS, REC, device=DEV)
    static_s = torch.zeros(T, B, 4, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ring.push_episodes(static_eps)
        out = ring.sample_windows(T, B, with_idx=True, prioritized=True, with_prob=True)
        ring.update_priorities(out[4], static_s)
    assert ring.counters() == (7, 1)                         # capturing runs nothing
    for k in range(3):                                       # 7 + 3 x 4 episodes through 12 slots: wraps
        eps, s = _episodes(4, 60 + k), _spiked((T, B, 4), 70 + k)
        static_eps.copy_(eps)
        static_s.copy_(s)
        g.replay()
        torch.cuda.synchronize()
        model.push_episodes(eps.cpu().numpy())
        want = model.sample_windows_prio(T, B)
        _same(out, want, ("replay", k))
        model.update(want[4], s.cpu().numpy())
        assert np.array_equal(_table(ring), model.q), k
    assert ring.counters() == (19, 4) == (model.pushed, model.draws)
    ring.close()


# -- the drivers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["record", "refresh"])
@pytest.mark.parametrize("driver", ["mlp", "lstm"])
def test_train_envs_with_replay_priority(driver, mode):
    from reacherdistilation_amd import lstm_train, mlp_train
    mod = mlp_train if driver == "mlp" else lstm_train
    tr, hist = mod.train_envs(64, 6, replay_capacity=128, replay_windows=256, replay_priority=mode, device=DEV)
    assert len(hist) == 6 and all(np.isfinite(h[1]) and np.isfinite(h[2]) for h in hist)
    ring = tr.replay
    assert ring.counters() == (6 * 64, 6)
    q = _table(ring)
    assert (q != 2 ** 24).any() and q.min() >= 1 and q.max() <= 2 ** 24   # the pushes scored the records
    idx = ring.last_idx.cpu().numpy()
    assert idx.shape == (256, 2) and idx[:, 0].min() >= 0 and idx[:, 0].max() < 128
    assert idx[:, 1].min() >= 0 and idx[:, 1].max() <= (49 if driver == "mlp" else 40)
    tr.close()


@pytest.mark.parametrize("driver", ["mlp", "lstm"])
def test_replay_priority_none_is_the_loop_without_it(driver):
    from reacherdistilation_amd import lstm_train, mlp_train
    mod = mlp_train if driver == "mlp" else lstm_train
    kw = dict(replay_capacity=128, replay_windows=256, device=DEV)
    a, ha = mod.train_envs(64, 6, replay_priority="none", **kw)
    b, hb = mod.train_envs(64, 6, **kw)
    assert ha == hb and torch.equal(a.params(), b.params()) and a.replay.priorities is None
    # and priorities do change the draws: "record" is another history
    c, hc = mod.train_envs(64, 6, replay_priority="record", **kw)
    assert hc != ha
    for t in (a, b, c):
        t.close()
    with pytest.raises(ValueError):
        mod.train_envs(64, 6, replay_priority="record", device=DEV)
